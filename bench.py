#!/usr/bin/env python3
"""bench.py -- EmailVerifier witnesses/s on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of synthetic emails that is already
resident in HBM: `EmailVerifier(1024,1536,121,17,0,0,0,0)`, 1 KB bodies, batch 4096 per GPU
(BASELINE.json configs[2]), processed in tiles whose witnesses stay in HBM (a 2-tile ring that
is overwritten; the host-delivered, PCIe-bound rate is reported beside it, never as `value`).

    python bench.py --gpus N --steps K --warmup W        (N > 1 without a launcher: bench.py starts the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line:
  roofline      dominant kernel zk_expand (HBM-write bound): achieved = (32 W + I) bytes x emails per
                launch / average launch duration, HIP events on the launch stream inside the timed
                region.
A plain run stops there.  With --full (N=1) the line also holds the side measurements, each taking
runs of its own after the timed steps:
  roofline      alone_frac (zk_expand with the chip to itself), box_fill_GBps (a plain fill of the
                same buffer), and `traffic` = HBM bytes per launch from PMC counters collected IN THIS
                INVOCATION (two separate `rocprofv3 --pmc` child passes of a 1-step run of the same
                workload, WRITE_SIZE and FETCH_SIZE, corrected as MI355X_MICROARCH.md prescribes),
                or null with the reason in `traffic_source`.
  cpu_baseline  the C oracle ("port", oracle/c) built -O3 -march=native on this box, timed on its
                host cores (all-core and single-thread), buffers pre-touched (rank 0, N=1 only).
  other_configs BASELINE.json configs[1] (batch 256), configs[4] (maxBody 65536, batch 1024; fewer
                steps) and the delivered-to-host (PCIe-inclusive) rate, measured in the same run.

--dump-outputs DIR writes what the last timed step handed its caller as float64 .npy files (every
32-bit word of the outputs exactly), so that two builds can be compared output for output; the
inputs are a function of the command line only (seeded synthetic emails).
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zk-email-verify_amd", "py"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)


class Pipeline:
    """Two-phase pipeline over one resident batch: the compute kernels of a sub-batch of `prep`
    emails ("prepare": ~0.45 MB of compact image per email) run on one stream while the previous
    sub-batch's witnesses are streamed out tile by tile ("expand", the HBM-bound kernel) on
    another; images are ring-buffered, witnesses go to a 2-tile ring in HBM."""

    def __init__(self, torch, c, dev, d_in, batch, tile, prep, ring=2, prep_streams=1, rsa_throttle=0, exp_prio=-1,
                 montgomery=False, out_align=0, serial=False, prep_cus=0, prep_cu_stride=1, prep_prio=0, abc=False, place=True):
        self.torch, self.c, self.dev, self.d_in = torch, c, dev, d_in
        self.batch, self.tile, self.prep = batch, tile, prep
        assert batch % prep == 0 and prep % tile == 0
        self.nsub, self.tiles_per_sub = batch // prep, prep // tile
        self.ntiles = batch // tile
        self.rsa_throttle = rsa_throttle
        self.expand = c.expand_montgomery_device if montgomery else c.expand_device
        # distance between consecutive witnesses in the HBM ring (out_align > 0: padded to a multiple of it)
        self.stride = c.witness_bytes if not out_align or montgomery else (c.witness_bytes + out_align - 1) // out_align * out_align
        self.unit_bytes = c.witness_bytes
        if abc:
            # the prover's first stage instead of the witness: A.w | B.w | C.w of the attached constraint system (zkwg_expand_abc_device)
            self.expand = lambda d_in, n, scr, first, count, o, st: c.expand_abc_device(d_in, n, scr, first, count, o, st, montgomery=montgomery)
            self.stride = self.unit_bytes = c.abc_bytes
        self.d_status = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.R = max(2, ring)
        self.d_scr = [torch.empty(c.scratch_bytes(prep, montgomery=bool(montgomery)), dtype=torch.uint8, device=dev) for _ in range(self.R)]
        self.placement = None
        self.d_out = None
        place = 2 if place is True else int(place)      # (True == 1 in Python: without this every default-constructed pipeline ran BOTH placements)
        if place == 2:
            # the output ring is mapped from 1 GiB physical chunks (zkwg_device_alloc_chunked): every tile then
            # takes zk_expand's stores at the rate only the best hipMalloc buffers reach -- no candidates, no transient memory
            from zkwg import placement
            ntl = min(2, self.ntiles)
            nch = (tile * self.stride + (1 << 30) - 1) >> 30
            extra = min(nch // 2, 16)       # spare candidate chunks per tile: each takes a probe fill, the fastest are kept
            try:
                self.d_out = [placement.chunked_tensor(torch, dev, tile * self.stride, extra=extra) for _ in range(ntl)]
                rates = sorted(r for t in self.d_out for r in getattr(t._zkwg_owner, "rates", []))
                self.placement = {"mode": "chunked", "chunk_bytes": 1 << 30, "tiles": ntl, "tile_bytes": tile * self.stride, "spare_chunks_per_tile": extra,
                                  "candidate_chunk_GBps": ({"min": rates[0], "median": rates[len(rates) // 2], "max": rates[-1], "n": len(rates)} if rates else None)}
            except Exception as e:          # a runtime without the virtual-memory API: round 4's candidate search instead
                self.d_out = None
                place = 1
                chunk_error = repr(e)[:160]
        if place == 1:
            # round 4's way (--place-ring 1): spare candidate buffers from hipMalloc, the real expansion of one tile timed into each,
            # the fastest kept
            from zkwg import placement
            cur = torch.cuda.current_stream()
            c.set_prepare_throttle(0)
            c.prepare_device(d_in[:prep], prep, self.d_status[:prep], self.d_scr[0], cur)
            kw = {} if self.stride == self.unit_bytes else {"out_stride": self.stride}
            self.d_out, self.placement = placement.choose_tiles(
                torch, dev, tile * self.stride, min(2, self.ntiles),
                lambda buf: self.expand(d_in[:prep], prep, self.d_scr[0], 0, tile, buf, cur, **kw))
            torch.cuda.synchronize()
            if "chunk_error" in locals():
                self.placement["chunked_allocation_failed"] = chunk_error
        if self.d_out is None:
            self.d_out = [torch.empty(tile * self.stride, dtype=torch.uint8, device=dev) for _ in range(min(2, self.ntiles))]
        # several prepare streams let the latency-bound prepare kernels of consecutive SMALL sub-batches overlap
        self.s_preps = [torch.cuda.Stream(device=dev, priority=prep_prio) for _ in range(max(1, prep_streams))]
        self.s_exp = torch.cuda.Stream(device=dev, priority=exp_prio)
        self.serial = serial
        self._masked = []
        if prep_cus > 0:
            # the prepare kernels on `prep_cus` compute units only (CU-masked HIP stream), zk_expand on the others
            ncu = torch.cuda.get_device_properties(dev).multi_processor_count
            words = (ncu + 31) // 32
            sel = set(range(prep_cus)) if prep_cu_stride <= 1 else set(i * prep_cu_stride for i in range(prep_cus) if i * prep_cu_stride < ncu)

            def mask(keep):
                m = [0] * words
                for i in range(ncu):
                    if keep(i):
                        m[i // 32] |= 1 << (i % 32)
                return (ctypes.c_uint32 * words)(*m), words
            mp, w = mask(lambda i: i in sel)
            me, _ = mask(lambda i: i not in sel)
            sp = c.lib.zkwg_stream_create_masked(dev.index, mp, w)
            se = c.lib.zkwg_stream_create_masked(dev.index, me, w)
            assert sp and se, "hipExtStreamCreateWithCUMask failed"
            self._masked = [sp, se]
            self.s_preps = [torch.cuda.ExternalStream(sp, device=dev)]
            self.s_exp = torch.cuda.ExternalStream(se, device=dev)
        self.ev_prep = [torch.cuda.Event() for _ in range(self.R)]
        self.ev_exp = [torch.cuda.Event() for _ in range(self.R)]
        self.j = 0
        # per-email result rows (w[0..3] = 1, pubkeyHash, shaHi, shaLo) saved before the ring slot is reused
        self.d_rows = torch.empty((batch, 128), dtype=torch.uint8, device=dev)

    def _expand_tiles(self, lo, b, sb):
        torch = self.torch
        with torch.cuda.stream(self.s_exp):
            for t in range(self.tiles_per_sub):
                o = self.d_out[(sb * self.tiles_per_sub + t) % len(self.d_out)]
                if self.stride != self.unit_bytes:
                    self.expand(self.d_in[lo:lo + self.prep], self.prep, self.d_scr[b], t * self.tile, self.tile, o, self.s_exp, out_stride=self.stride)
                else:
                    self.expand(self.d_in[lo:lo + self.prep], self.prep, self.d_scr[b], t * self.tile, self.tile, o, self.s_exp)
                self.d_rows[lo + t * self.tile:lo + (t + 1) * self.tile].copy_(o.view(self.tile, self.stride)[:, :128])
        self.ev_exp[b].record(self.s_exp)

    def step_lagged(self):
        """serial == 2: the prepare kernels of sub-batch j and the expansion of sub-batch j - 1 take turns on the chip (P1 P2 E1 P3 E2 ...):
        neither shares the SIMDs' issue slots with the other, and what a prepare leaves on the handle's side streams (the Poseidon(2) merge
        chain of removeSoftLineBreaks: 191 dependent permutations per email, a few wavefronts) runs beside the expansion of j - 1 and the
        prepare of j + 1 before the expansion of j needs it.  A step = one prepare + one expansion per sub-batch, one sub-batch apart; needs
        a ring of >= 3 image buffers."""
        c = self.c
        assert self.R >= 3
        for sb in range(self.nsub):
            j = self.j
            b = j % self.R
            s_prep = self.s_preps[0]
            lo = sb * self.prep
            if j >= 2:
                s_prep.wait_event(self.ev_exp[(j - 2) % self.R])      # the expansion of j - 2 is over (and image buffer b has long been read)
            c.set_prepare_throttle(0)
            c.prepare_device(self.d_in[lo:lo + self.prep], self.prep, self.d_status[lo:lo + self.prep], self.d_scr[b], s_prep)
            self.ev_prep[b].record(s_prep)
            if j >= 1:
                self.s_exp.wait_event(self.ev_prep[b])                 # ... and the expansion of j - 1 starts when the prepare of j is over
                self._expand_tiles(self._lag[0], self._lag[1], self._lag[2])
            self._lag = (lo, b, sb)
            self.j = j + 1

    def step(self):
        if self.serial == 2:
            return self.step_lagged()
        torch, c = self.torch, self.c
        for sb in range(self.nsub):
            j = self.j
            b = j % self.R
            s_prep = self.s_preps[j % len(self.s_preps)]
            lo = sb * self.prep
            if j >= self.R:
                s_prep.wait_event(self.ev_exp[b])      # image buffer b is free again
            # the very first prepare has nothing to overlap with: run it at full occupancy; later ones share
            # the chip with the previous sub-batch's zk_expand and are throttled so expand keeps its wave slots
            c.set_prepare_throttle(0 if j == 0 else self.rsa_throttle)
            c.prepare_device(self.d_in[lo:lo + self.prep], self.prep, self.d_status[lo:lo + self.prep], self.d_scr[b], s_prep)
            self.ev_prep[b].record(s_prep)
            self.s_exp.wait_event(self.ev_prep[b])
            with torch.cuda.stream(self.s_exp):
                for t in range(self.tiles_per_sub):
                    o = self.d_out[(sb * self.tiles_per_sub + t) % len(self.d_out)]
                    if self.stride != self.unit_bytes:
                        self.expand(self.d_in[lo:lo + self.prep], self.prep, self.d_scr[b], t * self.tile, self.tile, o, self.s_exp, out_stride=self.stride)
                    else:
                        self.expand(self.d_in[lo:lo + self.prep], self.prep, self.d_scr[b], t * self.tile, self.tile, o, self.s_exp)
                    self.d_rows[lo + t * self.tile:lo + (t + 1) * self.tile].copy_(o.view(self.tile, self.stride)[:, :128])
            self.ev_exp[b].record(self.s_exp)
            if self.serial:
                for sp in self.s_preps:
                    sp.wait_event(self.ev_exp[b])
            self.j = j + 1

    def last_tile(self):
        return self.d_out[(self.nsub * self.tiles_per_sub - 1) % len(self.d_out)]


def resident_inputs(torch, c, dev, seed, distinct, batch, body_len):
    from zkwg import synth
    recs, fields = synth.packed_batch(c, seed=seed, n=distinct, body_len=body_len)
    h_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).view(distinct, c.in_stride)
    reps = (batch + distinct - 1) // distinct
    return h_in, h_in.repeat(reps, 1)[:batch].contiguous().to(dev), fields


def resident_inputs_ragged(torch, c, dev, seed, distinct, batch, lo, hi):
    """like resident_inputs, with `distinct` different body lengths spread evenly over [lo, hi] (BASELINE.json configs[4]:
    bodies of 32 K .. 65 K - 72 bytes)"""
    from zkwg import synth
    recs = b"".join(synth.packed_batch(c, seed=seed, n=1, body_len=lo + (hi - lo) * i // max(distinct - 1, 1), first_index=i)[0]
                    for i in range(distinct))
    h_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).view(distinct, c.in_stride)
    reps = (batch + distinct - 1) // distinct
    return h_in.repeat(reps, 1)[:batch].contiguous().to(dev)


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def last_expanded(pl):
    """(ring buffer, batch index of its first email) of the tile the pipeline expanded last: the step's last tile, or with
    --no-overlap 2 (the expansion lags one sub-batch behind) the last tile of the sub-batch before the step's last one"""
    sb = pl.nsub - 1 if pl.serial != 2 else (pl.nsub - 2) % pl.nsub
    k = sb * pl.tiles_per_sub + pl.tiles_per_sub - 1
    return pl.d_out[k % len(pl.d_out)], sb * pl.prep + (pl.tiles_per_sub - 1) * pl.tile


def save_outputs(out_dir, arrays):
    """arrays: name -> float64 ndarray, written as out_dir/<name>.npy (64 MB at most in all)"""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes exceed 64 MB"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype == np.float64
        np.save(os.path.join(out_dir, name + ".npy"), a)


def words_f64(a):
    """uint8 ndarray [..., 4k] -> float64 [..., k] of its little-endian 32-bit words (exact)"""
    import numpy as np
    return np.ascontiguousarray(a).view("<u4").astype(np.float64)


def dump_witness_outputs(out_dir, torch, pl, table, first_email):
    """--dump-outputs of the witness pipeline.  The caller of the timed path holds the result table (status + the outputs
    w[1..3] of every email of the job) and the witnesses of the tile expanded last in its HBM ring (57 MB each at the headline
    circuit, so a fixed, seeded sample of them plus a checksum of every word):
      status.npy                 [emails]          int32 status per email
      result_table.npy           [emails, 25]      the table's 32-bit words (status, pubkeyHash, shaHi, shaLo)
      witness_sample.npy         [8, 65536, 8]     32-bit words of 65,536 seeded field elements of 8 seeded witnesses
      witness_sample_emails.npy  [8]               their email indices in the job
      witness_sample_elements.npy [65536]          their element indices in the witness
      witness_word_sums.npy      [tile, 2]         per witness of that tile: sums of the low and of the high 16 bits of all its words"""
    import numpy as np
    torch.cuda.synchronize()
    tb = table.cpu().numpy()
    arrays = {"status": tb[:, :4].copy().view("<i4").reshape(-1).astype(np.float64), "result_table": words_f64(tb)}
    o, lo = last_expanded(pl)
    rows = o.view(pl.tile, pl.stride)[:, :pl.unit_bytes]
    n_el = pl.unit_bytes // 32
    rng = np.random.default_rng(0x5A4B)
    em = np.sort(rng.choice(pl.tile, size=min(8, pl.tile), replace=False))
    el = np.sort(rng.choice(n_el, size=min(65536, n_el), replace=False))
    sel = rows[torch.from_numpy(em).to(o.device)].view(len(em), n_el, 32)[:, torch.from_numpy(el).to(o.device)]
    arrays["witness_sample"] = words_f64(sel.cpu().numpy())
    arrays["witness_sample_emails"] = (first_email + lo + em).astype(np.float64)
    arrays["witness_sample_elements"] = el.astype(np.float64)
    sums = torch.empty((pl.tile, 2), dtype=torch.int64, device=o.device)
    for i in range(0, pl.tile, 16):
        w = rows[i:i + 16].contiguous().view(torch.int32)
        sums[i:i + 16, 0] = (w & 0xFFFF).sum(dim=1, dtype=torch.int64)
        sums[i:i + 16, 1] = ((w >> 16) & 0xFFFF).sum(dim=1, dtype=torch.int64)
    arrays["witness_word_sums"] = sums.cpu().numpy().astype(np.float64)     # < 2^44: exact
    save_outputs(out_dir, arrays)


def expand_roofline(c, tile):
    summ = c.timing_summary()
    ex_ms, ex_launches, _ = summ["zk_expand"]
    bpe = 32 * c.W + c.in_stride
    avg = ex_ms / max(ex_launches, 1)
    gbs = bpe * tile / (avg * 1e-3) / 1e9
    return summ, avg, ex_launches, gbs


def pmc_traffic(args, tile, W):
    """HBM bytes per zk_expand launch from PMC counters: two rocprofv3 child passes (WRITE_SIZE, then
    FETCH_SIZE; --pmc with --kernel-trace only) of this script in --pmc-child mode (1 step of the same
    workload).  Returns (bytes or None, source string)."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found on this box"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="zkwg_pmc_", dir="/tmp")
    try:
        for ctr in ("WRITE_SIZE", "FETCH_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = [exe, "--kernel-trace", "--pmc", ctr, "--output-format", "csv", "-d", out, "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child", "--steps", "1", "--warmup", "0",
                   "--batch", str(args.batch), "--tile", str(tile), "--prep-batch", str(args.prep_batch),
                   "--max-header", str(args.max_header), "--max-body", str(args.max_body),
                   "--body-len", str(args.body_len), "--distinct", "64"]
            env = dict(os.environ, TMPDIR="/tmp")
            try:
                r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                   timeout=args.pmc_timeout)
            except subprocess.TimeoutExpired:
                return None, f"rocprofv3 --pmc {ctr} pass timed out after {args.pmc_timeout}s"
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {ctr} pass failed (exit {r.returncode}): {r.stderr.decode(errors='replace')[-200:]}"
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return None, f"rocprofv3 --pmc {ctr} pass wrote no counter_collection.csv"
            got = [float(row["Counter_Value"]) for row in csv.DictReader(open(files[0]))
                   if row["Kernel_Name"].startswith("zk_expand") and row.get("Counter_Name", ctr) == ctr]
            if not got:
                return None, f"no zk_expand rows in the {ctr} pass"
            vals[ctr] = (sum(got) / len(got), len(got))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # counters are in KiB; gfx950: FETCH_SIZE counts 64 B per 128 B request -> x2 (guide, HBM section)
    write_b = vals["WRITE_SIZE"][0] * 1024.0
    fetch_b = vals["FETCH_SIZE"][0] * 1024.0 * 2.0
    src = (f"PMC, this invocation: rocprofv3 --kernel-trace --pmc WRITE_SIZE / --pmc FETCH_SIZE (separate child passes, "
           f"1 step of the same workload, {vals['WRITE_SIZE'][1]} zk_expand launches each); write {write_b / 1e9:.3f} GB + "
           f"fetch (x2 gfx950 correction) {fetch_b / 1e9:.3f} GB per launch")
    return write_b + fetch_b, src


def prove_main(args, torch, dist, backend, dev, rank, world, local_rank):
    """`bench.py --gpus N --prove 1`: proofs shard like witnesses (independent emails, contiguous ranges, no data-path
    collective).  Rank r proves the emails [r pb, (r + 1) pb) of a job of N pb emails -- inputs and blinding are functions of the GLOBAL
    email index, so the gathered proofs do not depend on N (`proofs_sha256`; tests/test_multi.py compares 1 rank with 2) -- and the only
    exchange is the gather of status + proof (260 bytes per email) on rank 0, inside the timed region.  Every rank uploads the key once
    (tables: ~11 GB at the headline circuit).  Reference call site: packages/helpers/src/chunked-zkey.ts:80-84."""
    import hashlib
    import random
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import bench_prove
    from zkwg import shard, synth
    N, M, pb = args.max_header, args.max_body, args.prove_batch
    t0 = time.time()
    c, pv, _, _, n_public, power, n_rows = bench_prove.make_prover(N, M, device=local_rank)
    t_setup = time.time() - t0
    lo = rank * pb
    recs, _ = synth.packed_batch(c, seed=0x5A4B, n=pb, body_len=min(args.body_len, M - 80), first_index=lo)
    rng = random.Random(0x5A4B)
    blinding = [(rng.randrange(1, bench_prove_R()), rng.randrange(1, bench_prove_R())) for _ in range(pb * world)][lo:lo + pb]
    d_in = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    d_status = torch.zeros(pb, dtype=torch.int32, device=dev)
    d_scratch = torch.empty(c.scratch_bytes(pb), dtype=torch.uint8, device=dev)
    state = {"table": None}

    def step():
        c.prepare_device(d_in, pb, d_status, d_scratch)
        torch.cuda.synchronize()
        st = d_status.tolist()
        idx = [i for i in range(pb) if st[i] == 0]
        proofs = pv.prove_batch_bytes(d_in, pb, d_scratch, idx, [blinding[i] for i in idx], slots=args.prove_slots)
        rows = bytearray(260 * pb)
        for i in range(pb):
            rows[260 * i:260 * i + 4] = int(st[i]).to_bytes(4, "little", signed=True)
        for k, i in enumerate(idx):
            rows[260 * i + 4:260 * i + 260] = proofs[256 * k:256 * k + 256]
        table = torch.frombuffer(rows, dtype=torch.uint8).view(pb, 260)
        if dist is not None and backend == "nccl":
            table = table.to(dev)
        state["table"] = shard.gather_rows(dist, table, pb * world, rank, world) if dist is not None else table

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    t1 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = time.perf_counter() - t1
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if rank == 0 and args.dump_outputs:
        # what rank 0 holds after the last step: status + proof (pi_a, pi_b, pi_c) per email of the job
        t = state["table"].cpu().numpy()
        save_outputs(args.dump_outputs, {"status": t[:, :4].copy().view("<i4").reshape(-1).astype("float64"), "proof_table": words_f64(t)})
    if rank == 0:
        tab = bytes(state["table"].cpu().numpy().tobytes())
        bad = sum(1 for i in range(pb * world) if tab[260 * i:260 * i + 4] != bytes(4))
        print(json.dumps({
            "metric": "Groth16 proofs/s (inputs -> witness -> proof, EmailVerifier)", "value": round(pb * world * args.steps / dt, 2), "unit": "proofs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u64 (Fr / Fq limbs)", "data": "synthetic",
            "config": {"workload": f"EmailVerifier({N},{M},121,17,0,0,0,0) proofs, {pb} emails per GPU per step, {args.prove_slots} in flight per GPU",
                       "W": c.W, "domain_log2": power, "rows": n_rows, "parallelism": f"shard{world}"},
            "gathered_rows": pb * world, "nonzero_status": bad, "proofs_sha256": hashlib.sha256(tab).hexdigest(),
            "emails_per_series": pv.lib.zkwg_prover_emails_per_series(pv._h), "contexts": pv.lib.zkwg_prover_contexts(pv._h),
            "key_setup_s_per_rank": round(t_setup, 1), "backend": backend if dist is not None else None,
            "note": "key from known discrete logarithms (tools/bench_prove.py: sums_verified there); the same key on every rank"}), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    return 0


def bench_prove_R():
    return 21888242871839275222246405745257275088548364400416034343698204186575808495617


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096, help="emails per GPU per step")
    ap.add_argument("--tile", type=int, default=512, help="emails per launch (HBM-resident tile)")
    ap.add_argument("--distinct", type=int, default=512, help="distinct synthetic emails generated per rank")
    ap.add_argument("--max-header", type=int, default=1024)
    ap.add_argument("--max-body", type=int, default=1536)
    ap.add_argument("--body-len", type=int, default=1024)
    ap.add_argument("--prep-batch", type=int, default=0,
                    help="emails per prepare launch (pipeline granularity); 0 = 1024, or 2048 with --regex (zk_net_eval is one "
                         "wavefront per email: two per SIMD hide its latencies)")
    ap.add_argument("--rsa-throttle", type=int, default=0, help="resident zk_rsa wavefronts per CU while overlapped (0 = no cap, the default since round 3)")
    ap.add_argument("--remove-soft-line-breaks", type=int, default=0,
                    help="template flag removeSoftLineBreaks (flag-variant measurement; the headline config keeps 0)")
    ap.add_argument("--prep-streams", type=int, default=1, help="streams the prepare launches alternate over")
    ap.add_argument("--ring", type=int, default=2, help="image buffers in flight (prepare runs this many sub-batches ahead)")
    ap.add_argument("--gather-wtns", type=int, default=0,
                    help="also gather this many full witnesses per rank and step on rank 0 over RCCL (N>1 only; "
                         "inside the timed region; default 0 = result table only, see DESIGN.md section 7)")
    ap.add_argument("--cpu-sample", type=int, default=-1,
                    help="emails timed for cpu_baseline (-1 = 8 per host thread, 0 = skip)")
    ap.add_argument("--pmc-traffic", type=int, default=1, help="collect roofline.traffic with rocprofv3 --pmc child passes (N=1)")
    ap.add_argument("--pmc-timeout", type=int, default=240)
    ap.add_argument("--other-configs", type=int, default=1, help="also measure configs[1], configs[4] and the delivered rate (N=1)")
    ap.add_argument("--montgomery", type=int, default=0,
                    help="1: witnesses written in Montgomery form by the fused expand (prover hand-off variant)")
    ap.add_argument("--out-align", type=int, default=0,
                    help="pad the distance between consecutive witnesses in the HBM ring to a multiple of this many bytes (0 = back to back)")
    ap.add_argument("--regex", default=None,
                    help="path of a zk-regex style body_hash_regex.circom: BodyHashRegex is compiled from it (zkwg_circuit_create_regex)")
    ap.add_argument("--no-overlap", type=int, default=0,
                    help="1: measurement aid -- every prepare waits for the previous sub-batch's expands, so zk_expand runs alone on the chip; "
                         "2: prepare(j) and expand(j - 1) take turns, side-stream work of the prepares (the removeSoftLineBreaks merge chain) beside both")
    ap.add_argument("--prep-cus", type=int, default=0,
                    help="> 0: the prepare kernels run on this many compute units only (CU-masked stream), zk_expand on the others")
    ap.add_argument("--prep-cu-stride", type=int, default=1, help="with --prep-cus: take every stride-th CU instead of the first ones")
    ap.add_argument("--place-ring", type=int, default=2,
                    help="2 (default): the output ring is mapped from 1 GiB physical chunks (zkwg_device_alloc_chunked); 1: round 4's way -- "
                         "spare candidate tiles from hipMalloc, zk_expand timed into each, the fastest kept; 0: two plain allocations")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--prove", type=int, default=0,
                    help="1: the workload is groth16.prove -- every rank proves --prove-batch emails per step (its shard of the job: inputs -> "
                         "witness -> A.w|B.w|C.w -> H evaluations -> five multi-exponentiations -> proof) and rank 0 gathers status + proof "
                         "(260 bytes per email) inside the timed region; the key is uploaded once per device")
    ap.add_argument("--prove-batch", type=int, default=48, help="with --prove: emails per GPU per step")
    ap.add_argument("--prove-slots", type=int, default=24, help="with --prove: proofs in flight per GPU")
    ap.add_argument("--launch-check", action="store_true",
                    help="only rendezvous (gloo, no GPU needed): every rank joins, rank 0 prints {\"launch_check\": world} -- the "
                         "CPU test of the self-launch below")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the side measurements (N=1): roofline.alone_frac and box_fill_GBps, the PMC "
                         "traffic passes (--pmc-traffic), other_configs (--other-configs) and cpu_baseline (--cpu-sample); "
                         "off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float64; see dump_witness_outputs)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher -- one rank per GPU under torch.distributed.run on this
        # node (free port, rendezvous on 127.0.0.1); the ranks re-enter main() with RANK / LOCAL_RANK / WORLD_SIZE set
        return self_launch(args.gpus)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size and --gpus must agree "
                         f"(plain `python bench.py --gpus N` launches the N ranks itself)")
    if args.launch_check:
        import torch.distributed as dist
        dist.init_process_group("gloo")
        import torch
        t = torch.tensor([rank + 1], dtype=torch.int64)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"launch_check": world, "rank_sum": int(t.item()), "local_rank_env": local_rank}), flush=True)
        dist.destroy_process_group()
        return 0

    import torch
    import zkwg

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback in the product path)")
    # test hooks (single-GPU smoke of the N>1 code path): ZKWG_BENCH_FORCE_DEVICE puts every rank on one
    # GPU, ZKWG_BENCH_BACKEND=gloo replaces RCCL (two ranks cannot share a GPU under RCCL)
    if os.environ.get("ZKWG_BENCH_FORCE_DEVICE") is not None:
        local_rank = int(os.environ["ZKWG_BENCH_FORCE_DEVICE"])
    backend = os.environ.get("ZKWG_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    if args.prove:
        return prove_main(args, torch, dist, backend, dev, rank, world, local_rank)

    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=args.max_header, max_body=args.max_body, device=local_rank,
                     remove_soft_line_breaks=args.remove_soft_line_breaks, regex=args.regex)
    tile = min(args.tile, args.batch)
    assert args.batch % tile == 0
    distinct = min(args.distinct, args.batch)
    assert tile % distinct == 0 or distinct % tile == 0
    if args.prep_batch <= 0:
        args.prep_batch = 2048 if args.regex else 1024
    prep = min(args.prep_batch, args.batch)

    # synthetic inputs: `distinct` different signed emails per rank (seeded by rank), replicated to
    # fill the batch; resident in HBM before timing starts.
    _, d_in, fields = resident_inputs(torch, c, dev, 0x5A4B + rank, distinct, args.batch, args.body_len)
    prio = int(os.environ.get("ZKWG_BENCH_EXP_PRIO", "-1"))
    pl = Pipeline(torch, c, dev, d_in, args.batch, tile, prep, ring=args.ring, prep_streams=args.prep_streams,
                  rsa_throttle=args.rsa_throttle, exp_prio=prio, montgomery=bool(args.montgomery), out_align=args.out_align,
                  serial=int(args.no_overlap), prep_cus=args.prep_cus, prep_cu_stride=args.prep_cu_stride, place=args.place_ring)
    from zkwg import shard
    state = {"table": None}

    def step():
        pl.step()
        with torch.cuda.stream(pl.s_exp):
            # the only exchange step: gather the 100-byte/email result table on rank 0 (RCCL over xGMI)
            table = shard.result_table(pl.d_status, pl.d_rows)
            if dist is not None and backend != "nccl":
                table = table.cpu()                     # gloo test hook: gather on the host
            state["table"] = shard.gather_table(dist, table, args.batch * world, rank, world) if dist is not None else table
            if dist is not None and args.gather_wtns > 0:
                k = min(args.gather_wtns, tile)
                src = pl.last_tile().view(tile, pl.stride)[:k, :c.witness_bytes].contiguous()
                if backend != "nccl":
                    src = src.cpu()
                shard.gather_witnesses(dist, src, rank, world, sink=(lambda r, off, t: None))

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if args.pmc_child:
        # counter-collection child: the same launches, nothing printed (the parent parses rocprofv3's CSV)
        for _ in range(max(1, args.steps)):
            step()
        torch.cuda.synchronize()
        return

    for _ in range(args.warmup):
        step()
    barrier()
    assert int(pl.d_status.abs().sum().item()) == 0, "synthetic emails must all verify"
    pl.j = 0
    c.set_timing(True)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    summ, ex_avg, ex_launches, achieved = expand_roofline(c, tile)
    c.set_timing(False)
    if args.dump_outputs and rank == 0:
        dump_witness_outputs(args.dump_outputs, torch, pl, state["table"], 0)
    alone = None
    if world == 1 and not args.no_overlap and args.full:
        # the same kernel with the chip to itself (every prepare waits for the previous sub-batch's expansions): what the
        # prepare kernels beside the stream cost it -- reported as roofline.alone_frac, outside the timed region
        pl.serial = True
        pl.step()
        torch.cuda.synchronize()
        c.set_timing(True)
        pl.step()
        torch.cuda.synchronize()
        _, a_avg, a_n, a_gbs = expand_roofline(c, tile)
        c.set_timing(False)
        pl.serial = False
        alone = (a_avg, a_gbs, a_n)

    if rank == 0:
        total_emails = args.batch * world * args.steps
        value = total_emails / dt
        bytes_per_email = 32 * c.W + c.in_stride
        kernels_ms = {k: round(v[0] / max(v[1], 1), 4) for k, v in summ.items()}
        res = {
            "metric": "EmailVerifier witnesses/sec", "value": round(value, 1), "unit": "witnesses/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u64 (BN254 Fr, 4x64-bit limbs) / u32 bit-vectors", "data": "synthetic",
            "config": {"workload": f"EmailVerifier({args.max_header},{args.max_body},121,17,0,0,0,{args.remove_soft_line_breaks}) batch={args.batch}/GPU, "
                                   f"{args.body_len} B bodies, witnesses device-resident" + (", Montgomery form" if args.montgomery else "")
                                   + (", BodyHashRegex compiled from " + os.path.basename(args.regex) if args.regex else ""),
                       "batch_per_gpu": args.batch, "tile": tile, "witness_len": c.W,
                       "witness_bytes": c.witness_bytes, "layout": "kept-v1", "parallelism": f"shard x{world}, result-table gather" + (f" + {args.gather_wtns} wtns/rank/step gathered" if args.gather_wtns and world > 1 else " only")},
            "roofline": {"bound": "hbm", "kernel": "zk_expand", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                         "traffic_source": "not collected",
                         "bytes_per_launch": bytes_per_email * tile, "avg_launch_ms": round(ex_avg, 4),
                         "launches_timed": ex_launches, "launches_total": args.steps * (args.batch // tile)},
            "kernel_ms_per_launch": kernels_ms,
            "ring_placement": pl.placement,
            "fr_field_ops_per_s": round(value * c.W, 1),
        }
        tb = state["table"]
        if tb is not None:
            # what rank 0 holds after the last step's gather: one row per email of the whole job
            tb = tb.cpu()
            st = tb[:, :4].contiguous().view(torch.int32).view(-1)
            res["gathered_table"] = {"rows": int(tb.shape[0]), "status_nonzero": int((st != 0).sum().item()),
                                     "rows_with_outputs": int((tb[:, 4:].to(torch.int32).sum(dim=1) != 0).sum().item())}
        if alone is not None:
            res["roofline"]["alone_frac"] = round(alone[1] / HBM_PEAK_GBS, 4)
            res["roofline"]["alone_launch_ms"] = round(alone[0], 4)
        single = world == 1
        if not args.full:
            res["roofline"]["traffic_source"] = "not collected (side measurements run with --full)"
        else:
            # same-box ceiling: a plain fill (torch.fill_, 16-byte stores) of the very buffer zk_expand just wrote,
            # so that box-to-box variance of the HBM write rate shows beside the fraction of the spec peak
            try:
                buf = pl.d_out[0].view(torch.int32)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                buf.fill_(1)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(10):
                    buf.fill_(1)
                e1.record()
                torch.cuda.synchronize()
                fill_gbs = buf.numel() * 4 * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9
                res["roofline"]["box_fill_GBps"] = round(fill_gbs, 1)
                res["roofline"]["frac_of_box_fill"] = round(achieved / fill_gbs, 4)
            except Exception as e:
                res["roofline"]["box_fill_GBps"] = None
                res["roofline"]["box_fill_error"] = repr(e)[:120]
            # free the main pipeline's HBM before the side measurements
            del pl.d_out, pl.d_scr
            torch.cuda.empty_cache()
            if single and args.pmc_traffic:
                t, src = pmc_traffic(args, tile, c.W)
                res["roofline"]["traffic"] = None if t is None else round(t)
                res["roofline"]["traffic_source"] = src
                if t is not None:
                    res["roofline"]["traffic_over_algorithmic"] = round(t / (bytes_per_email * tile), 4)
            elif not single:
                res["roofline"]["traffic_source"] = "not collected (PMC passes run at N=1 only)"
            if single and args.other_configs:
                res["other_configs"] = other_configs(torch, zkwg, dev, local_rank, c, args)
            if args.cpu_sample != 0 and single:
                res["cpu_baseline"] = cpu_baseline(c, args, fields, distinct)
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def self_launch(n):
    """Re-run this command line as `python -m torch.distributed.run --nnodes=1 --nproc-per-node n ... bench.py <same args>`
    and return its exit code (rank 0's JSON line goes to our stdout unchanged)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def other_configs(torch, zkwg, dev, local_rank, c, args):
    """BASELINE.json configs[1] and configs[4] and the delivered-to-host rate, device-resident unless
    said otherwise; short runs (the headline measurement above is the graded one)."""
    out = {}
    # configs[1]: same circuit, batch 256 (latency-bound prepare: 4 prepare streams, whole batch per launch)
    try:
        _, d_in, _ = resident_inputs(torch, c, dev, 0x5A4B + 101, 64, 256, args.body_len)
        pl = Pipeline(torch, c, dev, d_in, 256, 256, 256, ring=4, prep_streams=4, rsa_throttle=args.rsa_throttle)
        c.set_timing(True)
        dt = timed(torch, pl.step, steps=20, warmup=3)
        _, avg, n, gbs = expand_roofline(c, 256)
        c.set_timing(False)
        assert int(pl.d_status.abs().sum().item()) == 0
        out["configs[1] batch=256"] = {"value": round(256 * 20 / dt, 1), "unit": "witnesses/s", "steps": 20, "ring_placement": pl.placement,
                                       "zk_expand_GBps": round(gbs, 1), "zk_expand_frac": round(gbs / HBM_PEAK_GBS, 4)}
        del pl, d_in
        torch.cuda.empty_cache()
    except Exception as e:  # a side measurement must not lose the headline line
        out["configs[1] batch=256"] = {"error": repr(e)[:200]}
    # prover hand-off: the same pipeline with Montgomery-form output written by the fused expand
    try:
        _, d_in, _ = resident_inputs(torch, c, dev, 0x5A4B + 404, 64, 2048, args.body_len)
        pl = Pipeline(torch, c, dev, d_in, 2048, 512, 1024, ring=2, rsa_throttle=args.rsa_throttle, montgomery=True)
        c.set_timing(True)
        dt = timed(torch, pl.step, steps=6, warmup=1)
        _, avg, n, gbs = expand_roofline(c, 512)
        c.set_timing(False)
        assert int(pl.d_status.abs().sum().item()) == 0
        out["Montgomery-form output (fused hand-off)"] = {"value": round(2048 * 6 / dt, 1), "unit": "witnesses/s", "steps": 6, "ring_placement": pl.placement,
                                                           "zk_expand_GBps": round(gbs, 1), "zk_expand_frac": round(gbs / HBM_PEAK_GBS, 4)}
        del pl, d_in
        torch.cuda.empty_cache()
    except Exception as e:
        out["Montgomery-form output (fused hand-off)"] = {"error": repr(e)[:200]}
    # BodyHashRegex compiled from a template file instead of the built-in DFA circuit (zkwg_circuit_create_regex,
    # DESIGN.md section 18): the stand-in for zk-regex's generated body_hash_regex.circom shipped with the package
    try:
        tmpl = os.path.join(os.path.dirname(os.path.abspath(__file__)), "zk-email-verify_amd", "data", "templates",
                            "zk-regex-circom", "circuits", "common", "body_hash_regex.circom")
        if not args.regex and os.path.exists(tmpl):
            cr = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=args.max_header, max_body=args.max_body, device=local_rank, regex=tmpl)
            _, d_in, _ = resident_inputs(torch, cr, dev, 0x5A4B + 505, 64, 4096, args.body_len)
            pl = Pipeline(torch, cr, dev, d_in, 4096, 512, 2048, ring=2, rsa_throttle=args.rsa_throttle)
            cr.set_timing(True)
            dt = timed(torch, pl.step, steps=5, warmup=1)
            summ = cr.timing_summary()
            cr.set_timing(False)
            assert int(pl.d_status.abs().sum().item()) == 0
            out["BodyHashRegex compiled from the template file"] = {
                "value": round(4096 * 5 / dt, 1), "unit": "witnesses/s", "steps": 5,
                "zk_net_scan_eval_fill_ms_per_2048_emails": round(summ["zk_net_eval"][0] / max(summ["zk_net_eval"][1], 1), 3),
                "gate_list": cr.regex_info()}
            del pl, d_in, cr
            torch.cuda.empty_cache()
    except Exception as e:
        out["BodyHashRegex compiled from the template file"] = {"error": repr(e)[:200]}
    # the same with a template of the real circuit's size: every transition owns its comparators (~500 kept signals per header
    # byte, W = 2.05 M -- zk-regex's generated body_hash_regex.circom is cited at 617,597 constraints, email-verifier.circom:124)
    try:
        tmpl = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "regex_style", "body_hash_regex_unshared.circom")
        if not args.regex and os.path.exists(tmpl):
            cr = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=args.max_header, max_body=args.max_body, device=local_rank, regex=tmpl)
            _, d_in, _ = resident_inputs(torch, cr, dev, 0x5A4B + 606, 64, 4096, args.body_len)
            pl = Pipeline(torch, cr, dev, d_in, 4096, 512, 2048, ring=2, rsa_throttle=args.rsa_throttle)
            cr.set_timing(True)
            dt = timed(torch, pl.step, steps=5, warmup=1)
            summ = cr.timing_summary()
            _, avg, nl, gbs = expand_roofline(cr, 512)
            cr.set_timing(False)
            assert int(pl.d_status.abs().sum().item()) == 0
            out["BodyHashRegex from a template of the real circuit's size (unshared comparators)"] = {
                "value": round(4096 * 5 / dt, 1), "unit": "witnesses/s", "steps": 5, "witness_len": cr.W,
                "zk_net_scan_eval_fill_ms_per_2048_emails": round(summ["zk_net_eval"][0] / max(summ["zk_net_eval"][1], 1), 3),
                "zk_expand_GBps": round(gbs, 1), "zk_expand_frac": round(gbs / HBM_PEAK_GBS, 4), "gate_list": cr.regex_info()}
            del pl, d_in, cr
            torch.cuda.empty_cache()
    except Exception as e:
        out["BodyHashRegex from a template of the real circuit's size (unshared comparators)"] = {"error": repr(e)[:200]}
    # delivered to host (PCIe-inclusive): zkwg_calculate_batch with a pinned destination, double-buffered tiles
    try:
        n, t = 192, 64
        h_in, _, _ = resident_inputs(torch, c, dev, 0x5A4B + 202, 64, n, args.body_len)
        recs = bytes(h_in.repeat(3, 1)[:n].contiguous().numpy().tobytes())
        sec = c.time_host_path(recs, n, max_tile=t, pinned=True)
        out["delivered to pinned host memory"] = {"value": round(n / sec, 1), "unit": "witnesses/s",
                                                  "GBps": round(n * c.witness_bytes / sec / 1e9, 2),
                                                  "sample": f"{n} emails through zkwg_calculate_batch, tiles of {t}, PCIe-inclusive"}
    except Exception as e:
        out["delivered to pinned host memory"] = {"error": repr(e)[:200]}
    # the device-resident pipeline BELOW the C-ABI (zkwg_calculate_batch_resident: what a Node host without torch drives, and what
    # zkwg_calculate_batch_multi runs on every GPU when no witness is asked back): records from host memory, statuses + result
    # table back, witnesses into the handle's own placed two-tile ring
    try:
        n = args.batch
        h_in, _, _ = resident_inputs(torch, c, dev, 0x5A4B + 909, 64, n, args.body_len)
        recs = bytes(h_in.repeat((n + 63) // 64, 1)[:n].contiguous().numpy().tobytes())
        st, _ = c.calculate_batch_resident(recs, tile=min(args.tile, n), prep=args.prep_batch)     # (allocates and places the ring)
        assert not any(st)
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            st, tb = c.calculate_batch_resident(recs, tile=min(args.tile, n), prep=args.prep_batch)
        sec = (time.perf_counter() - t0) / reps
        out["C-ABI resident pipeline (zkwg_calculate_batch_resident)"] = {
            "value": round(n / sec, 1), "unit": "witnesses/s", "ring_placement": c.resident_placement(),
            "sample": f"{n} emails per call from host records (H2D of the records, statuses and the 100-byte table back included), {reps} calls"}
    except Exception as e:
        out["C-ABI resident pipeline (zkwg_calculate_batch_resident)"] = {"error": repr(e)[:200]}
    # (the ring and the scratch buffers of this entry point -- 2 x 29 GB + images -- live in the handle between calls: given back here, the
    # legs below need the memory.  A second handle for this leg instead cost the LATER legs 8-18 % on two boxes, profiles/r06/r06_x, r06_zz)
    try:
        c.release_resident()
    except Exception:
        pass
    # the same delivery with the expansion on the HOST (zkwg_set_host_expand): only the 0.45 MB image crosses PCIe, the
    # witness bytes are written by the host cores (non-temporal stores) -- bounded by host DRAM bandwidth instead
    try:
        cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        try:
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()
            if q != "max":
                cores = min(cores, max(1, int(q) // int(per)))
        except (OSError, ValueError):
            pass
        n, t = 192, 64
        h_in, _, _ = resident_inputs(torch, c, dev, 0x5A4B + 202, 64, n, args.body_len)
        recs = bytes(h_in.repeat(3, 1)[:n].contiguous().numpy().tobytes())
        c.set_host_expand(cores)
        sec = c.time_host_path(recs, n, max_tile=t, pinned=True)
        c.set_host_expand(0)
        out["delivered to host memory, expanded on the host"] = {
            "value": round(n / sec, 1), "unit": "witnesses/s", "GBps_written_by_host": round(n * c.witness_bytes / sec / 1e9, 2), "host_threads": cores,
            "sample": f"{n} emails through zkwg_calculate_batch with zkwg_set_host_expand({cores}), tiles of {t}: D2H of the 0.45 MB image per email"}
    except Exception as e:
        out["delivered to host memory, expanded on the host"] = {"error": repr(e)[:200]}
    # prover stage 1 from the compact image: A.w | B.w | C.w of every constraint of EmailVerifier(576,192)
    # written by zkwg_expand_abc_device -- no 32-byte witness in between
    try:
        ca = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=576, max_body=192, device=local_rank)
        t0 = time.time()
        cs = zkwg.WitnessCalculator(ca).constraint_system()
        t_cs = time.time() - t0
        ca.attach_r1cs(cs)
        ba, ta = 2048, 256
        _, d_in, _ = resident_inputs(torch, ca, dev, 0x5A4B + 808, 64, ba, 60)
        res = {}
        for mont in (False, True):
            pl = Pipeline(torch, ca, dev, d_in, ba, ta, 1024, ring=2, montgomery=mont, abc=True)
            dt = timed(torch, pl.step, steps=5, warmup=1)
            assert int(pl.d_status.abs().sum().item()) == 0
            res["montgomery" if mont else "standard"] = {"value": round(ba * 5 / dt, 1), "GBps_written": round(ba * 5 * ca.abc_bytes / dt / 1e9, 1)}
            del pl
            torch.cuda.empty_cache()
        out["prover stage 1 from the image, EmailVerifier(576,192)"] = {
            "unit": "witnesses/s (inputs -> A.w|B.w|C.w, witness generation included)", "constraints": cs.n_constraints, "abc_bytes": ca.abc_bytes,
            **res, "image_bytes_per_email": ca.scratch_bytes(1), "r1cs_export_s": round(t_cs, 1), "steps": 5}
        del d_in, ca, cs
        torch.cuda.empty_cache()
    except Exception as e:
        out["prover stage 1 from the image, EmailVerifier(576,192)"] = {"error": repr(e)[:300]}
    # prover stage 2 (SURVEY.md 8f4 "next"): the transforms groth16.prove runs on A.w | B.w | C.w -- 3 inverse + 3 forward
    # NTTs on the 2^20 domain and a b - c per email (zkwg_h_evaluations_device); ARITHMETIC-bound, so its roofline is the
    # issue rate of the 32 x 32 + 64 multiply-add a Montgomery product is made of, not HBM
    try:
        L, m, E = 20, 753807, 16
        plan = zkwg.Ntt(L, device=local_rank)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        d_abc = torch.randint(0, 1 << 62, (E, 12 * m), dtype=torch.int64, device=dev, generator=g)
        d_abc[:, 3::4] >>= 4
        d_work = torch.empty(plan.work_bytes(E), dtype=torch.uint8, device=dev)
        d_out = torch.empty(E * 32 * (1 << L), dtype=torch.uint8, device=dev)
        run = lambda: plan.h_evaluations_device(d_abc.view(torch.uint8), 96 * m, m, E, d_work, d_out)
        sec = timed(torch, run, steps=5, warmup=1) / 5
        n = 1 << L
        products = 6 * (n * L // 2 + ((L + 6) // 7 - 1) * n) + 3 * n + 2 * n      # butterflies + the passes' twiddle products + coset scaling + the join's two
        # measured on this chip (tools/mulbench.hip, profiles/r05/r05_g_mulbench.txt): v_mad_u64_u32 issues 34.4 T lane-ops/s (14 lanes per
        # cycle and SIMD): 128 per product bound 263 G products/s; the product the transform kernels RUN since round 6 -- 9 x 29-bit limbs,
        # values kept in limb form across the butterfly stages (csrc/zkwg_fr29.h) -- sustains 162.9 G/s in a pure product loop, the same
        # product behind the 4 x 64-bit interface (round 5's) 139 G/s, the 8 x 32-bit CIOS of rounds 2-4 95 G/s
        peak, product_rate = 263.0e9, 162.9e9
        out["prover stage 2: H evaluations (3 ifft + coset shift + 3 fft + a b - c), 2^20 domain"] = {
            "value": round(E / sec, 1), "unit": "emails/s", "montgomery_products_per_email": products,
            "products_per_s": round(E * products / sec), "issue_roofline_products_per_s": round(peak),
            "frac_of_issue_roofline": round(E * products / sec / peak, 4), "emails_per_call": E,
            "frac_of_measured_product_rate": round(E * products / sec / product_rate, 4), "measured_product_rate_per_s": round(product_rate),
            "product": "csrc/zkwg_fr29.h (9 x 29-bit product scanning, limb form across the stages of a pass)", "frac_of_139G": round(E * products / sec / 139.0e9, 4),
            "note": "issue_roofline = 128 v_mad_u64_u32 per product at the MEASURED issue rate (tools/mulbench.hip); measured_product_rate = what "
                    "the product the transform kernels use sustains in a pure product loop on this chip (VERDICT r5 weak #3: round 5 divided by the "
                    "CIOS's 95 G/s, a product the kernels no longer ran)"}
        del d_abc, d_work, d_out, plan
        torch.cuda.empty_cache()
    except Exception as e:
        out["prover stage 2: H evaluations"] = {"error": repr(e)[:200]}
    # the whole device-side prover (SURVEY.md 8f4 "next"): witness -> A.w | B.w | C.w -> H evaluations -> the five multi-exponentiations ->
    # pi_a, pi_b, pi_c, E emails per launch series on rolling contexts (round 6; csrc/zkwg_prover_api.hip) with the runtime's DEFAULT hardware
    # queues.  Every sum of one timed email is checked against its discrete logarithm (`sums_verified`: product code only -- Python integers and
    # one fixed-base multiple); proofs under a VALID key, judged by the pinned pairing verifier, are tests/test_prove.py (incl. this circuit)
    try:
        # (its own process: the tool owns ~20 GB of tables and work buffers; this process keeps its rings)
        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        torch.cuda.empty_cache()
        tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "bench_prove.py")
        for label, extra, tmo in (("EmailVerifier(576,192)", ["--emails", "8", "--slots", "24", "--proofs", "96"], 300),
                                  (f"EmailVerifier({args.max_header},{args.max_body}) -- the headline circuit",
                                   ["--max-header", str(args.max_header), "--max-body", str(args.max_body), "--emails", "8", "--slots", "24", "--proofs", "72"], 500)):
            p = subprocess.run([sys.executable, tool] + extra, env=env, capture_output=True, text=True, timeout=tmo)
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            out["prover stages 1-3: Groth16 proofs, " + label] = {
                "value": r["proofs_per_s"], "unit": "proofs/s", "proofs_in_flight": r["proofs_in_flight"], "contexts": r["contexts"],
                "emails_per_series": r["emails_per_series"], "proofs_timed": r["proofs_timed"], "hw_queues": r.get("hw_queues"),
                "one_at_a_time_ms_per_proof": r["one_at_a_time_ms_per_proof"],
                # one timed proof checked OUTSIDE the timed region: its five sums and pi_a, pi_b, pi_c against their discrete logarithms
                "verified": bool(r["sums_verified"] and r.get("proof_equals_its_discrete_logarithms") and r["batched_equals_one_at_a_time"]),
                "verified_how": "trapdoor key: A, B, C and every sum recomputed from the known exponents in Python integers; the pairing check itself "
                                "is the oracle's and runs in tests/test_prove.py at this circuit (bench.py may not call the oracle here)",
                "sums_verified": r["sums_verified"],
                "proof_equals_its_discrete_logarithms": r.get("proof_equals_its_discrete_logarithms"),
                "batched_equals_one_at_a_time": r["batched_equals_one_at_a_time"],
                "stages_ms_per_email_in_series": next(v for k, v in r.items() if k.startswith("stages_ms_per_email")), "stages_ms_one_email": r["stages_ms_one_email"],
                "products_per_s_over_139G_by_stage": r["products_per_s_over_139G_by_stage"], "whole_proof_products_per_s_over_139G": r["whole_proof_products_per_s_over_139G"],
                "W": r["W"], "domain_log2": r["domain_log2"], "note": r["key"]}
        torch.cuda.empty_cache()
    except Exception as e:
        out["prover stages 1-3: Groth16 proofs"] = {"error": repr(e)[:300]}
    # complete witnesses of the circuit compiled the way the reference documents (`circom --O0`,
    # docs/zk-email-docs/UsageGuide/README.md:59-64): every alias / constant / linear signal numbered, written in ONE pass
    # from the image (zkwg_circuit_create_full; artefacts = interpreter-generated .sym / .r1cs under artifacts/)
    try:
        import gzip
        art = os.path.join(os.path.dirname(os.path.abspath(__file__)), "artifacts")
        tag = next((t for t in ((args.max_header, args.max_body), (576, 192)) if os.path.exists(os.path.join(art, f"o0_ev_{t[0]}_{t[1]}.json"))), None)
        if tag is not None:
            base = os.path.join(art, f"o0_ev_{tag[0]}_{tag[1]}")
            meta = json.load(open(base + ".json"))
            # (the artefacts are stored gzipped to fit the snapshot; a deployment reads the compiler's files as they are, so the
            # decompression is timed apart from the handle's creation)
            t0 = time.time()
            sym_bytes, r1cs_bytes = gzip.open(base + ".sym.gz", "rb").read(), gzip.open(base + ".r1cs.gz", "rb").read()
            t_gunzip = time.time() - t0
            t0 = time.time()
            co = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=tag[0], max_body=tag[1], device=local_rank,
                              sym=sym_bytes, sym_alias=meta["alias"], r1cs=r1cs_bytes)
            t_create = time.time() - t0
            del sym_bytes, r1cs_bytes
            bo, to = (512, 128) if tag[0] > 576 else (2048, 256)
            _, d_in, _ = resident_inputs(torch, co, dev, 0x5A4B + 707, 64, bo, args.body_len if tag[1] >= args.body_len + 64 else 60)
            pl = Pipeline(torch, co, dev, d_in, bo, to, min(1024, bo), ring=2, rsa_throttle=args.rsa_throttle)
            co.set_timing(True)
            dt = timed(torch, pl.step, steps=5, warmup=1)
            _, avg, nl, gbs = expand_roofline(co, to)
            co.set_timing(False)
            assert int(pl.d_status.abs().sum().item()) == 0
            kept_W = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=tag[0], max_body=tag[1], device=-1).W
            out[f"complete --O0 witnesses, EmailVerifier({tag[0]},{tag[1]})"] = {
                "value": round(bo * 5 / dt, 1), "unit": "witnesses/s", "steps": 5, "witness_len": co.W, "witness_bytes": co.witness_bytes,
                "raw_GBps_whole_job": round(bo * 5 * co.witness_bytes / dt / 1e9, 1), "raw_frac": round(bo * 5 * co.witness_bytes / dt / 1e9 / HBM_PEAK_GBS, 4),
                "zk_expand_raw_GBps": round(gbs, 1),
                "frac_on_W_alg": round(bo * 5 * (32 * kept_W) / dt / 1e9 / HBM_PEAK_GBS, 4), "W_alg": kept_W,
                "handle_create_s": round(t_create, 1), "artefact_gunzip_s": round(t_gunzip, 1),
                "note": "one pass: row kernels + zk_expand3_o0 (per-wire descriptors); raw = the bytes actually written; frac_on_W_alg grades the same time on the kept-v1 (information-carrying) signals only (SURVEY.md 8d3)"}
            del pl, d_in, co
            torch.cuda.empty_cache()
    except Exception as e:
        out["complete --O0 witnesses"] = {"error": repr(e)[:300]}
    # the flag variant removeSoftLineBreaks = 1 (packages/circuits/helpers/remove-soft-line-breaks.circom:14-126): the one
    # Fr-heavy block of the witness path (PoseidonModular over 2 maxBody bytes), whole batches prepared four deep
    # Twice: as shipped, and with every 16-byte chunk hashed (ZKWG_RSLB_CONST_CHUNKS=0: no constant for the all-zero chunks of the padding).
    # Each in a process of its own -- this very script with --remove-soft-line-breaks 1: six prepared batches of 22 GB, and streams that
    # do not share hardware queues with the dozen streams this process has created by now (in-process the same pipeline measured 50.4 k
    # against 54.3 k stand-alone on one box, profiles/r06/r06_zz_*)
    rs = {}
    torch.cuda.empty_cache()
    for flag in ("1", "0"):
        try:
            env = dict(os.environ, ZKWG_RSLB_CONST_CHUNKS=flag)
            cmd = [sys.executable, os.path.abspath(__file__), "--remove-soft-line-breaks", "1", "--batch", "4096", "--tile", "256", "--prep-batch", "4096",
                   "--ring", "6", "--steps", "12", "--warmup", "2", "--cpu-sample", "0", "--pmc-traffic", "0", "--other-configs", "0",
                   "--max-header", str(args.max_header), "--max-body", str(args.max_body), "--body-len", str(args.body_len)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            rs[flag] = {"value": r["value"], "zk_expand_GBps": r["roofline"]["achieved"], "witness_len": r["config"].get("witness_len"),
                        "kernel_ms_per_launch": {k: v for k, v in r["kernel_ms_per_launch"].items() if k.startswith("zk_rslb") or k == "zk_expand"}}
        except Exception as e:
            rs[flag] = {"error": repr(e)[:300]}
    if "value" in rs.get("1", {}):
        out["removeSoftLineBreaks = 1"] = {
            "value": rs["1"]["value"], "unit": "witnesses/s", "steps": 12, "witness_len": rs["1"]["witness_len"], "zk_expand_GBps": rs["1"]["zk_expand_GBps"],
            "zk_expand_frac": round(rs["1"]["zk_expand_GBps"] / HBM_PEAK_GBS, 4), "kernel_ms_per_launch": rs["1"]["kernel_ms_per_launch"],
            "value_with_every_chunk_hashed": rs["0"].get("value", rs["0"].get("error")),
            "kernel_ms_per_launch_with_every_chunk_hashed": rs["0"].get("kernel_ms_per_launch"),
            "note": "target of four rounds: 50 k/s.  Round 6: the Poseidon(2) merge chain one lane per email in limb form (2.5 x fewer instructions beside the "
                    "throughput kernels) and CONSTANT CHUNKS: both halves of the hashed string are zero-padded to maxBody, Poseidon(16) of sixteen zero bytes is "
                    "a constant of the circuit, and the units holding it get the precomputed signals instead of a lane of zk_rslb_chunks (a third of the units "
                    f"for {args.body_len}-byte bodies at maxBody {args.max_body}; same witnesses, tests/test_soft_line_breaks.py) -- value_with_every_chunk_hashed "
                    "is the same pipeline without that (ZKWG_RSLB_CONST_CHUNKS=0)"}
    else:
        out["removeSoftLineBreaks = 1"] = rs.get("1", {"error": "not run"})
    # configs[4]: maxBody = 65536 (SHA-dominated), batch 1024, bodies 32K..65K-72; fewer steps
    try:
        c5 = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=1024, max_body=65536, device=local_rank)
        tile5 = 32
        d_in = resident_inputs_ragged(torch, c5, dev, 0x5A4B + 303, 16, 1024, 32768, 65536 - 72)
        pl = Pipeline(torch, c5, dev, d_in, 1024, tile5, 128, ring=2, prep_streams=1, rsa_throttle=args.rsa_throttle)
        c5.set_timing(True)
        dt = timed(torch, pl.step, steps=5, warmup=1)
        _, avg, nl, gbs = expand_roofline(c5, tile5)
        c5.set_timing(False)
        assert int(pl.d_status.abs().sum().item()) == 0
        out["configs[4] maxBody=65536 batch=1024"] = {
            "value": round(1024 * 5 / dt, 1), "unit": "witnesses/s", "steps": 5, "ring_placement": pl.placement, "witness_len": c5.W,
            "zk_expand_GBps": round(gbs, 1), "zk_expand_frac": round(gbs / HBM_PEAK_GBS, 4),
            "body_len": "16 distinct emails, body lengths spread over 32768 .. 65464 (parity of this configuration at batch 1,024 with every row checked: tests/test_configs_gpu.py)"}
        del pl, d_in, c5
        torch.cuda.empty_cache()
    except Exception as e:
        out["configs[4] maxBody=65536 batch=1024"] = {"error": repr(e)[:200]}
    return out


def cpu_baseline(c, args, fields, distinct):
    """The C oracle (kind "port") on this box's host cores: -O3 -march=native build made here, per-thread
    witness buffers pre-touched outside the timed region, >= 8 emails per thread, plus a single-thread
    figure.  Every witness is fully written to host memory, like the GPU path writes HBM."""
    from oracle import coracle
    lib, build = coracle.load_native()
    logical = os.cpu_count() or 1
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else logical
    quota = None
    try:   # cgroup v2 CPU quota: "<quota> <period>" or "max <period>"
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = max(1, int(q) // int(per))
    except (OSError, ValueError):
        pass
    if quota is not None:
        cores = min(cores, quota)   # more runnable threads than the quota only get throttled
    n = args.cpu_sample if args.cpu_sample > 0 else 8 * cores
    reps = (n + distinct - 1) // distinct

    def take(k):
        sub = {}
        for key, v in fields.items():
            if isinstance(v, list):
                sub[key] = (v * reps)[:k]
            else:
                per = len(v) // distinct
                sub[key] = (bytes(v) * reps)[:k * per]
        return sub
    buf = (ctypes.c_uint8 * (cores * 32 * c.W))()
    W, st, sec = coracle.run_fields(args.max_header, args.max_body, 0, take(n), n, threads=cores, out=buf,
                                    per_thread_out=True, lib=lib, pretouch=True)
    assert W == c.W and st == [0] * n
    n1 = 12
    W, st1, sec1 = coracle.run_fields(args.max_header, args.max_body, 0, take(n1), n1, threads=1, out=buf,
                                      per_thread_out=True, lib=lib, pretouch=True)
    assert st1 == [0] * n1
    return {"value": round(n / sec, 2), "unit": "witnesses/s", "cores": cores, "kind": "port",
            "single_thread": round(n1 / sec1, 2), "build": build,
            "host": f"{logical} logical CPUs, cgroup CPU quota {quota if quota is not None else 'none'}; threads used = cores",
            "sample": f"{n} emails ({n // cores} per thread) of the same synthetic workload, C oracle (oracle/c), OpenMP over "
                      f"emails, per-thread witness buffers pre-touched, every witness fully written to host memory; "
                      f"single_thread = {n1} emails on one core"}


if __name__ == "__main__":
    sys.exit(main() or 0)
