"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as float64 .npy files.
CPU: which ring tile holds the last expansion, and the exact word conversion.  GPU: a small run's dump equals the
host path's witnesses for the same seeded emails (statuses, result table, sampled elements, per-witness word sums)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)


def test_last_expanded_tile_and_word_conversion():
    import bench
    ring = ["t0", "t1"]
    # batch 4096, prepare sub-batches of 1024, tiles of 512: the step's last tile is tile 7, ring slot 1, emails 3584..
    pl = types.SimpleNamespace(nsub=4, tiles_per_sub=2, prep=1024, tile=512, d_out=ring, serial=0)
    assert bench.last_expanded(pl) == ("t1", 3584)
    pl.serial = 1
    assert bench.last_expanded(pl) == ("t1", 3584)
    # --no-overlap 2: the expansion lags one sub-batch, so the step ends with sub-batch 2's last tile (tile 5)
    pl.serial = 2
    assert bench.last_expanded(pl) == ("t1", 2560)
    pl.nsub, pl.tiles_per_sub, pl.prep = 1, 1, 512
    assert bench.last_expanded(pl) == ("t0", 0)
    a = np.array([[0xFF, 0xFF, 0xFF, 0xFF, 1, 0, 0, 0x80]], dtype=np.uint8)
    w = bench.words_f64(a)
    assert w.dtype == np.float64 and w.tolist() == [[4294967295.0, 2147483649.0]]


def test_bench_help_names_the_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_bench_dump_equals_the_host_path(tmp_path):
    import zkwg
    from zkwg import synth
    N, M, body, distinct, batch, tile = 576, 192, 100, 8, 256, 128
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--max-header", str(N),
           "--max-body", str(M), "--body-len", str(body), "--distinct", str(distinct), "--batch", str(batch), "--tile", str(tile),
           "--prep-batch", str(batch), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and "other_configs" not in res and "cpu_baseline" not in res
    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(d) == {"status", "result_table", "witness_sample", "witness_sample_emails", "witness_sample_elements", "witness_word_sums"}
    assert all(a.dtype == np.float64 for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20

    c = zkwg.Circuit(zkwg.MAIN_EMAIL_VERIFIER, max_header=N, max_body=M, device=0)
    recs, _ = synth.packed_batch(c, seed=0x5A4B, n=distinct, body_len=body)      # bench.py's inputs of rank 0
    wit, status = c.calculate_batch_host(recs)
    assert status == [0] * distinct
    words = np.frombuffer(wit, dtype="<u4").reshape(distinct, c.W, 8).astype(np.float64)
    email = np.arange(batch) % distinct
    assert d["status"].tolist() == [0.0] * batch
    assert np.array_equal(d["result_table"][:, 1:], words[email, 1:4].reshape(batch, 24))
    em, el = d["witness_sample_emails"].astype(np.int64), d["witness_sample_elements"].astype(np.int64)
    assert len(em) == 8 and np.all((em >= batch - tile) & (em < batch)) and len(el) == min(65536, c.W)
    assert np.array_equal(d["witness_sample"], words[em % distinct][:, el])
    u = np.frombuffer(wit, dtype="<u4").reshape(distinct, -1).astype(np.int64)
    sums = np.stack([(u & 0xFFFF).sum(axis=1), (u >> 16).sum(axis=1)], axis=1).astype(np.float64)
    assert np.array_equal(d["witness_word_sums"], sums[np.arange(batch - tile, batch) % distinct])
