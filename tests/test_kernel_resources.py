"""Compile-time properties of the streaming kernels that the roofline depends on (checked with the cross-compiler, no GPU):
no scratch memory in any kernel of zkwg_kernels_expand3.hip -- a struct passed by reference to an out-of-line function once
cost the Montgomery kernels 1.39 x their algorithmic HBM writes -- and the register budgets that give
zk_expand3 8 wavefronts per SIMD and hold the other three streaming kernels at the occupancy they were measured with."""
import re

import kernel_resources

_SOURCES = ("zkwg_kernels_rslb.hip", "zkwg_kernels_expand3.hip", "zkwg_kernels_msm.hip", "zkwg_kernels_ntt.hip")


def _source_name(mangled):
    """_Z10zk_expand34ZkX3 -> zk_expand3"""
    m = re.match(r"_Z(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled


def _resource_usage(src):
    kernel_resources.start(*_SOURCES)       # the four cross-compilations of this module run side by side
    return kernel_resources.usage(src)


@kernel_resources.needs_hipcc
def test_soft_line_break_chunk_hashes_use_no_scratch_memory():
    # zk_rslb_chunks (one Poseidon(16) per lane, 786 k per batch): the dense mixes hold the old state in registers (153 VGPRs) and
    # fetch their 153 table limbs 9 at a time; if the compiler hoists those scalar loads, or does not unroll the 17
    # multiply-accumulates of an output, the state lands in scratch (624 B .. 6 KB per lane were seen on the way)
    info = _resource_usage("zkwg_kernels_rslb.hip")
    ks = [v for name, v in info.items() if "zk_rslb_chunks" in name]
    assert len(ks) == 1, sorted(info)               # one kernel: the evaluator's variant 6 (dense mixes through the staging area)
    chunks = ks[0]
    assert chunks.get("ScratchSize") == 0, chunks
    assert chunks["LDS Size"] <= 40 * 1024, chunks  # 4 wavefronts per CU
    # it leaves zk_expand six wavefronts per SIMD beside it
    assert chunks["VGPRs"] + chunks.get("AGPRs", 0) <= 128, chunks
    assert next(v for name, v in info.items() if "zk_rslb_scan" in name).get("ScratchSize") == 0
    # round 6: the merge chain one lane per email through the same evaluator (t = 3), the constant-chunk passes
    for frag in ("zk_rslb_merge1", "zk_rslb_classify", "zk_rslb_fill_const"):
        assert next(v for name, v in info.items() if frag in name).get("ScratchSize") == 0, frag


@kernel_resources.needs_hipcc
def test_streaming_kernels_use_no_scratch_memory_and_keep_their_occupancy():
    info = _resource_usage("zkwg_kernels_expand3.hip")
    kernels = {_source_name(k): v for k, v in info.items() if "zk_" in k}
    assert sorted(kernels) == sorted(("zk_expand3", "zk_expand3_mont", "zk_expand3_o0", "zk_expand3_o0_mont", "zk_image_to_mont", "zk_o0_generic",
                                      "zk_o0_rows_small", "zk_o0_rows_small_long", "zk_o0_chains_small", "zk_o0_rows_fr")), sorted(info)
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)
    # the headline kernel: <= 64 VGPRs = 8 wavefronts per SIMD
    assert kernels["zk_expand3"]["VGPRs"] <= 64 and kernels["zk_expand3"]["Occupancy"] == 8, kernels["zk_expand3"]
    # its Montgomery twin and the descriptor-driven pair (one slot per lane, emails in batches of 4): (VGPRs, occupancy) as compiled
    # before the variants they were chosen from were deleted (then zk_expand3_mont_k4, zk_expand3_o0b_k1, zk_expand3_o0b_mont_k1)
    for name, vgprs, occ in (("zk_expand3_mont", 66, 7), ("zk_expand3_o0", 74, 6), ("zk_expand3_o0_mont", 99, 4)):
        v = kernels[name]
        assert v["VGPRs"] + v.get("AGPRs", 0) <= vgprs and v["Occupancy"] >= occ, (name, v)
    assert kernels["zk_o0_rows_fr"]["Occupancy"] >= 4, kernels["zk_o0_rows_fr"]


@kernel_resources.needs_hipcc
def test_multi_exponentiation_kernels_use_no_scratch_memory():
    """every zk_msm_* kernel of the prover, G1 and G2 (the round-5 G2 kernels -- one lane per point, Fq2 products as
    function calls -- sat at 256 VGPRs + 1,168 bytes of scratch, occupancy 1).  Since round 6 G2 runs on lane pairs in lazy limb form:
    no scratch anywhere, the kernels of the mixed additions (level-0 slices, the ones' sums) at 4 wavefronts per SIMD for G1 and 3 for G2
    (no software prefetch of the next base: same or better measured rate, profiles/r06/r06_l, r06_s).  zk_msm_table (once per key: K shifted copies of the bases, canonical-word arithmetic with
    one inversion per copy) is exempt."""
    info = _resource_usage("zkwg_kernels_msm.hip")
    ks = {n: v for n, v in info.items() if "zk_msm_" in n and "zk_msm_table" not in n}
    assert len(ks) >= 30, sorted(info)
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0, (n, v)
    hot1 = [v for n, v in ks.items() if "ZkEcG1" in n and ("slice_sumI6ZkEcG1Lb1" in n or "zk_msm_onesI" in n)]
    hot2 = [v for n, v in ks.items() if "ZkEcG2" in n and ("slice_sumI6ZkEcG2Lb1" in n or "zk_msm_onesI" in n)]
    assert len(hot1) == 2 and len(hot2) == 2
    assert all(v["Occupancy"] >= 4 for v in hot1), hot1
    assert all(v["Occupancy"] >= 3 for v in hot2), hot2
    assert all(v["Occupancy"] >= 2 for n, v in ks.items()), ks


@kernel_resources.needs_hipcc
def test_transform_kernels_use_no_scratch_memory_and_keep_their_registers():
    """every zk_ntt_* kernel of the prover's transforms: no scratch, and no more VGPRs / no less occupancy than the kernels had before
    their bodies moved into zkwg_ntt_core.h (shared with the host mirror of the CPU tests).  The products keep a 9-limb value and its
    18 partial products in registers; a spill would put them in scratch."""
    info = _resource_usage("zkwg_kernels_ntt.hip")
    ks = {n: v for n, v in info.items() if "zk_ntt_" in n}
    assert len(ks) == 6, sorted(info)
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0, (n, v)
    # (name fragment, VGPRs, occupancy) as compiled before the refactor
    for frag, vgprs, occ in (("zk_ntt_colILb0E", 120, 4), ("zk_ntt_colILb1E", 126, 4), ("zk_ntt_rowILb0E", 120, 4), ("zk_ntt_rowILb1E", 119, 4),
                             ("zk_ntt_join", 53, 8), ("zk_ntt_bitrev", 23, 8)):
        v = next(v for n, v in ks.items() if frag in n)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= vgprs and v["Occupancy"] >= occ, (frag, v)
