"""Compile-time properties of zk_zkey_abc (csrc/zkwg_kernels_zkey.hip), checked with the cross-compiler, no GPU: no scratch memory and
no LDS in any variant -- a lane keeps the signed word columns of its G witnesses (8 x 64 bits each), the 17 product columns and the
gathered values in registers; an array indexed by a loop that is not unrolled would put them in scratch."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_zkey_row_kernels_use_no_scratch_memory():
    """as compiled for gfx950 (ROCm 7): zk_zkey_abc_short<2> / _long<2> (the default): 130 / 132 VGPRs, 3 wavefronts per SIMD; <4>
    (ZKWG_ZKEY_G=4): 242 VGPRs, 2 wavefronts per SIMD; zk_zkey_range 10 VGPRs, zk_zkey_scrub 8, both 8 wavefronts per SIMD."""
    info = kernel_resources.usage("zkwg_kernels_zkey.hip")
    ks = {n: v for n, v in info.items() if "zk_zkey_" in n}
    abc = {n: v for n, v in ks.items() if "zk_zkey_abc" in n}
    assert len(abc) == 4 and len(ks) == 6, sorted(info)          # short / long x G = 2, 4; range, scrub
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0 and v["LDS Size"] == 0, (n, v)
    for n, v in abc.items():
        assert v["Occupancy"] >= (3 if "ILi2E" in n else 2), (n, v)
