"""Compile-time properties of the kernels of the substring mains (csrc/zkwg_kernels_substr.hip), checked with the cross-compiler, no
GPU: NO SCRATCH MEMORY in zk_substr and in zk_expand3_subm -- the instantiation of zk_expand that carries the match matrix decoder so
that the headline kernel's switch does not (tests/test_kernel_resources.py holds that one at 64 VGPRs / occupancy 8, unchanged)."""
import kernel_resources

KERNELS = ("zk_substr", "zk_expand3_subm")
# as compiled when the kernels were written: (VGPRs, occupancy)
RECORDED = {"zk_substr": (67, 7), "zk_expand3_subm": (42, 8)}


@kernel_resources.needs_hipcc
def test_no_scratch_memory_in_the_substring_kernels():
    info = kernel_resources.usage("zkwg_kernels_substr.hip")
    for k in KERNELS:
        assert len([n for n in info if k in n]) == 1, (k, sorted(info))
    assert len(info) == len(KERNELS), sorted(info)                # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        k = next(k for k in KERNELS if k in n)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= RECORDED[k][0] and v["Occupancy"] >= RECORDED[k][1], (n, v)
    assert [v for n, v in info.items() if "zk_substr" in n][0].get("LDS Size") == 0   # in[] and the substring: dynamic LDS, sized per circuit
