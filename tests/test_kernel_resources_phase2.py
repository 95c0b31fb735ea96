"""Compile-time properties of the phase-2 kernel (csrc/zkwg_kernels_phase2.hip), checked with the cross-compiler, no GPU: NO SCRATCH
MEMORY in either instantiation -- the repository's standing rule for point kernels (tests/test_kernel_resources.py).  The digit strings
are kernel arguments whose words are selected, not indexed: an indexed argument array is what would land in scratch."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_phase2_kernels_use_no_scratch_memory():
    """as compiled for gfx950 (ROCm 7), VGPRs / wavefronts per SIMD: zk_phase2_scale<G1> 154 / 3, zk_phase2_scale<G2> 180 / 2.
    Recorded, not asserted: nobody has measured what this kernel needs."""
    info = kernel_resources.usage("zkwg_kernels_phase2.hip")
    ks = {n: v for n, v in info.items() if "zk_phase2_scale" in n}
    assert len(ks) == 2, sorted(info)
    assert sum(1 for n in ks if "ZkEcG1" in n) == 1 and sum(1 for n in ks if "ZkEcG2" in n) == 1, sorted(ks)
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0, (n, v)
        print(n, v)
