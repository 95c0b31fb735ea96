"""Compile-time properties of the kernels of `powersoftau verify` (csrc/zkwg_kernels_verify.hip), checked with the cross-compiler, no GPU:
NO SCRATCH MEMORY in any kernel -- the repository's standing rule for point kernels (tests/test_kernel_resources.py) -- and 2 wavefronts
per SIMD for the subgroup test, the floor the other G2 walks are held to (the walk is a chain of dependent field products; one wavefront
leaves its latency exposed)."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_verify_kernels_use_no_scratch_memory_and_the_subgroup_test_keeps_two_wavefronts():
    info = kernel_resources.usage("zkwg_kernels_verify.hip")
    subgroup = [n for n in info if "zk_verify_g2_subgroup" in n]
    widen = [n for n in info if "zk_verify_widen" in n]
    assert len(subgroup) == 1 and len(widen) == 1 and len(info) == 2, sorted(info)      # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("LDS Size") == 0, (n, v)
    assert info[subgroup[0]].get("Occupancy") >= 2, info[subgroup[0]]
