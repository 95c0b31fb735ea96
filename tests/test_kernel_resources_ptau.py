"""Compile-time properties of the kernels of the transform over points (csrc/zkwg_kernels_ptau.hip), checked with the cross-compiler, no
GPU: NO SCRATCH MEMORY in any instantiation -- the repository's standing rule for point kernels (tests/test_kernel_resources.py) -- and
an occupancy of at least zk_phase2_scale's for the same group: 3 wavefronts per SIMD for G1, 2 for G2 (the walk is a chain of dependent
field products; fewer wavefronts leave its latency exposed)."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_ptau_kernels_use_no_scratch_memory_and_keep_the_occupancy_of_phase2():
    info = kernel_resources.usage("zkwg_kernels_ptau.hip")
    stages = {n: v for n, v in info.items() if "zk_ptau_stage" in n}
    assert len(stages) == 4, sorted(info)                      # G1 / G2 x shared twiddle / twiddle per lane
    assert sum(1 for n in stages if "ZkEcG1" in n) == 2 and sum(1 for n in stages if "ZkEcG2" in n) == 2, sorted(stages)
    others = {n: v for n, v in info.items() if "zk_ptau_permute" in n}
    assert len(others) == 1 and len(info) == 5, sorted(info)   # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("LDS Size") == 0, (n, v)
        assert v.get("Occupancy") >= (2 if "ZkEcG2" in n else 3), (n, v)
