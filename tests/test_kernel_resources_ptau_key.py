"""Compile-time properties of the kernels of "each point times its own scalar" (csrc/zkwg_kernels_ptau_key.hip), checked with the
cross-compiler, no GPU: NO SCRATCH MEMORY in any instantiation -- the repository's standing rule for point kernels
(tests/test_kernel_resources.py) -- and the occupancy of the walk kernels: 3 wavefronts per SIMD for G1, 2 for G2 (the walk is a chain of
dependent field products; fewer wavefronts leave its latency, and here the reads of the table's rows, exposed)."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_ptau_key_kernels_use_no_scratch_memory_and_keep_the_occupancy_of_the_walks():
    info = kernel_resources.usage("zkwg_kernels_ptau_key.hip")
    walks = {n: v for n, v in info.items() if "zk_ptau_key_walk" in n}
    tables = {n: v for n, v in info.items() if "zk_ptau_key_table" in n}
    assert len(walks) == 4 and len(tables) == 2 and len(info) == 6, sorted(info)      # G1 / G2 x scalars read / computed; every kernel of the file is looked at
    for group in ("ZkEcG1", "ZkEcG2"):
        assert sum(1 for n in walks if group in n) == 2 and sum(1 for n in tables if group in n) == 1, sorted(info)
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("LDS Size") == 0, (n, v)
        assert v.get("Occupancy") >= (2 if "ZkEcG2" in n else 3), (n, v)
