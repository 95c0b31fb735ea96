"""Compile-time properties of the two input-generation kernels (csrc/zkwg_kernels_inputs.hip: zk_gen_inputs and its needle instantiation
zk_gen_reveal_inputs), checked with the cross-compiler, no GPU: NO SCRATCH MEMORY -- the repository's standing rule
(tests/test_kernel_resources.py) -- and the needle variant's LDS is lane 0's SHA block and adjusted selector plus the window and the
needle chunk of the search (csrc/zkwg_locate_core.h), nothing that grows with the needle."""
import kernel_resources

KERNELS = ("zk_gen_inputs", "zk_gen_reveal_inputs")


@kernel_resources.needs_hipcc
def test_no_scratch_memory_in_the_needle_instantiation_and_a_fixed_lds():
    info = kernel_resources.usage("zkwg_kernels_inputs.hip")
    by = {k: [v for n, v in info.items() if n.startswith(f"_Z{len(k)}{k}")] for k in KERNELS}
    assert all(len(v) == 1 for v in by.values()) and len(info) == len(KERNELS), sorted(info)
    for k, (v,) in by.items():
        print(k, v)
        assert v.get("ScratchSize") == 0, (k, v)
        assert v.get("Occupancy") >= 4, (k, v)
    stage = 64 + 160                                              # ZK_GEN_LDS
    search = 1024 + 256 + 256                                     # ZK_LOC_LDS: the tile, the bytes behind it, the needle chunk
    assert by["zk_gen_inputs"][0].get("LDS Size") == stage + 8, by["zk_gen_inputs"][0]            # + the error and the cut
    assert by["zk_gen_reveal_inputs"][0].get("LDS Size") == stage + search + 8, by["zk_gen_reveal_inputs"][0]
