"""Compile-time properties of the kernels of batched groth16 verification (csrc/zkwg_kernels_pair.hip), checked with the cross-compiler, no
GPU: NO SCRATCH MEMORY in either kernel -- the repository's standing rule for point kernels (tests/test_kernel_resources.py) -- no LDS
(the Fq12 temporaries stay in registers), and the occupancy zk_pair_miller compiles to as a floor: 1 wavefront per SIMD (256 vector
registers and the accumulation registers beside them; held to 2 wavefronts the compiler spills 820 bytes per lane to scratch memory).
Below 1 the kernel would not launch."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_pair_kernels_use_no_scratch_memory_and_the_miller_loop_keeps_its_occupancy():
    info = kernel_resources.usage("zkwg_kernels_pair.hip")
    miller = [n for n in info if "zk_pair_miller" in n]
    product = [n for n in info if "zk_pair_product" in n]
    assert len(miller) == 1 and len(product) == 1 and len(info) == 2, sorted(info)      # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("LDS Size") == 0, (n, v)
        assert v.get("Occupancy") >= 1, (n, v)
    assert info[miller[0]].get("Occupancy") >= 1, info[miller[0]]
