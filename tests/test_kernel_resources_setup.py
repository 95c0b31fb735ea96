"""Compile-time properties of the set-up kernels (csrc/zkwg_kernels_setup.hip), checked with the cross-compiler, no GPU: NO SCRATCH MEMORY
in any of them -- the repository's standing rule for point kernels (tests/test_kernel_resources.py): G2 runs on lane pairs, the exponent
of the inversion and the table pointers are selected, not indexed, and the batched inversion keeps its prefix products in device memory,
not in a lane's private array."""
import kernel_resources


@kernel_resources.needs_hipcc
def test_setup_kernels_use_no_scratch_memory():
    """as compiled for gfx950 (ROCm 7), VGPRs / wavefronts per SIMD, <G1> | <G2>: zk_setup_short 211 / 2 | 225 / 2, zk_setup_chunk
    209 / 2 | 224 / 2 (9,216 bytes of LDS: the wavefront's reduction), zk_setup_join_wave 154 / 3 | 167 / 3 (9,216 bytes of LDS),
    zk_setup_den_k 20 / 8 | 40 / 8, zk_setup_affine_k 63 / 8 | 107 / 4, zk_setup_prepare 73 / 6 | 92 / 5; zk_setup_inv_k 61 / 8,
    zk_setup_odd_copy 8 / 8.  Recorded, not asserted: nobody has measured what these kernels need."""
    info = kernel_resources.usage("zkwg_kernels_setup.hip")
    ks = {n: v for n, v in info.items() if "zk_setup_" in n}
    for stem, variants in (("zk_setup_short", 2), ("zk_setup_chunk", 2), ("zk_setup_join_wave", 2), ("zk_setup_den_k", 2), ("zk_setup_affine_k", 2),
                           ("zk_setup_prepare", 2), ("zk_setup_inv_k", 1), ("zk_setup_odd_copy", 1)):
        assert sum(1 for n in ks if stem in n) == variants, (stem, sorted(ks))
    assert len(ks) == 14, sorted(ks)
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0, (n, v)
        print(n, v)
