"""Compile-time properties of the kernels of per-proof groth16 verification (csrc/zkwg_kernels_fexp.hip), checked with the cross-compiler,
no GPU: NO SCRATCH MEMORY in any of them -- the repository's standing rule for these kernels (tests/test_kernel_resources.py), and the
reason the final exponentiation is cut into a program of small launches (the easy part as one kernel took 584 bytes a lane) -- no LDS, and
an occupancy of at least 1 wavefront per SIMD: below 1 a kernel would not launch."""
import kernel_resources

KERNELS = ("zk_fexp_fold", "zk_fexp_ninv", "zk_fexp_pow_u", "zk_fexp_step", "zk_g16_vkx")


@kernel_resources.needs_hipcc
def test_every_kernel_of_the_file_uses_no_scratch_memory_and_can_launch():
    info = kernel_resources.usage("zkwg_kernels_fexp.hip")
    for k in KERNELS:
        assert len([n for n in info if k in n]) == 1, (k, sorted(info))
    assert len(info) == len(KERNELS), sorted(info)                # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("LDS Size") == 0, (n, v)
        assert v.get("Occupancy") >= 1, (n, v)
