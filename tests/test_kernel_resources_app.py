"""Compile-time properties of the kernel of the application main EmailReveal (csrc/zkwg_kernels_app.hip), checked with the
cross-compiler, no GPU: NO SCRATCH MEMORY in zk_app_tail -- the two sparse-round Poseidon evaluations keep their state and the dense
mixes' temporaries in LDS columns, one per lane (2 x 10 x 64 field elements = 40 KiB), instead of lane-indexed arrays.  Metadata
only: nothing here looks at instruction streams."""
import kernel_resources

KERNELS = ("zk_app_tail",)
# as compiled when the kernel was written: (VGPRs, occupancy in wavefronts per SIMD -- the LDS columns allow four workgroups per CU)
RECORDED = {"zk_app_tail": (127, 1)}


@kernel_resources.needs_hipcc
def test_no_scratch_memory_in_the_application_tail_kernel():
    info = kernel_resources.usage("zkwg_kernels_app.hip")
    for k in KERNELS:
        assert len([n for n in info if k in n]) == 1, (k, sorted(info))
    assert len(info) == len(KERNELS), sorted(info)                # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        k = next(k for k in KERNELS if k in n)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= RECORDED[k][0] and v["Occupancy"] >= RECORDED[k][1], (n, v)
        assert v.get("LDS Size") == 2 * 10 * 64 * 32, (n, v)
