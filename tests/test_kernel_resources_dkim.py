"""Compile-time properties of the kernels of DKIM verification of raw emails (csrc/zkwg_kernels_dkim.hip), checked with the cross-compiler,
no GPU: NO SCRATCH MEMORY in any of the three -- the repository's standing rule (tests/test_kernel_resources.py) -- and zk_dkim_body, whose
state between tiles is a handful of registers, at four or more wavefronts per SIMD."""
import kernel_resources

KERNELS = ("zk_dkim_body", "zk_dkim_hash", "zk_dkim_verify")


@kernel_resources.needs_hipcc
def test_no_scratch_memory_and_the_body_kernel_keeps_its_occupancy():
    info = kernel_resources.usage("zkwg_kernels_dkim.hip")
    for k in KERNELS:
        assert len([n for n in info if k in n]) == 1, (k, sorted(info))
    assert len(info) == len(KERNELS), sorted(info)                # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("Occupancy") >= (4 if "zk_dkim_body" in n else 1), (n, v)
    body = [v for n, v in info.items() if "zk_dkim_body" in n][0]
    assert body.get("LDS Size") == 2048, body                     # the stage of one tile's emitted bytes
