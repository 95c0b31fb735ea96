"""Compile-time properties of the kernels of the CleanEmailAddress main (csrc/zkwg_kernels_cea.hip), checked with the cross-compiler,
no GPU: NO SCRATCH MEMORY in zk_cea_chunks (the limb-form Poseidon(16) evaluator with its state in LDS, as in zk_rslb_chunks), in
zk_cea_tail (merges, chains, inversion: one lane per email) and in zk_expand3_cea -- the instantiation of zk_expand that carries the
byte-local decoder ZSEG_CEA so that the headline kernel's switch does not (tests/test_kernel_resources.py holds that one unchanged).
Metadata only: nothing here looks at instruction streams."""
import kernel_resources

KERNELS = ("zk_cea_chunks", "zk_cea_tail", "zk_expand3_cea")
# as compiled when the kernels were written: (VGPRs, occupancy in wavefronts per SIMD)
RECORDED = {"zk_cea_chunks": (124, 1), "zk_cea_tail": (159, 3), "zk_expand3_cea": (42, 8)}


@kernel_resources.needs_hipcc
def test_no_scratch_memory_in_the_clean_address_kernels():
    info = kernel_resources.usage("zkwg_kernels_cea.hip")
    for k in KERNELS:
        assert len([n for n in info if k in n]) == 1, (k, sorted(info))
    assert len(info) == len(KERNELS), sorted(info)                # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        k = next(k for k in KERNELS if k in n)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= RECORDED[k][0] and v["Occupancy"] >= RECORDED[k][1], (n, v)
    lds = {k: [v for n, v in info.items() if k in n][0].get("LDS Size") for k in KERNELS}
    assert lds == {"zk_cea_chunks": 9 * 17 * 64 * 4, "zk_cea_tail": 9 * 3 * 64 * 4, "zk_expand3_cea": 0}
