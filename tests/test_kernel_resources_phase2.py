"""Compile-time properties of the phase-2 kernel (csrc/zkwg_kernels_phase2.hip), checked with the cross-compiler, no GPU: NO SCRATCH
MEMORY in either instantiation -- the repository's standing rule for point kernels (tests/test_kernel_resources.py).  The digit strings
are kernel arguments whose words are selected, not indexed: an indexed argument array is what would land in scratch."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "zk-email-verify_amd", "csrc")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_phase2_kernels_use_no_scratch_memory(tmp_path):
    """as compiled for gfx950 (ROCm 7), VGPRs / wavefronts per SIMD: zk_phase2_scale<G1> 154 / 3, zk_phase2_scale<G2> 180 / 2.
    Recorded, not asserted: nobody has measured what this kernel needs."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", os.path.join(CSRC, "zkwg_kernels_phase2.hip"), "-o", str(tmp_path / "phase2.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    info, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            info[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            info[cur][m.group(1).strip()] = int(m.group(2))
    ks = {n: v for n, v in info.items() if "zk_phase2_scale" in n}
    assert len(ks) == 2, sorted(info)
    assert sum(1 for n in ks if "ZkEcG1" in n) == 1 and sum(1 for n in ks if "ZkEcG2" in n) == 1, sorted(ks)
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0, (n, v)
        print(n, v)
