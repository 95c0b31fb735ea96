"""Compile-time properties of the kernels of `powersoftau verify` (csrc/zkwg_kernels_verify.hip), checked with the cross-compiler, no GPU:
NO SCRATCH MEMORY in any kernel -- the repository's standing rule for point kernels (tests/test_kernel_resources.py) -- and 2 wavefronts
per SIMD for the subgroup test, the floor the other G2 walks are held to (the walk is a chain of dependent field products; one wavefront
leaves its latency exposed)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "zk-email-verify_amd", "csrc")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_verify_kernels_use_no_scratch_memory_and_the_subgroup_test_keeps_two_wavefronts(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", os.path.join(CSRC, "zkwg_kernels_verify.hip"), "-o", str(tmp_path / "verify.o"),
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
    subgroup = [n for n in info if "zk_verify_g2_subgroup" in n]
    widen = [n for n in info if "zk_verify_widen" in n]
    assert len(subgroup) == 1 and len(widen) == 1 and len(info) == 2, sorted(info)      # every kernel of the file is looked at
    for n, v in info.items():
        print(n, v)
        assert v.get("ScratchSize") == 0, (n, v)
        assert v.get("LDS Size") == 0, (n, v)
    assert info[subgroup[0]].get("Occupancy") >= 2, info[subgroup[0]]
