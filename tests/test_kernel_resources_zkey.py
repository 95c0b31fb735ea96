"""Compile-time properties of zk_zkey_abc (csrc/zkwg_kernels_zkey.hip), checked with the cross-compiler, no GPU: no scratch memory and
no LDS in any variant -- a lane keeps the signed word columns of its G witnesses (8 x 64 bits each), the 17 product columns and the
gathered values in registers; an array indexed by a loop that is not unrolled would put them in scratch."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "zk-email-verify_amd", "csrc")


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_zkey_row_kernels_use_no_scratch_memory(tmp_path):
    """as compiled for gfx950 (ROCm 7): zk_zkey_abc_short<2> / _long<2> (the default): 130 / 132 VGPRs, 3 wavefronts per SIMD; <4>
    (ZKWG_ZKEY_G=4): 242 VGPRs, 2 wavefronts per SIMD; zk_zkey_range 10 VGPRs, zk_zkey_scrub 8, both 8 wavefronts per SIMD."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", os.path.join(CSRC, "zkwg_kernels_zkey.hip"), "-o", str(tmp_path / "zkey.o"),
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
    ks = {n: v for n, v in info.items() if "zk_zkey_" in n}
    abc = {n: v for n, v in ks.items() if "zk_zkey_abc" in n}
    assert len(abc) == 4 and len(ks) == 6, sorted(info)          # short / long x G = 2, 4; range, scrub
    for n, v in ks.items():
        assert v.get("ScratchSize") == 0 and v["LDS Size"] == 0, (n, v)
    for n, v in abc.items():
        assert v["Occupancy"] >= (3 if "ILi2E" in n else 2), (n, v)
