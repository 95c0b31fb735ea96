"""Test-only: what the cross-compiler reports for the kernels of one csrc/*.hip (-Rpass-analysis=kernel-resource-usage, no GPU) -- the
registers, scratch memory, LDS and occupancy that tests/test_kernel_resources*.py assert."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "zk-email-verify_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
MAX_COMPILES = 8
_tmp = None
_compiles = {}          # source -> (process, its stderr)
_usage = {}


def start(*sources):
    """begins the cross-compilations of `sources` side by side (each is one hipcc process of 30-60 s; never more than MAX_COMPILES
    of them run at once); usage() waits for the one it needs"""
    global _tmp
    _tmp = _tmp or tempfile.TemporaryDirectory(prefix="zkwg_res_")
    for src in sources:
        if src in _compiles:
            continue
        running = [p for p, _ in _compiles.values() if p.poll() is None]
        if len(running) >= MAX_COMPILES:
            running[0].wait()
        err = open(os.path.join(_tmp.name, src + ".err"), "w+")
        _compiles[src] = (subprocess.Popen([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", os.path.join(CSRC, src), "-o",
                                            os.path.join(_tmp.name, src + ".o"), "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.DEVNULL, stderr=err), err)


def usage(source):
    """-> {kernel: {remark: int}} of csrc/<source>, compiled once per process"""
    if source not in _usage:
        start(source)
        proc, err = _compiles[source]
        rc = proc.wait(timeout=900)
        err.seek(0)
        stderr = err.read()
        assert rc == 0, stderr
        info, cur = {}, None
        for line in stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                info[cur] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
            if m and cur:
                info[cur][m.group(1).strip()] = int(m.group(2))
        _usage[source] = info
    return _usage[source]
