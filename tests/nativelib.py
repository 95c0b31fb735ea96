"""Test-only: the host builds of product headers (tests/native/<name>.cpp -> tests/native/libzkwg_<name>.so) that the harness modules
(hosttest, phase2test, ptautest, ptaukeytest, setuptest, verifytest, zkeytest) put their argtypes on."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "zk-email-verify_amd", "csrc")
_libs = {}


def _headers(d):
    return [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".h")]


def build(name, extra_includes=()):
    """-> the ctypes.CDLL of tests/native/<name>.cpp (one per process), compiled again when the source, include/zkwg.h or a header of
    csrc/ or of extra_includes is newer than the library"""
    if name in _libs:
        return _libs[name]
    src, so = os.path.join(NATIVE, name + ".cpp"), os.path.join(NATIVE, f"libzkwg_{name}.so")
    deps = [src, os.path.join(ROOT, "include", "zkwg.h")] + _headers(CSRC) + [h for d in extra_includes for h in _headers(d)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC] + [a for d in extra_includes for a in ("-I", d)] + [src, "-o", so])
    _libs[name] = C.CDLL(so)
    return _libs[name]
