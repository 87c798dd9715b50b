"""Shared by the host-math tests (not a test module): the one build of a tests/host_math harness -- the scalar headers of
csrc compiled by g++ into a shared library the tests load with ctypes."""
import ctypes
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM = os.path.join(ROOT, "tests", "host_math")
CSRC = os.path.join(ROOT, "3d-gaussian-splat-attack_amd", "csrc")


def host_lib(name: str) -> ctypes.CDLL:
    """tests/host_math/lib<name>host.so of <name>_host.cpp ("math": libhostmath.so of host_math.cpp), rebuilt when the source or
    any header of csrc is newer."""
    src, so = (f"{name}_host.cpp", f"lib{name}host.so") if name != "math" else ("host_math.cpp", "libhostmath.so")
    src, so = os.path.join(HM, src), os.path.join(HM, so)
    deps = [src] + glob.glob(os.path.join(CSRC, "*.h"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        subprocess.run(["g++", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, src, "-o", so], check=True)
    return ctypes.CDLL(so)
