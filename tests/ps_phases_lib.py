"""tests/ps_phases_shim.cpp compiled for the host (g++, against oracle/liboracle.so for the analysis bank), once per test
session: the entry points tests/test_ps_phases_cpu.py and tests/test_ps_phases_gpu.py share."""
import ctypes
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P16 = ctypes.POINTER(ctypes.c_int16)
P32 = ctypes.POINTER(ctypes.c_int32)
P64 = ctypes.POINTER(ctypes.c_int64)
_keep = []


@functools.lru_cache(maxsize=None)
def load(oracle_path):
    """oracle_path: the built oracle/liboracle.so (the `oracle` fixture has made it)"""
    d = tempfile.TemporaryDirectory(prefix="ps_phases_")
    _keep.append(d)
    so = os.path.join(d.name, "ps_phases_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "ps_phases_shim.cpp"), "-o", so, oracle_path,
                           "-Wl,-rpath," + os.path.dirname(oracle_path)])
    lib = ctypes.CDLL(so)
    lib.xpt_group_sums.argtypes = [P32, ctypes.c_int, P32, P32]
    lib.xpt_group_sums.restype = None
    lib.xpt_ps_frame.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, P32] + [ctypes.c_int] * 6 + [P32, P32]
    lib.xpt_hq_group_sums.argtypes = [ctypes.c_void_p] * 5 + [P16, P64]
    return lib
