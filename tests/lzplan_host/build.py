"""Builds tests/lzplan_host/lzplan_host.cpp (agc_amd/csrc/lz_plan.h for the HOST, behind a C interface with mirrors of the kernels'
records) into tests/lzplan_host/_build/liblzplan_host.so.  TEST INFRASTRUCTURE ONLY: lets the CPU suite compare the LZ write
path's host arithmetic with values worked out independently; the product compiles the same header with hipcc and never loads this
library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(OUT, "liblzplan_host.so")
SRC = os.path.join(HERE, "lzplan_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "agc_amd", "csrc", h) for h in ("lz_plan.h", "lz_consts.h", "sym_view.h")]


def build(force=False):
    import fcntl
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, ".lock"), "w") as lock:  # (one build at a time: pytest-xdist workers)
        fcntl.flock(lock, fcntl.LOCK_EX)
        if force or not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in DEPS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", SRC, "-o", LIB + ".tmp"])
            os.replace(LIB + ".tmp", LIB)
        return LIB


def build_selftest(exe, sanitize=True):
    """the harness with its own main (a stand-alone program: seeded random batches through every function against a plain
    re-computation)"""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DLZPLAN_MAIN"] + flags + [SRC, "-o", exe])
    return exe


if __name__ == "__main__":
    print(build(force=True))
