"""Builds tests/ranges_host/ranges_host.cpp (agc_amd/csrc/range_clip.h and range_plan.h for the HOST, the windowed decode in the
order of lz_decode_window_kernel) into tests/ranges_host/_build/libranges_host.so.  TEST INFRASTRUCTURE ONLY: lets the CPU suite
compare every window with the full decode, sliced; the product compiles the same headers with hipcc and never loads this library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(OUT, "libranges_host.so")
SRC = os.path.join(HERE, "ranges_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "agc_amd", "csrc", h) for h in ("range_clip.h", "range_plan.h", "lz_decode.h", "sym_view.h")]


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
    """the harness with its own main (a stand-alone program: seeded random deltas and contigs, every window against the plain decode,
    sliced), under ASan + UBSan unless told otherwise"""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DRANGES_MAIN"] + flags + [SRC, "-o", exe])
    return exe


if __name__ == "__main__":
    print(build(force=True))
