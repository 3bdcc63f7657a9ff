"""Builds tests/inflate_host/inflate_host.cpp (agc_amd/csrc/inflate.h for the HOST, the wavefront's program with its lane sections as
loops) into tests/inflate_host/_build/libinflate_host.so.  TEST INFRASTRUCTURE ONLY: lets the CPU suite check the decoder against zlib
and gives the GPU suite the bytes and statuses the device must equal; the product compiles the same header with hipcc and never loads
this library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(OUT, "libinflate_host.so")
SELFTEST = os.path.join(OUT, "inflate_selftest")
SRC = os.path.join(HERE, "inflate_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "agc_amd", "csrc", "inflate.h"), os.path.join(ROOT, "agc_amd", "csrc", "bgzf.h")]


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


def _locked(fn):
    import fcntl
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, ".lock"), "w") as lock:  # (one build at a time: pytest-xdist workers)
        fcntl.flock(lock, fcntl.LOCK_EX)
        return fn()


def build(force=False):
    def go():
        if force or _stale(LIB):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", SRC, "-o", LIB + ".tmp"])
            os.replace(LIB + ".tmp", LIB)
        return LIB
    return _locked(go)


def build_selftest(force=False):
    """the harness with its own main under -fsanitize=address,undefined (a stand-alone program, run as a child process: seeded random
    members, two thirds of them damaged, through the decoder and through zlib's inflate)"""
    def go():
        if force or _stale(SELFTEST):
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DINF_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                   SRC, "-o", SELFTEST + ".tmp", "-lz"])
            os.replace(SELFTEST + ".tmp", SELFTEST)
        return SELFTEST
    return _locked(go)


def run_selftest(seed, rounds):
    """-> the CompletedProcess of `inflate_selftest seed rounds` (exit 0: what the decoder accepts zlib decodes to the same bytes, what
    it refuses zlib refuses, no guard byte touched, nothing for the sanitizers to report)"""
    return subprocess.run([build_selftest(), str(seed), str(rounds)], capture_output=True, text=True)


if __name__ == "__main__":
    print(build(force=True))
    print(build_selftest(force=True))
