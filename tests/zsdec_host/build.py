"""Builds tests/zsdec_host/zsdec_host.cpp (agc_amd/csrc/zstd/zs_decode.h for the HOST, the wave's program with its lane sections
as loops) into tests/zsdec_host/_build/libzsdec_host.so.  TEST INFRASTRUCTURE ONLY: lets the CPU suite compare the decoder with
libzstd; the product compiles the same header with hipcc and never loads this library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(OUT, "libzsdec_host.so")
SELFTEST = os.path.join(OUT, "zsdec_selftest")
SRC = os.path.join(HERE, "zsdec_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "agc_amd", "csrc", "zstd", h) for h in ("zs_decode.h", "zs_entropy.h", "zs_common.h")]


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
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", SRC, "-o", LIB + ".tmp"])
            os.replace(LIB + ".tmp", LIB)
        return LIB
    return _locked(go)


def build_selftest(force=False):
    """the harness with its own main under -fsanitize=address,undefined (a stand-alone program, run as a child process: frames of
    libzstd's and mutated ones through the decoder and through ZSTD_decompress)"""
    def go():
        if force or _stale(SELFTEST):
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-DZSDEC_MAIN", "-fsanitize=address,undefined",
                                   "-fno-sanitize-recover=all", SRC, "-o", SELFTEST + ".tmp", "-ldl"])
            os.replace(SELFTEST + ".tmp", SELFTEST)
        return SELFTEST
    return _locked(go)


def run_selftest(seed, rounds, dump=None):
    """-> the CompletedProcess of `zsdec_selftest seed rounds [dump]` (exit 0: no disagreement, nothing for the sanitizers to report)"""
    cmd = [build_selftest(), str(seed), str(rounds)] + ([dump] if dump else [])
    return subprocess.run(cmd, capture_output=True, text=True)


def read_dump(path):
    """the inputs a selftest run wrote with DUMP -> [(bytes, status)]"""
    import struct
    out = []
    with open(path, "rb") as f:
        while True:
            h = f.read(8)
            if len(h) < 8:
                return out
            n, st = struct.unpack("<II", h)
            out.append((f.read(n), st))


if __name__ == "__main__":
    print(build(force=True))
    print(build_selftest(force=True))
