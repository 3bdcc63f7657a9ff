"""CPU: the decode grammar and scan of agc_amd/csrc/lz_decode.h (the header the decode kernels are built from), walked in the
kernels' order by tests/lzdec_host -- 64-byte strips, token starts from the end bits with the carried bit, the scan with the
strip carry, pass 1 then pass 2 -- against the oracle's decode, and the malformed deltas it must refuse."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import lzdec_cases
from tests.cases import lz_cases
from tests.lzdec_host import build as lzdec_build

u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def decode():
    L = C.CDLL(lzdec_build.build())
    L.lzdec_decode.restype = C.c_uint32
    L.lzdec_decode.argtypes = [u8p, C.c_uint32, C.c_uint32, u8p, C.c_uint64, C.c_int, u8p, C.c_uint64, C.POINTER(C.c_uint64)]

    def run(ref, mml, enc, rc):
        """-> (status, out)"""
        ref, enc = np.ascontiguousarray(ref, np.uint8), np.ascontiguousarray(enc, np.uint8)
        n = C.c_uint64()
        st = L.lzdec_decode(ref.ctypes.data_as(u8p), ref.size, mml, enc.ctypes.data_as(u8p), enc.size, rc, None, 0, C.byref(n))
        if st:
            return st, None
        out = np.full(n.value + 8, 0xAA, np.uint8)
        st = L.lzdec_decode(ref.ctypes.data_as(u8p), ref.size, mml, enc.ctypes.data_as(u8p), enc.size, rc, out.ctypes.data_as(u8p), n.value, C.byref(n))
        assert (out[n.value:] == 0xAA).all()
        return st, out[:n.value]
    return run


def test_round_trip_of_the_lz_cases(decode, oracle):
    cases = lz_cases()
    assert len(cases) == 60
    for i, (mml, ref, text) in enumerate(cases):
        z = oracle.LZ(ref, mml)
        enc = z.encode(text)
        want = text if enc.size else text[:0]
        dec, n = z.decode(enc, text.size + 8)
        assert n == want.size and np.array_equal(dec, want)
        for rc in (0, 1):
            st, out = decode(ref, mml, enc, rc)
            assert st == 0, f"case {i} rc {rc}"
            assert np.array_equal(out, oracle.rev_comp(want) if rc else want), f"case {i} rc {rc}"


@pytest.mark.parametrize("name,ref_name,enc", lzdec_cases.valid_cases(), ids=[c[0] for c in lzdec_cases.valid_cases()])
def test_handcrafted_deltas(decode, oracle, name, ref_name, enc):
    ref = lzdec_cases.references()[ref_name]
    want, n = oracle.LZ(ref, lzdec_cases.MML).decode(enc, 1 << 16)
    assert n == want.size
    for rc in (0, 1):
        st, out = decode(ref, lzdec_cases.MML, enc, rc)
        assert st == 0
        assert np.array_equal(out, oracle.rev_comp(want) if rc else want), f"rc {rc}"


@pytest.mark.parametrize("name,ref_name,enc,status", lzdec_cases.rejected_cases(), ids=[c[0] for c in lzdec_cases.rejected_cases()])
def test_rejected_deltas(decode, name, ref_name, enc, status):
    ref = lzdec_cases.references()[ref_name]
    for rc in (0, 1):
        st, out = decode(ref, lzdec_cases.MML, enc, rc)
        assert st == status and out is None


def test_scan_equals_the_plain_walk_on_fuzzed_deltas():
    """the harness as a stand-alone program: random deltas over the grammar's bytes, two thirds of them malformed"""
    with tempfile.TemporaryDirectory() as d:
        exe = lzdec_build.build_selftest(os.path.join(d, "lzdec_selftest"), sanitize=False)
        out = subprocess.run([exe, "3", "4000"], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
