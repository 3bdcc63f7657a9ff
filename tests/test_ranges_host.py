"""CPU: the clip arithmetic of agc_amd/csrc/range_clip.h (the header the windowed writers of range_kernels.hip are built from) and
the window arithmetic of range_plan.h, through tests/ranges_host: the windowed decode walked in lz_decode_window_kernel's order --
64-byte strips, every token cut to the window before it writes, the walk stopped behind the window -- must give, for every window
of tests/ranges_cases.py on every handcrafted delta in both orientations, the oracle's full decode, sliced."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import lzdec_cases
from tests import ranges_cases as RC
from tests.ranges_host import build as rbuild

u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
GUARD = 0xAA


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(rbuild.build())
    L.ranges_decode_window.restype = C.c_uint32
    L.ranges_decode_window.argtypes = [u8p, C.c_uint32, C.c_uint32, u8p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, u8p, u32p]
    L.ranges_raw_window.restype = None
    L.ranges_raw_window.argtypes = [u8p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, u8p]
    L.ranges_contig_windows.restype = C.c_uint64
    L.ranges_contig_windows.argtypes = [C.c_uint64, u32p, C.c_uint32, C.c_int64, C.c_int64, u32p, u32p, u32p, C.POINTER(C.c_uint64)]
    return L


def window(L, ref, enc, rc, a, n):
    """-> (status, the window's bytes, strips walked); the output sits between guard bytes, which must stay"""
    out = np.full(8 + n + 8, GUARD, np.uint8)
    strips = C.c_uint32(0)
    st = L.ranges_decode_window(ref.ctypes.data_as(u8p), ref.size, lzdec_cases.MML, enc.ctypes.data_as(u8p), enc.size, rc, a, n,
                                out[8:].ctypes.data_as(u8p), C.byref(strips))
    assert (out[:8] == GUARD).all() and (out[8 + n:] == GUARD).all()
    return st, out[8:8 + n], strips.value


@pytest.mark.parametrize("name,ref_name,enc", lzdec_cases.valid_cases(), ids=[c[0] for c in lzdec_cases.valid_cases()])
def test_every_window_is_the_full_decode_sliced(lib, oracle, name, ref_name, enc):
    ref = lzdec_cases.references()[ref_name]
    enc = np.ascontiguousarray(enc) if enc.size else np.zeros(1, np.uint8)[:0]
    want, n = oracle.LZ(ref, lzdec_cases.MML).decode(enc, 1 << 16)
    starts, length = RC.token_starts(enc, ref.size)
    assert n == want.size == length
    if not length:  # (the delta of no bytes: no window has a symbol)
        assert window(lib, ref, enc, 0, 0, 1)[0] == 100
        return
    wins = RC.delta_windows(starts, length)
    assert (0, length) in wins and (0, 1) in wins and (length - 1, 1) in wins
    n_strips = (enc.size + 63) // 64
    for rc in (0, 1):
        full = oracle.rev_comp(want) if rc else want
        for a, m in wins:
            st, got, strips = window(lib, ref, enc, rc, a, m)
            assert st == 0 and np.array_equal(got, full[a:a + m]), (name, rc, a, m)
            assert 1 <= strips <= n_strips
        assert window(lib, ref, enc, rc, length, 1)[0] == 100 and window(lib, ref, enc, rc, length - 1, 2)[0] == 100  # one symbol past the end
        assert window(lib, ref, enc, rc, 0, 0)[0] == 100


def test_the_walk_stops_behind_the_window(lib):
    """five strips of literals: the first symbol's window walks one strip, the last symbol's all five"""
    ref = lzdec_cases.references()["clean"]
    enc = lzdec_cases.Delta(ref.size).pad_to(5 * 64).bytes()
    assert window(lib, ref, enc, 0, 0, 1)[2] == 1 and window(lib, ref, enc, 0, 64, 1)[2] == 2 and window(lib, ref, enc, 0, 319, 1)[2] == 5
    assert window(lib, ref, enc, 1, 319, 1)[2] == 1 and window(lib, ref, enc, 1, 0, 1)[2] == 5  # reverse-complemented: mirrored


def test_rejected_deltas_are_refused_before_the_window(lib):
    for name, ref_name, enc, status in lzdec_cases.rejected_cases():
        ref = lzdec_cases.references()[ref_name]
        assert window(lib, ref, np.ascontiguousarray(enc), 0, 0, 1)[0] == status, name


def test_raw_windows(lib, oracle):
    sym = np.random.default_rng(5).integers(0, 16, 300, dtype=np.uint8)
    for rc in (0, 1):
        full = oracle.rev_comp(sym) if rc else sym
        for a, m in RC.delta_windows([0, 150], sym.size):
            out = np.full(m + 8, GUARD, np.uint8)
            lib.ranges_raw_window(sym.ctypes.data_as(u8p), sym.size, rc, a, m, out.ctypes.data_as(u8p))
            assert np.array_equal(out[:m], full[a:a + m]) and (out[m:] == GUARD).all(), (rc, a, m)


def test_contig_windows_against_a_position_table(lib):
    rng = np.random.default_rng(9)
    for k, lengths in ((25, [60, 25, 80, 30]), (3, [1]), (4, [0, 4, 9]), (21, [21 + int(x) for x in rng.integers(0, 90, 7)])):
        table = [(s, i) for s, n in enumerate(lengths) for i in range(k if s else 0, n)]  # contig position -> (segment, offset in it)
        ln = np.ascontiguousarray(lengths, np.uint32)
        for f, t in RC.contig_ranges(lengths, k) + [(f, t) for f in range(-2, len(table) + 3, 7) for t in range(-2, len(table) + 3, 5)]:
            seg, wf, wl = (np.zeros(len(lengths), np.uint32) for _ in range(3))
            n_sym = C.c_uint64()
            n = lib.ranges_contig_windows(ln.size, ln.ctypes.data_as(u32p), k, f, t, seg.ctypes.data_as(u32p), wf.ctypes.data_as(u32p), wl.ctypes.data_as(u32p), C.byref(n_sym))
            lo, hi = max(f, 0), (len(table) - 1 if t < 0 else t)
            if t >= 0 and lo > hi:
                lo, hi = 0, len(table) - 1
            want = table[lo:hi + 1]
            got = [(int(seg[i]), int(wf[i]) + q) for i in range(n) for q in range(int(wl[i]))]
            assert got == want and n_sym.value == len(want) and (wl[:n] >= 1).all(), (k, lengths, f, t)
            assert all(wf[i] >= k for i in range(n) if seg[i] > 0)


def test_selftest_program_under_the_sanitizers(tmp_path):
    """the harness as a program of its own, built with -fsanitize=address,undefined and run directly: seeded random deltas, every
    window written into a heap block of exactly its size, and random contigs through range_plan.h"""
    exe = rbuild.build_selftest(str(tmp_path / "ranges_selftest"), sanitize=True)
    out = subprocess.run([exe, "5", "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
