"""CPU: the clip arithmetic of agc_amd/csrc/range_clip.h (the header the windowed writers of range_kernels.hip are built from) and
the window arithmetic of range_plan.h, through tests/ranges_host: the windowed decode walked in lz_decode_window_kernel's order --
64-byte strips, every token cut to the window before it writes, the walk stopped behind the window -- must give, for every window
of tests/ranges_cases.py on every handcrafted delta in both orientations, the oracle's full decode, sliced.  And range_plan.h's
layout of agc_hip_ranges_parts -- the output offsets, the windows' jobs, the first complaint -- on handmade batches."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from agc_amd import capi
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


# ---- range_plan.h: the layout of agc_hip_ranges_parts (steps 1 and 4) through rp_layout, tables in the device's place ------------------
RAW, REF, DELTA = capi.SEG_RAW, capi.SEG_REF, capi.SEG_DELTA
SEQ_CAP = 3
PACK_COUNT = [2, 5]  # pack 1 has more sequences than are indexed
SEQ = {(0, 0): (0, 50), (0, 1): (51, 70), (1, 0): (128, 40), (1, 1): (169, 9), (1, 2): (179, 33)}  # (part, index) -> (offset, bytes)
REF_SIZE = [-1, 60, -1, 80]  # group 1: "new" (its size from the parts), group 3: "registered" -- one table serves both, as ref_size() does


def win(kind, gid=0, part=0, index=0, length=0, rc=0, win_from=0, win_len=1):
    return (kind, gid, part, index, length, rc, win_from, win_len)


def layout(lib, q_seg, wins):
    """-> (code, message, out_off, win_out, dj, wj, cj, total); out_off beyond [0] and win_out start as 0xEE..EE"""
    n_q, n_win = len(q_seg) - 1, len(wins)
    q = np.ascontiguousarray(q_seg, np.uint64)
    w = np.array(wins, dtype=capi.SEG_WIN_DTYPE) if wins else np.zeros(0, capi.SEG_WIN_DTYPE)
    count = np.ascontiguousarray(PACK_COUNT, np.uint32)
    off, ln = np.zeros(len(PACK_COUNT) * SEQ_CAP, np.uint64), np.zeros(len(PACK_COUNT) * SEQ_CAP, np.uint32)
    for (p, i), (o, n) in SEQ.items():
        off[p * SEQ_CAP + i], ln[p * SEQ_CAP + i] = o, n
    refs = np.ascontiguousarray(REF_SIZE, np.int64)
    fill = 0xEEEEEEEEEEEEEEEE
    out_off, win_out = np.full(n_q + 1, fill, np.uint64), np.full(n_win, fill, np.uint64)
    dj, wj, cj, sizes = np.zeros((n_win, 7), np.uint64), np.zeros((n_win, 7), np.uint64), np.zeros((n_win, 8), np.uint64), np.zeros(4, np.uint64)
    why = C.create_string_buffer(300)
    u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    lib.rp_layout.restype = C.c_int
    lib.rp_layout.argtypes = [C.c_uint32, u64p, C.c_void_p, u32p, C.c_uint32, u64p, u32p, i64p, C.c_uint32] + [u64p] * 6 + [C.c_char_p, C.c_uint32]
    code = lib.rp_layout(n_q, q.ctypes.data_as(u64p), w.ctypes.data, count.ctypes.data_as(u32p), SEQ_CAP, off.ctypes.data_as(u64p), ln.ctypes.data_as(u32p),
                         refs.ctypes.data_as(i64p), refs.size, *(a.ctypes.data_as(u64p) for a in (out_off, win_out, dj, wj, cj, sizes)), why, 300)
    n_dj, n_wj, n_cj, total = (int(x) for x in sizes)
    return code, why.value.decode(), out_off, win_out, dj[:n_dj].tolist(), wj[:n_wj].tolist(), cj[:n_cj].tolist(), total


def decode_window(lib, win_from, win_len, length, rc):
    """rw::decode_window (range_clip.h) itself, through the harness"""
    lo, hi = C.c_uint32(), C.c_uint32()
    lib.ranges_window_in_decode_order(win_from, win_len, length, rc, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


GOOD = [win(RAW, part=0, index=1, length=70, rc=0, win_from=5, win_len=10), win(RAW, part=1, index=2, length=33, rc=1, win_from=0, win_len=33),
        win(REF, gid=1, length=60, rc=0, win_from=59, win_len=1), win(REF, gid=3, length=80, rc=1, win_from=7, win_len=20),
        win(DELTA, gid=3, part=0, index=0, length=900, rc=0, win_from=100, win_len=300), win(DELTA, gid=1, part=1, index=1, length=77, rc=1, win_from=3, win_len=11)]


def test_layout_of_a_good_batch(lib):
    """three queries, the middle one without a window; RAW, REF and DELTA in both orientations, a REF of a new and one of a
    registered reference: the offsets, every job member for member, w_lo / w_hi, the window each delta job reports"""
    code, why, out_off, win_out, dj, wj, cj, total = layout(lib, [0, 4, 4, 6], GOOD)
    assert (code, why) == (0, "")
    assert win_out.tolist() == [0, 10, 43, 44, 64, 364] and total == 375 and out_off.tolist() == [0, 64, 64, 375]
    assert cj == [[51, 0, 70, 5, 10, 0, 0, 0], [179, 10, 33, 0, 33, 0, 1, 0], [0, 43, 60, 59, 1, 1, 0, 1], [0, 44, 80, 7, 20, 3, 1, 1]]
    assert dj == [[4, 0, 50, 0, 900, 3, 0], [5, 169, 9, 0, 77, 1, 1]]  # the window, then enc_off, enc_len, out_off, out_len, ref_slot, rc
    assert wj == [[0, 50, 64, *decode_window(lib, 100, 300, 900, 0), 3, 0], [169, 9, 364, *decode_window(lib, 3, 11, 77, 1), 1, 1]]
    assert wj[0][3:5] == [100, 400] and wj[1][3:5] == [63, 74]


def test_query_ranges_that_do_not_ascend_from_0_set_nothing(lib):
    for q_seg in ([1, 4, 6], [0, 4, 3, 6]):
        code, _why, out_off, win_out, dj, wj, cj, _t = layout(lib, q_seg, GOOD)
        assert code == -1 and out_off[0] == 0 and (out_off[1:] == 0xEEEEEEEEEEEEEEEE).all() and (win_out == 0xEEEEEEEEEEEEEEEE).all()
        assert dj == wj == cj == []


def changed(w, **kw):
    rec = dict(zip(capi.SEG_WIN_DTYPE.names, GOOD[w]), **kw)
    return GOOD[:w] + [tuple(rec[f] for f in capi.SEG_WIN_DTYPE.names)] + GOOD[w + 1:]


STEP4_REFUSALS = [("an index at its pack's count", 0, dict(index=2)),  # pack 0 has 2 sequences
                  ("an index at seq_cap, below the count", 1, dict(index=3)),  # pack 1 has 5, 3 are indexed
                  ("a RAW sequence of another size", 1, dict(length=34, win_len=1)),
                  ("a REF of a new reference of another size", 2, dict(length=61)),
                  ("a REF of a registered reference of another size", 3, dict(length=79)),
                  ("a DELTA whose index is out of reach", 5, dict(index=3))]


@pytest.mark.parametrize("what,w,kw", STEP4_REFUSALS, ids=[r[0] for r in STEP4_REFUSALS])
def test_step_4_refusals_name_their_window(lib, what, w, kw):
    code, why, out_off, _at, dj, wj, cj, total = layout(lib, [0, 4, 4, 6], changed(w, **kw))
    assert code == capi.EINVAL and why.startswith("ranges_parts: ") and f"window {w} " in why, why
    assert out_off.tolist()[0] == 0 and total == out_off[-1]  # (step 1 ran: the offsets stand)
    assert len(cj) + len(wj) == w and len(dj) == len(wj)  # the windows in front of it got their jobs, it and those behind it none


def test_the_lower_numbered_of_two_bad_windows_is_reported(lib):
    wins = changed(3, length=79)
    wins[1] = changed(1, index=3)[1]
    code, why, *_ = layout(lib, [0, 4, 4, 6], wins)
    assert code == capi.EINVAL and "window 1 " in why and "window 3 " not in why


def test_selftest_program_under_the_sanitizers(tmp_path):
    """the harness as a program of its own, built with -fsanitize=address,undefined and run directly: seeded random deltas, every
    window written into a heap block of exactly its size, random contigs through range_plan.h, and random batches through its
    layout with every array an exact-size heap block"""
    exe = rbuild.build_selftest(str(tmp_path / "ranges_selftest"), sanitize=True)
    out = subprocess.run([exe, "5", "400"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
