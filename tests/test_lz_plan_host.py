"""CPU: agc_amd/csrc/lz_plan.h compiled for the host (tests/lzplan_host) -- the host arithmetic of the LZ write path (the order of a
batch, output offsets, the chunk decision and plan, a reference's layout, the dirty range of the descriptor table).  Every expected
value is worked out here in Python integers, never taken from the harness."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest

from tests.lzplan_host import build as lpbuild

u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
ENCODE, ESTIMATE, COSTVEC = 0, 1, 2  # lz_consts.h: MODE_*


@pytest.fixture(scope="module")
def lp():
    L = C.CDLL(lpbuild.build())
    L.lp_order.argtypes = [C.c_uint32, u32p, u32p]
    L.lp_order.restype = None
    L.lp_out_offsets.argtypes = [C.c_int, C.c_uint32, u32p, u64p]
    L.lp_out_offsets.restype = C.c_uint64
    L.lp_filter_word_offsets.argtypes = [C.c_uint32, u32p, u64p]
    L.lp_filter_word_offsets.restype = C.c_uint64
    L.lp_filter_jobs.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint32, u32p]
    L.lp_filter_jobs.restype = C.c_uint32
    L.lp_chunk_len_for.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64]
    L.lp_chunk_len_for.restype = C.c_uint32
    L.lp_count_chunk_jobs.argtypes = [C.c_uint32, u32p, C.c_uint32]
    L.lp_count_chunk_jobs.restype = C.c_uint64
    L.lp_chunks_fit.argtypes = [C.c_uint64]
    L.lp_plan_chunks.argtypes = [C.c_uint32, u32p, C.c_uint32, C.c_int, u32p, u32p, C.c_uint64, u32p, u64p]
    L.lp_logs_ahead_bytes.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64]
    L.lp_logs_ahead_bytes.restype = C.c_uint64
    L.lp_ht_size.argtypes = [C.c_uint32]
    L.lp_ht_size.restype = C.c_uint64
    L.lp_is_short.argtypes = [C.c_uint32]
    L.lp_is_short.restype = C.c_uint32
    L.lp_split_factor.argtypes = [C.c_uint32]
    L.lp_split_factor.restype = C.c_uint32
    L.lp_ref_layout.argtypes = [C.c_uint32, u32p, u32p, u8p, u64p, u64p, u64p, u64p, u64p]
    L.lp_ref_layout.restype = None
    L.lp_widen_dirty.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u64p]
    L.lp_widen_dirty.restype = None
    return L


def arr(values, dtype):
    return np.ascontiguousarray(np.array(list(values) + [0], dtype=dtype)[:len(values)])  # (never a zero-size pointer of the wrong type)


def ptr(a, t):
    return a.ctypes.data_as(t)


def order_of(lp, lens):
    a, out = arr(lens, np.uint32), np.full(len(lens) + 1, 0xAAAAAAAA, np.uint32)
    lp.lp_order(len(lens), ptr(a, u32p), ptr(out, u32p))
    assert out[len(lens)] == 0xAAAAAAAA
    return out[:len(lens)].tolist()


def longest_first(lens):
    return sorted(range(len(lens)), key=lambda i: (-lens[i], i))


# ---- order ----------------------------------------------------------------------------------------------------------------------
def test_order_of_nothing_and_of_one(lp):
    assert order_of(lp, []) == []
    assert order_of(lp, [7]) == [0]


def test_order_keeps_ties_in_index_order(lp):
    lens = [5, 9, 5, 9, 9, 0, 5, 0]
    assert order_of(lp, lens) == [1, 3, 4, 0, 2, 6, 5, 7]


def test_order_reads_all_three_radix_digits(lp):
    # (1 << 22, (1 << 22) + 1 and 1 << 23 differ in the third 11-bit digit alone or in the first and the third)
    lens = [1 << 22, 0, (1 << 22) + 1, 2047, 1 << 23, 2048, 0xFFFFFFFF, 1 << 22, 2047, 0]
    assert order_of(lp, lens) == longest_first(lens) == [6, 4, 2, 0, 7, 5, 3, 8, 1, 9]


def test_order_of_5000_random_lengths(lp):
    rng = random.Random(20)
    lens = [rng.choice((rng.randrange(1 << 32), rng.randrange(1 << 23), rng.randrange(70000), rng.randrange(40))) for _ in range(5000)]
    assert order_of(lp, lens) == longest_first(lens)


# ---- output offsets -------------------------------------------------------------------------------------------------------------
LENS = [0, 1, 15, 16, 17, 4095, 4096]


def offsets(fn, lens, *head):
    a, off = arr(lens, np.uint32), np.zeros(len(lens) + 1, np.uint64)
    total = fn(*head, len(lens), ptr(a, u32p), ptr(off, u64p))
    return off[:len(lens)].tolist(), total


def running(sizes):
    off, t = [], 0
    for s in sizes:
        off.append(t)
        t += s
    return off, t


def test_encode_offsets(lp):
    bound = [((n + 5 * n // 16 + 64) + 15) // 16 * 16 for n in LENS]
    assert bound == [64, 80, 96, 96, 96, 5440, 5440]  # (by hand: 4095 + 1279 + 64 = 5438 -> 5440; 4096 + 1280 + 64 = 5440)
    off, total = offsets(lp.lp_out_offsets, LENS, ENCODE)
    assert (off, total) == running(bound)
    assert all(o % 16 == 0 for o in off) and total % 16 == 0 and total == sum(bound)


def test_cost_vector_and_estimate_offsets(lp):
    assert offsets(lp.lp_out_offsets, LENS, COSTVEC) == running(LENS)  # one unit per symbol
    assert offsets(lp.lp_out_offsets, LENS, COSTVEC)[1] == 8240
    assert offsets(lp.lp_out_offsets, LENS, ESTIMATE) == ([0] * len(LENS), 0)  # an estimate writes no output


def test_filter_word_offsets(lp):
    words = [(n + 63) // 64 + 1 for n in LENS]
    assert words == [1, 2, 2, 2, 2, 65, 65]
    assert offsets(lp.lp_filter_word_offsets, LENS) == running(words)


def test_filter_jobs_cover_a_text_in_chunks_of_65536(lp):
    for n, want in ((0, []), (1, [0]), (65536, [0]), (65537, [0, 65536]), (200000, [0, 65536, 131072, 196608])):
        chunk, shift = np.zeros(8, np.uint32), C.c_uint32(0)
        assert lp.lp_filter_jobs(n, 60000, ptr(chunk, u32p), 8, C.byref(shift)) == len(want)
        assert chunk[:len(want)].tolist() == want
        assert not want or shift.value == 20  # (15 001 keys: the smallest filter, 4096 words = 32 - 20 bits)


# ---- the chunk decision ---------------------------------------------------------------------------------------------------------
def test_chunk_len_forced(lp):
    for forced, want in ((0, 0), (1, 64), (63, 64), (64, 64), (300, 300)):
        assert lp.lp_chunk_len_for(forced, 1, 3, 100, 250) == want
        assert lp.lp_chunk_len_for(forced, 1, 3, 1 << 20, 1 << 20) == want  # (forced: whatever the texts are)


def test_chunk_len_automatic(lp):
    auto = -1  # (the variable is not set)
    assert lp.lp_chunk_len_for(auto, 1, 1, 16383, 16383) == 0
    assert lp.lp_chunk_len_for(auto, 1, 1, 16384, 16384) == 4096
    assert 16384 * 6144 == 4 * (16384 * 1536)
    assert lp.lp_chunk_len_for(auto, 1, 1537, 16384, 16384 * 1536) == 0          # exact equality: not worth it
    assert lp.lp_chunk_len_for(auto, 1, 1537, 16384, 16384 * 1536 - 1) == 4096
    assert lp.lp_chunk_len_for(auto, 1, 1537, 16384, 16384 * 1536 + 1) == 0


def test_chunk_len_without_host_descriptors(lp):
    for forced in (-1, 300):
        assert lp.lp_chunk_len_for(forced, 1, 0, 0, 0) == 0                 # no descriptors
        assert lp.lp_chunk_len_for(forced, 0, 1, 1 << 20, 1 << 20) == 0     # a count made on the device


# ---- the chunk plan -------------------------------------------------------------------------------------------------------------
def plan(lp, lens, chunk, encode, jobs_cap=64):
    a = arr(lens, np.uint32)
    sizes, jobs, seg0, built = np.zeros(4, np.uint32), np.zeros(2 * jobs_cap, np.uint32), np.zeros(len(lens) + 1, np.uint32), C.c_uint64(0)
    ok = lp.lp_plan_chunks(len(lens), ptr(a, u32p), chunk, encode, ptr(sizes, u32p), ptr(jobs, u32p), jobs_cap, ptr(seg0, u32p), C.byref(built))
    return ok, sizes.tolist(), jobs.reshape(-1, 2).tolist(), seg0.tolist(), built.value


@pytest.mark.parametrize("chunk", [64, 300, 4096])
def test_chunk_plan_jobs_and_sizes(lp, chunk):
    lens = [0, chunk, chunk + 1, 3 * chunk - 1, 1]
    n_chunks = [1, 1, 2, 3, 1]  # (an empty text still has a job; a text of exactly one chunk has one)
    want_jobs = [[i, ch] for i, nc in enumerate(n_chunks) for ch in range(nc)]
    for encode in (0, 1):
        ok, sizes, jobs, seg0, _ = plan(lp, lens, chunk, encode)
        assert ok == 1
        stride = (chunk + 5 * chunk // 16 + 160 + 15) // 16 * 16 if encode else 0
        assert sizes == [8, chunk, chunk // 8 + 4, stride]
        assert jobs[:8] == want_jobs
        assert seg0 == [0, 1, 2, 4, 7, 8]
    assert {64: (12, 256), 300: (41, 560), 4096: (516, 5536)}[chunk] == (chunk // 8 + 4, (chunk + 5 * chunk // 16 + 160 + 15) // 16 * 16)


def test_chunk_plan_refuses_more_than_4194304_jobs(lp):
    limit = 1 << 22
    assert lp.lp_chunks_fit(limit) == 1 and lp.lp_chunks_fit(limit + 1) == 0
    # one text of exactly 2^22 chunks of 64 symbols, and one symbol more (counted, not listed)
    for n_sym, jobs in ((limit * 64, limit), (limit * 64 + 1, limit + 1)):
        a = arr([n_sym], np.uint32)
        assert lp.lp_count_chunk_jobs(1, ptr(a, u32p), 64) == jobs == -(-n_sym // 64)
    # ... and spread over texts: 4096 texts of 1024 chunks, then one empty text more (a job of its own)
    lens = [1024 * 4096] * 4096
    a = arr(lens + [0], np.uint32)
    assert lp.lp_count_chunk_jobs(4096, ptr(a, u32p), 4096) == limit
    assert lp.lp_count_chunk_jobs(4097, ptr(a, u32p), 4096) == limit + 1
    ok, _, _, _, built = plan(lp, lens + [0], 4096, 1, jobs_cap=0)
    assert ok == 0 and built == 0  # refused before anything was allocated


def test_logs_ahead(lp):
    mib32, state = 32 << 20, 16
    want = lambda n, total: (total // 4096 + n + (total // 4096 + n) // 2) * (4096 // 8 + 4) * state  # noqa: E731
    assert want(1024, mib32) == (9216 + 4608) * 516 * 16
    assert lp.lp_logs_ahead_bytes(0, 1024, mib32, 0, state) == want(1024, mib32)
    assert lp.lp_logs_ahead_bytes(0, 1023, mib32, 0, state) == 0          # a small batch
    assert lp.lp_logs_ahead_bytes(0, 1024, mib32 - 1, 0, state) == 0      # little text
    assert lp.lp_logs_ahead_bytes(1, 1024, mib32, 0, state) == 0          # an encode
    assert lp.lp_logs_ahead_bytes(0, 1024, mib32, want(1024, mib32), state) == 0  # the buffer is large enough
    assert lp.lp_logs_ahead_bytes(0, 1024, mib32, want(1024, mib32) - 1, state) == want(1024, mib32)
    assert lp.lp_logs_ahead_bytes(0, 3000, 200 << 20, 1 << 20, state) == want(3000, 200 << 20)


# ---- a reference ----------------------------------------------------------------------------------------------------------------
def ht_size(count):
    """lz_diff.cpp:117-125: the count over the load factor as a double, cut to its top bit, doubled, at least 8"""
    h = int(count / 0.7)
    return max(8, 2 * (1 << (h.bit_length() - 1))) if h else 8


def test_ht_size_small_counts(lp):
    assert [ht_size(c) for c in (0, 1, 2, 5, 6, 7, 11, 12)] == [8, 8, 8, 8, 16, 16, 16, 32]  # (5 / 0.7 = 7.1, 6 / 0.7 = 8.6, 11 / 0.7 = 15.7, 12 / 0.7 = 17.1)
    for c in (0, 1, 2, 5, 6, 7, 11, 12):
        assert lp.lp_ht_size(c) == ht_size(c), c


@pytest.mark.parametrize("k", range(4, 31))
def test_ht_size_at_the_power_of_two(lp, k):
    c = int((1 << k) * 0.7)
    while int((c + 1) / 0.7) < (1 << k):
        c += 1
    while int(c / 0.7) >= (1 << k):
        c -= 1
    assert int(c / 0.7) < (1 << k) <= int((c + 1) / 0.7)  # c: the largest count below 2^k
    assert ht_size(c) == 1 << k and ht_size(c + 1) == 2 << k
    assert lp.lp_ht_size(c) == 1 << k
    assert lp.lp_ht_size(c + 1) == 2 << k


def test_is_short(lp):
    assert 262139 // 4 == 65534 and 262140 // 4 == 65535  # lz_diff.cpp:146: size / hashing_step < 65535
    assert lp.lp_is_short(262139) == 1
    assert lp.lp_is_short(262140) == 0
    assert lp.lp_is_short(0) == 1


def key_bloom_bytes(ref_size):
    shift = 20
    while shift > 8 and (1 << (32 - shift)) < (ref_size // 4 + 1) // 4:
        shift -= 1
    return 2 * (1 << (32 - shift)) * 8


def test_reference_layout(lp):
    lens, keys, esc = [1000, 300000, 61], [250, 70000, 10], [0, 1, 0]
    n = len(lens)
    a, k, e = arr(lens, np.uint32), arr(keys, np.uint32), arr(esc, np.uint8)
    roff, toff, boff = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    tot, esc_at = np.zeros(3, np.uint64), np.zeros(2 * n, np.uint64)
    lp.lp_ref_layout(n, ptr(a, u32p), ptr(k, u32p), ptr(e, u8p), ptr(roff, u64p), ptr(toff, u64p), ptr(boff, u64p), ptr(tot, u64p), ptr(esc_at, u64p))
    stored = [(-(-n_sym // 16) + 4) * 4 for n_sym in lens]                                   # the 2-bit words and four of slack
    table = [ht_size(c) * (4 if n_sym // 4 < 65535 else 8) for c, n_sym in zip(keys, lens)]   # 16-bit positions below 262140 symbols
    assert stored == [268, 75016, 32] and table == [512 * 4, 131072 * 8, 16 * 4]
    filt = [key_bloom_bytes(n_sym) for n_sym in lens]
    assert filt == [65536, 2 * 32768 * 8, 65536]  # (75 001 keys / 4 = 18 750 words -> 32 768)
    for off, size, total, align in ((roff.tolist(), stored, int(tot[0]), 16), (toff.tolist(), table, int(tot[1]), 256), (boff.tolist(), filt, int(tot[2]), 8)):
        assert off[0] == 0 and off == sorted(off)
        assert all(o % align == 0 for o in off) and total % align == 0
        ends = off[1:] + [total]
        assert all(o + s <= end < o + s + align for o, s, end in zip(off, size, ends))  # nothing overlaps, nothing but the rounding between
    # the flagged reference: the escape index (a word per 1024-symbol block + 64 bytes), then a byte per symbol, 16-byte aligned, inside the block
    nb = -(-lens[1] // 1024)
    at, alloc = int(esc_at[2]), int(esc_at[3])
    assert nb == 293 and at % 16 == 0 and nb * 4 + 64 <= at < nb * 4 + 64 + 16
    assert alloc == nb * 4 + 64 + nb * 1024
    assert at + nb * 1024 <= -(-alloc // 256) * 256  # (the arena hands out multiples of 256 bytes)


def test_split_factor(lp):
    want = {1: 16, 127: 16, 128: 16, 129: 15, 2047: 1, 2048: 1}
    assert all(want[n] == (1 if n >= 2048 else min(16, 2048 // n)) for n in want)
    assert {n: lp.lp_split_factor(n) for n in want} == want


# ---- the dirty range ------------------------------------------------------------------------------------------------------------
def widen(lp, dirty, lo, hi, on_dev, min_gid, max_gid):
    out = np.zeros(2, np.uint64)
    lp.lp_widen_dirty(dirty, lo, hi, on_dev, min_gid, max_gid, ptr(out, u64p))
    return out.tolist()


def test_dirty_range(lp):
    assert widen(lp, 0, 0, 0, 10, 10, 12) == [10, 13]      # a clean table: the batch alone
    assert widen(lp, 0, 3, 9, 10, 10, 12) == [10, 13]      # (a stale range of a clean table does not count)
    assert widen(lp, 1, 5, 8, 20, 3, 9) == [3, 10]         # a dirty one, widened below and above
    assert widen(lp, 1, 5, 8, 20, 6, 6) == [5, 8]          # ... or not at all
    assert widen(lp, 0, 0, 0, 10, 15, 16) == [10, 17]      # a gap above the old end: its (invalid) descriptors go over too
    assert widen(lp, 1, 2, 4, 10, 15, 16) == [2, 17]


def test_selftest_program(tmp_path):
    """the harness as a program of its own: seeded random batches through every function against a plain re-computation.  (Built
    with tests/lzplan_host/build.py: build_selftest(sanitize=True) the same program runs under ASan + UBSan.)"""
    exe = lpbuild.build_selftest(str(tmp_path / "lzplan_selftest"), sanitize=False)
    out = subprocess.run([exe, "5", "300"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok 300 batches"), out.stdout + out.stderr
