"""CPU: agc_amd/csrc/fasta_out.h compiled for the host (tests/fastaout_host) -- the layout arithmetic, and the text kernel's
per-chunk walk run chunk after chunk over whole buffers -- against text built independently in numpy (tests/fastaout_cases.py:
the plans tests/test_gpu_fasta_out.py sends through the device)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import fastaout_cases as FC
from tests.fastaout_host import build as fobuild

u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def fo():
    L = C.CDLL(fobuild.build())
    L.fo_text.argtypes = [C.c_uint32, u64p, u64p, u64p, u64p, u8p, u64p, u64p, u32p, u8p, C.c_uint32, C.c_uint32, C.c_uint64, u8p]
    L.fo_text.restype = None
    L.fo_contig_text_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.fo_contig_text_bytes.restype = C.c_uint64
    L.fo_body_locate.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, u64p]
    L.fo_body_offset_of.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.fo_body_offset_of.restype = C.c_uint64
    L.fo_letter.argtypes = [C.c_uint32]
    L.fo_letter.restype = C.c_uint32
    L.fo_chunk_range.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, u64p, u32p]
    L.fo_chunk_range.restype = None
    L.fo_chunk_count.argtypes = [C.c_uint32, C.c_uint64]
    L.fo_chunk_count.restype = C.c_uint64
    return L


def host_text(fo, case, lay, a):
    p = lambda x, t: x.ctypes.data_as(t)  # noqa: E731
    names = np.frombuffer(lay["names"] + b"\0", np.uint8)
    out = np.full(lay["total"] + 32, 0xAA, np.uint8)
    fo.fo_text(len(case["contigs"]), p(lay["ctg_text"], u64p), p(lay["ctg_seg"], u64p), p(lay["ctg_sym"], u64p), p(lay["name_off"], u64p), p(names, u8p),
               p(lay["seg_start"], u64p), p(lay["seg_off"], u64p), p(lay["skip"], u32p), p(np.concatenate([lay["sym"], np.zeros(1, np.uint8)]), u8p),
               case["line_length"], a, lay["total"], p(out, u8p))
    assert (out[lay["total"]:] == 0xAA).all()
    return out[:lay["total"]].tobytes()


@pytest.mark.parametrize("case", FC.small_cases(), ids=lambda c: c["name"])
def test_chunk_walk_writes_the_text(fo, case):
    lay = FC.layout(case)
    FC.check_preconditions(case, lay)
    want = FC.expected_text(case)
    assert len(want) == lay["total"]
    for a in (0, 1, 7, 15):  # the text's first byte at these addresses modulo 16: every chunk's range moves
        assert host_text(fo, case, lay, a) == want, a


def test_chunk_walk_on_a_long_contig(fo):
    case = FC.big_case(31, 60)
    lay = FC.layout(case)
    FC.check_preconditions(case, lay)
    assert host_text(fo, case, lay, 5) == FC.expected_text(case)


def test_zero_keep_text_holds_none_of_the_skipped_symbols():
    """the case's own point, shown on the expected text: the overlap symbols (code 5 -> 'R', in the RAW ones) never appear"""
    case = FC.zero_keep_case()
    t = FC.expected_text(case)
    body = b"".join(l for l in t.split(b"\n") if not l.startswith(b">"))
    n_r = sum(int((FC.contig_symbols(s, case["k"]) == 5).sum()) for _n, s in case["contigs"])
    assert body.count(b"R") == n_r


def test_layout_arithmetic(fo):
    assert bytes(fo.fo_letter(c) for c in range(16)) == b"ACGTNRYSWKMBDHVU"
    assert all(fo.fo_letter(c) == 32 for c in range(16, 256))
    for ll in (1, 2, 3, 16, 60, 80, 0):
        for n in (0, 1, 2, 59, 60, 61, 79, 80, 81, 160, 1285):
            L = ll or n
            lines = -(-n // L) if n else 0
            assert fo.fo_contig_text_bytes(9, n, ll) == 11 + n + lines
            is_end = []
            for t in range(n + lines):
                s = C.c_uint64()
                e = fo.fo_body_locate(t, n, ll, C.byref(s))
                is_end.append(e)
                if not e:
                    assert fo.fo_body_offset_of(s.value, n, ll) == t
            assert sum(is_end) == lines and (not n or is_end[-1])
            assert [fo.fo_body_offset_of(i, n, ll) for i in range(n)] == [t for t, e in enumerate(is_end) if not e]


def test_layout_arithmetic_beyond_4_gib(fo):
    """a human sample's text: offsets that do not fit 32 bits (synthetic -- no buffer of that size exists here)"""
    n = 5_000_000_123
    for ll in (80, 60, 1, 0):
        L = ll or n
        lines = -(-n // L)
        assert fo.fo_contig_text_bytes(300, n, ll) == 302 + n + lines
        for i in (0, 1, L - 1, L, (1 << 32) - 1, 1 << 32, (1 << 32) + L, n - 1):
            if i >= n:  # (one line: L is the symbol count itself)
                continue
            t = fo.fo_body_offset_of(i, n, ll)
            assert t == i + i // L
            s = C.c_uint64()
            assert fo.fo_body_locate(t, n, ll, C.byref(s)) == 0 and s.value == i
        s = C.c_uint64()
        assert fo.fo_body_locate(n + lines - 1, n, ll, C.byref(s)) == 1  # the last byte is a line end
    # chunks of a text of 5 GiB at every alignment: they tile it, all but the ends are whole
    total = 5 << 30
    for a in (0, 3, 15):
        nc = fo.fo_chunk_count(a, total)
        b, m = C.c_uint64(), C.c_uint32()
        fo.fo_chunk_range(0, a, total, C.byref(b), C.byref(m))
        assert (b.value, m.value) == (0, 16 - a)
        j = (1 << 28) + 5
        fo.fo_chunk_range(j, a, total, C.byref(b), C.byref(m))
        assert (b.value, m.value) == (16 * j - a, 16) and (b.value + a) % 16 == 0
        fo.fo_chunk_range(nc - 1, a, total, C.byref(b), C.byref(m))
        assert b.value + m.value == total and 0 < m.value <= 16


def test_chunk_walk_equals_the_plain_builder_on_random_plans(tmp_path):
    """the harness as a stand-alone program (its own main, never loaded into Python): seeded random plans, many segments that keep
    nothing, names and symbols of every byte value.  (Built with tests/fastaout_host/build.py: build_selftest(sanitize=True) the
    same program runs under AddressSanitizer + UBSan.)"""
    exe = fobuild.build_selftest(str(tmp_path / "fastaout_selftest"), sanitize=False)
    r = subprocess.run([exe, "3", "3000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok 3000 plans"), r.stdout + r.stderr
