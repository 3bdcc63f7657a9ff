"""CPU: agc_amd/csrc/fasta_out.h compiled for the host (tests/fastaout_host) -- the layout arithmetic, and the text kernel's
per-chunk walk run chunk after chunk over whole buffers -- against text built independently in numpy (tests/fastaout_cases.py:
the plans tests/test_gpu_fasta_out.py sends through the device).  And agc_amd/csrc/fasta_plan.h, the host arithmetic of
agc_hip_sample_fasta: the layout it gives those plans against the one fastaout_cases lays by hand, its refusals, its packed block."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from agc_amd import capi
from tests import fastaout_cases as FC
from tests.fastaout_host import build as fobuild

u8p, u32p, u64p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
GID0 = 100  # the cases' references are groups 100, 101, ...: the groups below have none


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
    plan = [C.c_uint32, u64p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]  # n_ctg, ctg_seg, segs, n_bytes, k, line_length
    L.fp_layout.argtypes = plan + [u64p, i64p, C.c_uint32, u64p, u64p, u64p, u64p, u32p, u64p, u64p, u64p, C.c_char_p, C.c_uint32]
    L.fp_pack.argtypes = plan + [C.c_char_p, u64p, i64p, C.c_uint32, u8p, u64p]
    L.fp_pack.restype = C.c_uint64
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


# ---- fasta_plan.h: what agc_hip_sample_fasta computes on the host -----------------------------------------------------------------
def ref_table(case):
    return np.array([-1] * GID0 + [r.size for r in case["refs"]], np.int64)


def _plan(args):
    ctg_seg, segs, blob, k, ll, _names, _name_off = args
    return [ctg_seg.size - 1, ctg_seg.ctypes.data_as(u64p), segs.ctypes.data_as(C.c_void_p), blob.size, k, ll]


def host_layout(fo, args, refs):
    """fp::lay_out_sample of the arguments of Context.sample_fasta -> (code, message, its fields)"""
    ctg_seg, segs, _blob, _k, _ll, _names, name_off = args
    n_ctg, n_seg = ctg_seg.size - 1, segs.size
    o = {"ctg_text": np.full(n_ctg + 1, 0xAA, np.uint64), "ctg_sym": np.full(n_ctg, 0xAA, np.uint64), "seg_start": np.full(n_seg, 0xAA, np.uint64),
         "seg_off": np.full(n_seg, 0xAA, np.uint64), "skip": np.full(n_seg, 0xAA, np.uint32)}
    dj, cj, sizes, why = np.zeros((n_seg, 7), np.uint64), np.zeros((n_seg, 6), np.uint64), np.zeros(4, np.uint64), C.create_string_buffer(400)
    code = fo.fp_layout(*_plan(args), name_off.ctypes.data_as(u64p), refs.ctypes.data_as(i64p), refs.size, *(o[f].ctypes.data_as(u32p if f == "skip" else u64p) for f in o),
                        dj.ctypes.data_as(u64p), cj.ctypes.data_as(u64p), sizes.ctypes.data_as(u64p), why, 400)
    o.update(dj=dj[:int(sizes[0])], cj=cj[:int(sizes[1])], sym_total=int(sizes[2]), total=int(sizes[3]))
    return code, why.value.decode(), o


def plan_text_size(args):
    """the text's size by fastaout_cases' arithmetic, from the plan's declared lengths (a segment shorter than the overlap keeps nothing)"""
    ctg_seg, segs, _blob, k, ll, _names, name_off = args
    tot = 0
    for c in range(ctg_seg.size - 1):
        a, b = int(ctg_seg[c]), int(ctg_seg[c + 1])
        n_sym = sum(max(int(segs["length"][s]) - (k if s > a else 0), 0) for s in range(a, b))
        tot += FC.contig_text_size(int(name_off[c + 1] - name_off[c]), n_sym, ll)
    return tot


@pytest.mark.parametrize("case", FC.small_cases(), ids=lambda c: c["name"])
def test_product_layout_is_the_cases_layout(fo, oracle, case):
    lay = FC.layout(case)
    args = FC.plan_arrays(case, GID0, oracle)
    ctg_seg, segs = args[0], args[1]
    assert np.array_equal(ctg_seg, lay["ctg_seg"]) and np.array_equal(args[6], lay["name_off"])
    code, why, got = host_layout(fo, args, ref_table(case))
    assert (code, why) == (capi.OK, "")
    for f in ("ctg_text", "ctg_sym", "seg_start", "seg_off", "skip"):
        assert got[f].dtype == lay[f].dtype and np.array_equal(got[f], lay[f]), f
    assert got["total"] == lay["total"] == plan_text_size(args) and got["sym_total"] == lay["sym"].size
    # the jobs: every DELTA segment is decoded, every other one that has symbols is copied, to where the layout puts the segment
    want_dj = [(i, s["off"], s["n_bytes"], lay["seg_off"][i], s["length"], s["gid"], s["rc"]) for i, s in enumerate(segs) if s["kind"] == capi.SEG_DELTA]
    want_cj = [(s["off"], lay["seg_off"][i], s["length"], s["gid"], s["rc"], int(s["kind"] == capi.SEG_REF)) for i, s in enumerate(segs)
               if s["kind"] != capi.SEG_DELTA and s["length"]]
    assert got["dj"].tolist() == [[int(x) for x in r] for r in want_dj]
    assert got["cj"].tolist() == [[int(x) for x in r] for r in want_cj]
    assert len(want_dj) == sum(s["kind"] == FC.DELTA for _n, ss in case["contigs"] for s in ss)


def test_host_refusals(fo, oracle):
    """the refusals of test_gpu_fasta_out.py: test_refusals_leave_the_text_untouched that the host decides alone: code, a message
    that names the segment, and the text's size all the same -- every segment is laid out, also behind the complaint"""
    case = FC.kinds_case()
    args = FC.plan_arrays(case, GID0, oracle)
    refs = ref_table(case)
    ctg_seg, segs, blob, k, ll, names, name_off = args
    good = host_layout(fo, args, refs)[2]
    assert good["total"] == len(FC.expected_text(case))
    d_idx = [i for i, s in enumerate(segs) if s["kind"] == capi.SEG_DELTA]
    r_idx = [i for i, s in enumerate(segs) if s["kind"] == capi.SEG_REF]
    w_idx = [i for i, s in enumerate(segs) if s["kind"] == capi.SEG_RAW and i not in ctg_seg.tolist()]
    d0, r0, w0 = d_idx[0], r_idx[0], w_idx[0]

    def changed(i, **kw):
        s2 = segs.copy()
        for f, v in kw.items():
            s2[f][i] = v
        return i, (ctg_seg, s2, blob, k, ll, names, name_off)

    bad = [
        ("reference of another size", capi.EINVAL, changed(r0, length=int(segs["length"][r0]) - 1)),
        ("raw byte count", capi.EINVAL, changed(w0, n_bytes=int(segs["n_bytes"][w0]) - 1)),
        ("shorter than the overlap", capi.EINVAL, changed(w0, n_bytes=k - 1, length=k - 1)),
        ("unknown kind", capi.EINVAL, changed(d0, kind=3)),
        ("bytes past the buffer", capi.EINVAL, changed(d0, off=blob.size - 1)),
        ("offset past the buffer", capi.EINVAL, changed(w0, off=blob.size + 1)),
        ("unregistered group of a delta", capi.ENOREF, changed(d0, gid=7)),
        ("unregistered group of a reference", capi.ENOREF, changed(r0, gid=1 << 30)),
    ]
    for what, code, (i, a) in bad:
        got_code, why, got = host_layout(fo, a, refs)
        ci = int(np.searchsorted(ctg_seg, i, side="right")) - 1
        assert got_code == code, what
        assert f"sample_fasta: segment {i} (contig {ci}) " in why, (what, why)
        assert got["total"] == plan_text_size(a), what
        assert (got["total"] == good["total"]) == (int(a[1]["length"][i]) == int(segs["length"][i])), what  # (a changed length moves the size)
        # the refused segment gets no job; every other segment keeps its own
        n_jobs = len(got["dj"]) + len(got["cj"])
        assert n_jobs == len(good["dj"]) + len(good["cj"]) - 1 and i not in got["dj"][:, 0].tolist(), what
    # two complaints: the first one is reported
    s2 = changed(d0, kind=3)[1][1]
    s2["gid"][r0] = 7
    code, why, _got = host_layout(fo, (ctg_seg, s2, blob, k, ll, names, name_off), refs)
    assert min(d0, r0) == r0 and code == capi.ENOREF and f"segment {r0} " in why
    # ranges or name offsets that do not ascend from 0: refused before any segment is looked at -- the arrays stay as they were and
    # the size stays 0 (what agc_hip_sample_fasta reports then)
    up, down, names_down = ctg_seg.copy(), ctg_seg.copy(), name_off.copy()
    up[0] = 1
    down[1] = down[2] + 1
    names_down[1] = names_down[2] + 1
    for a in ((up, segs, blob, k, ll, names, name_off), (down, segs, blob, k, ll, names, name_off), (ctg_seg, segs, blob, k, ll, names, names_down)):
        code, why, got = host_layout(fo, a, refs)
        assert code == capi.EINVAL and "segment ranges or name offsets do not ascend" in why
        assert got["total"] == 0 and not len(got["dj"]) and not len(got["cj"]) and (got["seg_off"] == 0xAA).all() and (got["ctg_text"] == 0xAA).all()


def _raw_plan(contigs, prefix=b""):
    """(name, [segment lengths]) per contig, all RAW -> the arguments of Context.sample_fasta; the names lie behind `prefix`"""
    segs, ctg_seg, name_off, n = [], [0], [len(prefix)], 0
    for name, lens in contigs:
        for ln in lens:
            segs.append((capi.SEG_RAW, 0, n, ln, ln, 0, 0))
            n += ln
        ctg_seg.append(len(segs))
        name_off.append(name_off[-1] + len(name))
    return (np.array(ctg_seg, np.uint64), np.array(segs, capi.SEG_SRC_DTYPE), np.zeros(n, np.uint8), 5, 7, prefix + b"".join(nm for nm, _l in contigs),
            np.array(name_off, np.uint64))


def packed_plans(oracle):
    kinds = FC.kinds_case()
    return [("kinds", FC.plan_arrays(kinds, GID0, oracle), ref_table(kinds)),
            ("no segment", _raw_plan([(b"a", []), (b"bc", [])]), np.zeros(0, np.int64)),
            ("empty names", _raw_plan([(b"", [9, 5, 30]), (b"", []), (b"", [1])]), np.zeros(0, np.int64)),
            ("names behind a prefix", _raw_plan([(b"first", [40]), (b"", [6, 5]), (b"third one", [])], b"not a name: "), np.zeros(0, np.int64))]


def test_packed_block_gives_every_array_back(fo, oracle):
    """fp::pack_text_plan: through the offsets it returns, the block holds each array of the text kernel's plan, back to back"""
    seen = set()
    for what, args, refs in packed_plans(oracle):
        ctg_seg, segs, _blob, _k, _ll, names, name_off = args
        code, _why, lay = host_layout(fo, args, refs)
        assert code == capi.OK, what
        call = _plan(args) + [names, name_off.ctypes.data_as(u64p), refs.ctypes.data_as(i64p), refs.size]
        at = np.zeros(8, np.uint64)
        size = fo.fp_pack(*call, None, at.ctypes.data_as(u64p))
        block = np.full(size + 16, 0xAA, np.uint8)
        assert fo.fp_pack(*call, block.ctypes.data_as(u8p), at.ctypes.data_as(u64p)) == size and (block[size:] == 0xAA).all()
        n0 = int(name_off[0])
        fields = [lay["ctg_text"], ctg_seg, lay["ctg_sym"], name_off - name_off[0], lay["seg_start"], lay["seg_off"], lay["skip"],
                  np.frombuffer(names[n0:int(name_off[-1])], np.uint8)]
        end = 0
        for o, f in zip(at.tolist(), fields):
            assert o == end and block[o:o + f.nbytes].tobytes() == f.tobytes(), what
            end += f.nbytes
        assert end == size, what
        seen |= {w for w, c in (("n_seg 0", segs.size == 0), ("no names", name_off[-1] == n0), ("rebased", n0 > 0 and name_off[-1] > n0)) if c}
    assert seen == {"n_seg 0", "no names", "rebased"}
