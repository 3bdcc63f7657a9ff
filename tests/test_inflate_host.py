"""CPU: agc_amd/csrc/inflate.h compiled with g++ (tests/inflate_host) on every case of tests/inflate_cases.py -- every good member
equals zlib's bytes, every refused one gets its declared check and status with its good neighbours intact --, the walk's offsets
against Python integers, streams cut at member boundaries, and the stand-alone harness under -fsanitize=address,undefined against
zlib's inflate (a child process: no sanitizer touches anything loaded into Python)."""
import gzip
import zlib

import numpy as np
import pytest

from tests import inflate_cases as IC


@pytest.fixture(scope="module")
def run():
    return IC.host()


@pytest.fixture(scope="module")
def cases():
    out = IC.cases()
    out.update(IC.bgzf_host_streams())
    return out


def test_the_cases_are_what_they_claim(cases):
    """zlib reads every good member to its text; every check of the header's list has a case; the sizes and modes are there"""
    whys = set()
    for name, case in cases.items():
        for m, text, why in case:
            whys.add(why)
            if why == 0:
                assert gzip.decompress(m) == text, name
    assert whys == set(range(len(IC.WHY)))
    sizes = {len(t) for case in cases.values() for _m, t, w in case if w == 0}
    assert set(IC.SIZES) <= sizes
    assert len(cases["mixed_70_members"]) == 71 and len(cases["mixed_70_members_no_eof"]) == 70
    types = {(m[18] >> 1) & 3 for case in cases.values() for m, _t, w in case if w == 0 and len(m) > 26 and m[3] == 4 and m[10] == 6}
    assert types == {0, 1, 2}  # stored, fixed and dynamic first blocks


def test_every_case(run, cases):
    for name, case in cases.items():
        stream, rc, texts, statuses, whys, off = IC.expect(case)
        got_rc, got, got_off, got_st, got_why = run(stream)
        assert (got_rc, got_st) == (rc, statuses), name
        assert [IC.WHY[w] for w in got_why] == [IC.WHY[w] for w in whys], name
        assert np.array_equal(got_off, off), name
        if texts is not None:
            IC.same_text(got, texts, whys, off)
            if rc == 0:
                assert got == gzip.decompress(stream) if stream else got == b""


def test_zlib_refuses_or_agrees(cases):
    """whatever is refused zlib refuses as well -- but for the one stricter check, and for what gzip's framing checks, not inflate"""
    framing = {IC.W[k] for k in ("OUT_PAST", "OUT_SHORT", "LEFT_OVER", "CRC")}
    for name, case in cases.items():
        for m, _text, why in case:
            if why < IC.N_WALK or why in framing or name == "refused_incomplete_one_code":
                continue
            d = zlib.decompressobj(-15)
            payload = m[18:-8]
            try:
                d.decompress(payload)
                assert not d.eof, name
            except zlib.error:
                pass


def test_walk_offsets(run, cases):
    for name in ("mixed_70_members", "name_and_comment", "second_subfield_in_front_of_bc", "acgt80_level6"):
        case = cases[name]
        stream = b"".join(m for m, _t, _w in case)
        st, why, at, nm, tb, jobs, crcs = run.walk(stream)
        assert (st, why, at, nm, tb) == (0, 0, len(stream), len(case), sum(len(t) for _m, t, _w in case))
        p = o = 0
        for (m, t, _w), jb, crc in zip(case, jobs, crcs):
            assert stream[int(jb[0]):int(jb[0] + jb[2])] == m[int(jb[0]) - p:-8] and int(jb[0] + jb[2]) + 8 == p + len(m)
            assert zlib.decompress(stream[int(jb[0]):int(jb[0] + jb[2])], -15) == t
            assert (int(jb[1]), int(jb[3]), int(crc)) == (o, len(t), zlib.crc32(t))
            p += len(m)
            o += len(t)


def test_a_walk_complaint_names_the_member_and_the_byte(run, cases):
    case = cases["refused_isize_65537"]
    stream = b"".join(m for m, _t, _w in case)
    st, why, at, nm, tb, _jobs, _crcs = run.walk(stream)
    assert (st, IC.WHY[why], at, nm, tb) == (IC.MALFORMED, "ISIZE", len(case[0][0]), 1, len(case[0][1]))
    st, why, at, nm, _tb, _jobs, _crcs = run.walk(stream[:len(case[0][0])] + b"\x1f\x8b\x08")  # bytes left over behind the last member
    assert (st, IC.WHY[why], at, nm) == (IC.MALFORMED, "HEADER_TRUNCATED", len(case[0][0]), 1)
    assert run.walk(gzip.compress(b"ACGT"))[:2] == (IC.UNSUPPORTED, IC.W["NO_BC"])


def test_a_stream_cut_at_member_boundaries_is_a_stream(run, cases):
    case = cases["mixed_70_members"]
    ends = np.cumsum([0] + [len(m) for m, _t, _w in case])
    texts = [t for _m, t, _w in case]
    stream = b"".join(m for m, _t, _w in case)
    for a, b in ((0, 1), (0, 70), (3, 9), (17, 18), (40, 71), (70, 71), (5, 5)):
        rc, got, off, st, _why = run(stream[ends[a]:ends[b]])
        assert rc == 0 and got == b"".join(texts[a:b]) and st == [0] * (b - a) and len(off) == b - a + 1
    rc, _got, _off, st, why = run(stream[ends[3]:ends[9] - 1])  # not a boundary
    assert rc == IC.EINVAL and st[-1] == IC.MALFORMED and IC.WHY[why[-1]] == "BSIZE_PAST"


def test_capacity(run, cases):
    stream, _rc, texts, _st, _whys, _off = IC.expect(cases["acgt80_level1"])
    need = sum(len(t) for t in texts)
    assert run(stream, cap=need - 1)[0] == IC.ECAP
    assert run(stream, cap=need)[1] == b"".join(texts)


def test_the_fast_memory_is_small():
    """four waves to a workgroup at under 4 KB each: the LDS does not limit the occupancy"""
    import ctypes
    from tests.inflate_host import build as ib
    assert ctypes.CDLL(ib.build()).inflate_host_work_bytes() == 3932


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_selftest_under_sanitizers(seed):
    from tests.inflate_host import build as ib
    r = ib.run_selftest(seed, 400)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    ok, refused = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert ok >= 100 and refused >= 200  # about two thirds are damaged, and most damage is noticed
