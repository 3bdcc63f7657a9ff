"""CPU: the windows and stored parts of a batch of contig ranges (libagc_read.so: agc_get_range_parts, agc_amd/reader.py:
GetRangeParts; the arithmetic: agc_amd/csrc/range_plan.h).  Every query is reassembled in numpy from the decoded segments of the
sample's plan (GetSamplePlan) and the windows the call returns, and must be what GetCtgSeq gives for the same range.  Archives: the
committed reference-built toy archive, and syn_mixed written through the device stand-in (the fixtures of test_read_plan_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import fastaout_cases as FC
from tests import ranges_cases as RC
from tests import readfuzz_cases as RF
from tests.test_read_plan_cpu import TOY_AGC, mixed_agc, rd  # noqa: F401  (fixtures)

ALPHA = np.frombuffer(b"ACGTNRYSWKMBDHVU", np.uint8)


def oriented_segments(plan, mml, oracle):
    """every segment of the plan decoded and oriented, as the contig is stitched from them"""
    refs = {int(g): plan["ref_bytes"][int(plan["ref_off"][i]):int(plan["ref_off"][i + 1])] for i, g in enumerate(plan["groups"])}
    out = []
    for s in range(plan["kind"].size):
        kind, g = int(plan["kind"][s]), int(plan["group_id"][s])
        b = plan["bytes"][int(plan["off"][s]):int(plan["off"][s]) + int(plan["seg_bytes"][s])]
        sym = b if kind == 0 else refs[g] if kind == 1 else oracle.LZ(refs[g], mml).decode(b, int(plan["length"][s]) + 64)[0]
        assert sym.size == plan["length"][s]
        out.append(FC.rev_comp(sym) if plan["rc"][s] else sym)
    return out


def check_archive(rd, oracle, path):
    a = rd.CAGCFile()
    assert a.Open(path)
    prm = a.GetParams()
    k = prm["k"]
    n_boundaries = 0
    for s in a.ListSample():
        plan = a.GetSamplePlan(s)
        segs = oriented_segments(plan, prm["min_match_len"], oracle)
        key = {}  # (group, in-group id) -> the segment: what a window entry names
        for i in range(plan["kind"].size):
            key[(int(plan["group_id"][i]), int(plan["in_group_id"][i]), int(plan["rc"][i]))] = segs[i]
        names = a.ListCtg(s)
        queries = []
        # a name finds the first contig that has it: the later copy of a repeated name (a contig of no segments where the writer
        # placed its pieces under the first) has no query of its own, and the first copy's length is the one the name must give
        for c in RF.addressable(names):
            name = names[c]
            lo, hi = int(plan["ctg_seg"][c]), int(plan["ctg_seg"][c + 1])
            lens = plan["length"][lo:hi].tolist()
            n_boundaries += len(lens) - 1
            assert lens and a.GetCtgLen(s, name) == sum(lens) - k * (len(lens) - 1)
            queries += [(s, name, f, t) for f, t in RC.contig_ranges(lens, k)]
        r = a.GetRangeParts(queries)
        assert r["q_seg"].size == len(queries) + 1 and r["q_len"].size == len(queries) and r["q_seg"][0] == 0
        assert (r["win_len"] >= 1).all() and (r["win_from"] + r["win_len"] <= r["length"]).all()
        for q, (_s, name, f, t) in enumerate(queries):
            want = a.GetCtgSeq(s, name, f, t).encode()
            got = []
            for w in range(int(r["q_seg"][q]), int(r["q_seg"][q + 1])):
                seg = key[(int(r["group_id"][w]), int(r["in_group_id"][w]), int(r["rc"][w]))]
                assert seg.size == r["length"][w]
                assert r["kind"][w] == (0 if r["group_id"][w] < 16 else 1 if r["in_group_id"][w] == 0 else 2)
                got.append(seg[int(r["win_from"][w]):int(r["win_from"][w]) + int(r["win_len"][w])])
            got = ALPHA[np.concatenate(got + [np.zeros(0, np.uint8)])].tobytes()
            assert got == want and r["q_len"][q] == len(want), (s, name, f, t)
        # the first entry of a query may start anywhere; every later one starts behind the overlap
        first = np.zeros(r["kind"].size, bool)
        first[r["q_seg"][:-1][np.diff(r["q_seg"].astype(np.int64)) > 0].astype(np.int64)] = True
        assert (r["win_from"][~first] >= k).all()
        # the parts: those of the sample's own list that a window names, in its order
        whole = a.GetSampleParts(s)
        sub = set(zip(r["part_content"].tolist(), r["part_group"].tolist(), r["part_no"].tolist()))
        all_ = list(zip(whole["part_content"].tolist(), whole["part_group"].tolist(), whole["part_no"].tolist()))
        assert len(sub) == r["part_off"].size and [p for p in all_ if p in sub] == list(zip(r["part_content"].tolist(), r["part_group"].tolist(), r["part_no"].tolist()))
        is_ref = r["part_content"] != rd.PART_PACK
        assert set(r["part_group"][is_ref].tolist()) == set(r["group_id"][r["kind"] != rd.PLAN_RAW].tolist())
        for w in np.flatnonzero(r["kind"] != rd.PLAN_REF):
            pi = int(r["seg_part"][w])
            idx = int(r["in_group_id"][w]) - (r["kind"][w] == rd.PLAN_DELTA)
            assert (r["part_content"][pi], r["part_group"][pi], r["part_no"][pi], r["seg_index"][w]) == (
                rd.PART_PACK, r["group_id"][w], idx // prm["pack_cardinality"], idx % prm["pack_cardinality"])
        # have_groups removes exactly those references
        groups = sorted(set(r["part_group"][is_ref].tolist()))
        some = groups[::2]
        again = a.GetRangeParts(queries, have=some)
        ref2 = again["part_content"] != rd.PART_PACK
        assert again["part_group"][ref2].tolist() == [g for g in groups if g not in some]
        assert np.array_equal(again["part_off"][~ref2], r["part_off"][~is_ref]) and np.array_equal(again["win_from"], r["win_from"])
    assert a.Close()
    return n_boundaries


def test_toy_archive_ranges(rd, oracle):  # noqa: F811
    check_archive(rd, oracle, TOY_AGC)


def test_mixed_archive_ranges(rd, oracle, mixed_agc):  # noqa: F811
    assert check_archive(rd, oracle, mixed_agc) > 0  # contigs of several segments: the boundary ranges are there


def test_two_queries_in_one_segment_list_its_pack_once(rd, mixed_agc):  # noqa: F811
    a = rd.CAGCFile()
    assert a.Open(mixed_agc)
    k = a.GetParams()["k"]
    # a delta segment that keeps 40 symbols or more, and where its contig has them
    long_delta = lambda p: np.flatnonzero((p["kind"] == rd.PLAN_DELTA) & (p["length"] >= k + 40))  # noqa: E731
    s = [x for x in a.ListSample() if long_delta(a.GetSampleParts(x)).size][0]
    whole = a.GetSampleParts(s)
    g = int(long_delta(whole)[0])
    c = int(np.searchsorted(whole["ctg_seg"], g, side="right")) - 1
    first = int(whole["ctg_seg"][c])
    b = int(whole["length"][first:g].sum()) - k * (g - first) + (k if g > first else 0)
    name = a.ListCtg(s)[c]
    r = a.GetRangeParts([(s, name, b + 1, b + 10), (s, name, b + 20, b + 39)])
    assert r["q_len"].tolist() == [10, 20] and r["q_seg"].tolist() == [0, 1, 2]
    assert r["kind"].tolist() == [rd.PLAN_DELTA] * 2 and r["group_id"][0] == r["group_id"][1] and r["in_group_id"][0] == r["in_group_id"][1]
    assert (r["win_from"][1] - r["win_from"][0], r["win_len"].tolist()) == (19, [10, 20])
    assert r["part_content"].tolist() == [r["part_content"][0], rd.PART_PACK] and r["part_content"][0] != rd.PART_PACK  # its reference, its pack: each once
    assert r["seg_part"].tolist() == [1, 1]
    assert a.Close()


def test_an_empty_batch_and_empty_ranges(rd):  # noqa: F811
    a = rd.CAGCFile()
    assert a.Open(TOY_AGC)
    r = a.GetRangeParts([])
    assert r["q_seg"].tolist() == [0] and r["q_len"].size == 0 and r["kind"].size == 0 and r["part_off"].size == 0
    s = a.ListSample()[0]
    name = a.ListCtg(s)[0]
    n = a.GetCtgLen(s, name)
    r = a.GetRangeParts([(s, name, n, n + 4), (s, name, n + 7, -1)])
    assert r["q_seg"].tolist() == [0, 0, 0] and r["q_len"].tolist() == [0, 0] and r["part_off"].size == 0
    assert a.Close()


def test_unknown_and_ambiguous_contigs(rd):  # noqa: F811
    a = rd.CAGCFile()
    assert a.Open(TOY_AGC)
    samples = a.ListSample()
    s = samples[0]
    name = a.ListCtg(s)[0]
    good = (s, name, 0, 3)
    for at, bad in ((1, (s, "no such contig", 0, 3)), (2, ("no such sample", name, 0, 3)), (0, (s, "no such contig", 0, 3))):
        qs = [good, good, good]
        qs[at] = bad
        with pytest.raises(KeyError) as e:
            a.GetRangeParts(qs)
        assert e.value.args[0] == at
    # a short name two samples have, without a sample
    short = {}
    for smp in samples:
        for c in a.ListCtg(smp):
            short.setdefault(c.split()[0], set()).add(smp)
    twice = sorted(n for n, ss in short.items() if len(ss) > 1)
    once = sorted(n for n, ss in short.items() if len(ss) == 1)
    assert twice and once, "the toy archive has a contig name in two samples and one in a single sample"
    assert a.GetCtgLen("", twice[0]) == -2
    with pytest.raises(KeyError) as e:
        a.GetRangeParts([good, (None, once[0], 0, 3), (None, twice[0], 0, 3)])
    assert e.value.args[0] == 2
    r = a.GetRangeParts([(None, once[0], 0, 3), ("", once[0], 1, 2)])  # unique: found without a sample
    assert r["q_len"].tolist() == [4, 2]
    # the C entry point itself: NULL and bad_query
    L = rd.load()
    bad = C.c_int64(7)
    names = (C.c_char_p * 1)(b"no such contig")
    z = (C.c_int64 * 1)(0)
    assert not L.agc_get_range_parts(a.h, 1, None, names, z, z, None, 0, C.byref(bad)) and bad.value == 0
    assert not L.agc_get_range_parts(a.h, 1, None, names, z, z, None, 0, None)
    assert not L.agc_get_range_parts(None, 0, None, None, None, None, None, 0, C.byref(bad)) and bad.value == -1
    assert not L.agc_get_range_parts(a.h, 1, None, None, z, z, None, 0, None)
    assert not L.agc_get_range_parts(a.h, 0, None, None, None, None, None, 2, None)  # a count without the groups
    assert L.agc_ranges_destroy(None) == 0 and L.agc_ranges_fields(None, None) != 0
    assert a.Close()
