"""CPU: the plan of a sample (libagc_read.so: agc_get_sample_plan, agc_amd/reader.py: GetSamplePlan) reassembled in numpy -- the
deltas through the oracle's decode, then orientation, the k-symbol overlap, the alphabet and the line wrapping -- must give the
text the host reader itself writes, byte for byte.  Archives: the committed reference-built toy archive, and the one the host
pipeline writes for syn_mixed (tests/test_host_devsim.py's path: the host sources against the CPU device stand-in)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import collections as COLL
from tests import fastaout_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY_AGC = os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc")


@pytest.fixture(scope="module")
def rd():
    from agc_amd import build, reader
    build.build_read()
    return reader


@pytest.fixture(scope="module")
def mixed_agc(tmp_path_factory):
    """syn_mixed (N-runs, IUPAC codes, indels; a contig too short for a splitter) written by the host pipeline"""
    import subprocess
    from tests.devsim import build as simbuild
    cli = simbuild.build()
    d = tmp_path_factory.mktemp("plan_mixed")
    args, _ = COLL.CONFIGS["syn_mixed"]
    out = str(d / "mixed.agc")
    r = subprocess.run([cli, "create"] + args + ["-t", "4", "-o", out] + COLL.build("syn_mixed", str(d / "in")), capture_output=True, text=True, timeout=300)
    assert os.path.exists(out), r.stderr[-2000:]
    return out


def assemble(plan, k, mml, oracle, line_length):
    """the plan's text, the slow and plain way; also checks every segment's declared length against its decoded size"""
    refs = {int(g): plan["ref_bytes"][int(plan["ref_off"][i]):int(plan["ref_off"][i + 1])] for i, g in enumerate(plan["groups"])}
    out = []
    for c in range(plan["ctg_seg"].size - 1):
        parts = []
        for s in range(int(plan["ctg_seg"][c]), int(plan["ctg_seg"][c + 1])):
            kind, g = int(plan["kind"][s]), int(plan["group_id"][s])
            b = plan["bytes"][int(plan["off"][s]):int(plan["off"][s]) + int(plan["seg_bytes"][s])]
            assert kind == (0 if g < 16 else 1 if plan["in_group_id"][s] == 0 else 2)
            if kind == 0:
                sym = b
            elif kind == 1:
                sym = refs[g]
            else:
                sym, n = oracle.LZ(refs[g], mml).decode(b, int(plan["length"][s]) + 64)
                assert n == sym.size
            assert sym.size == int(plan["length"][s]), (c, s, kind)
            if plan["rc"][s]:
                sym = FC.rev_comp(sym)
            assert not parts or sym.size >= k
            parts.append(sym if not parts else sym[k:])
        name = plan["names"][int(plan["name_off"][c]):int(plan["name_off"][c + 1])]
        out.append(FC.contig_text(name, np.concatenate(parts + [np.zeros(0, np.uint8)]), line_length))
    return b"".join(out)


def check_archive(rd, oracle, path):
    a = rd.CAGCFile()
    assert a.Open(path)
    prm = a.GetParams()
    samples = a.ListSample()
    assert samples
    kinds = set()
    for s in samples:
        plan = a.GetSamplePlan(s)
        assert plan is not None
        assert plan["names"] == "".join(a.ListCtg(s)).encode() and plan["ctg_seg"].size == a.NCtg(s) + 1
        assert np.all(np.diff(plan["groups"].astype(np.int64)) > 0) and (plan["groups"] >= 16).all()
        assert set(plan["group_id"][plan["kind"] != 0].tolist()) == set(plan["groups"].tolist())
        kinds |= set(plan["kind"].tolist())
        for ll in (80, 1, 0):
            assert assemble(plan, prm["k"], prm["min_match_len"], oracle, ll) == a.GetSampleFasta(s, ll), (s, ll)
    assert a.GetSamplePlan("no such sample") is None
    assert a.Close()
    return kinds


def test_toy_archive_plans(rd, oracle):
    assert 0 in check_archive(rd, oracle, TOY_AGC)  # (contigs without a splitter: raw groups)


def test_mixed_archive_plans(rd, oracle, mixed_agc):
    assert check_archive(rd, oracle, mixed_agc) >= {1, 2}  # references as they are, deltas


def test_null_handles(rd):
    L = rd.load()
    a = rd.CAGCFile()
    assert a.Open(TOY_AGC)
    assert not L.agc_get_sample_plan(a.h, b"no such sample")
    assert not L.agc_get_sample_plan(None, b"ref") and not L.agc_get_sample_plan(a.h, None)
    assert L.agc_plan_destroy(None) == 0
    v = rd.PlanView()
    assert L.agc_plan_fields(None, C.byref(v)) != 0
    h = L.agc_get_sample_plan(a.h, b"ref")
    assert h and L.agc_plan_fields(h, None) != 0 and L.agc_plan_fields(h, C.byref(v)) == 0
    assert v.n_ctg == a.NCtg("ref") and v.n_seg >= v.n_ctg
    assert L.agc_plan_destroy(h) == 0
    assert a.Close()
