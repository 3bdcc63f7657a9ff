"""CPU: the stored parts of a sample (libagc_read.so: agc_get_sample_parts, agc_amd/reader.py: GetSampleParts) decoded the plain way --
libzstd, the numpy tuple routine, a cut at every 0xFF -- must give, segment by segment and reference by reference, what the plan of
the same sample (GetSamplePlan, which the reader decodes itself) holds.  And every zstd part goes through the CPU build of the GPU's
decoder (tests/zsdec_host): the GPU tests of tests/test_gpu_sample_parts.py rest on none of them being refused.  Archives: the
committed reference-built toy archive, and syn_mixed written through the device stand-in (the fixtures of test_read_plan_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import partsunpack_cases as PC
from tests import zsdec_cases as zd
from tests.test_read_plan_cpu import TOY_AGC, mixed_agc, rd  # noqa: F401  (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unzstd(frame):
    Z = zd._z()
    Z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    n = Z.ZSTD_getFrameContentSize(bytes(frame), len(frame))
    assert n < 1 << 31, "a frame without a content size"
    out = zd.ref_decode(frame, n)
    assert out is not None and len(out) == n
    return out


def decoded_parts(rd, parts, gpu_decoder):
    """every part's final bytes: a pack's decoded bytes, a reference's symbols"""
    out = []
    for i in range(parts["part_off"].size):
        b = parts["part"](i)
        assert len(b) == parts["part_bytes"][i]
        if parts["part_coding"][i] == rd.PART_ZSTD:
            st, ours = gpu_decoder(b)
            assert st == 0, (i, st)  # the decoder the GPU runs refuses none of the archive's frames
            b = unzstd(b)
            assert ours == b
        else:
            assert parts["part_coding"][i] == rd.PART_STORED
        if parts["part_content"][i] == rd.PART_REF_TUPLES:
            b = PC.symbols_of(b)
            assert b is not None
            b = b.tobytes()
        out.append(b)
    return out


def check_archive(rd, path, gpu_decoder):
    a = rd.CAGCFile()
    assert a.Open(path)
    pack_card = a.GetParams()["pack_cardinality"]
    seen = set()
    for s in a.ListSample():
        plan, parts = a.GetSamplePlan(s), a.GetSampleParts(s)
        assert plan is not None and parts is not None
        assert parts["names"] == plan["names"]
        for f in ("name_off", "ctg_seg", "group_id", "in_group_id", "rc", "kind", "length"):
            assert np.array_equal(parts[f], plan[f]), (s, f)  # (length: the collection's raw_length is what the segments decode to)
        is_ref = parts["part_content"] != rd.PART_PACK
        # the references: the plan's groups, ascending, in front of the packs; then the distinct packs
        assert np.array_equal(parts["part_group"][is_ref], plan["groups"]) and not is_ref[int(is_ref.sum()):].any()
        keys = list(zip(parts["part_group"][~is_ref].tolist(), parts["part_no"][~is_ref].tolist()))
        assert keys == sorted(set(keys))
        final = decoded_parts(rd, parts, gpu_decoder)
        n_ref = int(is_ref.sum())
        for i in range(n_ref):
            assert final[i] == plan["ref_bytes"][int(plan["ref_off"][i]):int(plan["ref_off"][i + 1])].tobytes(), (s, i)
        cut = {i: PC.pack_sequences(final[i]) for i in range(n_ref, len(final))}
        for g in range(parts["kind"].size):
            if parts["kind"][g] == rd.PLAN_REF:
                continue
            pi, qi = int(parts["seg_part"][g]), int(parts["seg_index"][g])
            idx = int(parts["in_group_id"][g]) - (parts["kind"][g] == rd.PLAN_DELTA)
            assert (parts["part_group"][pi], parts["part_no"][pi], qi) == (parts["group_id"][g], idx // pack_card, idx % pack_card)
            assert qi < len(cut[pi]) <= pack_card
            assert cut[pi][qi] == plan["bytes"][int(plan["off"][g]):int(plan["off"][g]) + int(plan["seg_bytes"][g])].tobytes(), (s, g)
        seen |= {(int(c), int(t)) for c, t in zip(parts["part_coding"], parts["part_content"])}
        # with every group at hand no reference part is handed out, and the packs are the same
        again = a.GetSampleParts(s, have=plan["groups"].tolist())
        assert (again["part_content"] == rd.PART_PACK).all()
        assert np.array_equal(again["part_off"], parts["part_off"][~is_ref]) and np.array_equal(again["seg_index"], parts["seg_index"])
        assert np.array_equal(again["seg_part"][parts["kind"] != rd.PLAN_REF] + n_ref, parts["seg_part"][parts["kind"] != rd.PLAN_REF])
        some = plan["groups"].tolist()[::2]
        assert a.GetSampleParts(s, have=some)["part_group"][:n_ref - len(some)].tolist() == [g for g in plan["groups"].tolist() if g not in some]
    assert a.GetSampleParts("no such sample") is None
    assert a.Close()
    return seen


@pytest.fixture(scope="module")
def gpu_decoder():
    return zd.host_decoder()


def test_toy_archive_parts(rd, gpu_decoder):  # noqa: F811
    seen = check_archive(rd, TOY_AGC, gpu_decoder)
    assert (rd.PART_ZSTD, rd.PART_PACK) in seen  # (contigs without a splitter: raw groups, packs alone)


def test_mixed_archive_parts(rd, gpu_decoder, mixed_agc):  # noqa: F811
    seen = check_archive(rd, mixed_agc, gpu_decoder)
    print(sorted(seen))
    assert (rd.PART_ZSTD, rd.PART_PACK) in seen and (rd.PART_ZSTD, rd.PART_REF_TUPLES) in seen


def test_null_handles(rd):  # noqa: F811
    L = rd.load()
    a = rd.CAGCFile()
    assert a.Open(TOY_AGC)
    assert not L.agc_get_sample_parts(a.h, b"no such sample", None, 0)
    assert not L.agc_get_sample_parts(None, b"ref", None, 0) and not L.agc_get_sample_parts(a.h, None, None, 0)
    assert not L.agc_get_sample_parts(a.h, b"ref", None, 3)  # a count without the groups
    assert L.agc_parts_destroy(None) == 0
    v = rd.PartsView()
    assert L.agc_parts_fields(None, C.byref(v)) != 0
    h = L.agc_get_sample_parts(a.h, b"ref", None, 0)
    assert h and L.agc_parts_fields(h, None) != 0 and L.agc_parts_fields(h, C.byref(v)) == 0
    assert v.n_ctg == a.NCtg("ref") and v.n_seg >= v.n_ctg and v.n_parts >= 1 and v.src_bytes == os.path.getsize(TOY_AGC)
    assert L.agc_parts_destroy(h) == 0
    assert a.Close()
