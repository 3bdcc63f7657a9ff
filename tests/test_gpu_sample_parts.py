"""GPU: agc_hip_parts_unpack / _dev (parts_unpack_kernels.hip behind the zstd decode stage) on the shapes of
tests/partsunpack_cases.py against their numpy restatements; its per-part refusals; agc_amd/devread.py:
DeviceReader.sample_fasta_parts / _dev against the host reader on the toy archive and on archives written on the spot; and the
contract of agc_hip_sample_fasta_parts -- what a failed call leaves registered and written: nothing.  A context of its own."""
import os
import subprocess

import numpy as np
import pytest

from agc_amd import capi
from tests import collections as COLL
from tests import partsunpack_cases as PC
from tests import zstd_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")
TOY_AGC = os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc")
FILL = 0xABABABAB


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def batch(items):
    """[(coding, content, bytes)] -> (PART_DTYPE array, the source buffer: the parts back to back behind 3 bytes of something else)"""
    parts, src = np.zeros(len(items), capi.PART_DTYPE), bytearray(b"\x01\x02\x03")
    for i, (coding, content, b) in enumerate(items):
        parts[i] = (len(src), len(b), coding, content, 0)
        src += bytes(b)
    return parts, bytes(src)


def shape_items():
    """every pack and tuple shape, stored and as frames of libzstd at the archive's levels -> [(coding, content, stored bytes, final bytes)]"""
    out = []
    plain = [(capi.PART_PACK, p, p) for _n, p in PC.pack_shapes() + PC.capped_packs(1) + PC.capped_packs(50)]
    plain += [(capi.PART_REF_TUPLES, t, s.tobytes()) for _n, t, s in PC.tuple_shapes()]
    plain += [(capi.PART_REF_BYTES, s.tobytes(), s.tobytes()) for _n, _t, s in PC.tuple_shapes()[::7]]
    for i, (content, b, final) in enumerate(plain):
        out.append((capi.PART_STORED, content, b, final))
        out.append((capi.PART_ZSTD, content, zstd_cases.ref_frame(b, (13, 17, 19)[i % 3]), final))
    return out


def check_results(items, seq_cap, finals, cnt, ends, st):
    assert not st.any()
    for i, (_coding, content, _b, want) in enumerate(items):
        assert finals[i] == want, i
        if content == capi.PART_PACK:
            e = PC.pack_ends(want)
            kept = min(e.size, seq_cap)
            assert cnt[i] == e.size and np.array_equal(ends[i, :kept], e[:kept]) and (ends[i, kept:] == FILL).all(), i
        else:
            assert cnt[i] == FILL and (ends[i] == FILL).all(), i


@pytest.mark.parametrize("seq_cap", [1, 50])
def test_parts_unpack_on_the_shapes(ctx, seq_cap):
    import torch
    items = shape_items()
    parts, src = batch([(c, t, b) for c, t, b, _f in items])
    ctx.timing(True)
    try:
        rc, ooff, cnt, ends, st = ctx.parts_unpack_raw(parts, src, seq_cap, None, 0, fill=FILL)
        total = sum(len(f) for _c, _t, _b, f in items)
        assert rc == capi.ECAP and int(ooff[-1]) == total  # the sizes are reported, nothing is written
        assert np.array_equal(np.diff(ooff.astype(np.int64)), [len(f) for _c, _t, _b, f in items])
        assert ctx.timing_get()["parts_unpack"][1] == 2  # the pack index and the references' sizes: no write launch
        out = np.full(total + 64, 0xAA, np.uint8)
        rc, ooff2, cnt, ends, st = ctx.parts_unpack_raw(parts, src, seq_cap, out.ctypes.data, total, fill=FILL)
        assert rc == capi.OK and np.array_equal(ooff2, ooff) and (out[total:] == 0xAA).all()
        assert ctx.timing_get()["parts_unpack"][1] == 5 and ctx.timing_get()["zstd_decode"][1] == 2
        check_results(items, seq_cap, [out[int(ooff[i]):int(ooff[i + 1])].tobytes() for i in range(len(items))], cnt, ends, st)
    finally:
        ctx.timing(False)
    # the same left on the device, at an odd address
    d = torch.full((16 + total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, ooff3, cnt3, ends3, st3 = ctx.parts_unpack_raw(parts, src, seq_cap, d.data_ptr() + 5, total, dev=True, fill=FILL)
    got = d.cpu().numpy()
    assert rc == capi.OK and np.array_equal(ooff3, ooff) and np.array_equal(cnt3, cnt) and np.array_equal(ends3, ends) and not st3.any()
    assert got[5:5 + total].tobytes() == out[:total].tobytes() and (got[:5] == 0x5A).all() and (got[5 + total:] == 0x5A).all()


def test_parts_unpack_of_nothing(ctx):
    rc, ooff, _cnt, _ends, _st = ctx.parts_unpack_raw(np.zeros(0, capi.PART_DTYPE), b"", 4, None, 0)
    assert rc == capi.OK and ooff.tolist() == [0]
    finals, cnt, _ends, st = ctx.parts_unpack(*batch([(capi.PART_STORED, capi.PART_PACK, b"")]), 4)
    assert finals == [b""] and cnt.tolist() == [0] and not st.any()
    bad = np.zeros(1, capi.PART_DTYPE)
    bad[0] = (2, 5, capi.PART_STORED, capi.PART_PACK, 0)
    for change in ({}, {"off": 1 << 40}, {"n_bytes": 3, "coding": 2}, {"n_bytes": 3, "content": 3}):
        p = bad.copy()
        for f, v in change.items():
            p[f][0] = v
        assert ctx.parts_unpack_raw(p, b"123456", 4, None, 0)[0] == capi.EINVAL  # outside the source, unknown coding, unknown content
        assert "part 0" in ctx.L.agc_hip_last_error(ctx.h).decode()


def test_parts_unpack_refusals(ctx):
    """good, zstd-malformed, tuple-malformed and unsupported parts interleaved: statuses per part, the good ones byte-exact"""
    good_pack = PC.pack_of([b"first", b"", b"third" * 300], b"xy")
    sym = np.random.default_rng(3).integers(0, 4, 5000, dtype=np.uint8)
    good_t = PC.tuples_of(sym, 4)
    fr = zstd_cases.ref_frame(good_pack, 17)
    torn = fr[:len(fr) - 3]                                   # truncated behind a good header: the decoder finds out
    magic = b"\x00" + fr[1:]                                  # refused by its header
    checksum = fr[:4] + bytes([fr[4] | 0x04]) + fr[5:] + b"\0\0\0\0"  # unsupported
    bad_t = [t for n, t in PC.refused_tuples() if n in ("size 1", "nb 3, low nibble 4", "nb 4, low nibble 15")]
    items = [(capi.PART_ZSTD, capi.PART_PACK, fr, good_pack, 0),
             (capi.PART_ZSTD, capi.PART_PACK, torn, None, capi.ZD_MALFORMED),
             (capi.PART_ZSTD, capi.PART_REF_TUPLES, zstd_cases.ref_frame(good_t, 13), sym.tobytes(), 0),
             (capi.PART_STORED, capi.PART_REF_TUPLES, bad_t[0], None, capi.PART_BAD_TUPLES),
             (capi.PART_ZSTD, capi.PART_PACK, magic, None, capi.ZD_MALFORMED),
             (capi.PART_STORED, capi.PART_PACK, good_pack, good_pack, 0),
             (capi.PART_ZSTD, capi.PART_REF_TUPLES, zstd_cases.ref_frame(bad_t[1], 13), None, capi.PART_BAD_TUPLES),
             (capi.PART_ZSTD, capi.PART_REF_BYTES, checksum, None, capi.ZD_UNSUPPORTED),
             (capi.PART_ZSTD, capi.PART_REF_TUPLES, torn, None, capi.ZD_MALFORMED),
             (capi.PART_STORED, capi.PART_REF_TUPLES, bad_t[2], None, capi.PART_BAD_TUPLES),
             (capi.PART_STORED, capi.PART_REF_TUPLES, good_t, sym.tobytes(), 0)]
    parts, src = batch([(c, t, b) for c, t, b, _f, _s in items])
    want_st = [s for *_x, s in items]
    total = sum(len(f) for _c, _t, _b, f, _s in items if f is not None)
    out = np.full(64 + total + 64, 0xAA, np.uint8)
    rc, ooff, cnt, ends, st = ctx.parts_unpack_raw(parts, src, 8, out.ctypes.data + 64, total, fill=FILL)
    assert rc == capi.EINVAL and "part 1 is refused" in ctx.L.agc_hip_last_error(ctx.h).decode()
    assert st.tolist() == want_st and int(ooff[-1]) == total
    assert (out[:64] == 0xAA).all() and (out[64 + total:] == 0xAA).all()  # the guard bytes around the output
    for i, (_c, content, _b, final, _s) in enumerate(items):
        got = out[64 + int(ooff[i]):64 + int(ooff[i + 1])].tobytes()
        assert got == (final or b""), i  # a refused part has no bytes: nothing of it is written anywhere
        if final is not None and content == capi.PART_PACK:
            assert cnt[i] == 3 and ends[i, :3].tolist() == PC.pack_ends(final).tolist() and (ends[i, 3:] == FILL).all()
        else:
            assert cnt[i] == FILL and (ends[i] == FILL).all()
    finals, _cnt, _ends, st = ctx.parts_unpack(parts, src, 8)
    assert st.tolist() == want_st and [f is None for f in finals] == [s != 0 for s in want_st]
    # every header refused: nothing is launched for the frames, the statuses are the host's
    rc, _o, _c, _e, st = ctx.parts_unpack_raw(*batch([(capi.PART_ZSTD, capi.PART_PACK, magic), (capi.PART_ZSTD, capi.PART_REF_TUPLES, checksum)]), 8, None, 0)
    assert rc == capi.EINVAL and st.tolist() == [capi.ZD_MALFORMED, capi.ZD_UNSUPPORTED]


# ---- DeviceReader.sample_fasta_parts against the host reader -------------------------------------------------------------------------
def test_reader_on_the_toy_archive(ctx):
    from agc_amd import devread, reader
    host = reader.CAGCFile()
    assert host.Open(TOY_AGC)
    r = devread.DeviceReader(ctx, TOY_AGC, gid_base=20000)
    for s in host.ListSample():
        for ll in (80, 40, 0):
            assert r.sample_fasta_parts(s, ll) == host.GetSampleFasta(s, ll), (s, ll)
        assert r.sample_fasta_parts_dev(s, 80).cpu().numpy().tobytes() == host.GetSampleFasta(s, 80)
    with pytest.raises(KeyError):
        r.sample_fasta_parts("no such sample")
    r.close()
    host.Close()


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """archives written on the spot by the product's CLI: name -> (archive, input files)"""
    out = {}
    for name in ("syn_mixed", "syn_c4_twin"):
        d = tmp_path_factory.mktemp(name)
        args, _ = COLL.CONFIGS[name]
        files = COLL.build(name, str(d / "in"))
        agc = str(d / "o.agc")
        r = subprocess.run([AGC_AMD, "create"] + args + ["-t", "8", "-o", agc] + files, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and os.path.exists(agc), r.stderr[-2000:]
        out[name] = (agc, files)
    return out


def test_reader_on_syn_mixed(ctx, written):
    """every sample twice: the second call finds its references registered -- it adds none and hands no reference part in"""
    from agc_amd import devread, reader
    agc, files = written["syn_mixed"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    r = devread.DeviceReader(ctx, agc, gid_base=30000)
    n_new = 0
    for f in files:
        s = os.path.basename(f)[:-3]
        want = host.GetSampleFasta(s, 80)
        before = len(r.registered)
        assert r.sample_fasta_parts(s) == want, s
        n_new += len(r.registered) - before
        reg = set(r.registered)
        assert set(host.GetSamplePlan(s)["groups"].tolist()) <= reg
        (parts, *_rest), _names, new = r.parts(s)
        assert not new and (parts["content"] == capi.PART_PACK).all()
        assert r.sample_fasta_parts(s) == want and r.registered == reg, s
        assert r.sample_fasta_parts(s, 0) == host.GetSampleFasta(s, 0), s
    assert n_new == len(r.registered) > 0
    r.close()
    host.Close()


def test_reader_on_syn_c4_twin(ctx, written):
    """pieces in either orientation, raw groups, hundreds of contigs: two samples in turn, one of them as a device tensor"""
    from agc_amd import devread, reader
    agc, files = written["syn_c4_twin"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    r = devread.DeviceReader(ctx, agc, gid_base=100000)
    names = [os.path.basename(f)[:-3] for f in files]
    plan = host.GetSamplePlan(names[1])
    assert plan["rc"].any() and (plan["kind"] == reader.PLAN_RAW).any() and plan["ctg_seg"].size > 200
    assert r.sample_fasta_parts(names[1]) == host.GetSampleFasta(names[1], 80)
    assert r.sample_fasta_parts_dev(names[4], 60).cpu().numpy().tobytes() == host.GetSampleFasta(names[4], 60)
    r.close()
    host.Close()


def test_two_readers_two_ways_on_one_archive(ctx, written):
    """sample_fasta and sample_fasta_parts interleaved on two readers with disjoint group ranges: each keeps its own registrations"""
    from agc_amd import devread, reader
    agc, files = written["syn_mixed"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    a, b = devread.DeviceReader(ctx, agc, gid_base=200000), devread.DeviceReader(ctx, agc, gid_base=300000)
    for i, f in enumerate(files):
        s = os.path.basename(f)[:-3]
        want = host.GetSampleFasta(s, 80)
        first, second = (a, b) if i % 2 else (b, a)
        assert first.sample_fasta(s) == want and second.sample_fasta_parts(s) == want, s
        assert first.sample_fasta_parts(s) == want and second.sample_fasta(s) == want, s  # each the other way, its references known
    assert a.registered == b.registered
    a.close()
    b.close()
    host.Close()


# ---- the contract of agc_hip_sample_fasta_parts ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_sample(ctx, written):
    """a sample of syn_mixed with references and deltas, as the arguments of the call, for a range of groups nobody else uses"""
    from agc_amd import devread, reader
    agc, files = written["syn_mixed"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    s = os.path.basename(files[2])[:-3]
    want = host.GetSampleFasta(s, 80)
    host.Close()
    return agc, s, want


def fresh_reader(ctx, agc, base):
    from agc_amd import devread
    return devread.DeviceReader(ctx, agc, gid_base=base)


def call(ctx, args, names, out):
    return ctx.sample_fasta_parts_raw(*args, 80, names[0], names[1], out.ctypes.data if out is not None else None, out.size if out is not None else 0)


def none_registered(ctx, parts):
    gids = parts["gid"][parts["content"] != capi.PART_PACK].tolist()
    assert gids
    return not any(ctx.ref_registered(g) for g in gids)  # (agc_hip_ref_get answers ENOREF for each)


def test_capacity_leaves_buffer_and_registrations(ctx, one_sample):
    agc, s, want = one_sample
    r = fresh_reader(ctx, agc, 400000)
    args, names, new = r.parts(s)
    assert new
    out = np.full(len(want) - 1, 0xAA, np.uint8)
    ctx.timing(True)
    try:
        assert call(ctx, args, names, out) == (capi.ECAP, len(want))
        assert call(ctx, args, names, None) == (capi.ECAP, len(want))
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # before any launch
    finally:
        ctx.timing(False)
    assert (out == 0xAA).all() and none_registered(ctx, args[0])
    out = np.full(len(want) + 64, 0xAA, np.uint8)
    assert ctx.sample_fasta_parts_raw(*args, 80, names[0], names[1], out.ctypes.data, len(want)) == (capi.OK, len(want))
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xAA).all() and not none_registered(ctx, args[0])
    r.close()


def test_a_torn_pack_registers_nothing(ctx, one_sample):
    """one pack part with a flipped byte in its frame header: EINVAL, the text untouched, NO group of the call's parts registered --
    and the same call with the archive's own bytes then succeeds"""
    agc, s, want = one_sample
    r = fresh_reader(ctx, agc, 500000)
    args, names, new = r.parts(s)
    parts, (src, src_bytes) = args[0], args[1]
    import ctypes as C
    good = np.frombuffer(C.string_at(src, src_bytes), np.uint8)
    pi = int(np.flatnonzero((parts["content"] == capi.PART_PACK) & (parts["coding"] == capi.PART_ZSTD))[0])
    for at in (0, 4):  # the magic number; the frame header descriptor (a reserved bit)
        bad = good.copy()
        bad[int(parts["off"][pi]) + at] ^= 0x08
        out = np.full(len(want) + 64, 0xAA, np.uint8)
        rc, n = call(ctx, (parts, bad) + args[2:], names, out)
        assert rc == capi.EINVAL and n == len(want) and f"part {pi} is refused" in ctx.L.agc_hip_last_error(ctx.h).decode()
        assert (out == 0xAA).all() and none_registered(ctx, parts)
    out = np.full(len(want), 0xAA, np.uint8)
    assert call(ctx, (parts, good) + args[2:], names, out) == (capi.OK, len(want)) and out.tobytes() == want
    assert not none_registered(ctx, parts)
    r.close()


def test_an_index_at_the_packs_count_registers_nothing(ctx, one_sample):
    agc, s, want = one_sample
    r = fresh_reader(ctx, agc, 600000)
    args, names, _new = r.parts(s)
    parts, segs = args[0], args[4].copy()
    _f, cnt, _e, _st = ctx.parts_unpack(parts, args[1], args[2])
    g = int(np.flatnonzero(segs["kind"] == capi.SEG_DELTA)[0])
    segs["index"][g] = cnt[int(segs["part"][g])]
    out = np.full(len(want) + 64, 0xAA, np.uint8)
    rc, _n = call(ctx, args[:4] + (segs,) + args[5:], names, out)
    assert rc == capi.EINVAL and f"segment {g} " in ctx.L.agc_hip_last_error(ctx.h).decode()
    assert (out == 0xAA).all() and none_registered(ctx, parts)
    # likewise a segment whose length is not what its reference has: the layout's refusal, still in front of the registration
    g = int(np.flatnonzero(segs["kind"] == capi.SEG_REF)[0])
    segs = args[4].copy()
    segs["length"][g] += 1
    out = np.full(len(want) + 64, 0xAA, np.uint8)
    rc, _n = call(ctx, args[:4] + (segs,) + args[5:], names, out)
    assert rc == capi.EINVAL and (out == 0xAA).all() and none_registered(ctx, parts)
    r.close()


def test_plan_errors_are_refused_before_any_launch(ctx, one_sample):
    agc, s, want = one_sample
    r = fresh_reader(ctx, agc, 700000)
    assert r.sample_fasta_parts(s) == want  # its groups are registered now
    again = fresh_reader(ctx, agc, 700000)  # ... which this reader does not know: it hands their parts in a second time
    args, names, new = again.parts(s)
    parts, segs = args[0], args[4]
    assert new
    out = np.full(len(want) + 64, 0xAA, np.uint8)
    d = int(np.flatnonzero(segs["kind"] == capi.SEG_DELTA)[0])
    ref_part = int(np.flatnonzero(parts["content"] != capi.PART_PACK)[0])

    def changed(**kw):
        s2 = segs.copy()
        for f, v in kw.items():
            s2[f][d] = v
        return args[:4] + (s2,) + args[5:]

    known = r.parts(s)[0]  # (the parts without the references: what the first reader would hand in)
    moved, moved_segs = parts.copy(), changed(part=ref_part)[4]  # the same plan for groups nobody has registered, a delta naming a reference part
    moved["gid"][moved["content"] != capi.PART_PACK] += 50000
    moved_segs["gid"][moved_segs["kind"] != capi.SEG_RAW] += 50000
    bad = [("a reference part of a registered group", capi.EINVAL, args),
           ("a group neither registered nor among the parts", capi.ENOREF, (known[0],) + known[1:4] + (changed(gid=4_000_000)[4],) + known[5:]),
           ("a part that is not a pack", capi.EINVAL, (moved,) + args[1:4] + (moved_segs,) + args[5:]),
           ("a part outside the batch", capi.EINVAL, (known[0],) + known[1:4] + (changed(part=known[0].size)[4],) + known[5:])]
    ctx.timing(True)
    try:
        for what, code, a in bad:
            assert call(ctx, a, names, out)[0] == code, what
            assert (out == 0xAA).all(), what
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # no launch in any slot
    finally:
        ctx.timing(False)
    assert r.sample_fasta_parts(s) == want
    r.close()
    again.close()
