"""GPU: agc_hip_lz_decode_window_batch / _dev (range_kernels.hip: lz_decode_window_kernel) on the handcrafted deltas and the windows
of tests/ranges_cases.py against the full decode of the same context, sliced; agc_amd/devread.py: DeviceReader.ranges / ranges_dev
against the host reader on the toy archive and on archives written on the spot; and the contract of agc_hip_ranges_parts -- what a
failed call leaves registered and written: nothing.  A context of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from agc_amd import capi
from tests import collections as COLL
from tests import lzdec_cases
from tests import ranges_cases as RC
from tests import readfuzz_cases as RF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")
TOY_AGC = os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc")
HAND_GID = {"clean": 1, "esc": 2}
ALPHA = np.frombuffer(b"ACGTNRYSWKMBDHVU", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


# ---- the windowed decode batch ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(ctx):
    """the handcrafted references registered; one job per (delta, orientation, window): (enc, enc_off, gids, rc, win_from, win_len,
    want) with `want` the full decode of the same context, sliced"""
    refs = lzdec_cases.references()
    for name, gid in HAND_GID.items():
        ctx.ref_register(gid, refs[name], lzdec_cases.MML)
    deltas, gids, rcs, wf, wl, want = [], [], [], [], [], []
    for _name, ref_name, enc in lzdec_cases.valid_cases():
        starts, length = RC.token_starts(enc, refs[ref_name].size)
        if not length:
            continue  # (the delta of no bytes: no window has a symbol)
        for rc in (0, 1):
            full, _o = ctx.lz_decode_batch(enc, [0, enc.size], [HAND_GID[ref_name]], rc=[rc])
            assert full.size == length
            for a, n in RC.delta_windows(starts, length):
                deltas.append(enc), gids.append(HAND_GID[ref_name]), rcs.append(rc), wf.append(a), wl.append(n), want.append(full[a:a + n].copy())
    off = np.zeros(len(deltas) + 1, np.uint64)
    off[1:] = np.cumsum([d.size for d in deltas])
    return np.concatenate(deltas), off, np.array(gids, np.uint32), np.array(rcs, np.uint8), np.array(wf, np.uint32), np.array(wl, np.uint32), want


def test_windows_of_the_handcrafted_deltas(ctx, hand):
    enc, off, gids, rc, wf, wl, want = hand
    assert len(want) > 500
    out, ooff = ctx.lz_decode_window_batch(enc, off, gids, wf, wl, rc=rc)
    assert np.array_equal(np.diff(ooff.astype(np.int64)), wl)
    for i, w in enumerate(want):
        assert np.array_equal(out[int(ooff[i]):int(ooff[i + 1])], w), (i, int(gids[i]), int(rc[i]), int(wf[i]), int(wl[i]))


def test_windows_on_the_device_at_an_odd_address(ctx, hand):
    import torch
    enc, off, gids, rc, wf, wl, want = hand
    total = int(wl.sum())
    d = torch.full((16 + total + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ooff = ctx.lz_decode_window_batch_dev(enc, off, gids, wf, wl, d.data_ptr() + 5, total, rc=rc)
    got = d.cpu().numpy()
    assert int(ooff[-1]) == total and got[5:5 + total].tobytes() == np.concatenate(want).tobytes()
    assert (got[:5] == 0x5A).all() and (got[5 + total:] == 0x5A).all()  # the guard bytes in front and behind


def test_window_capacity_one_short(ctx, hand):
    enc, off, gids, rc, wf, wl, _want = hand
    total = int(wl.sum())
    out = np.full(total + 8, 0xAA, np.uint8)
    ctx.timing(True)
    try:
        rc_, ooff = ctx.lz_decode_window_batch_raw(enc, off, gids, wf, wl, out.ctypes.data, total - 1, rc=rc)
        assert rc_ == capi.ECAP and int(ooff[-1]) == total and np.array_equal(np.diff(ooff.astype(np.int64)), wl)
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # the size follows from the arguments: before any launch
    finally:
        ctx.timing(False)
    assert (out == 0xAA).all()


def test_window_refusals_between_good_ones(ctx, hand):
    refs = lzdec_cases.references()
    good = lzdec_cases.Delta(refs["clean"].size).lit(1, 2, 3).match(100, 40).lit(0).bytes()  # 44 symbols
    bad = [c for c in lzdec_cases.rejected_cases() if c[0] == "bad_token_in_the_third_strip"][0][2]

    def call(deltas, wf, wl):
        off = np.zeros(len(deltas) + 1, np.uint64)
        off[1:] = np.cumsum([d.size for d in deltas])
        out = np.full(int(sum(wl)) + 8, 0xAA, np.uint8)
        rc_, _o = ctx.lz_decode_window_batch_raw(np.concatenate(deltas), off, [1] * len(deltas), wf, wl, out.ctypes.data, out.size)
        return rc_, out, ctx.L.agc_hip_last_error(ctx.h).decode()

    rc_, out, _e = call([good, good, good], [0, 40, 43], [44, 4, 1])
    assert rc_ == capi.OK and (out[49:] == 0xAA).all() and np.array_equal(out[44:48], out[40:44])
    rc_, out, err = call([good, good, good], [0, 41, 3], [10, 4, 5])  # one symbol past the delta's 44
    assert rc_ == capi.EINVAL and "delta 1 " in err and "44" in err and (out == 0xAA).all()
    rc_, out, err = call([good, good, good], [0, 44, 3], [10, 1, 5])
    assert rc_ == capi.EINVAL and "delta 1 " in err and (out == 0xAA).all()
    rc_, out, err = call([good, good, bad, good], [0, 1, 0, 3], [10, 4, 1, 5])
    assert rc_ == capi.EINVAL and "delta 2 is rejected" in err and (out == 0xAA).all()
    rc_, out, err = call([good, good], [0, 1], [10, 0])  # a window of no symbols
    assert rc_ == capi.EINVAL and "delta 1 " in err and (out == 0xAA).all()
    off = np.array([0, good.size], np.uint64)
    assert ctx.lz_decode_window_batch_raw(good, off, [77], [0], [1], None, 0)[0] == capi.ECAP  # (the capacity comes first)
    out = np.zeros(8, np.uint8)
    assert ctx.lz_decode_window_batch_raw(good, off, [77], [0], [1], out.ctypes.data, 8)[0] == capi.EINVAL  # an unknown group
    assert ctx.lz_decode_window_batch_raw(good[:0], [0], [], [], [], None, 0)[0] == capi.OK  # n == 0


# ---- DeviceReader.ranges against the host reader -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """archives written on the spot by the product's CLI: name -> (archive, input files)"""
    out = {}
    for name in ("syn_mixed", "syn_c4_twin"):
        d = tmp_path_factory.mktemp("ranges_" + name)
        args, _ = COLL.CONFIGS[name]
        files = COLL.build(name, str(d / "in"))
        agc = str(d / "o.agc")
        r = subprocess.run([AGC_AMD, "create"] + args + ["-t", "8", "-o", agc] + files, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and os.path.exists(agc), r.stderr[-2000:]
        out[name] = (agc, files)
    return out


def check_reader(ctx, path, base, seed, must_have=()):
    from agc_amd import devread, reader
    host = reader.CAGCFile()
    assert host.Open(path)
    queries, in_batch, in_archive = RF.queries(host, seed)
    # the condition on the inputs: a window in every kind x orientation the archive has
    assert in_batch == in_archive and in_archive >= set(must_have), (sorted(in_batch), sorted(in_archive))
    want = [host.GetCtgSeq(s, name, f, t).encode() for s, name, f, t in queries]
    assert any(len(w) == 0 for w in want) and sum(len(w) for w in want) > 100
    r = devread.DeviceReader(ctx, path, gid_base=base)
    got = r.ranges(queries)
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g == w, (q, queries[q])
    codes = r.ranges(queries, letters=False)
    for q, (g, w) in enumerate(zip(codes, want)):
        assert ALPHA[np.frombuffer(g, np.uint8)].tobytes() == w, (q, queries[q])
    # a second call of the same batch registers nothing new and hands in no reference part
    reg = set(r.registered)
    (parts, *_rest), new = r.range_parts(queries)
    assert not new and (parts["content"] == capi.PART_PACK).all()
    d, off = r.ranges_dev(queries)
    assert r.registered == reg and d.cpu().numpy().tobytes() == b"".join(want)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64))
    d, off = r.ranges_dev(queries[:40], letters=False)
    assert ALPHA[d.cpu().numpy()].tobytes() == b"".join(want[:40])
    # nothing asked for, and nothing but empty ranges
    assert r.ranges([]) == [] and r.ranges_dev([])[0].numel() == 0
    s, name, _f, _t = queries[0]
    n = host.GetCtgLen(s, name)
    assert r.ranges([(s, name, n, n + 9), (s, name, n + 1, -1)]) == [b"", b""]
    d, off = r.ranges_dev([(s, name, n, n + 9)])
    assert d.numel() == 0 and off.tolist() == [0, 0]
    with pytest.raises(KeyError) as e:
        r.ranges([queries[0], (s, "no such contig", 0, 5)])
    assert e.value.args[0] == 1
    r.close()
    host.Close()


def test_ranges_on_the_toy_archive(ctx):
    check_reader(ctx, TOY_AGC, 20000, 1)


def test_ranges_on_syn_mixed(ctx, written):
    check_reader(ctx, written["syn_mixed"][0], 30000, 2, must_have=[(capi.SEG_REF, 0), (capi.SEG_DELTA, 0)])


def test_ranges_on_syn_c4_twin(ctx, written):
    """pieces in either orientation, raw groups"""
    from agc_amd import reader
    host = reader.CAGCFile()
    assert host.Open(written["syn_c4_twin"][0])
    kinds = set()
    for s in host.ListSample():
        p = host.GetSamplePlan(s)
        kinds |= set(zip(p["kind"].tolist(), p["rc"].tolist()))
    host.Close()
    assert any(rc for _k, rc in kinds) and any(k == capi.SEG_RAW for k, _rc in kinds)  # it supplies rc and RAW
    check_reader(ctx, written["syn_c4_twin"][0], 100000, 3)


# ---- the contract of agc_hip_ranges_parts ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_batch(written):
    """a batch on syn_mixed with references and deltas: (archive, queries, the letters wanted back to back)"""
    from agc_amd import reader
    agc, files = written["syn_mixed"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    s = os.path.basename(files[2])[:-3]
    queries = [(s, name, 100 * i, 100 * i + 2500) for i, name in enumerate(host.ListCtg(s))]
    want = b"".join(host.GetCtgSeq(*q).encode() for q in queries)
    p = host.GetRangeParts(queries)
    assert (p["kind"] == reader.PLAN_DELTA).any() and (p["part_content"] != reader.PART_PACK).any() and len(want) > 2000
    host.Close()
    return agc, queries, want


def fresh_reader(ctx, agc, base):
    from agc_amd import devread
    return devread.DeviceReader(ctx, agc, gid_base=base)


def call(ctx, args, out, cap=None):
    rc, off = ctx.ranges_parts_raw(*args, 1, out.ctypes.data if out is not None else None, (out.size if cap is None else cap) if out is not None else 0)
    return rc, int(off[-1])


def none_registered(ctx, parts):
    gids = parts["gid"][parts["content"] != capi.PART_PACK].tolist()
    assert gids
    return not any(ctx.ref_registered(g) for g in gids)


def test_capacity_leaves_buffer_and_registrations(ctx, one_batch):
    agc, queries, want = one_batch
    r = fresh_reader(ctx, agc, 400000)
    args, new = r.range_parts(queries)
    assert new
    out = np.full(len(want) + 64, 0xAA, np.uint8)
    ctx.timing(True)
    try:
        assert call(ctx, args, out, len(want) - 1) == (capi.ECAP, len(want))
        assert call(ctx, args, None) == (capi.ECAP, len(want))
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # before any launch
    finally:
        ctx.timing(False)
    assert (out == 0xAA).all() and none_registered(ctx, args[0])
    assert call(ctx, args, out, len(want)) == (capi.OK, len(want))
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xAA).all() and not none_registered(ctx, args[0])
    r.close()


def test_a_torn_pack_registers_nothing(ctx, one_batch):
    """one pack part with a flipped byte in its frame header: EINVAL, the output untouched, NO group of the call's parts registered --
    and the same call with the archive's own bytes then succeeds"""
    agc, queries, want = one_batch
    r = fresh_reader(ctx, agc, 500000)
    args, _new = r.range_parts(queries)
    parts, (src, src_bytes) = args[0], args[1]
    good = np.frombuffer(C.string_at(src, src_bytes), np.uint8)
    pi = int(np.flatnonzero((parts["content"] == capi.PART_PACK) & (parts["coding"] == capi.PART_ZSTD))[0])
    for at in (0, 4):  # the magic number; the frame header descriptor (a reserved bit)
        bad = good.copy()
        bad[int(parts["off"][pi]) + at] ^= 0x08
        out = np.full(len(want) + 64, 0xAA, np.uint8)
        rc, n = call(ctx, (parts, bad) + args[2:], out)
        assert rc == capi.EINVAL and n == len(want) and f"part {pi} is refused" in ctx.L.agc_hip_last_error(ctx.h).decode()
        assert (out == 0xAA).all() and none_registered(ctx, parts)
    out = np.full(len(want), 0xAA, np.uint8)
    assert call(ctx, (parts, good) + args[2:], out) == (capi.OK, len(want)) and out.tobytes() == want
    assert not none_registered(ctx, parts)
    r.close()


def test_bad_windows_are_refused_before_any_launch(ctx, one_batch):
    agc, queries, want = one_batch
    r = fresh_reader(ctx, agc, 600000)
    args, _new = r.range_parts(queries)
    parts, wins = args[0], args[4]
    out = np.full(len(want) + 64, 0xAA, np.uint8)
    w = int(np.flatnonzero(wins["kind"] == capi.SEG_DELTA)[0])

    def changed(**kw):
        w2 = wins.copy()
        for f, v in kw.items():
            w2[f][w] = v
        return args[:4] + (w2,) + args[5:]

    past = int(wins["length"][w]) - int(wins["win_len"][w]) + 1  # win_from + win_len == length + 1
    bad = [("a window past its segment's length", capi.EINVAL, changed(win_from=past)),
           ("a window of no symbols", capi.EINVAL, changed(win_len=0)),
           ("a group neither registered nor among the parts", capi.ENOREF, changed(gid=4_000_000)),
           ("a part outside the batch", capi.EINVAL, changed(part=parts.size)),
           ("an unknown kind", capi.EINVAL, changed(kind=3))]
    ctx.timing(True)
    try:
        for what, code, a in bad:
            rc, _n = call(ctx, a, out)
            assert rc == code and f"window {w} " in ctx.L.agc_hip_last_error(ctx.h).decode(), what
            assert (out == 0xAA).all(), what
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # no launch in any slot
    finally:
        ctx.timing(False)
    assert none_registered(ctx, parts)
    assert b"".join(r.ranges(queries)) == want
    r.close()
