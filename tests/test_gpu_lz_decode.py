"""GPU parity: agc_hip_lz_decode_batch / _dev (lz_decode_kernels.hip) against the oracle's decode, through the C ABI (bit-exact)."""
import numpy as np
import pytest

from agc_amd import capi
from tests import lzdec_cases
from tests.cases import lz_cases

pytestmark = pytest.mark.gpu

GID_CASES = 60000  # the 60 references of lz_cases() (gids no other file registers on the shared context: they stay below 53000)
GID_HAND = 60100   # the handcrafted references
HAND_GID = {"clean": GID_HAND, "esc": GID_HAND + 1}


def _batch(deltas):
    off = np.zeros(len(deltas) + 1, np.uint64)
    off[1:] = np.cumsum([d.size for d in deltas])
    return (np.concatenate(deltas) if deltas else np.zeros(0, np.uint8)).astype(np.uint8), off


@pytest.fixture(scope="module")
def cases(hip_ctx, oracle):
    """lz_cases() registered, with the oracle's deltas: (cases, deltas, enc, enc_off, gids)"""
    cs = lz_cases()
    for i, (mml, ref, _t) in enumerate(cs):
        hip_ctx.ref_register(GID_CASES + i, ref, mml)
    deltas = [oracle.LZ(ref, mml).encode(text) for (mml, ref, text) in cs]
    enc, off = _batch(deltas)
    return cs, deltas, enc, off, GID_CASES + np.arange(len(cs))


@pytest.fixture(scope="module")
def hand(hip_ctx, oracle):
    """the handcrafted references registered, the valid deltas with the oracle's decode: (refs, [(name, gid, delta, want)])"""
    refs = lzdec_cases.references()
    for name, gid in HAND_GID.items():
        hip_ctx.ref_register(gid, refs[name], lzdec_cases.MML)
    out = []
    for name, ref_name, enc in lzdec_cases.valid_cases():
        want, n = oracle.LZ(refs[ref_name], lzdec_cases.MML).decode(enc, 1 << 16)
        assert n == want.size
        out.append((name, HAND_GID[ref_name], enc, want))
    return refs, out


def _expected(cs, deltas):
    return [text if d.size else text[:0] for (_m, _r, text), d in zip(cs, deltas)]


def test_round_trip_of_the_lz_cases(hip_ctx, oracle, cases):
    cs, deltas, enc, off, gids = cases
    assert len(cs) == 60
    out, ooff = hip_ctx.lz_decode_batch(enc, off, gids)
    rc = (np.arange(len(cs)) % 2).astype(np.uint8)
    out_rc, ooff_rc = hip_ctx.lz_decode_batch(enc, off, gids, rc=rc)
    assert np.array_equal(ooff, ooff_rc)
    for i, want in enumerate(_expected(cs, deltas)):
        a, b = int(ooff[i]), int(ooff[i + 1])
        assert b - a == want.size, f"case {i}"
        assert np.array_equal(out[a:b], want), f"case {i}"
        assert np.array_equal(out_rc[a:b], oracle.rev_comp(want) if rc[i] else want), f"case {i} rc {rc[i]}"


def test_handcrafted_deltas(hip_ctx, oracle, hand):
    _refs, hs = hand
    enc, off = _batch([h[2] for h in hs])
    gids = np.array([h[1] for h in hs], np.uint32)
    for rc in (0, 1):
        out, ooff = hip_ctx.lz_decode_batch(enc, off, gids, rc=np.full(len(hs), rc, np.uint8))
        for i, (name, _g, _e, want) in enumerate(hs):
            got = out[int(ooff[i]):int(ooff[i + 1])]
            assert np.array_equal(got, oracle.rev_comp(want) if rc else want), f"{name} rc {rc}"
    # each one alone as well: a batch of one, nothing in front of it in the buffers
    for name, g, e, want in hs:
        out, ooff = hip_ctx.lz_decode_batch(e, [0, e.size], [g])
        assert np.array_equal(out, want) and int(ooff[1]) == want.size, name


def _raw_decode(hip_ctx, enc, off, gids, out):
    """the entry point itself: -> (return code, out_off)"""
    C, u8p, u32p, u64p = capi.C, capi.u8p, capi.u32p, capi.u64p
    enc, off, gids = np.ascontiguousarray(enc, np.uint8), np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(gids, np.uint32)
    ooff = np.zeros(gids.size + 1, np.uint64)
    rc = hip_ctx.L.agc_hip_lz_decode_batch(hip_ctx.h, gids.size, gids.ctypes.data_as(u32p), enc.ctypes.data_as(u8p), off.ctypes.data_as(u64p), None,
                                           out.ctypes.data_as(u8p), out.size, ooff.ctypes.data_as(u64p))
    return rc, ooff


def test_capacity_contract(hip_ctx, cases):
    cs, deltas, enc, off, gids = cases
    need = sum(w.size for w in _expected(cs, deltas))
    out = np.full(need - 1, 0xAA, np.uint8)
    rc, ooff = _raw_decode(hip_ctx, enc, off, gids, out)
    assert rc == capi.ECAP and int(ooff[-1]) == need
    assert (out == 0xAA).all()
    out = np.full(need, 0xAA, np.uint8)
    rc, ooff2 = _raw_decode(hip_ctx, enc, off, gids, out)
    assert rc == capi.OK and np.array_equal(ooff, ooff2)
    assert np.array_equal(out, np.concatenate(_expected(cs, deltas)))
    assert hip_ctx.lz_decode_batch(enc[:0], [0], [])[0].size == 0  # n == 0


def test_dev_variant(hip_ctx, cases):
    import torch
    cs, deltas, enc, off, gids = cases
    rc = (np.arange(len(cs)) % 2).astype(np.uint8)
    want, woff = hip_ctx.lz_decode_batch(enc, off, gids, rc=rc)
    d = torch.full((want.size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ooff = hip_ctx.lz_decode_batch_dev(enc, off, gids, d.data_ptr(), want.size, rc=rc)
    got = d.cpu().numpy()
    assert np.array_equal(ooff, woff)
    assert np.array_equal(got[:want.size], want)
    assert (got[want.size:] == 0x5A).all()


def test_rejected_input(hip_ctx, oracle, cases, hand):
    cs, deltas, enc, off, gids = cases
    _refs, hs = hand
    good = hs[0][2]  # a well-formed delta in front of and behind the bad one
    bad = [(name, HAND_GID[ref_name], e) for name, ref_name, e, _st in lzdec_cases.rejected_cases()]
    bad.append(("unknown_gid", GID_CASES - 1, good))
    for name, gid, e in bad:
        b_enc, b_off = _batch([hs[1][2], hs[2][2], e, hs[3][2]])
        out = np.full(4096, 0xAA, np.uint8)
        rc, _ooff = _raw_decode(hip_ctx, b_enc, b_off, [hs[1][1], hs[2][1], gid, hs[3][1]], out)
        assert rc == capi.EINVAL, name
        assert "delta 2" in hip_ctx.L.agc_hip_last_error(hip_ctx.h).decode(), name
        assert (out == 0xAA).all(), name
    # the context is as good as before
    out, ooff = hip_ctx.lz_decode_batch(enc, off, gids)
    assert np.array_equal(out, np.concatenate(_expected(cs, deltas)))


def test_decode_beside_an_encode_in_flight(hip_ctx, oracle, cases):
    import torch
    cs, deltas, enc, off, gids = cases
    texts = [t for (_m, _r, t) in cs]
    ln = np.array([t.size for t in texts], np.uint32)
    toff = np.zeros(len(texts), np.uint64)
    toff[1:] = np.cumsum(ln[:-1].astype(np.uint64))
    d = torch.from_numpy(np.concatenate(texts + [np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    hip_ctx.lz_encode_begin_dev(d.data_ptr(), gids, toff, ln)
    out, ooff = hip_ctx.lz_decode_batch(enc, off, gids)
    got_enc, got_off = hip_ctx.lz_encode_end()
    assert np.array_equal(out, np.concatenate(_expected(cs, deltas)))
    assert np.array_equal(got_enc, enc) and np.array_equal(got_off, off)
