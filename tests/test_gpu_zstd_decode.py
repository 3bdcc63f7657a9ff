"""GPU: agc_hip_zstd_decode_batch / _dev (zstd_decode_kernels.hip) against libzstd's ZSTD_decompress and against the CPU build of
the same decoder (tests/zsdec_host), through the C ABI: the shapes at which the wave-wide copies and the stream split can go wrong,
a mixed batch, the library's own frames, the archive's parts, the call's contract, and mutated frames."""
import os
import tempfile

import numpy as np
import pytest

from agc_amd import capi
from tests import zsdec_cases as zd
from tests import zstd_cases
from tests.zsdec_host import build as zsdec_build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p = capi.u8p


@pytest.fixture(scope="module")
def host_decode():
    return zd.host_decoder()


@pytest.fixture(scope="module")
def corpus_frames(oracle):
    """about 200 frames: the mixed corpus at the five levels -> [(input, frame)]"""
    return [(d, zstd_cases.ref_frame(d, lv)) for d in zstd_cases.corpus(oracle, 11, 24) for lv in zd.LEVELS]


def _check(hip_ctx, frames, wants):
    outs, st = hip_ctx.zstd_decode_batch(frames)
    assert not st.any(), np.flatnonzero(st)
    for i, (got, want) in enumerate(zip(outs, wants)):
        assert got == want, f"frame {i}: {len(got)} bytes, {len(want)} expected"


def test_shapes(hip_ctx):
    """every shape from inputs that make libzstd emit it, the shape asserted from the frame's headers (and, for offsets and literal
    lengths, from the sequences libzstd's level-17 parser reports) before the device sees it"""
    inputs = zd.shape_inputs()
    frames = {name: zstd_cases.ref_frame(d, 17) for name, d in inputs.items()}
    w = {name: zd.walk(fr) for name, fr in frames.items()}
    assert "frame_empty" in w["empty"] and len(inputs["one_byte"]) == 1
    assert "blk_rle" in w["rle_block"] and w["raw_block"] == {"blk_raw", "fcs2", "hdr_single"}
    assert {"lit_comp", "lit_treeless", "blocks_many"} <= w["treeless"]
    assert "blocks_many" in w["cross_block_match"] and "streams4_uneven" in w["four_streams"]
    seqs = {name: zstd_cases.ref_sequences(d) for name, d in inputs.items() if name.startswith(("offset", "litrun", "cross"))}
    assert any(o == 1 and ml > 64 for o, _ll, ml, _r in seqs["offset1_long"])
    for off in (63, 64, 65):
        assert any(o == off and ml > off for o, _ll, ml, _r in seqs["offset%d" % off]), off
    for ll in (0, 1, 63, 64, 65):
        assert any(l == ll and ml > 0 for _o, l, ml, _r in seqs["litrun%d" % ll]), ll
    pos, crossing = 0, 0
    for o, ll, ml, _r in seqs["cross_block_match"]:  # (a match written in the second block that reads the first)
        pos += ll
        crossing += ml > 0 and pos >= 131072 and pos - o < 131072
        pos += ml
    assert crossing and pos == len(inputs["cross_block_match"])
    names = sorted(frames)
    wants = [zd.ref_decode(frames[n], len(inputs[n])) for n in names]
    assert wants == [inputs[n] for n in names]
    _check(hip_ctx, [frames[n] for n in names], wants)
    for n in names:  # each one alone as well: nothing in front of it in the buffers
        _check(hip_ctx, [frames[n]], [inputs[n]])


def test_mixed_batch_equals_libzstd_and_dev_equals_host(hip_ctx, corpus_frames):
    import torch
    frames = [fr for _d, fr in corpus_frames]
    wants = [zd.ref_decode(fr, len(d)) for d, fr in corpus_frames]
    assert len(frames) >= 200 and wants == [d for d, _fr in corpus_frames]
    _check(hip_ctx, frames, wants)
    total = sum(len(x) for x in wants)
    buf = torch.full((total + 128,), 0xAA, dtype=torch.uint8, device="cuda")
    ooff, st = hip_ctx.zstd_decode_batch_dev(frames, buf.data_ptr() + 64, total)
    assert not st.any() and int(ooff[-1]) == total
    got = buf.cpu().numpy()
    assert (got[:64] == 0xAA).all() and (got[64 + total:] == 0xAA).all()
    assert got[64:64 + total].tobytes() == b"".join(wants)


def test_round_trip_of_the_library_s_own_frames(hip_ctx, oracle):
    inputs = [d for d in zstd_cases.corpus(oracle, 3, 8, max_len=12000)]
    levels = [(13, 17, 19)[i % 3] for i in range(len(inputs))]
    frames = hip_ctx.zstd_batch(inputs, levels)
    _check(hip_ctx, frames, [bytes(d) for d in inputs])


def test_archive_parts(hip_ctx):
    parts = zd.archive_frames(os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc"))
    assert parts and all(fr[:4] == zd.MAGIC.to_bytes(4, "little") for _n, fr in parts)
    wants = [zd.ref_decode(fr, 1 << 20) for _n, fr in parts]
    assert all(x is not None and len(x) > 0 for x in wants)
    _check(hip_ctx, [fr for _n, fr in parts], wants)


def test_contract(hip_ctx, host_decode, corpus_frames):
    import torch
    good = [(d, fr) for d, fr in corpus_frames if 0 < len(d) < 30000][:12]
    frames = [fr for _d, fr in good]
    total = sum(len(d) for d, _fr in good)
    # too small a buffer: the sizes are reported, nothing is written
    out = np.full(total, 0xAA, np.uint8)
    rc, ooff, st = hip_ctx.zstd_decode_batch_raw(frames, out.ctypes.data_as(u8p), total - 1)
    assert rc == capi.ECAP and (out == 0xAA).all()
    assert list(np.diff(ooff.astype(np.int64))) == [len(d) for d, _fr in good] and not st.any()
    # no frames
    rc, ooff, st = hip_ctx.zstd_decode_batch_raw([], None, 0)
    assert rc == capi.OK and int(ooff[0]) == 0
    # some frames bad: a header refused (size 0), bodies refused by the kernel (their ranges stay theirs), good ones between them
    bad_body = bytearray(frames[1])
    bad_body[len(bad_body) // 2:] = b"\xff" * (len(bad_body) - len(bad_body) // 2)
    mixed = [frames[0], bytes(bad_body), frames[2], b"\x00" + frames[3][1:], frames[4], frames[5][:-3], frames[6], frames[5] + b"\x00"]
    host = [host_decode(fr) for fr in mixed]
    assert [s for s, _b in host] == [0, 2, 0, 2, 0, 2, 0, 2]
    sizes = [len(good[0][0]), len(good[1][0]), len(good[2][0]), 0, len(good[4][0]), len(good[5][0]), len(good[6][0]), len(good[5][0])]
    tot = sum(sizes)
    buf = torch.full((tot + 256,), 0xAA, dtype=torch.uint8, device="cuda")
    rc, ooff, st = hip_ctx.zstd_decode_batch_raw(mixed, buf.data_ptr() + 128, tot, dev=True)
    assert rc == capi.EINVAL
    err = hip_ctx.L.agc_hip_last_error(hip_ctx.h).decode()
    assert "frame 1 " in err and "status 2" in err, err
    assert list(st) == [s for s, _b in host]
    assert list(np.diff(ooff.astype(np.int64))) == sizes
    got = buf.cpu().numpy()
    assert (got[:128] == 0xAA).all() and (got[128 + tot:] == 0xAA).all()  # (the ranges are back to back: the guards are around them)
    for i, (s, want) in enumerate(host):
        if s == 0:  # (the good frames lie between the refused ones: a write outside a refused frame's range would show in them)
            assert got[128 + int(ooff[i]):128 + int(ooff[i + 1])].tobytes() == want, i
    outs, st2 = hip_ctx.zstd_decode_batch(mixed)
    assert list(st2) == list(st) and [o for o in outs] == [b for _s, b in host]
    # the context decodes a good batch afterwards
    _check(hip_ctx, frames, [d for d, _fr in good])


def test_timer_slot_counts_launches():
    ctx = capi.Context(0)  # (a context of its own: the shared one's timers belong to the tests that switch them on)
    try:
        ctx.timing(True)
        assert ctx.timing_get()["zstd_decode"] == (0.0, 0)
        fr = zstd_cases.ref_frame(b"abcabcabcabcabcabc" * 20, 17)
        assert ctx.zstd_decode_batch([fr, fr])[0] == [b"abcabcabcabcabcabc" * 20] * 2
        ms, n = ctx.timing_get()["zstd_decode"]
        assert n == 1 and ms > 0  # one launch for the batch
        assert ctx.zstd_decode_batch([b"junk"])[1].tolist() == [zd.MALFORMED]  # (refused by its header: nothing is launched)
        assert ctx.timing_get()["zstd_decode"][1] == 1
    finally:
        ctx.close()


def test_mutated_frames_equal_the_cpu_build(hip_ctx, host_decode):
    """the inputs of a run of the sanitizer program that ended clean on the CPU, then on the device: its statuses and, where the
    status is 0, its bytes are the CPU build's"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dump.bin")
        out = zsdec_build.run_selftest(seed=7, rounds=6, dump=path)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
        items = zsdec_build.read_dump(path)
    assert len(items) > 200
    frames = [f for f, _st in items]
    outs, st = hip_ctx.zstd_decode_batch(frames)
    assert list(st) == [s for _f, s in items]
    assert sum(1 for s in st if s == 0) > 20 and sum(1 for s in st if s) > 50
    for i, fr in enumerate(frames):
        if st[i] == 0:
            assert outs[i] == host_decode(fr)[1], i
