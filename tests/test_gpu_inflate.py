"""GPU: agc_hip_bgzf_inflate / _dev (inflate_kernels.hip) on every case of tests/inflate_cases.py -- bytes and statuses those of the CPU
build of the same header (tests/inflate_host) --, guard bytes around the device output, the capacity contract and the timer slot, the
round trip with agc_hip_bgzf and with the device reader's BGZF output, block ranges, and agc_amd/bgzf_in.py in front of
pack_fasta_dev.  A context of its own."""
import os

import numpy as np
import pytest

from agc_amd import capi
from tests import bgzf_cases as BC
from tests import inflate_cases as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY_AGC = os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc")
CASES = dict(IC.cases())
NAMES = list(CASES) + ["bgzf_host_" + n for n in BC.cases()]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """name -> (stream, what the CPU build answers: rc, text, text_off, statuses, whys), each checked against the case's own claim"""
    run = IC.host()
    cases = dict(CASES)
    cases.update(IC.bgzf_host_streams())
    out = {}
    for name, case in cases.items():
        stream, rc, _texts, statuses, _whys, off = IC.expect(case)
        got = run(stream)
        assert (got[0], got[3]) == (rc, statuses) and np.array_equal(got[2], off), name
        out[name] = (stream, got)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_bytes_and_statuses_equal_the_cpu_build_s(ctx, expected, name):
    import torch
    stream, (rc, text, off, statuses, _whys) = expected[name]
    walk_bad = len(statuses) == len(off)
    good = [i for i, s in enumerate(statuses) if s == 0 and i + 1 < len(off)]
    out = np.full(len(text) + 16, 0xAA, np.uint8)
    g_rc, g_len, g_off, g_st = ctx.bgzf_inflate_raw(stream, out.ctypes.data, len(text))
    assert (g_rc, g_len, g_st.tolist()) == (rc, len(text), statuses) and np.array_equal(g_off, off)
    assert (out[len(text):] == 0xAA).all()
    if walk_bad:
        assert (out == 0xAA).all()  # nothing was launched
    else:
        for i in good:
            assert out[int(off[i]):int(off[i + 1])].tobytes() == text[int(off[i]):int(off[i + 1])]
    if rc == capi.OK:
        assert ctx.bgzf_inflate(stream) == text
    else:
        with pytest.raises(capi.AgcHipError) as e:
            ctx.bgzf_inflate(stream)
        assert e.value.code == capi.EINVAL and "member %d" % statuses.index(next(s for s in statuses if s)) in str(e.value)
    # the same into device memory at an odd address, guard bytes on both sides
    d_out = torch.full((64 + len(text) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g_rc, g_len, g_off, g_st = ctx.bgzf_inflate_raw(stream, d_out.data_ptr() + 61, len(text), dev=True)
    back = d_out.cpu().numpy()
    assert (g_rc, g_len, g_st.tolist()) == (rc, len(text), statuses)
    assert (back[:61] == 0x5A).all() and (back[61 + len(text):] == 0x5A).all()
    if not walk_bad:
        for i in good:
            assert back[61 + int(off[i]):61 + int(off[i + 1])].tobytes() == text[int(off[i]):int(off[i + 1])]


def test_capacity_is_checked_before_any_launch(ctx, expected):
    stream, (_rc, text, _off, statuses, _whys) = expected["acgt80_level6"]
    assert capi.Context.bgzf_members(stream) == (capi.OK, len(statuses), len(text))
    out = np.full(len(text), 0xAA, np.uint8)
    ctx.timing(True)
    try:
        assert ctx.bgzf_inflate_raw(stream, out.ctypes.data, len(text) - 1)[:2] == (capi.ECAP, len(text))
        assert ctx.bgzf_inflate_raw(stream, None, 0)[:2] == (capi.ECAP, len(text))
        assert (out == 0xAA).all()
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # before any launch, in every slot
        rc, n, _off, st = ctx.bgzf_inflate_raw(stream, out.ctypes.data, len(text))
        assert (rc, n) == (capi.OK, len(text)) and out.tobytes() == text and not st.any()
        tm = ctx.timing_get()
        assert tm["inflate"][1] == 1 and (capi.K_NAMES + capi.K_NAMES_MORE)[19] == "inflate"
        assert all(k == "inflate" or n == 0 for k, (_ms, n) in tm.items())
    finally:
        ctx.timing(False)
    assert ctx.bgzf_inflate_raw(b"", None, 0)[:2] == (capi.OK, 0)
    assert ctx.bgzf_inflate_raw(stream, None, len(text))[0] == capi.EINVAL  # a capacity, and nowhere to write
    assert capi.Context.bgzf_members(stream[:-1])[:2] == (capi.EINVAL, len(statuses) - 1)


@pytest.mark.parametrize("name", list(BC.cases()))
def test_round_trip_with_the_device_coder(ctx, name):
    data = BC.cases()[name]
    assert ctx.bgzf_inflate(ctx.bgzf(data)) == data


def test_sample_and_block_ranges_on_the_toy_archive(ctx):
    from agc_amd import devread, reader
    host = reader.CAGCFile()
    assert host.Open(TOY_AGC)
    samples = host.ListSample()
    host.Close()
    for i, s in enumerate(samples[:3]):
        r = devread.DeviceReader(ctx, TOY_AGC, gid_base=5000000 + 200000 * i)
        want = r.sample_fasta_parts(s)
        r.close()
        r = devread.DeviceReader(ctx, TOY_AGC, gid_base=5100000 + 200000 * i)
        assert ctx.bgzf_inflate(r.sample_fasta_bgzf(s)) == want
        r.close()


def test_a_block_range_inflates_to_its_slice(ctx):
    """cut with the block offsets of the writer: any run of members is a stream"""
    import torch
    data = BC.cases()["fasta_ll80"]
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    d_out = torch.empty(BC.bound(len(data)), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, off = ctx.bgzf_dev(d_in.data_ptr(), len(data), d_out.data_ptr(), d_out.numel())
    stream = d_out[:n].cpu().numpy().tobytes()
    off = [int(x) for x in off]
    assert len(off) == 4  # three blocks and the EOF member
    for a, b in ((0, 1), (1, 2), (1, 3), (2, 3), (0, 3)):
        assert ctx.bgzf_inflate(stream[off[a]:off[b]]) == data[a * BC.BLOCK:b * BC.BLOCK]
    t, text_off = ctx.bgzf_inflate_dev(stream[off[1]:])
    assert t.cpu().numpy().tobytes() == data[BC.BLOCK:] and [int(x) for x in text_off] == [0, BC.BLOCK, len(data) - BC.BLOCK, len(data) - BC.BLOCK]


def plain_framing(text):
    """FastaReader::read_all_mapped in plain Python -> (ids, begins, ends)"""
    ids, rb, re_ = [], [], []
    n, s = len(text), 0
    while s < n:
        e = s
        while e < n and text[e] not in (10, 13):
            e += 1
        if e >= n:
            break
        nxt = text.find(b">", e + 1)
        nxt = n if nxt < 0 else nxt
        if e <= s + 1 or nxt <= e + 1:
            break
        ids.append(text[s + 1:e])
        rb.append(e + 1)
        re_.append(nxt)
        s = nxt
    return ids, rb, re_


def test_fasta_from_bgzf_in_front_of_pack_fasta(ctx):
    import torch
    from agc_amd import bgzf_in
    rng = np.random.default_rng(5)
    def seq(n, n_run=0):
        a = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
        a[n // 2:n // 2 + n_run] = ord("N")  # escaped blocks
        return b"\n".join(a.tobytes()[p:p + 60] for p in range(0, n, 60))
    text = (b">ctg1 a>b in the header\n" + seq(70000, 1500) + b"\n>ctg2\r\n" + seq(999).replace(b"\n", b"\r\n") + b"\r\n>c3 x\n" + seq(61) + b"\n>last\nACGT")
    ids, rb, re_ = plain_framing(text)
    assert ids == [b"ctg1 a>b in the header", b"ctg2", b"c3 x", b"last"]
    stream = ctx.bgzf(text)
    d_text, g_ids, g_rb, g_re = bgzf_in.fasta_from_bgzf_dev(ctx, stream)
    assert d_text.is_cuda and d_text.cpu().numpy().tobytes() == text
    assert (g_ids, g_rb.tolist(), g_re.tolist()) == (ids, rb, re_)
    up = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    pk_a, bufs_a, off_a = ctx.pack_fasta_dev(d_text, d_text.numel(), g_rb, g_re)
    pk_b, bufs_b, off_b = ctx.pack_fasta_dev(up, up.numel(), rb, re_)
    n = int(off_a[-1])
    assert np.array_equal(off_a, off_b) and pk_a.n_symbols == pk_b.n_symbols == n == 70000 + 999 + 61 + 4
    n_blocks = (n + 1023) // 1024
    esc_a, esc_b = bufs_a[1][:n_blocks].cpu().numpy(), bufs_b[1][:n_blocks].cpu().numpy()
    assert np.array_equal(esc_a >= 0, esc_b >= 0) and 1 <= (esc_a >= 0).sum() <= 3  # the escape index names the same blocks
    words_a, words_b = bufs_a[0][:(n + 15) // 16].cpu().numpy(), bufs_b[0][:(n + 15) // 16].cpu().numpy()
    plain = np.repeat(esc_a < 0, 64)[:words_a.size]  # (an escaped block's symbols are its bytes, not its words)
    assert np.array_equal(words_a[plain], words_b[plain])
    sym_a, sym_b = torch.zeros(n + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.expand_dev(pk_a, sym_a.data_ptr())
    ctx.expand_dev(pk_b, sym_b.data_ptr())
    assert torch.equal(sym_a, sym_b) and int((sym_a[:n] == 4).sum()) == 1500
    # an empty stream, and one without a record
    t0, ids0, b0, e0 = bgzf_in.fasta_from_bgzf_dev(ctx, ctx.bgzf(b""))
    assert t0.numel() == 0 and ids0 == [] and b0.size == 0 and e0.size == 0
    t1, ids1, b1, _e1 = bgzf_in.fasta_from_bgzf_dev(ctx, ctx.bgzf(b">only a header"))
    assert t1.numel() == 14 and ids1 == [] and b1.size == 0
