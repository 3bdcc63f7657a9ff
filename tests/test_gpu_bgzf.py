"""GPU: agc_hip_bgzf / _dev (bgzf_kernels.hip) on every case of tests/bgzf_cases.py -- the stream byte for byte the one the CPU build of
the same header writes (tests/bgzf_host) --, the capacity contract, the timer slot, and agc_hip_sample_fasta_parts_bgzf / _dev through
agc_amd/devread.py on the toy archive and on an archive written on the spot.  A context of its own."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from agc_amd import capi
from tests import bgzf_cases as BC
from tests import collections as COLL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")
TOY_AGC = os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """name -> (data, the CPU harness's stream, its block offsets), each walked against zlib"""
    enc = BC.host_encoder()
    out = {}
    for name, data in BC.cases().items():
        stream, off = enc(data)
        BC.walk(stream, data, off)
        out[name] = (data, stream, off)
    return out


@pytest.mark.parametrize("name", list(BC.cases()))
def test_stream_equals_the_cpu_build_s(ctx, expected, name):
    import torch
    data, want, want_off = expected[name]
    got, off = ctx.bgzf(data, want_offsets=True)
    assert got == want and np.array_equal(off, want_off)
    # the same between device buffers: guard bytes on both sides of d_out, an odd d_in and an odd d_out
    cap = BC.bound(len(data))
    d_in = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda")
    d_in[3:3 + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else d_in[3:3]
    d_out = torch.full((64 + cap + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, off = ctx.bgzf_dev(d_in.data_ptr() + 3, len(data), d_out.data_ptr() + 61, cap)
    back = d_out.cpu().numpy()
    assert n == len(want) and np.array_equal(off, want_off)
    assert back[61:61 + n].tobytes() == want
    assert (back[:61] == 0x5A).all() and (back[61 + n:] == 0x5A).all()


def test_capacity_is_checked_before_any_launch(ctx, expected):
    data = expected["fasta_65281"][0]
    cap = BC.bound(len(data))
    assert capi.Context.bgzf_bound(len(data)) == cap == len(data) + 2 * 31 + 28
    d = np.frombuffer(data, np.uint8)
    out = np.full(cap, 0xAA, np.uint8)
    ctx.timing(True)
    try:
        assert ctx.bgzf_raw(d.ctypes.data, d.size, out.ctypes.data, cap - 1) == (capi.ECAP, cap)
        assert ctx.bgzf_raw(d.ctypes.data, d.size, None, 0) == (capi.ECAP, cap)
        assert (out == 0xAA).all()
        assert all(n == 0 for _ms, n in ctx.timing_get().values())  # before any launch, in every slot
        rc, n = ctx.bgzf_raw(d.ctypes.data, d.size, out.ctypes.data, cap)
        assert rc == capi.OK and out[:n].tobytes() == expected["fasta_65281"][1] and (out[n:] == 0xAA).all()
        tm = ctx.timing_get()
        assert tm["bgzf"][1] == 2 and capi.K_NAMES_MORE[3] == "bgzf"  # the block launch and the placing launch
        assert all(k == "bgzf" or n == 0 for k, (_ms, n) in tm.items())
    finally:
        ctx.timing(False)
    assert ctx.bgzf_raw(None, 5, out.ctypes.data, cap)[0] == capi.EINVAL        # bytes, and nowhere to read them
    assert ctx.bgzf_raw(d.ctypes.data, d.size, None, cap)[0] == capi.EINVAL     # a capacity, and nowhere to write
    assert ctx.bgzf_raw(None, 65280 << 32, None, 0)[0] == capi.EINVAL           # 2^32 blocks
    rc, n = ctx.bgzf_raw(None, 0, out.ctypes.data, 28)
    assert (rc, n) == (capi.OK, 28) and out[:28].tobytes() == BC.EOF_MEMBER


# ---- agc_hip_sample_fasta_parts_bgzf through the device reader ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """an archive written on the spot by the product's CLI -> (archive, input files)"""
    d = tmp_path_factory.mktemp("syn_mixed")
    args, _ = COLL.CONFIGS["syn_mixed"]
    files = COLL.build("syn_mixed", str(d / "in"))
    agc = str(d / "o.agc")
    r = subprocess.run([AGC_AMD, "create"] + args + ["-t", "8", "-o", agc] + files, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and os.path.exists(agc), r.stderr[-2000:]
    return agc, files


def check_sample(ctx, agc, sample, base, multi_block):
    """both line lengths, each with a fresh reader and group range: the host variant, the device variant, and the refused call"""
    from agc_amd import devread
    for i, ll in enumerate((0, 80)):
        plain = devread.DeviceReader(ctx, agc, gid_base=base + 3 * i * 100000)
        want = plain.sample_fasta_parts(sample, ll)
        plain.close()
        assert not multi_block or len(want) > BC.BLOCK  # the text spans more than one block
        r = devread.DeviceReader(ctx, agc, gid_base=base + (3 * i + 1) * 100000)
        args, (names, name_off), new = r.parts(sample)
        gids = args[0]["gid"][args[0]["content"] != capi.PART_PACK].tolist()
        out = np.full(BC.bound(len(want)), 0xAA, np.uint8)
        ctx.timing(True)
        try:
            rc, need, text = ctx.sample_fasta_parts_bgzf_raw(*args, ll, names, name_off, out.ctypes.data, out.size - 1)
            assert (rc, need, text) == (capi.ECAP, BC.bound(len(want)), len(want))
            assert all(n == 0 for _ms, n in ctx.timing_get().values())
        finally:
            ctx.timing(False)
        assert (gids or not multi_block) and (out == 0xAA).all() and not any(ctx.ref_registered(g) for g in gids)  # (agc_hip_ref_get answers ENOREF for each)
        off = np.zeros((len(want) + BC.BLOCK - 1) // BC.BLOCK + 1, np.uint64)
        rc, n, text = ctx.sample_fasta_parts_bgzf_raw(*args, ll, names, name_off, out.ctypes.data, out.size, block_off=off)
        assert (rc, text) == (capi.OK, len(want)) and (out[n:] == 0xAA).all() and all(ctx.ref_registered(g) for g in gids)
        stream = out[:n].tobytes()
        assert gzip.decompress(stream) == want
        BC.walk(stream, want, off)
        r.registered.update(new)
        assert r.sample_fasta_bgzf(sample, ll) == stream  # the reader's own call, its references known now
        r.close()
        rd = devread.DeviceReader(ctx, agc, gid_base=base + (3 * i + 2) * 100000)
        t, off_d = rd.sample_fasta_bgzf_dev(sample, ll)
        assert t.cpu().numpy().tobytes() == stream and np.array_equal(off_d, off)
        rd.close()


def test_sample_on_the_toy_archive(ctx):
    from agc_amd import reader
    host = reader.CAGCFile()
    assert host.Open(TOY_AGC)
    sample = max(host.ListSample(), key=lambda s: len(host.GetSampleFasta(s, 80)))
    host.Close()
    check_sample(ctx, TOY_AGC, sample, 1000000, multi_block=False)  # (the toy's samples are a few dozen bytes)


def test_sample_on_an_archive_written_on_the_spot(ctx, written):
    agc, files = written
    check_sample(ctx, agc, os.path.basename(files[2])[:-3], 2000000, multi_block=True)
