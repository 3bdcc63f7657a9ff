"""GPU: agc_hip_sample_fasta / _dev (fasta_out_kernels.hip) through the C ABI -- hand-laid plans against text built in numpy
(tests/fastaout_cases.py), the capacity and refusal contract, and agc_amd/devread.py: DeviceReader against the host reader on the
toy archive and on archives written on the spot.  A context of its own: its group ids collide with no other file's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from agc_amd import capi
from tests import collections as COLL
from tests import fastaout_cases as FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")
TOY_AGC = os.path.join(ROOT, "tests", "golden", "toy_c1_reference.agc")
TOY = os.path.join(ROOT, "tests", "golden", "toy_ex")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    c.next_gid = 100  # (the cases' references: every case registers its own, upwards from here)
    yield c
    c.close()


def call_args(ctx, oracle, case):
    """registers the case's references and lays its plan out -> the arguments of Context.sample_fasta"""
    gid0 = ctx.next_gid
    ctx.next_gid += len(case["refs"])
    for i, r in enumerate(case["refs"]):
        ctx.ref_register(gid0 + i, r, FC.MML)
    return FC.plan_arrays(case, gid0, oracle)


def run_case(ctx, oracle, case):
    lay = FC.layout(case)
    FC.check_preconditions(case, lay)  # what the arrangement is there for, before the device runs
    want = FC.expected_text(case)
    got = ctx.sample_fasta(*call_args(ctx, oracle, case))
    assert got.size == len(want)
    if got.tobytes() != want:
        g = np.frombuffer(want, np.uint8)
        i = int(np.flatnonzero(got != g)[0])
        raise AssertionError(f"{case['name']}: text byte {i} of {g.size} is {got[i]!r}, expected {g[i]!r}: ...{want[max(0, i - 20):i + 20]!r}")


# ---- 1. hand-laid plans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FC.small_cases(), ids=lambda c: c["name"])
def test_hand_laid_plan(ctx, oracle, case):
    run_case(ctx, oracle, case)


@pytest.mark.parametrize("case", FC.big_cases(), ids=lambda c: c["name"])
def test_long_contig(ctx, oracle, case):
    run_case(ctx, oracle, case)


# ---- 2. capacity and refusals ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kinds(ctx, oracle):
    case = FC.kinds_case()
    return case, call_args(ctx, oracle, case), FC.expected_text(case)


def raw_call(ctx, args, out):
    return ctx.sample_fasta_raw(ctx.L.agc_hip_sample_fasta, *args, out.ctypes.data if out is not None else None, out.size if out is not None else 0)


def test_capacity_contract(ctx, kinds):
    _case, args, want = kinds
    need = len(want)
    out = np.full(need - 1, 0xAA, np.uint8)
    assert raw_call(ctx, args, out) == (capi.ECAP, need)
    assert (out == 0xAA).all()
    assert raw_call(ctx, args, None) == (capi.ECAP, need)
    out = np.full(need, 0xAA, np.uint8)
    assert raw_call(ctx, args, out) == (capi.OK, need)
    assert out.tobytes() == want
    # no contig at all
    empty = (np.zeros(1, np.uint64), np.zeros(0, capi.SEG_SRC_DTYPE), np.zeros(0, np.uint8), 21, 80, b"", np.zeros(1, np.uint64))
    assert raw_call(ctx, empty, None) == (capi.OK, 0)
    assert ctx.sample_fasta(*empty).size == 0


@pytest.mark.parametrize("shift", [0, 1, 9, 15])
def test_dev_variant_leaves_the_guard_bytes(ctx, kinds, shift):
    """the text at a device address of every kind of alignment: 64 guard bytes behind it, and the bytes in front, stay as they were"""
    import torch
    _case, args, want = kinds
    need = len(want)
    d = torch.full((16 + need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.sample_fasta_dev(*args, d.data_ptr() + shift, need) == need
    got = d.cpu().numpy()
    assert got[shift:shift + need].tobytes() == want
    assert (got[:shift] == 0x5A).all() and (got[shift + need:] == 0x5A).all()


def test_refusals_leave_the_text_untouched(ctx, oracle, kinds):
    """return codes for input the call checks before anything is written; a good call on the same context afterwards"""
    case, args, want = kinds
    ctg_seg, segs, blob, k, ll, names, name_off = args
    d_idx = [i for i, s in enumerate(segs) if s["kind"] == capi.SEG_DELTA]
    r_idx = [i for i, s in enumerate(segs) if s["kind"] == capi.SEG_REF]
    w_idx = [i for i, s in enumerate(segs) if s["kind"] == capi.SEG_RAW and i not in ctg_seg.tolist()]
    assert d_idx and r_idx and w_idx

    def changed(i, blob_=None, **kw):
        s2 = segs.copy()
        for f, v in kw.items():
            s2[f][i] = v
        return (ctg_seg, s2, blob if blob_ is None else blob_, k, ll, names, name_off)

    d0 = d_idx[0]
    o, n = int(segs["off"][d0]), int(segs["n_bytes"][d0])
    torn = blob.copy()
    torn[o + n - 1] = ord("7")  # the delta now ends inside a number: a truncated token
    wild = np.concatenate([blob, np.frombuffer(b"999999,5.", np.uint8)])  # a match far outside the reference
    shorter = np.concatenate([blob, oracle.LZ(case["refs"][0], FC.MML).encode(case["refs"][0][:2000])])
    bad = [
        ("malformed delta", capi.EINVAL, changed(d0, torn)),
        ("match outside the reference", capi.EINVAL, changed(d0, wild, off=blob.size, n_bytes=9)),
        ("delta of another length", capi.EINVAL, changed(d0, shorter, off=blob.size, n_bytes=shorter.size - blob.size, gid=int(segs["gid"][r_idx[0]]))),
        ("declared length off by one", capi.EINVAL, changed(d0, length=int(segs["length"][d0]) + 1)),
        ("reference of another size", capi.EINVAL, changed(r_idx[0], length=int(segs["length"][r_idx[0]]) - 1)),
        ("raw byte count", capi.EINVAL, changed(w_idx[0], n_bytes=int(segs["n_bytes"][w_idx[0]]) - 1)),
        ("shorter than the overlap", capi.EINVAL, changed(w_idx[0], n_bytes=k - 1, length=k - 1)),
        ("unknown kind", capi.EINVAL, changed(d0, kind=3)),
        ("bytes past the buffer", capi.EINVAL, changed(d0, off=blob.size - 1)),
        ("offset past the buffer", capi.EINVAL, changed(w_idx[0], off=blob.size + 1)),
        ("unregistered group of a delta", capi.ENOREF, changed(d0, gid=7)),
        ("unregistered group of a reference", capi.ENOREF, changed(r_idx[0], gid=1 << 30)),
    ]
    assert int(segs["gid"][r_idx[0]]) == int(segs["gid"][d0])  # "another length": a delta that is well formed against ITS reference
    for what, code, a in bad:
        out = np.full(len(want) + 4096, 0xAA, np.uint8)
        rc, _n = raw_call(ctx, a, out)
        assert rc == code, what
        assert (out == 0xAA).all(), what
        assert "segment" in ctx.L.agc_hip_last_error(ctx.h).decode(), what
    # the dev variant refuses the same way and leaves device memory alone
    import torch
    d = torch.full((len(want) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc, _n = ctx.sample_fasta_raw(ctx.L.agc_hip_sample_fasta_dev, *bad[0][2], d.data_ptr(), len(want))
    assert rc == capi.EINVAL and bool((d == 0x5A).all())
    # the context is as good as before
    assert ctx.sample_fasta(*args).tobytes() == want


# ---- 3. DeviceReader against the host reader -------------------------------------------------------------------------------------
def parse_fasta(path):
    out, name, seq = [], None, []
    with open(path, "rt") as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(seq).upper()))
                name, seq = line[1:], []
            else:
                seq.append(line)
    if name is not None:
        out.append((name, "".join(seq).upper()))
    return out


def fasta_text(contigs, line=80):
    t = []
    for n, s in contigs:
        t.append(">" + n + "\n")
        for i in range(0, len(s), line):
            t.append(s[i:i + line] + "\n")
    return "".join(t).encode()


def test_device_reader_on_the_toy_archive(ctx):
    from agc_amd import devread, reader
    host = reader.CAGCFile()
    assert host.Open(TOY_AGC)
    r = devread.DeviceReader(ctx, TOY_AGC, gid_base=20000)
    for s in host.ListSample():
        for ll in (80, 40):
            want = host.GetSampleFasta(s, ll)
            assert r.sample_fasta(s, ll) == want, (s, ll)
            assert want == fasta_text(parse_fasta(os.path.join(TOY, s + ".fa")), ll)
        assert r.sample_fasta_dev(s, 80).cpu().numpy().tobytes() == host.GetSampleFasta(s, 80)
    with pytest.raises(KeyError):
        r.sample_fasta("no such sample")
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


def test_device_reader_on_syn_mixed(ctx, written):
    """N-runs, IUPAC codes, indels: every sample, twice (the second time its references are registered already), two line lengths"""
    from agc_amd import devread, reader
    agc, files = written["syn_mixed"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    r = devread.DeviceReader(ctx, agc, gid_base=30000)
    for f in files:
        s = os.path.basename(f)[:-3]
        want = host.GetSampleFasta(s, 80)
        assert want == fasta_text(parse_fasta(f))
        assert r.sample_fasta(s) == want, s
        n_reg = len(r.registered)
        assert r.sample_fasta(s) == want and len(r.registered) == n_reg, s
        assert r.sample_fasta(s, 0) == host.GetSampleFasta(s, 0), s
    r.close()
    host.Close()


def test_device_reader_on_syn_c4_twin(ctx, written):
    """pieces in either orientation, hundreds of contigs, scaffold gaps: two samples in turn, one of them as a device tensor"""
    from agc_amd import devread, reader
    agc, files = written["syn_c4_twin"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    r = devread.DeviceReader(ctx, agc, gid_base=100000)
    names = [os.path.basename(f)[:-3] for f in files]
    plan = host.GetSamplePlan(names[1])
    assert plan["rc"].any() and (plan["kind"] == reader.PLAN_RAW).any() and plan["ctg_seg"].size > 200
    for s, f in ((names[1], files[1]), (names[4], files[4])):
        want = host.GetSampleFasta(s, 80)
        assert want == fasta_text(parse_fasta(f))
        assert r.sample_fasta(s) == want, s
    assert r.sample_fasta_dev(names[1], 60).cpu().numpy().tobytes() == host.GetSampleFasta(names[1], 60)
    r.close()
    host.Close()


def test_beside_an_encode_in_flight(ctx, oracle, written):
    """a sample's text while lane 0 encodes: the text is right and the encode delivers what the synchronous call does"""
    import torch
    from agc_amd import devread, reader
    rng = np.random.default_rng(9)
    gids = np.arange(8) + 90000
    refs = [rng.integers(0, 4, size=20_000, dtype=np.uint8) for _ in gids]
    for g, rf in zip(gids, refs):
        ctx.ref_register(int(g), rf, 20)
    from agc_amd import synth
    texts = [synth.mutate(rng, rf, 0.01, n_runs=1) for rf in refs]
    ln = np.array([t.size for t in texts], np.uint32)
    off = np.zeros(len(texts), np.uint64)
    off[1:] = np.cumsum(ln[:-1].astype(np.uint64))
    d = torch.from_numpy(np.concatenate(texts + [np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    pk = ctx.sample_pack(d.data_ptr(), int(ln.sum()))
    want_enc, want_off = ctx.lz_encode_batch_packed(pk, gids, off, ln)
    agc, files = written["syn_mixed"]
    host = reader.CAGCFile()
    assert host.Open(agc)
    r = devread.DeviceReader(ctx, agc, gid_base=30000 + 40000)
    s = os.path.basename(files[2])[:-3]
    r.plan(s)  # (its references registered before the encode starts: a registration in between is not what this test is about)
    ctx.lz_encode_begin_packed(pk, gids, off, ln)
    text = r.sample_fasta(s)
    got_enc, got_off = ctx.lz_encode_end()
    assert text == host.GetSampleFasta(s, 80)
    assert np.array_equal(got_enc, want_enc) and np.array_equal(got_off, want_off)
    for i, t in enumerate(texts):
        assert np.array_equal(got_enc[int(got_off[i]):int(got_off[i + 1])], oracle.LZ(refs[i], 20).encode(t)), i
    r.close()
    host.Close()


# ---- 4. the timer slot -------------------------------------------------------------------------------------------------------------
def test_timer_slot_counts_launches(ctx, kinds):
    _case, args, want = kinds
    assert capi.K_NAMES[14] == "fasta_out" and len(capi.K_NAMES) == 15
    ctx.timing(True)
    try:
        assert ctx.timing_get()["fasta_out"] == (0.0, 0)
        assert ctx.sample_fasta(*args).tobytes() == want
        ms, n = ctx.timing_get()["fasta_out"]
        assert n == 2 and ms > 0  # the copies of the REF / RAW segments, and the text
        raw_only = (np.array([0, 1], np.uint64), np.array([(capi.SEG_RAW, 0, 0, 0, 0, 0, 0)], capi.SEG_SRC_DTYPE), np.zeros(0, np.uint8), 21, 80, b"x",
                    np.array([0, 1], np.uint64))
        assert ctx.sample_fasta(*raw_only).tobytes() == b">x\n"
        assert ctx.timing_get()["fasta_out"][1] == 3  # (a segment without symbols is not copied: the text kernel alone)
        assert ctx.timing_get()["decode_write"][1] == 1
    finally:
        ctx.timing(False)
