"""GPU: agc_amd/devread.py: DeviceReader against the host reader on the fuzz archives of tests/readfuzz_cases.py -- every k, min-match
lengths up to 32, segments barely longer than k, contigs shorter than k, -c, -a, archives grown by appends, groups of several packs,
a contig name twice in a sample.  The archives are written once per case by the product's CLI; three of them a second time by the
reference CLI (oracle/_ref/agc, where it is built).  Per case and stage a test of its own: the precondition (the host reader gives
back the input), whole samples three ways in, BGZF out and in, batches of contig ranges.  What the cases supply is asserted in
tests/test_read_fuzz_cpu.py.  A context of its own; every reader registers its groups in a range of its own."""
import gzip
import os

import numpy as np
import pytest

from agc_amd import capi
from tests import fuzz
from tests import readfuzz_cases as RF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")
REF_AGC = os.path.join(ROOT, "oracle", "_ref", "agc")
REF_ENV = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "oracle", "_ref", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
ALPHA = np.frombuffer(b"ACGTNRYSWKMBDHVU", np.uint8)
CASES = range(len(RF.SEEDS))
REF_WRITTEN = [i for i, (seed, kw) in enumerate(RF.SEEDS) if seed in (3, 30, 93) and not kw]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """i -> (archive, case, files) of RF.SEEDS[i], written once by the product's CLI (fuzz.run_case: every step under a timeout)"""
    done = {}

    def get(i):
        if i not in done:
            seed, kw = RF.SEEDS[i]
            done[i] = RF.write(AGC_AMD, seed, tmp_path_factory.mktemp(f"readfuzz_{RF.IDS[i]}"), **kw)
        return done[i]
    return get


class Readers:
    """fresh DeviceReaders on one context, each with as many group ids of its own as its archive has groups"""

    def __init__(self, ctx):
        self.ctx, self.next = ctx, 0

    def open(self, path, host):
        from agc_amd import devread
        n = 16 + max([0] + [int(g) for s in host.ListSample() for g in host.GetSamplePlan(s)["groups"][-1:]])
        r = devread.DeviceReader(self.ctx, path, gid_base=self.next)
        self.next += n + 1
        return r


@pytest.fixture(scope="module")
def readers(ctx):
    return Readers(ctx)


def opened(path):
    from agc_amd import reader
    host = reader.CAGCFile()
    assert host.Open(path)
    return host


def check_samples(readers, path):
    """every sample: the stored parts decoded on the device (three line lengths, and left on the device), and the plan of segments
    the host decoded, on a second reader; a second call registers nothing new and hands in only pack parts"""
    host = opened(path)
    r, r2 = readers.open(path, host), readers.open(path, host)
    samples = host.ListSample()
    assert samples
    for s in samples:
        want = {ll: host.GetSampleFasta(s, ll) for ll in (80, 0, 61)}
        assert want[80] is not None and want[80].startswith(b">")
        for ll in (80, 0, 61):
            assert r.sample_fasta_parts(s, ll) == want[ll], (s, ll)
        reg = set(r.registered)
        assert set(host.GetSamplePlan(s)["groups"].tolist()) <= reg
        (parts, *_rest), _names, new = r.parts(s)
        assert not new and (parts["content"] == capi.PART_PACK).all()
        assert r.sample_fasta_parts(s) == want[80] and r.registered == reg, s
        for ll in (80, 0):
            assert r2.sample_fasta(s, ll) == want[ll], (s, ll)
        assert r.sample_fasta_parts_dev(s, 61).cpu().numpy().tobytes() == want[61], s
    assert r.registered == r2.registered
    r.close()
    r2.close()
    host.Close()


def check_ranges(readers, path, seed):
    """readfuzz_cases.queries, three ways: letters, codes, left on the device"""
    host = opened(path)
    queries, in_batch, in_archive = RF.queries(host, seed)
    # the condition on the inputs: a window in every kind x orientation the archive has
    assert in_batch == in_archive and in_archive, (sorted(in_batch), sorted(in_archive))
    want = [host.GetCtgSeq(s, name, f, t).encode() for s, name, f, t in queries]
    assert any(len(w) == 0 for w in want) and sum(len(w) for w in want) > 100
    r = readers.open(path, host)
    got = r.ranges(queries)
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert g == w, (q, queries[q])
    for q, (g, w) in enumerate(zip(r.ranges(queries, letters=False), want)):
        assert ALPHA[np.frombuffer(g, np.uint8)].tobytes() == w, (q, queries[q])
    d, off = r.ranges_dev(queries)
    assert d.cpu().numpy().tobytes() == b"".join(want)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64))
    r.close()
    host.Close()


@pytest.mark.parametrize("i", CASES, ids=RF.IDS)
def test_precondition_the_host_reader_gives_back_the_input(archives, i):
    path, _case, files = archives(i)
    assert fuzz.archive_round_trips(path, files)


@pytest.mark.parametrize("i", CASES, ids=RF.IDS)
def test_samples(readers, archives, i):
    check_samples(readers, archives(i)[0])


@pytest.mark.parametrize("i", CASES, ids=RF.IDS)
def test_bgzf(ctx, readers, archives, i):
    """the text compressed where it is made: read back by zlib and by the device's own inflate"""
    path = archives(i)[0]
    host = opened(path)
    r = readers.open(path, host)
    for s in host.ListSample():
        want = host.GetSampleFasta(s, 80)
        gz = r.sample_fasta_bgzf(s)
        assert gzip.decompress(gz) == want, s
        assert ctx.bgzf_inflate(gz) == want, s
    r.close()
    host.Close()


@pytest.mark.parametrize("i", CASES, ids=RF.IDS)
def test_ranges(readers, archives, i):
    check_ranges(readers, archives(i)[0], RF.SEEDS[i][0])


@pytest.mark.parametrize("i", REF_WRITTEN, ids=[RF.IDS[i] for i in REF_WRITTEN])
def test_reference_written_archives(readers, tmp_path, i):
    """the same cases as the reference CLI writes them (one thread: with a repeated contig name its records depend on the thread that
    writes last); none is an `append -c` case, which the reference dies on"""
    if not os.path.exists(REF_AGC):
        pytest.skip("oracle/_ref/agc not prebuilt")
    seed, kw = RF.SEEDS[i]
    path, case, files = RF.write(REF_AGC, seed, tmp_path, threads="1", env=REF_ENV, **kw)
    assert not ("-c" in case["carry"] and len(case["steps"]) > 1)
    assert fuzz.archive_round_trips(path, files)
    check_samples(readers, path)
    check_ranges(readers, path, seed)
