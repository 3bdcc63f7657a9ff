"""bench.py --dump-outputs.  CPU: its writer (bench.dump_outputs) on a stand-in archive -- the files it promises, byte values exact
in float32, under 64 MB in all, the same bytes from two calls; run in a child process (importing bench.py sets the HIP runtime's
queue count for the process that imports it).  GPU: the whole bench at a small size with more steps than sample slots -- the dump's
files, the archive they describe, and every step's sample its own."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import bench
stats = {k: 1000.0 + i for i, k in enumerate(bench.DUMP_COUNTERS)}
stats["t_zstd"] = 0.5  # (a timing: not dumped)
bench.dump_outputs(sys.argv[3], sys.argv[2], stats)
"""


def _dump(arc, out):
    subprocess.run([sys.executable, "-c", CHILD, ROOT, arc, out], check=True, timeout=300)
    return {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_dump_outputs_of_an_archive(tmp_path):
    data = np.random.default_rng(3).integers(0, 256, 12_000_000, dtype=np.uint8)
    arc = str(tmp_path / "a.agc")
    data.tofile(arc)
    a = _dump(arc, str(tmp_path / "d1"))
    b = _dump(arc, str(tmp_path / "d2"))
    assert sorted(a) == ["archive_sample", "archive_sha256", "archive_size", "archive_tail", "counters"]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(os.path.getsize(str(tmp_path / "d1" / (n + ".npy"))) for n in a) < 64 << 20
    assert all(np.array_equal(a[n], b[n]) for n in a)
    assert bytes(a["archive_sha256"].astype(np.uint8)) == hashlib.sha256(data.tobytes()).digest()
    assert a["archive_size"].tolist() == [data.size]
    assert np.array_equal(a["archive_tail"], data[-(4 << 20):].astype(np.float32))
    # the bytes at 8 Mi positions drawn with the writer's fixed seed over the archive's size, in ascending order
    pos = np.sort(np.random.default_rng(20240531).integers(0, data.size, 8 << 20))
    assert np.array_equal(a["archive_sample"], data[pos].astype(np.float32))
    assert a["counters"].tolist() == [1000.0 + i for i in range(a["counters"].size)]


def _fasta_seq(txt):
    return b"".join(l for l in txt.split(b"\n") if not l.startswith(b">"))


@pytest.mark.gpu
def test_bench_dump_run_with_reused_sample_slots(tmp_path):
    """51 steps at 30 Mbp: the samples of steps 48-50 are written over slots 0-2 while the run goes on.  The dump must describe
    the archive a second run writes, leave no temporary archive behind, and the refilled samples must be new samples at the
    --div distance from the reference."""
    from agc_amd import build, synth_dev
    build.build_host()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--gbp", "0.03", "--steps", "50", "--warmup", "1"]
    env = {k: v for k, v in os.environ.items() if k != "AGC_BENCH_ARCHIVE"}
    out = tmp_path / "dump"
    r = subprocess.run(cmd + ["--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    c = line["config"]
    assert line["steps"] == 50 and c["sample_slots"] == 48 and c["resampled_samples"] == 3 and c["dump_run"] is True
    assert sorted(os.listdir(out)) == ["archive_sample.npy", "archive_sha256.npy", "archive_size.npy", "archive_tail.npy", "counters.npy"]
    tot = int(synth_dev.contig_lengths(int(0.03e9)).sum())
    assert np.load(out / "counters.npy")[0] == 50 * tot
    arc = tmp_path / "a.agc"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(env, AGC_BENCH_ARCHIVE=str(arc)))
    assert r.returncode == 0, r.stderr[-3000:]
    data = np.fromfile(arc, np.uint8)
    assert bytes(np.load(out / "archive_sha256.npy").astype(np.uint8)) == hashlib.sha256(data.tobytes()).digest()
    assert np.load(out / "archive_size.npy").tolist() == [data.size]
    assert np.array_equal(np.load(out / "archive_tail.npy"), data[-(4 << 20):].astype(np.float32))

    def getset(name):
        g = subprocess.run([build.HOST_BIN, "getset", str(arc), name], capture_output=True, timeout=300)
        assert g.returncode == 0, g.stderr[-1000:]
        return np.frombuffer(_fasta_seq(g.stdout), np.uint8)
    ref = getset("ref")
    assert ref.size == tot
    for new, old in (("s0_48", "w0_0"), ("s0_49", "s0_1"), ("s0_50", "s0_2")):
        a, b = getset(new), getset(old)
        assert a.size == b.size == tot and not np.array_equal(a, b), new
        d = int((a != ref).sum())
        assert 0.8e-3 * tot < d < 1.2e-3 * tot, (new, d)  # (--div 1e-3 from the reference, the old sample's substitutions gone)
        assert int((a != b).sum()) > 1.5e-3 * tot, (new, old)
