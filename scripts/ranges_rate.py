"""Batches of contig ranges from the archive's stored parts on the GPU (agc_amd/devread.py: DeviceReader.ranges_dev) next to the two ways
there were before, on the 300 Mbp synthetic sample of scripts/sample_parts_rate.py.

    python scripts/ranges_rate.py [symbols=3e8] [divergence=1e-3] [repeats=5]

Four batches of seeded random ranges on the sample "smp": 1, 256 and 4 096 ranges of 1 kb, and 256 ranges of 100 kb.  Per batch, each
the median of `repeats` calls of a reader whose references are registered (a warm-up call of the same batch registers them):
  ranges_dev               the call, the symbols left on the device as letters; and its kernel time by HIP events
                           (agc_hip_timing_get): the ranges, zstd_decode and parts_unpack slots
  host GetCtgSeq loop      the host reader's GetCtgSeq, one range per call on one thread, caches warm (a pass of the same batch first)
and once for all batches: sample_fasta_parts_dev of the whole sample (a later call), the only way to a range on the device before.
The ranges' letters are compared with the host reader's before anything is timed.  Prints one JSON line at the end."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from agc_amd import capi, devread, reader, synth, synth_dev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")
BATCHES = (("1x1kb", 1, 1000), ("256x1kb", 256, 1000), ("4096x1kb", 4096, 1000), ("256x100kb", 256, 100_000))


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def main():
    total = int(float(sys.argv[1])) if len(sys.argv) > 1 else 300_000_000
    d = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-3
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(2025)
    med = statistics.median
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        ln = synth_dev.contig_lengths(total)
        names = [f"chr{i + 1}" for i in range(len(ln))]
        ref = [synth.random_seq(rng, int(n)) for n in ln]
        synth.to_fasta(os.path.join(tmp, "ref.fa"), ref, names)
        synth.to_fasta(os.path.join(tmp, "smp.fa"), [synth.mutate(rng, c, d) for c in ref], names)
        del ref
        agc = os.path.join(tmp, "c.agc")
        subprocess.check_call([AGC_AMD, "create", "-t", "16", "-o", agc, os.path.join(tmp, "ref.fa"), os.path.join(tmp, "smp.fa")], stderr=subprocess.DEVNULL)
        print(f"{len(ln)} contigs, {sum(int(n) for n in ln) / 1e6:.1f} Mbp per sample, archive of {os.path.getsize(agc) / 1e6:.1f} MB, prepared in {time.time() - t0:.1f} s", flush=True)
        host = reader.CAGCFile()
        assert host.Open(agc)
        lens = [host.GetCtgLen("smp", n) for n in names]
        ctx = capi.Context(0)
        r = devread.DeviceReader(ctx, agc, gid_base=0)
        res = {"symbols": int(sum(lens)), "repeats": repeats}
        qrng = np.random.default_rng(7)
        for label, n_q, size in BATCHES:
            queries = []
            for _ in range(n_q):
                c = int(qrng.integers(len(names)))
                f = int(qrng.integers(max(lens[c] - size, 1)))
                queries.append(("smp", names[c], f, f + size - 1))
            want = [host.GetCtgSeq(*q).encode() for q in queries]  # (warms the host reader's caches for this batch)
            assert r.ranges(queries) == want, label  # (registers the batch's references, grows the buffers)
            dev_s, slots = [], []
            for _ in range(repeats):
                ctx.timing(True)  # (resets the slots)
                dev_s.append(timed(lambda: r.ranges_dev(queries))[0])
                tm = ctx.timing_get()
                slots.append({k: tm[k][0] for k in ("ranges", "zstd_decode", "parts_unpack", "decode_scan")})
            ctx.timing(False)
            host_s = [timed(lambda: [host.GetCtgSeq(*q) for q in queries])[0] for _ in range(repeats)]
            res[label] = {"symbols": sum(len(w) for w in want), "ranges_dev_s": med(dev_s), "host_getctgseq_loop_s": med(host_s),
                          **{k + "_ms": med(x[k] for x in slots) for k in slots[0]}}
            print(f"  {label:10s} {res[label]}", flush=True)
        whole = devread.DeviceReader(ctx, agc, gid_base=1_000_000)
        whole.sample_fasta_parts_dev("smp", 80)
        res["sample_fasta_parts_dev_again_s"] = med(timed(lambda: whole.sample_fasta_parts_dev("smp", 80))[0] for _ in range(repeats))
        whole.close()
        r.close()
        host.Close()
        ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
