"""A sample's FASTA text from the archive's stored parts on the GPU (agc_amd/devread.py: DeviceReader.sample_fasta_parts) next to the
two readers that decode zstd on the host, on the workload of scripts/sample_fasta_rate.py.

    python scripts/sample_parts_rate.py [symbols=3e8] [divergence=1e-3] [repeats=5]

Four rows, each the median of `repeats` calls:
  host reader, cold        a fresh CAGCFile per call: its zstd and tuple decoding included
  DeviceReader.sample_fasta            first call of a fresh reader (plan on the host, references registered one by one), and a later call
  DeviceReader.sample_fasta_parts      first call of a fresh reader: every reference part decoded, unpacked and registered on the device
  DeviceReader.sample_fasta_parts      second call: the references are registered, only the packs are handed in
and the kernel time of the new path's slots by HIP events (agc_hip_timing_get): parts_unpack and zstd_decode, first and second call.
A fresh reader takes a group range of its own on the one context.  Prints one JSON line at the end."""
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
GID_STEP = 100_000  # more than the groups of the collection: every fresh reader registers under a range of its own


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def main():
    total = int(float(sys.argv[1])) if len(sys.argv) > 1 else 300_000_000
    d = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-3
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(2025)
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

        def cold_host():
            h = reader.CAGCFile()
            assert h.Open(agc)
            text = h.GetSampleFasta("smp", 80)
            h.Close()
            return text

        want = cold_host()  # (the file is in the page cache from here on, for every row alike)
        host_s = [timed(cold_host)[0] for _ in range(repeats)]

        ctx = capi.Context(0)
        warm = devread.DeviceReader(ctx, agc, gid_base=0)  # buffers, pinned memory and the arena grow here, outside every row
        assert warm.sample_fasta("smp", 80) == want
        base = GID_STEP
        plan_first_s, plan_again_s, parts_first_s, parts_again_s = [], [], [], []
        slots = {"first": [], "again": []}
        n_parts = {}
        for _ in range(repeats):
            r = devread.DeviceReader(ctx, agc, gid_base=base)
            r._pinned, r._pinned_cap = warm._pinned, warm._pinned_cap
            s, text = timed(lambda: r.sample_fasta("smp", 80))
            assert text == want
            plan_first_s.append(s)
            plan_again_s.append(timed(lambda: r.sample_fasta("smp", 80))[0])
            r._pinned = None
            r.close()
            base += GID_STEP
        warm_parts = devread.DeviceReader(ctx, agc, gid_base=base)
        warm_parts._pinned, warm_parts._pinned_cap = warm._pinned, warm._pinned_cap
        assert warm_parts.sample_fasta_parts("smp", 80) == want, "the text from the parts differs from the host reader's"
        base += GID_STEP
        ctx.timing(True)
        for _ in range(repeats):
            r = devread.DeviceReader(ctx, agc, gid_base=base)
            r._pinned, r._pinned_cap = warm._pinned, warm._pinned_cap
            for which, into in (("first", parts_first_s), ("again", parts_again_s)):
                n_parts[which] = int(r.parts("smp")[0][0].size)
                ctx.timing(True)  # (resets the slots)
                s, text = timed(lambda: r.sample_fasta_parts("smp", 80))
                assert text == want
                into.append(s)
                tm = ctx.timing_get()
                slots[which].append({k: tm[k][0] for k in ("parts_unpack", "zstd_decode", "refstore", "index", "decode_scan", "decode_write", "fasta_out")})
            r._pinned = None
            r.close()
            base += GID_STEP
        ctx.timing(False)
        med = statistics.median
        res = {"symbols": int(sum(int(n) for n in ln)), "text_bytes": len(want), "repeats": repeats,
               "host_reader_cold_s": med(host_s), "sample_fasta_first_s": med(plan_first_s), "sample_fasta_again_s": med(plan_again_s),
               "sample_fasta_parts_first_s": med(parts_first_s), "sample_fasta_parts_again_s": med(parts_again_s),
               "parts_first": n_parts["first"], "parts_again": n_parts["again"]}
        for which in ("first", "again"):
            for k in slots[which][0]:
                res[f"{k}_ms_{which}"] = med(x[k] for x in slots[which])
        warm_parts._pinned = None
        warm_parts.close()
        warm.close()
        ctx.close()
    for k_, v in res.items():
        print(f"  {k_:32s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
