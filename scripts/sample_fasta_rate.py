"""Rate of a sample's FASTA text written on the GPU (agc_amd/devread.py: DeviceReader.sample_fasta) next to the host reader
(agc_amd/reader.py: CAGCFile.GetSampleFasta) on the same archive.

    python scripts/sample_fasta_rate.py [symbols=3e8] [divergence=1e-3] [repeats=5]

A synthetic collection from the package's own generator (agc_amd.synth; contigs proportioned like GRCh38, synth_dev.contig_lengths):
a reference and one sample at the given divergence, written as FASTA files and compressed by `agc_amd create` with default
parameters.  After one warm-up call of each reader: the median of `repeats` calls, and for the device reader its stages -- the
plan (the host reader's zstd and tuple decoding, cutting the packs), the registration of the references (once per archive, not
per call), the device call (upload, kernels, the copy of the text into pinned memory) -- and the kernels by HIP events
(agc_hip_timing_get): the text kernel's slot also holds the copies of the reference segments.  GB/s of the text slot: the symbol
bytes read plus the text bytes written.  Prints one JSON line at the end."""
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

        host = reader.CAGCFile()
        assert host.Open(agc)
        want = host.GetSampleFasta("smp", 80)  # warm-up (its caches hold the decoded parts from here on) and the text to compare with
        host_s = []
        for _ in range(repeats):
            t = time.perf_counter()
            host.GetSampleFasta("smp", 80)
            host_s.append(time.perf_counter() - t)

        ctx = capi.Context(0)
        r = devread.DeviceReader(ctx, agc)
        t = time.perf_counter()
        p = r.file.GetSamplePlan("smp")
        plan_first_s = time.perf_counter() - t
        t = time.perf_counter()
        args = r.plan("smp")
        register_s = time.perf_counter() - t - plan_first_s  # (plan() gets the plan again: what is left is the registration)
        assert r.sample_fasta("smp", 80) == want, "the device reader's text differs from the host reader's"
        ctx.timing(True)
        plan_s, call_s, whole_s = [], [], []
        for _ in range(repeats):
            t = time.perf_counter()
            args = r.plan("smp")
            t1 = time.perf_counter()
            ctg_seg, segs, data, nm, no = args
            rc, n = ctx.sample_fasta_raw(ctx.L.agc_hip_sample_fasta, ctg_seg, segs, data, r.k, 80, nm, no, r._pinned, r._pinned_cap)
            t2 = time.perf_counter()
            assert rc == capi.OK and n == len(want)
            plan_s.append(t1 - t)
            call_s.append(t2 - t1)
        for _ in range(repeats):
            t = time.perf_counter()
            r.sample_fasta("smp", 80)
            whole_s.append(time.perf_counter() - t)
        tm = ctx.timing_get()
        n_timed = 2 * repeats
        text_ms = tm["fasta_out"][0] / n_timed
        sym_bytes = int(p["length"].astype(np.uint64).sum())
        med = statistics.median
        res = {"symbols": int(sum(int(n) for n in ln)), "text_bytes": len(want), "segments": int(p["kind"].size), "delta_bytes": int(p["bytes"].size),
               "host_reader_s": med(host_s), "device_reader_s": med(whole_s), "plan_s": med(plan_s), "plan_first_s": plan_first_s, "register_once_s": register_s,
               "call_s": med(call_s), "decode_scan_ms": tm["decode_scan"][0] / n_timed, "decode_write_ms": tm["decode_write"][0] / n_timed,
               "fasta_out_ms": text_ms, "fasta_out_launches_per_call": tm["fasta_out"][1] / n_timed,
               "fasta_out_GBps": (sym_bytes + len(want)) / (text_ms / 1e3) / 1e9 if text_ms else None, "repeats": repeats}
        r.close()
        host.Close()
        ctx.close()
    for k_, v in res.items():
        print(f"  {k_:28s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
