"""A sample's FASTA text as a BGZF stream, compressed on the GPU (agc_amd/devread.py: DeviceReader.sample_fasta_bgzf), next to the
same text handed to the host uncompressed, on the workload of scripts/sample_parts_rate.py.

    python scripts/bgzf_rate.py [symbols=3e8] [divergence=1e-3] [repeats=5]

One reader whose references are registered (the later call of scripts/sample_parts_rate.py); after a warm-up of every row the rows
take turns, `repeats` times, and each reports its median:
  (a) sample_fasta_parts       the text to the host: the baseline
  (b) sample_fasta_bgzf        the BGZF stream to the host
  (c) sample_fasta_bgzf_dev    the BGZF stream left on the device
  (d) the bgzf slot            kernel time of bgzf_block_kernel + bgzf_place_kernel by HIP events (agc_hip_timing_get), from the calls of (b)
  (e) Python's zlib            levels 1 and 6, one thread, on the first 32 MiB of the same text (seconds per GB and ratio), once each
The first stream of (b) is checked with gzip.decompress against (a)'s text before anything is timed.  Also: the ratio of the coder on a
text of N lines, its known weak case.  Prints one JSON line at the end."""
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from agc_amd import capi, devread, synth, synth_dev  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGC_AMD = os.path.join(ROOT, "agc_amd", "bin", "agc_amd")


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

        ctx = capi.Context(0)
        r = devread.DeviceReader(ctx, agc, gid_base=0)
        want = r.sample_fasta_parts("smp", 80)  # registers the references; buffers and pinned memory grow here
        gz = r.sample_fasta_bgzf("smp", 80)
        assert gzip.decompress(gz) == want, "the BGZF stream does not decompress to the text"
        t, off = r.sample_fasta_bgzf_dev("smp", 80)
        assert t.cpu().numpy().tobytes() == gz and int(off[-1]) + 28 == len(gz)
        del t
        print(f"text {len(want)} bytes, stream {len(gz)} bytes ({len(gz) / len(want):.4f}), {off.size - 1} blocks", flush=True)
        text_s, gz_s, gz_dev_s, slot_ms = [], [], [], []
        for _ in range(repeats):
            text_s.append(timed(lambda: r.sample_fasta_parts("smp", 80))[0])
            ctx.timing(True)  # (resets the slots)
            gz_s.append(timed(lambda: r.sample_fasta_bgzf("smp", 80))[0])
            slot_ms.append(ctx.timing_get()["bgzf"][0])
            ctx.timing(False)
            gz_dev_s.append(timed(lambda: r.sample_fasta_bgzf_dev("smp", 80))[0])
        med = statistics.median
        res = {"symbols": int(sum(int(n) for n in ln)), "text_bytes": len(want), "stream_bytes": len(gz), "ratio": len(gz) / len(want), "repeats": repeats,
               "sample_fasta_parts_s": med(text_s), "sample_fasta_bgzf_s": med(gz_s), "sample_fasta_bgzf_dev_s": med(gz_dev_s), "bgzf_slot_ms": med(slot_ms),
               "sample_fasta_parts_all_s": text_s, "sample_fasta_bgzf_all_s": gz_s}
        piece = want[:32 << 20]
        for level in (1, 6):
            s, z = timed(lambda: zlib.compress(piece, level))
            res[f"zlib{level}_s_per_gb"] = s / len(piece) * 1e9
            res[f"zlib{level}_ratio"] = len(z) / len(piece)
        res["zlib_piece_bytes"] = len(piece)
        n_text = (b">gap\n" + (b"N" * 80 + b"\n") * 50000)
        res["n_lines_ratio"] = len(ctx.bgzf(n_text)) / len(n_text)
        res["n_lines_zlib1_ratio"] = len(zlib.compress(n_text, 1)) / len(n_text)
        r.close()
        ctx.close()
    for k_, v in res.items():
        print(f"  {k_:32s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
