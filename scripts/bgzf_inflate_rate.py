"""A BGZF stream inflated on the GPU (Context.bgzf_inflate / bgzf_inflate_dev: agc_hip_bgzf_inflate, a wavefront per member) next to
zlib on one thread, on the workload of scripts/bgzf_rate.py.

    python scripts/bgzf_inflate_rate.py [symbols=3e8] [divergence=1e-3] [repeats=5]

Two streams of the same FASTA text (a sample read back from an archive, 80 columns):
  literal   what DeviceReader.sample_fasta_bgzf writes: members of one dynamic block without matches (65 280 dependent symbols each)
  matches   the text cut into blocks of 65 280 bytes, each deflated by Python's zlib at level 6: members with matches
After a warm-up of every row the rows take turns, `repeats` times, and each reports its median:
  (a) bgzf_inflate        the whole call: walk, upload, kernel, the text back to the host
  (b) bgzf_inflate_dev    the same, the text left on the device
  (c) the inflate slot    kernel time of bgzf_inflate_kernel by HIP events (agc_hip_timing_get), from the calls of (a)
  (d) zlib, one thread    gzip.decompress of the same stream (zlib's inflate member after member)
Every result is compared with the text before anything is timed.  Prints one JSON line at the end."""
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
BLOCK = 65280
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def reblock(text, level):
    """the text as BGZF members deflated by zlib"""
    out = []
    for p in range(0, len(text), BLOCK):
        blk = text[p:p + BLOCK]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        pay = c.compress(blk) + c.flush()
        out.append(bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", "")) + (len(pay) + 25).to_bytes(2, "little") + pay +
                   zlib.crc32(blk).to_bytes(4, "little") + len(blk).to_bytes(4, "little"))
    return b"".join(out) + EOF_MEMBER


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
        ctx = capi.Context(0)
        r = devread.DeviceReader(ctx, agc, gid_base=0)
        want = r.sample_fasta_parts("smp", 80)
        streams = {"literal": r.sample_fasta_bgzf("smp", 80)}
        r.close()
    streams["matches"] = reblock(want, 6)
    print(f"text {len(want)} bytes, prepared in {time.time() - t0:.1f} s", flush=True)
    res = {"symbols": int(sum(int(n) for n in ln)), "text_bytes": len(want), "repeats": repeats}
    med = statistics.median
    for name, gz in streams.items():
        assert ctx.bgzf_inflate(gz) == want, name + ": the device's bytes are not the text"
        t, off = ctx.bgzf_inflate_dev(gz)
        assert t.cpu().numpy().tobytes() == want and int(off[-1]) == len(want)
        del t
        assert gzip.decompress(gz) == want
        call_s, dev_s, slot_ms, zlib_s = [], [], [], []
        for _ in range(repeats):
            ctx.timing(True)  # (resets the slots)
            call_s.append(timed(lambda: ctx.bgzf_inflate(gz))[0])
            slot_ms.append(ctx.timing_get()["inflate"][0])
            ctx.timing(False)
            dev_s.append(timed(lambda: ctx.bgzf_inflate_dev(gz))[0])
            zlib_s.append(timed(lambda: gzip.decompress(gz))[0])
        res[name] = {"stream_bytes": len(gz), "ratio": len(gz) / len(want), "members": int(off.size - 1), "bgzf_inflate_s": med(call_s), "bgzf_inflate_dev_s": med(dev_s),
                     "inflate_slot_ms": med(slot_ms), "zlib_one_thread_s": med(zlib_s), "text_gb_per_s_slot": len(want) / med(slot_ms) / 1e6,
                     "text_gb_per_s_call": len(want) / med(call_s) / 1e9, "text_gb_per_s_zlib": len(want) / med(zlib_s) / 1e9}
        print(name, json.dumps(res[name]), flush=True)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
