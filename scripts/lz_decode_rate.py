"""Rate of the GPU LZ-diff decode (agc_hip_lz_decode_batch) at a size a user would run, next to the single-thread CPU decode.

    python scripts/lz_decode_rate.py [symbols=3e8] [divergence=1e-3] [repeats=5]

One synthetic sample against its reference sample (agc_amd.synth), both cut into 60 kb segments: segment i of the reference is
group i's reference, segment i of the sample is encoded against it with the product's encode path; the deltas are then decoded
in one batch.  After one warm-up call: symbols per second of the whole call (host clock around it; it includes the upload of
the deltas and the device-to-host copy of one byte per symbol) and of the two kernels (HIP events, agc_hip_timing_get), and the
rate of the oracle's decode over the same deltas on one thread of this machine.  Prints one JSON line at the end."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from agc_amd import capi, synth  # noqa: E402
from oracle import agc_oracle  # noqa: E402

SEG, MML, GID0, CHUNK = 60_000, 20, 16, 500


def main():
    total = int(float(sys.argv[1])) if len(sys.argv) > 1 else 300_000_000
    d = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-3
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    n_seg = max(1, total // SEG)
    rng = np.random.default_rng(2024)
    ctx = capi.Context(0)
    refs, texts, deltas = [], [], []
    t0 = time.time()
    for c0 in range(0, n_seg, CHUNK):  # (in chunks: the generator's temporaries stay small)
        n = min(CHUNK, n_seg - c0)
        ref = synth.random_seq(rng, n * SEG)
        smp = synth.mutate(rng, ref, d)
        off = (np.arange(n, dtype=np.uint64) * SEG)
        ln = np.full(n, SEG, np.uint32)
        gids = GID0 + c0 + np.arange(n)
        d_ref, d_smp = torch.from_numpy(np.concatenate([ref, np.zeros(64, np.uint8)])).cuda(), torch.from_numpy(np.concatenate([smp, np.zeros(64, np.uint8)])).cuda()
        torch.cuda.synchronize()
        ctx.ref_register_batch_dev(gids, d_ref.data_ptr(), off, ln, np.zeros(n, np.uint8), MML)
        enc, eoff = ctx.lz_encode_batch_dev(d_smp.data_ptr(), gids, off, ln)
        refs.append(ref)
        texts.append(smp)
        deltas.append((enc.copy(), eoff.copy()))
    enc = np.concatenate([e for e, _o in deltas])
    enc_off = np.zeros(n_seg + 1, np.uint64)
    base, k = 0, 0
    for e, o in deltas:
        enc_off[k:k + o.size] = o + base
        base, k = base + e.size, k + o.size - 1
    text = np.concatenate(texts)
    gids = GID0 + np.arange(n_seg)
    print(f"{n_seg} segments of {SEG}, {text.size / 1e6:.1f} Mbp, {enc.size / 1e6:.2f} MB of deltas, prepared in {time.time() - t0:.1f} s", flush=True)

    out, ooff = ctx.lz_decode_batch(enc, enc_off, gids, out_cap=text.size)  # warm-up (and the check)
    assert np.array_equal(out, text), "the decode does not give the sample back"
    ctx.timing(True)
    calls = []
    for _ in range(repeats):
        t = time.perf_counter()
        ctx.lz_decode_batch(enc, enc_off, gids, out_cap=text.size)
        calls.append(time.perf_counter() - t)
    tm = ctx.timing_get()
    scan_s, write_s = tm["decode_scan"][0] / 1e3 / repeats, tm["decode_write"][0] / 1e3 / repeats
    assert tm["decode_write"][1] == repeats

    # the oracle's decode (CLZDiff_V2::Decode restated), one thread, the same deltas
    L, u8p = agc_oracle.lib(), agc_oracle.u8p
    ref_all = np.concatenate(refs)
    buf = np.empty(SEG + 64, np.uint8)
    t = time.perf_counter()
    n_cpu = 0
    for i in range(n_seg):
        r, e = ref_all[i * SEG:(i + 1) * SEG], enc[int(enc_off[i]):int(enc_off[i + 1])]
        n_cpu += L.agco_lz_decode(r.ctypes.data_as(u8p), r.size, MML, e.ctypes.data_as(u8p), e.size, buf.ctypes.data_as(u8p), buf.size)
    cpu_s = time.perf_counter() - t
    assert n_cpu == text.size

    call_s = float(np.median(calls))
    res = {"symbols": int(text.size), "segments": n_seg, "delta_bytes": int(enc.size), "divergence": d, "repeats": repeats,
           "call_ms_median": round(call_s * 1e3, 3), "call_ms_min": round(min(calls) * 1e3, 3), "call_ms_max": round(max(calls) * 1e3, 3),
           "call_gsym_per_s": round(text.size / call_s / 1e9, 3),
           "scan_kernel_ms": round(scan_s * 1e3, 3), "write_kernel_ms": round(write_s * 1e3, 3),
           "scan_kernel_gsym_per_s": round(text.size / scan_s / 1e9, 2), "write_kernel_gsym_per_s": round(text.size / write_s / 1e9, 2),
           "cpu_one_thread_gsym_per_s": round(text.size / cpu_s / 1e9, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
