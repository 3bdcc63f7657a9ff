"""Rate of the GPU zstd decode (agc_hip_zstd_decode_batch) on the frames the read of one sample needs, next to libzstd's
ZSTD_decompress on the CPU.

    python scripts/zstd_decode_rate.py [symbols=3e8] [distinct=48] [repeats=5]

A sample of `symbols` bases in 60 kb segments needs, per group, one delta pack and one reference:
  - packs: tests/zstd_cases.delta_pack data (50 deltas of a 60 kb segment at divergence 1e-3, 0xFF between them), level 17;
  - references: nine in ten as 2-bit tuples (four symbols a byte: 15 kB) at level 13, one in ten as symbol bytes (60 kB) at level 19.
`distinct` frames of each kind are made (libzstd, on the CPU) and repeated to the sample's number: a frame costs the same to
decode every time it occurs.  After one warm-up call that is also the check against ZSTD_decompress: median of `repeats` of the
whole call (host clock: upload of the frames, kernel, copy of the decoded bytes to pageable host memory), the kernel's HIP-event
time (agc_hip_timing_get), the kernel time of one pack frame alone, and ZSTD_decompress of the same frames on one thread and on 16 threads of the same machine.
Prints one JSON line at the end."""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from agc_amd import capi, synth  # noqa: E402
from oracle import agc_oracle  # noqa: E402
from tests import zstd_cases  # noqa: E402

SEG = 60_000


def main():
    total = int(float(sys.argv[1])) if len(sys.argv) > 1 else 300_000_000
    distinct = int(sys.argv[2]) if len(sys.argv) > 2 else 48
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    n_groups = max(1, total // SEG)
    rng = np.random.default_rng(2024)
    agc_oracle.lib()
    t0 = time.time()
    packs, tuples, syms = [], [], []
    for _ in range(distinct):
        packs.append(zstd_cases.ref_frame(zstd_cases.delta_pack(agc_oracle, rng, 50, SEG, 1e-3), 17))
        ref = synth.random_seq(rng, SEG)
        t = ref.reshape(-1, 4)
        tuples.append(zstd_cases.ref_frame((t[:, 0] * 64 + t[:, 1] * 16 + t[:, 2] * 4 + t[:, 3]).astype(np.uint8).tobytes(), 13))
    for _ in range(max(1, distinct // 8)):
        blk = synth.random_seq(rng, 3000)  # (a repetitive reference: what store_in_archive keeps as bytes at level 19)
        syms.append(zstd_cases.ref_frame(synth.mutate(rng, np.tile(blk, SEG // 3000), 5e-3).tobytes(), 19))
    frames = []
    for g in range(n_groups):
        frames.append(packs[g % len(packs)])
        frames.append(syms[(g // 10) % len(syms)] if g % 10 == 9 else tuples[g % len(tuples)])
    Z = zstd_cases.libzstd()
    Z.ZSTD_decompress.restype = C.c_size_t
    Z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    Z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    Z.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    sizes = [int(Z.ZSTD_getFrameContentSize(f, len(f))) for f in frames]
    out_bytes, src_bytes = sum(sizes), sum(len(f) for f in frames)
    print(f"{len(frames)} frames for {n_groups} groups: {src_bytes / 1e6:.1f} MB of frames, {out_bytes / 1e6:.1f} MB decoded, prepared in {time.time() - t0:.1f} s", flush=True)

    def cpu(lo, hi):
        buf = C.create_string_buffer(max(sizes) + 8)
        n = 0
        for i in range(lo, hi):
            n += Z.ZSTD_decompress(buf, len(buf), frames[i], len(frames[i]))
        return n

    ctx = capi.Context(0)
    out = np.empty(out_bytes, np.uint8)
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    batch = (np.frombuffer(b"".join(frames), np.uint8), off)  # (joined once: the call is timed, not Python's copy)
    u8p = capi.u8p
    rc, ooff, st = ctx.zstd_decode_batch_raw(batch, out.ctypes.data_as(u8p), out.size)  # warm-up (and the check)
    assert rc == capi.OK and not st.any(), (rc, np.flatnonzero(st)[:5])
    ref = C.create_string_buffer(max(sizes) + 8)
    for i in range(0, len(frames), max(1, len(frames) // 200)):  # (every distinct frame several times over)
        k = Z.ZSTD_decompress(ref, len(ref), frames[i], len(frames[i]))
        assert out[int(ooff[i]):int(ooff[i + 1])].tobytes() == ref.raw[:k], f"frame {i} differs from ZSTD_decompress"
    ctx.timing(True)
    calls = []
    for _ in range(repeats):
        t = time.perf_counter()
        rc, _o, _s = ctx.zstd_decode_batch_raw(batch, out.ctypes.data_as(u8p), out.size)
        calls.append(time.perf_counter() - t)
        assert rc == capi.OK
    tm = ctx.timing_get()
    assert tm["zstd_decode"][1] == repeats
    kernel_s = tm["zstd_decode"][0] / 1e3 / repeats

    # one frame alone (the first delta pack): what a frame costs a wave, next to what it costs a CPU thread
    ctx.timing(True)
    for _ in range(repeats):
        rc, _o, _s = ctx.zstd_decode_batch_raw(frames[:1], out.ctypes.data_as(u8p), out.size)
        assert rc == capi.OK
    one_kernel_s = ctx.timing_get()["zstd_decode"][0] / 1e3 / repeats
    t = time.perf_counter()
    for _ in range(20):
        cpu(0, 1)
    one_cpu_s = (time.perf_counter() - t) / 20

    t = time.perf_counter()
    assert cpu(0, len(frames)) == out_bytes
    cpu1_s = time.perf_counter() - t
    cuts = [len(frames) * j // 16 for j in range(17)]
    with ThreadPoolExecutor(16) as ex:
        t = time.perf_counter()
        assert sum(ex.map(lambda j: cpu(cuts[j], cuts[j + 1]), range(16))) == out_bytes
        cpu16_s = time.perf_counter() - t

    call_s = float(np.median(calls))
    res = {"symbols": total, "groups": n_groups, "frames": len(frames), "distinct": distinct, "frame_bytes": src_bytes, "decoded_bytes": out_bytes,
           "repeats": repeats, "call_ms_median": round(call_s * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2), "call_ms_max": round(max(calls) * 1e3, 2),
           "call_gb_per_s": round(out_bytes / call_s / 1e9, 3), "kernel_ms": round(kernel_s * 1e3, 2), "kernel_gb_per_s": round(out_bytes / kernel_s / 1e9, 3),
           "one_pack_frame_kernel_ms": round(one_kernel_s * 1e3, 3), "one_pack_frame_cpu_ms": round(one_cpu_s * 1e3, 3),
           "cpu_one_thread_ms": round(cpu1_s * 1e3, 1), "cpu_one_thread_gb_per_s": round(out_bytes / cpu1_s / 1e9, 3),
           "cpu_one_thread_us_per_frame": round(cpu1_s * 1e6 / len(frames), 1),
           "cpu_16_threads_ms": round(cpu16_s * 1e3, 1), "cpu_16_threads_gb_per_s": round(out_bytes / cpu16_s / 1e9, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
