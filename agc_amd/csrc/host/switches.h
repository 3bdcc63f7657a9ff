// switches.h -- every AGC_AMD_* environment switch of the compressor in one table (documented in profiles/SWITCHES.md).
// Impl::open_session reads it once per session (Create and Append alike); nothing else in the compressor calls getenv, but for
// the process-wide measuring aids of host_support.h (laps_on, start_lap) and the library path of ZstdApi::load.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>

namespace agc {

struct Switches {
    // ---- threads beside the one that drives the steps (compressor_impl.h: the bookkeeping stage, the entropy stage)
    bool async_book = true;         // AGC_AMD_ASYNC_BOOK=0: bookkeeping on the calling thread
    bool async_encode = true;       // AGC_AMD_ASYNC_ENCODE=0: encodes collected by the calling thread
    bool early_collect = true;      // the whole-sample encode is collected by an early task of the book thread (AGC_AMD_EARLY_COLLECT=0: by the registration's own)
    bool ref_store_async = true;    // AGC_AMD_REF_STORE_ASYNC=0: lag counters and symbols are waited for where they are asked for
    bool sync_entropy = false;      // AGC_AMD_SYNC_ENTROPY=1: every registration waits for its zstd jobs
    bool entropy_stream = true;     // AGC_AMD_ENTROPY_STREAM=0: a parallel_for per host-only batch, as before the stream
    size_t par_min = 4096;          // lists shorter than this are walked by the calling thread (AGC_AMD_PAR_MIN: tests force the pool paths)
    // AGC_AMD_ENCODE_OVERLAP: off (default) | early (from the key lookup on) | late (from the placement on).  Measured on the
    // 3 Gbp step: the encode kernel hidden behind estimates / split points costs those kernels what it saves (27.8 ms per step
    // off, 26.4-29.6 ms early), so the default keeps the kernels one after the other and their timings clean
    int overlap_mode = 0;
    // ---- the steps of a registration
    bool dev_segments = true;       // AGC_AMD_DEV_SEGMENTS=0: scan hits to the host, cut and key look-up there (the round-3 path)
    uint32_t dev_encode_min = 2048; // segments a sample needs for the device-launched whole-sample encode (AGC_AMD_DEV_ENCODE_MIN: tests)
    bool pre_launch_encode = true;  // the whole-sample encode launched inside agc_hip_segments_packed (AGC_AMD_PRE_LAUNCH_ENCODE=0: behind the table)
    int place_ahead = 1;            // placement of the segments without a split-point job beside the wait for the split points (AGC_AMD_PLACE_AHEAD=0: after it; 2: for windows of any size -- tests)
    int spec_fill_ahead = 1;        // the table of speculative deltas of the whole-sample encode filled by a helper thread (AGC_AMD_SPEC_FILL_AHEAD=0: in line; 2: any size)
    // ---- the entropy stage (Impl::choose_entropy_stage, Impl::plan_entropy_round)
    bool gpu_zstd_force = false;    // AGC_AMD_GPU_ZSTD=force: the device stage whatever libzstd's version
    bool host_zstd = false;         // AGC_AMD_HOST_ZSTD set: everything on libzstd
    double gpu_zstd_share = 0;      // AGC_AMD_GPU_ZSTD_SHARE: the device's share of the pack bytes, clamped to 0..1 ...
    bool share_fixed = false;       // ... and no longer updated from the measured rates when it is set
    uint32_t gpu_zstd_min = 64;     // fewer packs than this in one call stay on the host (AGC_AMD_GPU_ZSTD_MIN)
    uint32_t gpu_zstd_refs_min = 512; // references on the device when a call brings at least this many (AGC_AMD_GPU_ZSTD_REFS; 0: never)
    // ---- AddSampleFiles
    uint32_t window_max = 256;      // AGC_AMD_WINDOW_MAX: tests pin the window, e.g. to 1 = every registration on its own, bookkeeping beside the next one
    uint64_t map_min = 64ull << 20; // AGC_AMD_MAP_MIN: plain files of at least this many bytes go through the mapped reader
    bool fasta_pack = true;         // AGC_AMD_FASTA_PACK=0 switches the one-pass conversion off ...
    uint64_t fasta_pack_min = 1ull << 20; // ... AGC_AMD_FASTA_PACK_MIN=<bytes> moves its threshold
    // ---- packs kept for the ranks' entropy stages: AGC_AMD_DEFER_MAX_MB, else a quarter of the machine's memory within 2..16 GiB
    uint64_t defer_cap = 0;
    bool producer_tag = false;      // AGC_AMD_PRODUCER_TAG: an honest producer string (one stream differs from the reference's archive)
    // ---- checking aids
    bool dump_packs = false;        // AGC_AMD_DUMP_PACKS=dir: the packs of every device call, for scripts/zstd_gpu_probe.py
    std::string dump_packs_dir;
    bool verify_dev_frames = false; // AGC_AMD_VERIFY_DEV_FRAMES: every device frame against libzstd (`bench.py --verify-entropy`)

    static Switches read()
    {
        Switches s;
        if (const char *e = getenv("AGC_AMD_ASYNC_BOOK"))
            s.async_book = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_ASYNC_ENCODE"))
            s.async_encode = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_EARLY_COLLECT"))
            s.early_collect = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_REF_STORE_ASYNC"))
            s.ref_store_async = atoi(e) != 0;
        s.sync_entropy = getenv("AGC_AMD_SYNC_ENTROPY") != nullptr;
        if (const char *e = getenv("AGC_AMD_ENTROPY_STREAM"))
            s.entropy_stream = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_PAR_MIN"))
            s.par_min = (size_t)std::max(1LL, atoll(e));
        if (const char *e = getenv("AGC_AMD_ENCODE_OVERLAP"))
            s.overlap_mode = !strcmp(e, "early") || !strcmp(e, "1") ? 1 : !strcmp(e, "late") || !strcmp(e, "2") ? 2 : 0;
        if (const char *e = getenv("AGC_AMD_DEV_SEGMENTS"))
            s.dev_segments = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_DEV_ENCODE_MIN"))
            s.dev_encode_min = (uint32_t)std::max(0, atoi(e));
        if (const char *e = getenv("AGC_AMD_PRE_LAUNCH_ENCODE"))
            s.pre_launch_encode = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_PLACE_AHEAD"))
            s.place_ahead = atoi(e);
        if (const char *e = getenv("AGC_AMD_SPEC_FILL_AHEAD"))
            s.spec_fill_ahead = atoi(e);
        if (const char *e = getenv("AGC_AMD_GPU_ZSTD"))
            s.gpu_zstd_force = std::string(e) == "force";
        s.host_zstd = getenv("AGC_AMD_HOST_ZSTD") != nullptr;
        if (const char *e = getenv("AGC_AMD_GPU_ZSTD_SHARE")) {
            s.gpu_zstd_share = std::min(1.0, std::max(0.0, atof(e)));
            s.share_fixed = true;
        }
        if (const char *e = getenv("AGC_AMD_GPU_ZSTD_MIN"))
            s.gpu_zstd_min = (uint32_t)std::max(1, atoi(e));
        if (const char *e = getenv("AGC_AMD_GPU_ZSTD_REFS"))
            s.gpu_zstd_refs_min = (uint32_t)std::max(0, atoi(e));
        if (const char *e = getenv("AGC_AMD_WINDOW_MAX"))
            s.window_max = (uint32_t)std::max(1, atoi(e));
        if (const char *e = getenv("AGC_AMD_MAP_MIN"))
            s.map_min = strtoull(e, nullptr, 10);
        if (const char *e = getenv("AGC_AMD_FASTA_PACK"))
            s.fasta_pack = atoi(e) != 0;
        if (const char *e = getenv("AGC_AMD_FASTA_PACK_MIN"))
            s.fasta_pack_min = strtoull(e, nullptr, 10);
        if (const char *e = getenv("AGC_AMD_DEFER_MAX_MB"))
            s.defer_cap = (uint64_t)strtoull(e, nullptr, 10) << 20;
        else {
            const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGE_SIZE);
            const uint64_t quarter = pages > 0 && psz > 0 ? (uint64_t)pages * (uint64_t)psz / 4 : (4ull << 30);
            s.defer_cap = std::min<uint64_t>(16ull << 30, std::max<uint64_t>(2ull << 30, quarter));
        }
        s.producer_tag = getenv("AGC_AMD_PRODUCER_TAG") != nullptr;
        if (const char *e = getenv("AGC_AMD_DUMP_PACKS")) {
            s.dump_packs = true;
            s.dump_packs_dir = e;
        }
        s.verify_dev_frames = getenv("AGC_AMD_VERIFY_DEV_FRAMES") != nullptr;
        return s;
    }
};

} // namespace agc
