// api.hip -- the C ABI of include/agc_hip.h: context, HBM arenas, kernel launches.
// Host-side logic here is orchestration only (buffer management, sorting sparse hit
// lists; the LZ write path's arithmetic -- batch order, offsets, the chunk plan, a reference's layout -- is lz_plan.h); all
// symbol-level work is done by the kernels in scan_kernels.hip / lz_kernels.hip.  There is no CPU fallback.
// This file: the context, the helpers every entry point shares (ensure, upload, KTimer, ...) and the create path.  The read path
// (LZ decode, a sample's FASTA text, zstd decode) is read_api.hip, included at the end with splitters.hip and segments.hip: the
// library stays one translation unit.
#include "../../include/agc_hip.h"
#include "dev_common.h"
#include "lz_plan.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <future>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "scan_kernels.hip"
#include "pack_kernels.hip"
#include "lz_kernels.hip"
#include "seg_kernels.hip"
#include "lz_decode_kernels.hip"
#include "fasta_out_kernels.hip"
#include "zstd_kernels.hip"
#include "zstd_decode_kernels.hip"
#include "parts_unpack_kernels.hip"
#include "range_kernels.hip"
#include "bgzf_kernels.hip"
#include "inflate_kernels.hip"

using namespace agc;

namespace {

// What the context holds, it holds through these: each frees its memory or destroys its handle when it goes, and can be moved but
// not copied.  Nothing else in the library calls hipFree, hipHostFree, hipEventDestroy or hipStreamDestroy (agc_hip_host_free, which
// hands a pinned buffer back early, goes through release() too).
template <hipError_t (*Free)(void *)> struct OwnedMem {
    void *p = nullptr;
    size_t cap = 0;
    OwnedMem() = default;
    OwnedMem(void *p_, size_t cap_) : p(p_), cap(cap_) {}
    OwnedMem(OwnedMem &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    OwnedMem &operator=(OwnedMem &&o) noexcept
    {
        if (this != &o) {
            (void)release();
            std::swap(p, o.p), std::swap(cap, o.cap);
        }
        return *this;
    }
    ~OwnedMem() { (void)release(); }
    hipError_t release()
    {
        const hipError_t e = p ? Free(p) : hipSuccess;
        p = nullptr, cap = 0;
        return e;
    }
    template <class T> T *as() const { return (T *)p; }
};
using DevBuf = OwnedMem<hipFree>;        // device memory (grown by ensure)
using PinnedBuf = OwnedMem<hipHostFree>; // pinned host memory (grown by ensure_pinned)

template <class H, hipError_t (*Destroy)(H)> struct OwnedHandle {
    H h = nullptr; // (made where it is first needed: hipStreamCreate* / hipEventCreate* write here)
    OwnedHandle() = default;
    OwnedHandle(OwnedHandle &&o) noexcept : h(o.h) { o.h = nullptr; }
    OwnedHandle &operator=(OwnedHandle &&) = delete;
    ~OwnedHandle()
    {
        if (h)
            (void)Destroy(h);
    }
    operator H() const { return h; }
};
using Stream = OwnedHandle<hipStream_t, hipStreamDestroy>;
using Event = OwnedHandle<hipEvent_t, hipEventDestroy>;

// a chunk of the reference arena: mem.cap usable bytes (the allocation has a tail slack behind them), `used` of them handed out
struct ArenaChunk {
    DevBuf mem;
    size_t used = 0;
};

// a 2-bit packed buffer the LZ entry points read sequences from (sym_view.h): the caller's sample, or a temporary one
struct PackedSrc {
    const uint32_t *words = nullptr;
    const int32_t *esc_index = nullptr;
    const uint8_t *esc_bytes = nullptr;
    uint64_t n_symbols = 0;
};

// context-owned packed form of byte input (the entry points that take one byte per symbol pack what they are given first:
// every LZ kernel reads the 2-bit layout only)
struct PackTemp {
    DevBuf words, index, esc, cnt;
};

} // namespace

struct agc_hip_ctx {
    int device = 0;
    Stream stream;  // the steps' stream
    Stream zstream; // the entropy stage's own stream: agc_hip_zstd17_batch may run beside every other entry point
    Stream zstream2; // ... and a second one: the one-lane kernel (inputs > 16 KiB) runs BESIDE the group kernel
    Event zev_a, zev_b;
    Event zev_wait; // (blocking-sync: the thread that waits for a launch of the entropy stage sleeps, its core is the host pool's)
    bool zstd_background = false;  // agc_hip_zstd17_background: launches leave the LDS to the kernels of the other streams
    std::string err;

    // splitter set
    std::vector<uint64_t> spl;       // host copy (unique)
    DevBuf d_table, d_bloom, d_bloom2, d_sbloom;
    uint32_t sbloom_k = 0;          // the packed scan's suffix filter: built for this k ...
    size_t sbloom_n = ~(size_t)0;   // ... and this many splitters
    uint64_t table_mask = 0;

    // references
    std::vector<RefDesc> refs;       // indexed by gid
    DevBuf d_refs;
    bool refs_dirty = true;
    size_t refs_dirty_lo = 0, refs_dirty_hi = 0; // groups [lo, hi) changed since the table went to the device (refs_on_dev entries are there)
    size_t refs_on_dev = 0;
    std::vector<ArenaChunk> arena;
    // agc_hip_ref_store_begin_packed / _end: two slots, a stream and buffers of their own (the steps' stream never waits for them)
    struct RefStore {
        DevBuf d_slices, d_lag, d_out;
        Event done;
        std::atomic<bool> pending{false}; // (_end may run on the caller's bookkeeping thread)
    } ref_store[2];
    Stream ref_store_stream;
    // the NEXT chunk, allocated ahead of need by a helper thread (arena_alloc): a hipMalloc of GBs is 30 ms per GB on a box whose
    // VRAM this process touches for the first time -- 150 ms in the middle of a step (profiles/r6/)
    std::future<ArenaChunk> arena_spare;

    // the > 64 KiB dynamic-LDS attribute of a kernel is a property of the device the context runs on: set once per context
    bool lds_scan_set = false, lds_lookup_set = false;

    // scratch
    DevBuf d_esc_jobs, d_flags;
    // the (k1, k2) -> group table (mirror of the host's map_segments) and the work area of agc_hip_segments_packed
    DevBuf d_gmap, d_gmap_stage, d_segwork, d_segtmp;
    uint64_t gmap_slots = 0;
    PinnedBuf h_gmap_stage; // staging of agc_hip_group_map_update
    Event gmap_ev;
    bool gmap_ev_valid = false;
    // frame sizes of the entropy launch in flight (a pageable destination makes the "async" copy wait for the launch inside the call,
    // spinning: a core of the host pool's for the whole launch)
    PinnedBuf h_zsizes;
    PinnedBuf h_segcounts; // SegCounts of the call in flight (+ 64: the count of the encode launched from them)
    // what agc_hip_segments_packed left on the device for agc_hip_segments_encode_known
    struct SegState {
        bool valid = false;
        uint32_t n_ub = 0;
        uint64_t total = 0;
        agc_hip_packed pk{};
        void *segs = nullptr, *counts = nullptr, *d_ctg_off = nullptr;
        void *flag = nullptr, *capv = nullptr, *known_rank = nullptr, *cap_off = nullptr, *descs = nullptr, *lcnt = nullptr;
    } seg_state;
    DevBuf d_ranges, d_hits, d_counter, d_slices, d_jobs, d_counts, d_in, d_pp_cnt, d_pp_off, d_pp_total, d_lag, d_sample, d_zsrc, d_zdst, d_zws, d_zjobs, d_zsize, d_zout, d_zdstoff, d_maybe, d_fjobs;
    struct ReadBufs { // the read path (read_api.hip)
        DevBuf d_dec_enc, d_dec_jobs, d_dec_res, d_dec_out; // agc_hip_lz_decode_batch*: the deltas, their descriptors, lengths + status, the symbols
        DevBuf d_fa_sym, d_fa_copy, d_fa_plan, d_fa_text;   // agc_hip_sample_fasta*: the sample's symbols, the copy jobs, the text plan, the text
        DevBuf d_zd_src, d_zd_jobs, d_zd_status, d_zd_ws, d_zd_out; // agc_hip_zstd_decode_batch*: the frames, their descriptors, their statuses, the literals workspaces, the bytes
        DevBuf d_pu_dec, d_pu_jobs, d_pu_res, d_pu_wjobs, d_pu_out; // agc_hip_parts_unpack*: the decoded parts, their descriptors, infos + end offsets, the write jobs, the final bytes
        DevBuf d_rg_jobs, d_rg_copy, d_rg_out; // agc_hip_lz_decode_window_batch*, agc_hip_ranges_parts*: the delta window jobs, the RAW / REF window jobs, the symbols
        DevBuf d_bz_in, d_bz_slots, d_bz_sizes, d_bz_off, d_bz_out; // agc_hip_bgzf*: the input, a slot of 65312 bytes per block, the members' sizes, their offsets, the stream
        DevBuf d_inf_in, d_inf_jobs, d_inf_status, d_inf_out; // agc_hip_bgzf_inflate*: the stream, a job per member, the members' statuses, the bytes
    } rd;

    PackTemp pk1;        // byte-input entry points on the first stream
    PackTemp pk_sample;  // agc_hip_sample_pack
    std::mutex host_alloc_mtx; // host_allocs: agc_hip_host_alloc / _free may be called from the thread that collects an encode
    // pinned staging ring of the small host -> device uploads (descriptors, offsets, tables): a copy from pageable memory makes the
    // calling thread wait for the copy engine -- behind whatever else it is moving, e.g. the 22 MB of a sample's deltas
    PinnedBuf up_ring;
    size_t up_head = 0;
    std::mutex up_mtx;
    // the ring in UP_PARTS parts: a part remembers the streams that copied out of it and, when the head leaves it, an event on each;
    // the head waits for those events when it comes back (a ring's length later: they are long done -- the whole-ring wait for
    // every stream at the wrap cost a step 7 ms once in 16 samples)
    static constexpr int UP_PARTS = 4, UP_STREAMS = 12;
    struct UpPart {
        hipStream_t st[UP_STREAMS] = {};
        Event ev[UP_STREAMS];
        int n = 0;         // streams noted since the head came in
        int n_recorded = 0; // events recorded when it left
    } up_part[UP_PARTS];

    // An LZ parse stream: a stream, the parse's buffers and the chunk buffers of a parse in chunks.  lane(0) is the steps' stream (the
    // estimates, cost vectors, one-call encodes; other entry points of that stream share d_scratch, d_dstoff and d_compact with the
    // parse); lane(1) and lane(2) are the encode lanes: agc_hip_lz_encode_begin_* / _end run the encode of a whole sample on the
    // lane's stream with their own scratch, beside what the caller goes on with on `stream`.  lane(2): a second encode in flight --
    // the segments of a sample whose group was minted by that very sample, launched at commit time behind the whole-sample encode
    // of lane(1) and collected by the same bookkeeping task
    struct LzLane {
        hipStream_t s = nullptr; // lane 0: the context's `stream`; an encode lane: `own`, at the first stream's priority
        Stream own;
        DevBuf d_segs, d_resv, d_resp, d_scratch, d_dstoff, d_compact;
        struct Chunks { // launch_parse: chunk list, logs and per-chunk output
            DevBuf d_jobs, d_seg0, d_logs, d_logn, d_out;
            // the chunk logs of a human-size batch are 0.7 GB: a launch of thousands of parses that is NOT parsed in chunks has a helper
            // thread allocate them, so that the first batch that is -- one text of a few hundred kb among 3 000, twice in twenty samples --
            // does not pay a hipMalloc inside a step (27-41 ms on a box whose VRAM the process touches for the first time)
            std::future<DevBuf> logs_ahead;
            bool logs_asked = false;
        } chunks;
        // ---- the encode lanes only
        DevBuf d_n; // the lane's own copy of a segment count made on the device (the work area it came from is re-laid-out by the next sample)
        PackTemp pk;
        PinnedBuf h_lens; // (a device-to-host copy into pageable memory would make begin wait for the kernel)
        uint32_t n = 0;          // segments of the encode in flight
        const uint32_t *n_pinned = nullptr; // != nullptr: their number arrives with the parse (descriptors made on the device)
        bool pending = false, timed = false;
        Event e0, e1, ready;
        // `done`: recorded behind the parse of the encode in flight.  A caller may collect that encode from another thread while
        // this one already works on the next sample (agc_hip_lz_encode_end only touches this lane): whatever overwrites a buffer
        // the parse reads -- the sample staging buffers -- waits for the event on its own stream (sample_buffer, prefetch)
        Event done;
        bool done_valid = false;
    } lanes[3];
    LzLane &lane(int which) { return lanes[which]; }

    // the NEXT sample, started ahead of its turn (agc_hip_prefetch_packed_dev): expansion into one of two staging buffers and the
    // packed splitter scan, on a stream of their own with their own scratch -- they fill the gaps the sample in front leaves on the
    // GPU while the host registers its segments
    struct Prefetch {
        Stream stream;
        DevBuf d_ranges, d_hits, d_counter;
        PinnedBuf h_count; // one word
        const void *words = nullptr; // identity of the packed sample in flight
        uint64_t n_symbols = 0;
        uint32_t dev_cap = 0, k = 0, n_ctg = 0;
        uint64_t first_off = 0, last_off = 0;
        bool valid = false, scanned = false;
        Event e0, e1;
        bool timed = false;
    } pf;

    // agc_hip_pack_fasta_begin / _end: raw FASTA bodies -> the packed sample on a stream of its own (pack_kernels.hip)
    struct PackFasta {
        Stream stream;
        DevBuf d_state, d_rng, d_off; // the three counters; the ranges; n_ctg + 1 symbol offsets + the total
        DevBuf d_tcnt, d_toff;        // two-pass variant: symbols per tile, symbols in front of every tile
        PinnedBuf h_res;              // offsets, total, escaped-block count
        uint32_t n_ctg = 0;
        uint64_t n_raw = 0, esc_cap = 0;
        bool pending = false, timed = false;
        Event e0, e1;
    } pfa;

    // pinned host allocations handed out by agc_hip_host_alloc
    std::vector<PinnedBuf> host_allocs;

    // timing
    bool timing = false;
    Event zev0, zev1; // ZTimer
    // KTimer's event pairs: recorded around a launch and READ LATER (when the ring comes round, or by agc_hip_timing_get) -- timing a
    // run must not add a wait behind every kernel of the steps' stream (rounds 1-5 did: hipEventSynchronize in KTimer's destructor)
    struct TimerPair {
        Event a, b;
        int which = -1; // >= 0: recorded, not read yet
    };
    std::vector<TimerPair> tpairs;
    size_t tpair_next = 0;
    double ms[AGC_HIP_K_COUNT] = {0};
    uint64_t launches[AGC_HIP_K_COUNT] = {0};
};

#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return e_ == hipErrorOutOfMemory ? AGC_HIP_ENOMEM : AGC_HIP_ENODEV;                    \
        }                                                                                          \
    } while (0)

#define CHK(expr)                                                                                  \
    do {                                                                                           \
        int r_ = (expr);                                                                           \
        if (r_ != AGC_HIP_OK)                                                                      \
            return r_;                                                                             \
    } while (0)

namespace {

// host time between the marks of a call with many items (n > 10000; ~0u: of every call), on stderr under AGC_HIP_LAPS
struct Laps {
    const char *who;
    bool on;
    double last = 0;
    static bool enabled()
    {
        static const bool e = getenv("AGC_HIP_LAPS") != nullptr;
        return e;
    }
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    Laps(const char *who_, uint32_t n) : who(who_), on(enabled() && n > 10000) { last = on ? now() : 0; }
    void operator()(const char *what)
    {
        if (!on)
            return;
        const double t = now();
        fprintf(stderr, "    %s lap %s %.3f ms\n", who, what, t - last);
        last = t;
    }
};

int ensure(agc_hip_ctx *c, DevBuf &b, size_t bytes, hipStream_t stream = nullptr)
{
    if (bytes <= b.cap)
        return AGC_HIP_OK;
    if (!stream)
        stream = c->stream;
    // headroom: batches of one collection differ by a few percent in size; growing in big steps keeps
    // hipFree/hipMalloc (hundreds of ms for multi-GB buffers) out of the steady state
    size_t want = std::max(bytes + bytes / 4, b.cap + b.cap / 2);
    want = (want + 255) & ~(size_t)255;
    const double t0 = Laps::now();
    const size_t had = b.cap;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(stream));
        HIPCHK(c, b.release());
    }
    HIPCHK(c, hipMalloc(&b.p, want));
    b.cap = want;
    if (Laps::enabled() && want >= ((size_t)16 << 20))
        fprintf(stderr, "    ensure: a device buffer grows from %.1f to %.1f MB (asked: %.1f) in %.3f ms\n", had / 1e6, want / 1e6, bytes / 1e6, Laps::now() - t0);
    return AGC_HIP_OK;
}

// pinned memory of at least `need` bytes in b: what is there, or a new buffer of `alloc` bytes (the headroom is the caller's: every
// buffer grows by its own rule).  Whatever read or wrote the old one is done: the callers have waited for it.
int ensure_pinned(agc_hip_ctx *c, PinnedBuf &b, size_t need, size_t alloc)
{
    if (need <= b.cap)
        return AGC_HIP_OK;
    HIPCHK(c, b.release());
    HIPCHK(c, hipHostMalloc(&b.p, alloc, hipHostMallocDefault));
    b.cap = alloc;
    return AGC_HIP_OK;
}

size_t arena_next_size(const agc_hip_ctx *c)
{
    // a chunk is at least half of what the arena holds already: the number of hipMalloc calls of a run grows with the logarithm of
    // its references, not with their number
    size_t held = 0;
    for (const ArenaChunk &ch : c->arena)
        held += ch.mem.cap;
    return std::max((size_t)256 << 20, std::min(held / 2, (size_t)8 << 30));
}

int arena_alloc(agc_hip_ctx *c, size_t bytes, uint8_t **out)
{
    bytes = (bytes + 255) & ~(size_t)255;
    if (c->arena.empty() || c->arena.back().used + bytes > c->arena.back().mem.cap) {
        const double t0 = Laps::now();
        ArenaChunk nc;
        if (c->arena_spare.valid()) { // (allocated since the current chunk was half full: long done)
            nc = c->arena_spare.get();
            if (nc.mem.cap < bytes)
                nc = ArenaChunk(); // (too small for this request: given back)
        }
        if (!nc.mem.p) {
            const size_t sz = std::max(bytes, arena_next_size(c));
            HIPCHK(c, hipMalloc(&nc.mem.p, sz + 4096)); // tail slack: 16-byte over-reads never leave the allocation
            nc.mem.cap = sz;
        }
        c->arena.push_back(std::move(nc));
        if (Laps::enabled())
            fprintf(stderr, "    arena: a chunk of %.1f MB becomes current in %.3f ms\n", c->arena.back().mem.cap / 1e6, Laps::now() - t0);
    }
    ArenaChunk &ch = c->arena.back();
    *out = ch.mem.as<uint8_t>() + ch.used;
    ch.used += bytes;
    // the chunk after this one is asked for as soon as this one is half full, on a thread of its own
    if (!c->arena_spare.valid() && ch.used * 2 >= ch.mem.cap) {
        const size_t sz = arena_next_size(c);
        const int dev = c->device;
        c->arena_spare = std::async(std::launch::async, [sz, dev] {
            ArenaChunk sp; // (left empty on failure: arena_alloc then allocates when the chunk is needed, and reports)
            if (hipSetDevice(dev) == hipSuccess && hipMalloc(&sp.mem.p, sz + 4096) == hipSuccess)
                sp.mem.cap = sz;
            else
                sp.mem.p = nullptr;
            return sp;
        });
    }
    return AGC_HIP_OK;
}

void ktimer_read(agc_hip_ctx *c, agc_hip_ctx::TimerPair &p)
{
    if (p.which < 0)
        return;
    float ms = 0;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
        c->ms[p.which] += ms;
        c->launches[p.which] += 1;
    }
    p.which = -1;
}

void ktimer_read_all(agc_hip_ctx *c)
{
    for (auto &p : c->tpairs)
        ktimer_read(c, p);
}

struct KTimer {
    agc_hip_ctx *c;
    agc_hip_ctx::TimerPair *p = nullptr;
    int which;
    KTimer(agc_hip_ctx *c_, int w) : c(c_), which(w) // (w < 0: not timed -- a launch on the second lane)
    {
        if (!c->timing || which < 0)
            return;
        if (c->tpairs.empty())
            c->tpairs.resize(256);
        p = &c->tpairs[c->tpair_next];
        c->tpair_next = (c->tpair_next + 1) % c->tpairs.size();
        ktimer_read(c, *p); // (a pair recorded 256 launches ago: long done)
        if ((!p->a && hipEventCreate(&p->a.h) != hipSuccess) || (!p->b && hipEventCreate(&p->b.h) != hipSuccess)) {
            p = nullptr;
            return;
        }
        (void)hipEventRecord(p->a, c->stream);
    }
    ~KTimer()
    {
        if (p) {
            (void)hipEventRecord(p->b, c->stream);
            p->which = which;
        }
    }
};

// the entropy stage's kernels: own events, own stream (only that call writes ms[AGC_HIP_K_ZSTD])
struct ZTimer {
    agc_hip_ctx *c;
    explicit ZTimer(agc_hip_ctx *c_) : c(c_)
    {
        if (c->timing)
            (void)hipEventRecord(c->zev0, c->zstream);
    }
    ~ZTimer()
    {
        if (c->timing) {
            (void)hipEventRecord(c->zev1, c->zstream);
            (void)hipEventSynchronize(c->zev1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->zev0, c->zev1);
            c->ms[AGC_HIP_K_ZSTD] += ms;
            c->launches[AGC_HIP_K_ZSTD] += 1;
        }
    }
};

int ensure_z(agc_hip_ctx *c, DevBuf &b, size_t bytes) { return ensure(c, b, bytes, c->zstream); }

// one piece of an upload (at most half a part of the ring): copied into the ring, the copy to the device queued on `st` from there
int upload_piece(agc_hip_ctx *c, void *d_dst, const void *h_src, size_t bytes, hipStream_t st, size_t RING, size_t PART)
{
    // (the lock is held until the copy is queued: the event a part records on a stream when the head leaves is then behind every
    // copy out of that part)
    std::lock_guard<std::mutex> lk(c->up_mtx);
    CHK(ensure_pinned(c, c->up_ring, RING, RING));
    const size_t need = (bytes + 255) & ~(size_t)255;
    size_t part = c->up_head ? (c->up_head - 1) / PART : 0; // (a head at a part's very end still belongs to it)
    if (c->up_head + need > (part + 1) * PART) {
        agc_hip_ctx::UpPart &old_part = c->up_part[part];
        for (int i = 0; i < old_part.n; ++i) {
            if (!old_part.ev[i])
                HIPCHK(c, hipEventCreateWithFlags(&old_part.ev[i].h, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(old_part.ev[i], old_part.st[i]));
        }
        old_part.n_recorded = old_part.n;
        old_part.n = 0;
        part = (part + 1) % agc_hip_ctx::UP_PARTS;
        c->up_head = part * PART;
        agc_hip_ctx::UpPart &new_part = c->up_part[part];
        for (int i = 0; i < new_part.n_recorded; ++i)
            HIPCHK(c, hipEventSynchronize(new_part.ev[i]));
        new_part.n_recorded = 0;
    }
    agc_hip_ctx::UpPart &P = c->up_part[part];
    int k = 0;
    while (k < P.n && P.st[k] != st)
        ++k;
    if (k == P.n) {
        if (P.n == agc_hip_ctx::UP_STREAMS) { // (more streams than a part has room for: make room the slow way)
            HIPCHK(c, hipStreamSynchronize(P.st[0]));
            P.st[0] = st;
        } else
            P.st[P.n++] = st;
    }
    uint8_t *slot = c->up_ring.as<uint8_t>() + c->up_head;
    c->up_head += need;
    std::memcpy(slot, h_src, bytes);
    HIPCHK(c, hipMemcpyAsync(d_dst, slot, bytes, hipMemcpyHostToDevice, st));
    return AGC_HIP_OK;
}

// host -> device on `st`, without the calling thread waiting for the copy engine (a copy from pageable memory would make it wait).
// THE CONTRACT: when upload() returns, the caller may free or overwrite h_src.  Every byte goes through the context's pinned ring,
// in pieces of at most MAX_PIECE, and the device copies are queued out of the ring; a slot is reused a ring's length later (tens
// of steps), after the head has waited for the events of the part it comes back to.
int upload(agc_hip_ctx *c, void *d_dst, const void *h_src, size_t bytes, hipStream_t st)
{
    // (AGC_HIP_UPLOAD_RING_MB: a smaller ring for the tests -- the head then comes back to a part, and waits for its events, many
    // times in a small archive; a piece is at most half a part)
    static const size_t RING = [] {
        const char *e = getenv("AGC_HIP_UPLOAD_RING_MB");
        const long mb = e ? atol(e) : 64;
        return (size_t)(mb < 1 ? 1 : mb > 64 ? 64 : mb) << 20;
    }();
    const size_t PART = RING / agc_hip_ctx::UP_PARTS, MAX_PIECE = std::min<size_t>((size_t)8 << 20, PART / 2);
    for (size_t o = 0; o < bytes; o += MAX_PIECE)
        CHK(upload_piece(c, (uint8_t *)d_dst + o, (const uint8_t *)h_src + o, std::min(bytes - o, MAX_PIECE), st, RING, PART));
    return AGC_HIP_OK;
}

// the entropy stage's stream yields to the streams of the steps wherever the hardware queues let it
hipError_t create_low_priority_stream(hipStream_t *s)
{
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess)
        return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, lo);
}

// what agc_hip_create makes at once (everything else is made by the entry point that first needs it).  The entropy stage: two
// low-priority streams, the events that order them, and the one its caller sleeps on
bool make_entropy_lane(agc_hip_ctx *c)
{
    return create_low_priority_stream(&c->zstream.h) == hipSuccess && create_low_priority_stream(&c->zstream2.h) == hipSuccess &&
           hipEventCreateWithFlags(&c->zev_a.h, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->zev_b.h, hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&c->zev_wait.h, hipEventDisableTiming | hipEventBlockingSync) == hipSuccess;
}

// An encode lane, at the first stream's priority: measured with a low-priority lane the whole-sample encode is starved by the
// classification kernels until they are done and ends up on the critical path of the NEXT sample's launch
bool make_encode_lane(agc_hip_ctx::LzLane &L)
{
    const bool ok = hipStreamCreateWithFlags(&L.own.h, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&L.e0.h) == hipSuccess && hipEventCreate(&L.e1.h) == hipSuccess &&
                    hipEventCreateWithFlags(&L.ready.h, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&L.done.h, hipEventDisableTiming) == hipSuccess;
    L.s = L.own;
    return ok;
}

int upload_refs(agc_hip_ctx *c)
{
    if (!c->refs_dirty)
        return AGC_HIP_OK;
    // Only what changed goes over: a registration adds descriptors (a group gets its reference once, agc_hip_ref_register* refuses a
    // second), it never changes one a parse in flight may be reading -- so no lane is waited for and a step moves some KB instead of
    // the whole table (2.8 MB for the 50 k groups of a human sample: 0.3 ms of the driving thread and a twentieth of the pinned ring
    // per sample; the wait for the whole-sample encode on lane 0 was 7 ms of the first step after an idle pipeline).  A table that has
    // to move to a larger buffer is the exception: lanes first, then everything.
    size_t lo = c->refs_dirty_lo, hi = std::min(c->refs_dirty_hi, c->refs.size());
    const size_t need = std::max<size_t>(1, c->refs.size()) * sizeof(RefDesc);
    if (need > c->d_refs.cap || c->refs_on_dev == 0) {
        for (auto *ln : {&c->lane(1), &c->lane(2)})
            if (ln->pending)
                HIPCHK(c, hipStreamSynchronize(ln->s)); // the encode in flight reads the buffer that is about to be freed
        CHK(ensure(c, c->d_refs, need));
        lo = 0;
        hi = c->refs.size();
    }
    if (hi > lo)
        CHK(upload(c, (RefDesc *)c->d_refs.p + lo, c->refs.data() + lo, (hi - lo) * sizeof(RefDesc), c->stream));
    c->refs_on_dev = c->refs.size();
    c->refs_dirty = false;
    c->refs_dirty_lo = c->refs_dirty_hi = 0;
    return AGC_HIP_OK;
}

uint32_t grid_for(uint32_t n_items, uint32_t per_block, uint32_t max_blocks)
{
    uint64_t b = ((uint64_t)n_items + per_block - 1) / per_block;
    if (b < 1)
        b = 1;
    return (uint32_t)std::min<uint64_t>(b, max_blocks);
}

// bytes (one per symbol, device) -> 2-bit layout in the context-owned buffers of `t`, queued on `st`; every block may be
// escaped (room for all of them), so nothing has to be read back
int pack_bytes(agc_hip_ctx *c, const uint8_t *d_codes, uint64_t n, PackTemp &t, hipStream_t st, PackedSrc &out)
{
    out = PackedSrc();
    if (!n)
        return AGC_HIP_OK;
    const uint64_t n_blocks = (n + PACK_BLOCK - 1) / PACK_BLOCK;
    CHK(ensure(c, t.words, n_blocks * (PACK_BLOCK / 4) + 64, st));
    CHK(ensure(c, t.index, n_blocks * 4 + 64, st));
    CHK(ensure(c, t.esc, n_blocks * PACK_BLOCK + 64, st));
    CHK(ensure(c, t.cnt, 64, st));
    HIPCHK(c, hipMemsetAsync(t.cnt.p, 0, 4, st));
    hipLaunchKernelGGL(pack_codes_kernel, dim3((uint32_t)std::min<uint64_t>((n_blocks + 3) / 4, 65536)), dim3(256), 0, st, d_codes, n, (uint32_t *)t.words.p,
                       (int32_t *)t.index.p, (uint8_t *)t.esc.p, (uint32_t *)t.cnt.p, (uint32_t)std::min<uint64_t>(n_blocks, 0x7fffffffu));
    HIPCHK(c, hipGetLastError());
    out.words = (const uint32_t *)t.words.p;
    out.esc_index = (const int32_t *)t.index.p;
    out.esc_bytes = (const uint8_t *)t.esc.p;
    out.n_symbols = n;
    return AGC_HIP_OK;
}

// What every byte-input entry point does once its arguments are checked: the range its sequences [h_off[i], h_off[i] + h_len[i])
// span is packed into `t` on `st`, and `then(src, off2)` -- the work of the packed entry point of the same name -- runs on that
// copy, off2 = their offsets in it
template <class F>
int with_packed_bytes(agc_hip_ctx *c, const uint8_t *d_base, uint32_t n, const uint64_t *h_off, const uint32_t *h_len, PackTemp &t, hipStream_t st, F then)
{
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t lo = ~0ULL, hi = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (h_len[i]) {
            lo = std::min<uint64_t>(lo, h_off[i]);
            hi = std::max<uint64_t>(hi, h_off[i] + h_len[i]);
        }
    PackedSrc src;
    std::vector<uint64_t> off2(n, 0);
    if (hi > lo) {
        for (uint32_t i = 0; i < n; ++i)
            off2[i] = h_len[i] ? h_off[i] - lo : 0;
        CHK(pack_bytes(c, d_base + lo, hi - lo, t, st, src));
    }
    return then(src, off2.data());
}

// ... and every host-text entry point: the texts go to d_in back to back (16-byte aligned; h_text is the caller's, and every entry
// point waits for the stream before it returns), `then(d_base, doff)` is the byte-input entry point of the same name
template <class F>
int with_host_texts(agc_hip_ctx *c, uint32_t n, const uint8_t *h_text, const uint64_t *h_off, const uint32_t *h_len, F then)
{
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> doff(n);
    size_t tot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        doff[i] = tot;
        tot += ((size_t)h_len[i] + 15) & ~(size_t)15;
    }
    CHK(ensure(c, c->d_in, tot + 64));
    for (uint32_t i = 0; i < n; ++i)
        if (h_len[i])
            HIPCHK(c, hipMemcpyAsync((uint8_t *)c->d_in.p + doff[i], h_text + h_off[i], h_len[i], hipMemcpyHostToDevice, c->stream));
    return then((const uint8_t *)c->d_in.p, doff.data());
}

PackedSrc src_of(const agc_hip_packed *pk)
{
    PackedSrc s;
    s.words = pk->d_words;
    s.esc_index = pk->d_esc_index;
    s.esc_bytes = pk->d_esc_bytes;
    s.n_symbols = pk->n_symbols;
    return s;
}

bool slices_inside(const PackedSrc &src, uint32_t n, const uint64_t *h_off, const uint32_t *h_len)
{
    for (uint32_t i = 0; i < n; ++i)
        if (h_len[i] && (h_off[i] > src.n_symbols || h_len[i] > src.n_symbols - h_off[i]))
            return false;
    return true;
}

// Slice jobs (ViewJob) run out of the first stream's buffers or out of those of a reference-store slot.  The three helpers below
// queue on `st` and wait for nothing; `which` is the launch's timing row (KTimer; < 0: not timed).
struct SliceBufs {
    DevBuf &slices, &out, &lag;
};
SliceBufs slice_bufs(agc_hip_ctx *c) { return {c->d_slices, c->lane(0).d_compact, c->d_lag}; }
SliceBufs slice_bufs(agc_hip_ctx::RefStore &r) { return {r.d_slices, r.d_out, r.d_lag}; }

// the jobs of n slices of `src` in b.slices: slice i goes to b.out + h_out_off[i] (h_out_off[n] bytes in all), or nowhere when
// h_out_off is nullptr (counted only)
int put_view_jobs(agc_hip_ctx *c, SliceBufs b, hipStream_t st, uint32_t n, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc,
                  const uint64_t *h_out_off)
{
    if (!slices_inside(src, n, h_off, h_len))
        return AGC_HIP_EINVAL;
    if (h_out_off)
        CHK(ensure(c, b.out, h_out_off[n] + 64, st));
    CHK(ensure(c, b.slices, (size_t)n * sizeof(ViewJob), st));
    std::vector<ViewJob> sl(n);
    for (uint32_t i = 0; i < n; ++i)
        sl[i] = {{src.words, src.esc_index, src.esc_bytes, h_off[i], h_len[i], h_rc ? (uint32_t)(h_rc[i] != 0) : 0u},
                 h_out_off ? (uint8_t *)b.out.p + h_out_off[i] : nullptr};
    return upload(c, b.slices.p, sl.data(), (size_t)n * sizeof(ViewJob), st);
}

// the repetitiveness counters of the first n jobs in b.slices (n > 0), 28 + 28 words each, to h_cnt and h_cur
int queue_lag_counts(agc_hip_ctx *c, SliceBufs b, hipStream_t st, uint32_t n, uint32_t *h_cnt, uint32_t *h_cur, int which)
{
    const size_t half = (size_t)n * 28 * 4;
    CHK(ensure(c, b.lag, 2 * half, st));
    uint32_t *d_cnt = (uint32_t *)b.lag.p, *d_cur = d_cnt + (size_t)n * 28;
    // few slices (steady state): each spread over several blocks to fill the chip
    const uint32_t split = n >= 2048 ? 1u : std::min<uint32_t>(32u, 2048u / n);
    HIPCHK(c, hipMemsetAsync(b.lag.p, 0, 2 * half, st));
    {
        KTimer t(c, which);
        hipLaunchKernelGGL(lag_counts_kernel, dim3(n * split), dim3(256), 0, st, (const ViewJob *)b.slices.p, d_cnt, d_cur, split);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_cnt, d_cnt, half, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_cur, d_cur, half, hipMemcpyDeviceToHost, st));
    return AGC_HIP_OK;
}

// the symbols of the n jobs in b.slices, one byte each, into b.out and from there to h_out (tot bytes)
int queue_expand(agc_hip_ctx *c, SliceBufs b, hipStream_t st, uint32_t n, uint8_t *h_out, uint64_t tot, int which)
{
    {
        KTimer t(c, which);
        hipLaunchKernelGGL(slice_expand_kernel, dim3(grid_for(n, 1, 65536)), dim3(256), 0, st, (const ViewJob *)b.slices.p, n);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_out, b.out.p, tot, hipMemcpyDeviceToHost, st));
    return AGC_HIP_OK;
}

} // namespace

// ===========================================================================
extern "C" {

uint32_t agc_hip_abi_version(void) { return 2; }

int agc_hip_create(agc_hip_ctx **out, int device)
{
    if (!out)
        return AGC_HIP_EINVAL;
    *out = nullptr;
    // The ROCm runtime maps the HIP streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4).  A context has eight
    // streams (steps, two encode lanes, scan prefetch, FASTA pack, two entropy streams + the caller's): on four queues they share, and a
    // wait on an idle stream lasts until the kernels of the stream it shares a queue with are done (measured: pack_fasta_end's
    // hipStreamSynchronize 1 ms behind the followers' encode, profiles/r6/).  Only effective when this is the process's first HIP call
    // (the CLI); a Python caller that initialises HIP first sets the variable itself (bench.py does).
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
        return AGC_HIP_ENODEV;
    agc_hip_ctx *c = new agc_hip_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess || !make_entropy_lane(c) ||
        !make_encode_lane(c->lane(1)) || !make_encode_lane(c->lane(2)) || hipEventCreate(&c->zev0.h) != hipSuccess || hipEventCreate(&c->zev1.h) != hipSuccess) {
        delete c; // (releases what was made)
        return AGC_HIP_ENODEV;
    }
    c->lane(0).s = c->stream;
    *out = c;
    return AGC_HIP_OK;
}

void agc_hip_destroy(agc_hip_ctx *c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->device);
    // Every stream the context has made runs dry and both helper threads hand over what they allocated BEFORE the first member
    // goes: nothing on the device or on a thread refers to a member any more, so the order in which the members' destructors run
    // does not matter.
    for (hipStream_t s_ : {c->stream.h, c->zstream.h, c->zstream2.h, c->lane(1).s, c->lane(2).s, c->pfa.stream.h, c->pf.stream.h, c->ref_store_stream.h})
        if (s_)
            (void)hipStreamSynchronize(s_);
    if (c->arena_spare.valid())
        (void)c->arena_spare.get();
    for (auto &L : c->lanes)
        if (L.chunks.logs_ahead.valid())
            (void)L.chunks.logs_ahead.get();
    delete c;
}

const char *agc_hip_last_error(const agc_hip_ctx *c) { return c ? c->err.c_str() : "no context"; }

int agc_hip_sync(agc_hip_ctx *c)
{
    if (!c)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

int agc_hip_timing_enable(agc_hip_ctx *c, int on)
{
    if (!c)
        return AGC_HIP_EINVAL;
    c->timing = on != 0;
    return AGC_HIP_OK;
}

int agc_hip_timing_reset(agc_hip_ctx *c)
{
    if (!c)
        return AGC_HIP_EINVAL;
    ktimer_read_all(c);
    for (int i = 0; i < AGC_HIP_K_COUNT; ++i) {
        c->ms[i] = 0;
        c->launches[i] = 0;
    }
    return AGC_HIP_OK;
}

int agc_hip_timing_get(agc_hip_ctx *c, int which, double *ms, uint64_t *launches)
{
    if (!c || which < 0 || which >= AGC_HIP_K_COUNT)
        return AGC_HIP_EINVAL;
    ktimer_read_all(c); // (the pairs recorded since the last call: waits for the last of them)
    if (ms)
        *ms = c->ms[which];
    if (launches)
        *launches = c->launches[which];
    return AGC_HIP_OK;
}

int agc_hip_sample_buffer(agc_hip_ctx *c, uint64_t bytes, uint8_t **d_ptr)
{
    if (!c || !d_ptr)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    // (the encode of the previous sample may still be reading the buffer on the second lane: see LzLane::done)
    for (auto *ln : {&c->lane(1), &c->lane(2)})
        if (ln->done_valid) {
            if (bytes + 4096 > c->d_sample.cap)
                HIPCHK(c, hipEventSynchronize(ln->done)); // the buffer is about to be replaced
            else
                HIPCHK(c, hipStreamWaitEvent(c->stream, ln->done, 0));
        }
    for (auto &rs : c->ref_store) // (agc_hip_ref_store_begin_dev does not exist: only packed samples take that path -- kept for symmetry)
        if (rs.pending)
            HIPCHK(c, hipEventSynchronize(rs.done));
    CHK(ensure(c, c->d_sample, bytes + 4096));
    *d_ptr = (uint8_t *)c->d_sample.p;
    return AGC_HIP_OK;
}

int agc_hip_copy_to_device(agc_hip_ctx *c, uint8_t *d_dst, const uint8_t *h_src, uint64_t n)
{
    if (!c || (n && (!d_dst || !h_src)))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d_dst, h_src, n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return AGC_HIP_OK;
}

int agc_hip_sample_pack(agc_hip_ctx *c, const uint8_t *d_codes, uint64_t n_symbols, agc_hip_packed *out)
{
    if (!c || !out || (n_symbols && !d_codes))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    // (the encode of the previous sample may still be reading these buffers on the second lane: see LzLane::done; and the copy of
    // its new references on the reference-store stream)
    for (auto *ln : {&c->lane(1), &c->lane(2)})
        if (ln->done_valid)
            HIPCHK(c, hipEventSynchronize(ln->done));
    for (auto &rs : c->ref_store)
        if (rs.pending)
            HIPCHK(c, hipEventSynchronize(rs.done));
    PackedSrc src;
    {
        KTimer t(c, AGC_HIP_K_PREPROCESS);
        CHK(pack_bytes(c, d_codes, n_symbols, c->pk_sample, c->stream, src));
    }
    out->d_words = src.words;
    out->d_esc_index = src.esc_index;
    out->d_esc_bytes = src.esc_bytes;
    out->n_symbols = n_symbols;
    return AGC_HIP_OK;
}

// ---------------------------------------------------------------------------
// a1
// ---------------------------------------------------------------------------
int agc_hip_preprocess_dev(agc_hip_ctx *c, const uint8_t *d_raw, uint64_t n_raw, uint8_t *d_codes, uint64_t *h_n_codes)
{
    if (!c || !h_n_codes || (n_raw && (!d_raw || !d_codes)))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    *h_n_codes = 0;
    if (!n_raw)
        return AGC_HIP_OK;
    const uint64_t nb64 = (n_raw + PP_TILE - 1) / PP_TILE;
    if (nb64 > 0x7fffffffULL)
        return AGC_HIP_EINVAL;
    const uint32_t nb = (uint32_t)nb64;
    CHK(ensure(c, c->d_pp_cnt, (size_t)nb * 4));
    CHK(ensure(c, c->d_pp_off, (size_t)nb * 8));
    CHK(ensure(c, c->d_pp_total, 8));
    {
        KTimer t(c, AGC_HIP_K_PREPROCESS);
        hipLaunchKernelGGL(pp_count_kernel, dim3(nb), dim3(256), 0, c->stream, d_raw, n_raw, (uint32_t *)c->d_pp_cnt.p);
        hipLaunchKernelGGL(pp_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t *)c->d_pp_cnt.p, nb,
                           (uint64_t *)c->d_pp_off.p, (uint64_t *)c->d_pp_total.p);
        hipLaunchKernelGGL(pp_scatter_kernel, dim3(nb), dim3(256), 0, c->stream, d_raw, n_raw, (const uint64_t *)c->d_pp_off.p, d_codes);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_n_codes, c->d_pp_total.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

int agc_hip_preprocess(agc_hip_ctx *c, const uint8_t *h_raw, uint64_t n_raw, uint8_t *d_codes, uint64_t *h_n_codes)
{
    if (!c || !h_n_codes || (n_raw && (!h_raw || !d_codes)))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    *h_n_codes = 0;
    if (!n_raw)
        return AGC_HIP_OK;
    CHK(ensure(c, c->d_in, n_raw + 64));
    HIPCHK(c, hipMemcpyAsync(c->d_in.p, h_raw, n_raw, hipMemcpyHostToDevice, c->stream));
    return agc_hip_preprocess_dev(c, (const uint8_t *)c->d_in.p, n_raw, d_codes, h_n_codes);
}

// ---------------------------------------------------------------------------
// splitters
// ---------------------------------------------------------------------------
static int splitters_upload(agc_hip_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t cap = 1024;
    while (cap < 2 * (uint64_t)c->spl.size())
        cap <<= 1;
    std::vector<uint64_t> tab(cap, ~0ULL);
    std::vector<uint32_t> bloom(BLOOM_WORDS, 0), bloom2(BLOOM2_WORDS, 0);
    for (uint64_t x : c->spl) {
        const uint64_t h = splitter_hash(x);
        uint64_t s = h & (cap - 1);
        while (tab[s] != ~0ULL)
            s = (s + 1) & (cap - 1);
        tab[s] = x;
        uint32_t w, m;
        bloom_slot((uint32_t)(x >> 32), (uint32_t)x, w, m);
        bloom[w] |= m;
        bloom2_slot(h, w, m);
        bloom2[w] |= m;
    }
    CHK(ensure(c, c->d_table, cap * 8));
    CHK(ensure(c, c->d_bloom, BLOOM_WORDS * 4));
    CHK(ensure(c, c->d_bloom2, BLOOM2_WORDS * 4));
    CHK(upload(c, c->d_bloom2.p, bloom2.data(), BLOOM2_WORDS * 4, c->stream));
    CHK(upload(c, c->d_table.p, tab.data(), cap * 8, c->stream));
    CHK(upload(c, c->d_bloom.p, bloom.data(), BLOOM_WORDS * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the prefetch stream scans with these tables too, ordered behind nothing but this)
    c->table_mask = cap - 1;
    return AGC_HIP_OK;
}

int agc_hip_splitters_set(agc_hip_ctx *c, const uint64_t *h_kmers, uint64_t n)
{
    if (!c || (n && !h_kmers))
        return AGC_HIP_EINVAL;
    c->spl.assign(h_kmers, h_kmers + n);
    std::sort(c->spl.begin(), c->spl.end());
    c->spl.erase(std::unique(c->spl.begin(), c->spl.end()), c->spl.end());
    return splitters_upload(c);
}

int agc_hip_splitters_insert(agc_hip_ctx *c, const uint64_t *h_kmers, uint64_t n)
{
    if (!c || (n && !h_kmers))
        return AGC_HIP_EINVAL;
    c->spl.insert(c->spl.end(), h_kmers, h_kmers + n);
    std::sort(c->spl.begin(), c->spl.end());
    c->spl.erase(std::unique(c->spl.begin(), c->spl.end()), c->spl.end());
    return splitters_upload(c);
}

uint64_t agc_hip_splitters_count(const agc_hip_ctx *c) { return c ? c->spl.size() : 0; }

// ---------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------
} // extern "C"

// sorts the raw hits and applies the reference's "reset the k-mer after a hit" rule (agc_compressor.cpp:2029): the next hit of the
// same contig must end at least k symbols later
static int deliver_hits(agc_hip_ctx *c, uint32_t n_found, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k, uint64_t cap, uint64_t *h_n_hits,
                        uint32_t *h_hit_ctg, uint64_t *h_hit_pos, uint64_t *h_hit_dir, uint64_t *h_hit_rc, const void *d_hits = nullptr,
                        hipStream_t stream = nullptr)
{
    if (!d_hits) {
        d_hits = c->d_hits.p;
        stream = c->stream;
    }
    std::vector<ScanHit> hits(n_found);
    if (n_found) {
        HIPCHK(c, hipMemcpyAsync(hits.data(), d_hits, (size_t)n_found * sizeof(ScanHit), hipMemcpyDeviceToHost, stream));
        HIPCHK(c, hipStreamSynchronize(stream));
    }
    // by position (positions are unique): LSD radix sort, 11 bits a pass, as many passes as the largest position needs
    if (n_found > 1) {
        uint64_t max_pos = 0;
        for (const ScanHit &h : hits)
            max_pos = std::max<uint64_t>(max_pos, h.pos);
        std::vector<ScanHit> tmp(n_found);
        ScanHit *src = hits.data(), *dst = tmp.data();
        for (int sh = 0; sh < 64 && (max_pos >> sh) != 0; sh += 11) {
            uint32_t cnt[2049] = {0};
            for (uint32_t i = 0; i < n_found; ++i)
                ++cnt[(((uint64_t)src[i].pos >> sh) & 2047u) + 1];
            for (int t = 0; t < 2048; ++t)
                cnt[t + 1] += cnt[t];
            for (uint32_t i = 0; i < n_found; ++i)
                dst[cnt[((uint64_t)src[i].pos >> sh) & 2047u]++] = src[i];
            std::swap(src, dst);
        }
        if (src != hits.data())
            std::memcpy(hits.data(), src, (size_t)n_found * sizeof(ScanHit));
    }

    // accept_hits: after a hit the reference resets the k-mer (agc_compressor.cpp:2029), so the next
    // hit of the same contig must end at least k symbols later.
    uint64_t n_acc = 0;
    uint32_t ci = 0;
    bool have_last = false;
    uint64_t last = 0;
    for (const ScanHit &h : hits) {
        while (ci + 1 < n_ctg && h.pos >= h_ctg_off[ci + 1]) {
            ++ci;
            have_last = false;
        }
        if (have_last && h.pos < last + k)
            continue;
        have_last = true;
        last = h.pos;
        if (n_acc < cap) {
            h_hit_ctg[n_acc] = ci;
            h_hit_pos[n_acc] = h.pos - h_ctg_off[ci];
            h_hit_dir[n_acc] = h.dir;
            h_hit_rc[n_acc] = h.rc;
        }
        ++n_acc;
    }
    *h_n_hits = n_acc;
    return n_acc > cap ? AGC_HIP_ECAP : AGC_HIP_OK;
}


extern "C" {

int agc_hip_scan_contigs_dev(agc_hip_ctx *c, const uint8_t *d_codes, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k,
                             uint64_t cap, uint64_t *h_n_hits, uint32_t *h_hit_ctg, uint64_t *h_hit_pos, uint64_t *h_hit_dir,
                             uint64_t *h_hit_rc)
{
    if (!c || !h_ctg_off || !h_n_hits || k < 2 || k > 32)
        return AGC_HIP_EINVAL;
    if (cap && (!h_hit_ctg || !h_hit_pos || !h_hit_dir || !h_hit_rc))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    *h_n_hits = 0;
    if (!c->d_table.p)
        CHK(splitters_upload(c)); // empty set
    const uint64_t total = n_ctg ? h_ctg_off[n_ctg] - h_ctg_off[0] : 0;
    if (!total)
        return AGC_HIP_OK;
    if (!d_codes)
        return AGC_HIP_EINVAL;

    // ranges: contigs cut into pieces of range_len symbols (multiple of one 1 KiB wave step)
    const uint64_t target_waves = 8192ULL * 4;
    uint64_t range_len = (total / target_waves + 1023) / 1024 * 1024;
    range_len = std::min<uint64_t>(std::max<uint64_t>(range_len, 4096), 65536);
    std::vector<ScanRange> ranges;
    for (uint32_t ci = 0; ci < n_ctg; ++ci) {
        const uint64_t b = h_ctg_off[ci], e = h_ctg_off[ci + 1];
        if (e < b)
            return AGC_HIP_EINVAL;
        if (e - b < k)
            continue;
        for (uint64_t p = b; p < e; p += range_len)
            ranges.push_back({b, e, p, std::min(e, p + range_len)});
    }
    if (ranges.empty())
        return AGC_HIP_OK;
    if (ranges.size() > 0x7fffffffULL)
        return AGC_HIP_EINVAL;
    CHK(ensure(c, c->d_ranges, ranges.size() * sizeof(ScanRange)));
    CHK(ensure(c, c->d_counter, 64));
    CHK(upload(c, c->d_ranges.p, ranges.data(), ranges.size() * sizeof(ScanRange), c->stream));

    uint32_t dev_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(total / 2000 + 4096, c->d_hits.cap / sizeof(ScanHit)), 1u << 30);
    uint32_t n_found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        CHK(ensure(c, c->d_hits, (size_t)dev_cap * sizeof(ScanHit)));
        HIPCHK(c, hipMemsetAsync(c->d_counter.p, 0, 4, c->stream));
        ScanArgs a;
        a.codes = d_codes;
        a.ranges = (const ScanRange *)c->d_ranges.p;
        a.n_ranges = (uint32_t)ranges.size();
        a.k = k;
        a.table = (const uint64_t *)c->d_table.p;
        a.table_mask = c->table_mask;
        a.bloom = (const uint32_t *)c->d_bloom.p;
        a.bloom2 = (const uint32_t *)c->d_bloom2.p;
        a.hits = (ScanHit *)c->d_hits.p;
        a.n_hits = (uint32_t *)c->d_counter.p;
        a.cap = dev_cap;
        const uint32_t grid = grid_for((uint32_t)ranges.size(), 16, 512);
        {
            KTimer t(c, AGC_HIP_K_SCAN);
            hipLaunchKernelGGL(scan_kernel, dim3(grid), dim3(1024), 0, c->stream, a);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&n_found, c->d_counter.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n_found <= dev_cap)
            break;
        dev_cap = n_found;
    }
    return deliver_hits(c, n_found, h_ctg_off, n_ctg, k, cap, h_n_hits, h_hit_ctg, h_hit_pos, h_hit_dir, h_hit_rc);
}

int agc_hip_scan_contigs(agc_hip_ctx *c, const uint8_t *h_codes, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k,
                         uint64_t cap, uint64_t *h_n_hits, uint32_t *h_hit_ctg, uint64_t *h_hit_pos, uint64_t *h_hit_dir,
                         uint64_t *h_hit_rc)
{
    if (!c || !h_ctg_off)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t lo = n_ctg ? h_ctg_off[0] : 0, hi = n_ctg ? h_ctg_off[n_ctg] : 0;
    if (hi > lo && !h_codes)
        return AGC_HIP_EINVAL;
    CHK(ensure(c, c->d_in, (hi - lo) + 64));
    if (hi > lo)
        HIPCHK(c, hipMemcpyAsync(c->d_in.p, h_codes + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    std::vector<uint64_t> off(n_ctg + 1, 0);
    for (uint32_t i = 0; i <= n_ctg && n_ctg; ++i)
        off[i] = h_ctg_off[i] - lo;
    return agc_hip_scan_contigs_dev(c, (const uint8_t *)c->d_in.p, off.data(), n_ctg, k, cap, h_n_hits, h_hit_ctg, h_hit_pos,
                                    h_hit_dir, h_hit_rc);
}


// ---------------------------------------------------------------------------
// 2-bit packed samples
// ---------------------------------------------------------------------------
uint64_t agc_hip_packed_words_bytes(uint64_t n_symbols) { return ((n_symbols + PACK_BLOCK - 1) / PACK_BLOCK) * (PACK_BLOCK / 4) + 64; }
uint64_t agc_hip_packed_index_bytes(uint64_t n_symbols) { return ((n_symbols + PACK_BLOCK - 1) / PACK_BLOCK) * 4 + 64; }

int agc_hip_pack_dev(agc_hip_ctx *c, const uint8_t *d_codes, uint64_t n_symbols, uint32_t *d_words, int32_t *d_esc_index, uint8_t *d_esc_bytes,
                     uint64_t esc_cap_blocks, uint64_t *h_n_esc_blocks)
{
    if (!c || !h_n_esc_blocks || (n_symbols && (!d_codes || !d_words || !d_esc_index)) || (esc_cap_blocks && !d_esc_bytes))
        return AGC_HIP_EINVAL;
    *h_n_esc_blocks = 0;
    if (!n_symbols)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure(c, c->d_counter, 64));
    HIPCHK(c, hipMemsetAsync(c->d_counter.p, 0, 4, c->stream));
    const uint64_t n_blocks = (n_symbols + PACK_BLOCK - 1) / PACK_BLOCK;
    {
        KTimer t(c, AGC_HIP_K_PREPROCESS);
        hipLaunchKernelGGL(pack_codes_kernel, dim3((uint32_t)std::min<uint64_t>((n_blocks + 3) / 4, 65536)), dim3(256), 0, c->stream, d_codes, n_symbols,
                           d_words, d_esc_index, d_esc_bytes, (uint32_t *)c->d_counter.p, (uint32_t)std::min<uint64_t>(esc_cap_blocks, 0x7fffffffu));
    }
    HIPCHK(c, hipGetLastError());
    uint32_t cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, c->d_counter.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *h_n_esc_blocks = cnt;
    return cnt > esc_cap_blocks ? AGC_HIP_ECAP : AGC_HIP_OK;
}

int agc_hip_expand_dev(agc_hip_ctx *c, const agc_hip_packed *pk, uint8_t *d_codes)
{
    if (!c || !pk || (pk->n_symbols && (!pk->d_words || !pk->d_esc_index || !d_codes)))
        return AGC_HIP_EINVAL;
    if (!pk->n_symbols)
        return AGC_HIP_OK;
    if ((uintptr_t)d_codes & 15)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const PackedView pv = {pk->d_words, pk->d_esc_index, pk->d_esc_bytes, pk->n_symbols};
    const uint64_t n_blocks = (pk->n_symbols + PACK_BLOCK - 1) / PACK_BLOCK;
    {
        KTimer t(c, AGC_HIP_K_PREPROCESS);
        hipLaunchKernelGGL(expand_codes_kernel, dim3((uint32_t)std::min<uint64_t>((n_blocks + 3) / 4, 65536)), dim3(256), 0, c->stream, pv, d_codes);
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

// raw FASTA bodies (device) -> the packed sample, one pass (pack_kernels.hip), on a stream of its own
int agc_hip_pack_fasta_begin(agc_hip_ctx *c, const uint8_t *d_raw, uint64_t n_raw, const uint64_t *h_raw_begin, const uint64_t *h_raw_end, uint32_t n_ctg,
                             uint32_t *d_words, int32_t *d_esc_index, uint8_t *d_esc_bytes, uint64_t esc_cap_blocks)
{
    if (!c || (n_ctg && (!h_raw_begin || !h_raw_end)) || (n_raw && n_ctg && (!d_raw || !d_words || !d_esc_index)) || (esc_cap_blocks && !d_esc_bytes) ||
        ((uintptr_t)d_raw & 15) || ((uintptr_t)d_words & 15))
        return AGC_HIP_EINVAL;
    uint64_t prev = 0;
    for (uint32_t i = 0; i < n_ctg; ++i) {
        if (h_raw_begin[i] < prev || h_raw_end[i] < h_raw_begin[i] || h_raw_end[i] > n_raw)
            return AGC_HIP_EINVAL;
        prev = h_raw_end[i];
    }
    const uint64_t n_tiles64 = (n_raw + PF_TILE - 1) / PF_TILE;
    if (n_tiles64 > 0x7fffffffULL)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    agc_hip_ctx::PackFasta &P = c->pfa;
    if (!P.stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&P.stream.h, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreate(&P.e0.h));
        HIPCHK(c, hipEventCreate(&P.e1.h));
    }
    if (P.pending) { // (a pack nobody collected: dropped)
        HIPCHK(c, hipStreamSynchronize(P.stream));
        P.pending = false;
    }
    P.n_ctg = n_ctg;
    P.n_raw = n_raw;
    P.esc_cap = esc_cap_blocks;
    const size_t res_words = (size_t)n_ctg + 4;
    CHK(ensure_pinned(c, P.h_res, res_words * 8, (res_words + 1024) * 8));
    uint64_t *const h_res = P.h_res.as<uint64_t>();
    const uint32_t n_tiles = (uint32_t)n_tiles64;
    // the counters: [4, 8) escaped blocks, [8, 16) the total
    CHK(ensure(c, P.d_state, 64, P.stream));
    CHK(ensure(c, P.d_rng, std::max<size_t>(16, (size_t)n_ctg * 16), P.stream));
    CHK(ensure(c, P.d_off, ((size_t)n_ctg + 2) * 8, P.stream));
    HIPCHK(c, hipMemsetAsync(P.d_state.p, 0, 64, P.stream));
    HIPCHK(c, hipMemsetAsync(P.d_off.p, 0xFF, ((size_t)n_ctg + 1) * 8, P.stream));
    if (n_ctg) {
        CHK(upload(c, P.d_rng.p, h_raw_begin, (size_t)n_ctg * 8, P.stream));
        CHK(upload(c, (uint8_t *)P.d_rng.p + (size_t)n_ctg * 8, h_raw_end, (size_t)n_ctg * 8, P.stream));
    }
    P.timed = c->timing;
    if (P.timed)
        (void)hipEventRecord(P.e0, P.stream);
    if (n_tiles && n_ctg) {
        PackFastaArgs a;
        a.raw = d_raw;
        a.n_raw = n_raw;
        a.rng_begin = (const uint64_t *)P.d_rng.p;
        a.rng_end = a.rng_begin + n_ctg;
        a.n_rng = n_ctg;
        a.n_tiles = n_tiles;
        a.esc_count = (uint32_t *)P.d_state.p + 1;
        a.total = (unsigned long long *)P.d_state.p + 1;
        a.words = d_words;
        a.esc_index = d_esc_index;
        a.esc_bytes = d_esc_bytes;
        a.esc_cap = (uint32_t)std::min<uint64_t>(esc_cap_blocks, 0x7fffffffu);
        a.ctg_off = (unsigned long long *)P.d_off.p;
        {
            const uint32_t n_sb = (n_tiles + PF_SCAN_TILES - 1) / PF_SCAN_TILES;
            // d_tcnt: counts per tile, then the scan blocks' totals; d_toff: offsets inside a scan block (u32), then the blocks' offsets (u64)
            const size_t tl_bytes = ((size_t)n_tiles * 4 + 255) & ~(size_t)255;
            CHK(ensure(c, P.d_tcnt, tl_bytes + (size_t)n_sb * 4 + 64, P.stream));
            CHK(ensure(c, P.d_toff, tl_bytes + (size_t)n_sb * 8 + 64, P.stream));
            uint32_t *d_cnt = (uint32_t *)P.d_tcnt.p, *d_tot = (uint32_t *)((uint8_t *)P.d_tcnt.p + tl_bytes);
            uint32_t *d_local = (uint32_t *)P.d_toff.p;
            uint64_t *d_boff = (uint64_t *)((uint8_t *)P.d_toff.p + tl_bytes);
            a.tile_local = d_local;
            a.block_off = d_boff;
            hipLaunchKernelGGL(pack_fasta_count_kernel, dim3(n_tiles), dim3(256), 0, P.stream, a, d_cnt);
            hipLaunchKernelGGL(pack_fasta_scan_kernel, dim3(n_sb), dim3(1024), 0, P.stream, (const uint32_t *)d_cnt, n_tiles, d_local, d_tot);
            hipLaunchKernelGGL(pp_scan_kernel, dim3(1), dim3(1024), 0, P.stream, (const uint32_t *)d_tot, n_sb, d_boff,
                               (uint64_t *)((uint8_t *)P.d_state.p + 32)); // (its total: unused, the last tile writes a.total)
            hipLaunchKernelGGL(pack_fasta_kernel, dim3(n_tiles), dim3(256), 0, P.stream, a);
        }
        HIPCHK(c, hipGetLastError());
    }
    if (P.timed)
        (void)hipEventRecord(P.e1, P.stream);
    HIPCHK(c, hipMemcpyAsync(h_res, P.d_off.p, ((size_t)n_ctg + 1) * 8, hipMemcpyDeviceToHost, P.stream));
    HIPCHK(c, hipMemcpyAsync(h_res + n_ctg + 1, P.d_state.p, 16, hipMemcpyDeviceToHost, P.stream));
    P.pending = true;
    return AGC_HIP_OK;
}

int agc_hip_pack_fasta_end(agc_hip_ctx *c, uint64_t *h_ctg_off, uint64_t *h_n_esc_blocks)
{
    if (!c || !h_ctg_off || !h_n_esc_blocks)
        return AGC_HIP_EINVAL;
    agc_hip_ctx::PackFasta &P = c->pfa;
    if (!P.pending)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(P.stream));
    P.pending = false;
    if (P.timed) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, P.e0, P.e1);
        c->ms[AGC_HIP_K_PACK] += ms;
        c->launches[AGC_HIP_K_PACK] += 1;
        P.timed = false;
    }
    const uint32_t n = P.n_ctg;
    const uint64_t *const h_res = P.h_res.as<uint64_t>();
    const uint32_t *cnt = (const uint32_t *)(h_res + n + 1); // (unused), escaped blocks; the total in the next 8 bytes
    const uint64_t total = (P.n_raw && n) ? h_res[n + 2] : 0;
    for (uint32_t i = 0; i < n; ++i) // (a contig whose first byte no tile holds -- it begins at the end of the buffer -- is empty and begins at the total)
        h_ctg_off[i] = h_res[i] == ~0ULL ? total : h_res[i];
    h_ctg_off[n] = total;
    *h_n_esc_blocks = (P.n_raw && n) ? cnt[1] : 0;
    return *h_n_esc_blocks > P.esc_cap ? AGC_HIP_ECAP : AGC_HIP_OK;
}

int agc_hip_pack_fasta_dev(agc_hip_ctx *c, const uint8_t *d_raw, uint64_t n_raw, const uint64_t *h_raw_begin, const uint64_t *h_raw_end, uint32_t n_ctg,
                           uint32_t *d_words, int32_t *d_esc_index, uint8_t *d_esc_bytes, uint64_t esc_cap_blocks, uint64_t *h_ctg_off, uint64_t *h_n_esc_blocks)
{
    if (!h_ctg_off || !h_n_esc_blocks)
        return AGC_HIP_EINVAL;
    CHK(agc_hip_pack_fasta_begin(c, d_raw, n_raw, h_raw_begin, h_raw_end, n_ctg, d_words, d_esc_index, d_esc_bytes, esc_cap_blocks));
    return agc_hip_pack_fasta_end(c, h_ctg_off, h_n_esc_blocks);
}

// A window of FASTA bodies in HOST memory -> the packed sample in the context's own buffers (those of agc_hip_sample_pack): the
// bodies go to HBM as they are, back to back, and the pack_fasta kernels make the 2-bit layout from them -- what a host that reads
// FASTA files calls once per window (include/agc_hip.h).
int agc_hip_sample_pack_fasta(agc_hip_ctx *c, uint32_t n_ctg, const uint8_t *const *h_raw, const uint64_t *h_len, agc_hip_packed *out, uint64_t *h_ctg_off)
{
    if (!c || !out || !h_ctg_off || (n_ctg && (!h_raw || !h_len)))
        return AGC_HIP_EINVAL;
    *out = agc_hip_packed{};
    HIPCHK(c, hipSetDevice(c->device));
    if (c->pfa.pending) {
        c->err = "sample_pack_fasta: a conversion queued by agc_hip_pack_fasta_begin is pending";
        return AGC_HIP_EINVAL;
    }
    std::vector<uint64_t> rb(n_ctg), re(n_ctg);
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_ctg; ++i) {
        if (h_len[i] && !h_raw[i])
            return AGC_HIP_EINVAL;
        rb[i] = tot;
        tot += h_len[i];
        re[i] = tot;
    }
    for (uint32_t i = 0; i <= n_ctg; ++i)
        h_ctg_off[i] = 0;
    if (!tot)
        return AGC_HIP_OK;
    // (the encode of the previous sample may still be reading the packed buffers on a lane: see LzLane::done; and the copy of its new
    // references on the reference-store stream)
    for (auto *ln : {&c->lane(1), &c->lane(2)})
        if (ln->done_valid)
            HIPCHK(c, hipEventSynchronize(ln->done));
    for (auto &rs : c->ref_store)
        if (rs.pending)
            HIPCHK(c, hipEventSynchronize(rs.done));
    CHK(ensure(c, c->d_in, tot + 64));
    for (uint32_t i = 0; i < n_ctg; ++i)
        if (h_len[i])
            HIPCHK(c, hipMemcpyAsync((uint8_t *)c->d_in.p + rb[i], h_raw[i], h_len[i], hipMemcpyHostToDevice, c->stream));
    // every byte may be a symbol and every block escaped: room for all of them, nothing has to be asked twice
    PackTemp &t = c->pk_sample;
    const uint64_t n_blocks = (tot + PACK_BLOCK - 1) / PACK_BLOCK;
    CHK(ensure(c, t.words, n_blocks * (PACK_BLOCK / 4) + 64));
    CHK(ensure(c, t.index, n_blocks * 4 + 64));
    CHK(ensure(c, t.esc, n_blocks * PACK_BLOCK + 64));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the bodies are in HBM, the buffers are where they will stay)
    uint64_t n_esc = 0;
    CHK(agc_hip_pack_fasta_begin(c, (const uint8_t *)c->d_in.p, tot, rb.data(), re.data(), n_ctg, (uint32_t *)t.words.p, (int32_t *)t.index.p, (uint8_t *)t.esc.p,
                                 n_blocks));
    CHK(agc_hip_pack_fasta_end(c, h_ctg_off, &n_esc));
    out->d_words = (const uint32_t *)t.words.p;
    out->d_esc_index = (const int32_t *)t.index.p;
    out->d_esc_bytes = (const uint8_t *)t.esc.p;
    out->n_symbols = h_ctg_off[n_ctg];
    return AGC_HIP_OK;
}

// filter over the last 16 symbols of every splitter and of its reverse complement, for k-mer length k (cached per k)
static int sbloom_upload(agc_hip_ctx *c, uint32_t k)
{
    if (c->sbloom_k == k && c->sbloom_n == c->spl.size() && c->d_sbloom.p)
        return AGC_HIP_OK;
    std::vector<uint32_t> bl(SBLOOM_WORDS, 0);
    const uint32_t lshift = 64 - 2 * k;
    const uint64_t kmask = k == 32 ? ~0ULL : ((1ULL << (2 * k)) - 1ULL);
    auto rev2h = [](uint64_t x) {
        x = ((x >> 2) & 0x3333333333333333ULL) | ((x & 0x3333333333333333ULL) << 2);
        x = ((x >> 4) & 0x0F0F0F0F0F0F0F0FULL) | ((x & 0x0F0F0F0F0F0F0F0FULL) << 4);
        return __builtin_bswap64(x);
    };
    for (uint64_t x : c->spl) {
        const uint64_t dir = (x >> lshift) & kmask;                 // right-aligned, last symbol in the low bits
        const uint64_t rc = (rev2h(~dir) >> lshift) & kmask;
        for (uint64_t v : {dir, rc}) {
            uint32_t w, m;
            sbloom_slot((uint32_t)v, w, m);
            bl[w] |= m;
        }
    }
    CHK(ensure(c, c->d_sbloom, SBLOOM_WORDS * 4));
    CHK(upload(c, c->d_sbloom.p, bl.data(), SBLOOM_WORDS * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (as in splitters_upload: the prefetch stream reads the filter)
    c->sbloom_k = k;
    c->sbloom_n = c->spl.size();
    return AGC_HIP_OK;
}

} // extern "C"

// the ranges of the 2-bit scan: the contigs of at least k symbols in pieces of about range_len symbols whose inner boundaries are
// multiples of PACK_BLOCK in the buffer
static int packed_ranges(const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k, uint64_t total, std::vector<ScanRange> &out)
{
    const uint64_t target_waves = 4096ULL * 4;
    uint64_t range_len = (total / target_waves + PACK_BLOCK - 1) / PACK_BLOCK * PACK_BLOCK;
    range_len = std::min<uint64_t>(std::max<uint64_t>(range_len, 8 * PACK_BLOCK), 256 * PACK_BLOCK);
    for (uint32_t ci = 0; ci < n_ctg; ++ci) {
        const uint64_t b = h_ctg_off[ci], e = h_ctg_off[ci + 1];
        if (e < b)
            return AGC_HIP_EINVAL;
        if (e - b < k)
            continue;
        for (uint64_t p = b; p < e;) {
            uint64_t q = (p + range_len) & ~(uint64_t)(PACK_BLOCK - 1);
            if (q >= e || e - q < PACK_BLOCK)
                q = e;
            out.push_back({b, e, p, q});
            p = q;
        }
    }
    return AGC_HIP_OK;
}

// the packed scan of n_ranges ranges (in `ranges`) queued on `st`: up to dev_cap raw hits into `hits`, their number -- which may be
// larger -- into the word at `counter`, which the caller has cleared on `st`.  timer_slot: KTimer's row (< 0: not timed)
static int launch_packed_scan(agc_hip_ctx *c, const PackedView &pv, const DevBuf &ranges, uint32_t n_ranges, uint32_t k, const DevBuf &hits, const DevBuf &counter,
                              uint32_t dev_cap, hipStream_t st, int timer_slot)
{
    if (!c->lds_scan_set) {
        HIPCHK(c, hipFuncSetAttribute((const void *)scan_packed_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SBLOOM_WORDS * 4));
        c->lds_scan_set = true;
    }
    ScanPackedArgs a;
    a.pv = pv;
    a.ranges = (const ScanRange *)ranges.p;
    a.n_ranges = n_ranges;
    a.k = k;
    a.table = (const uint64_t *)c->d_table.p;
    a.table_mask = c->table_mask;
    a.sbloom = (const uint32_t *)c->d_sbloom.p;
    a.bloom2 = (const uint32_t *)c->d_bloom2.p;
    a.hits = (ScanHit *)hits.p;
    a.n_hits = (uint32_t *)counter.p;
    a.cap = dev_cap;
    const uint32_t grid = grid_for(n_ranges, 16, 256); // one 1024-thread block per CU (128 KiB of LDS each)
    {
        KTimer t(c, timer_slot);
        hipLaunchKernelGGL(scan_packed_kernel, dim3(grid), dim3(1024), SBLOOM_WORDS * 4, st, a);
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

// the packed splitter scan of a sample on the context's stream: raw hits (unsorted, before the reset rule) in c->d_hits
static int packed_scan_raw(agc_hip_ctx *c, const agc_hip_packed *pk, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k, uint32_t *n_found_out)
{
    *n_found_out = 0;
    if (!c->d_table.p)
        CHK(splitters_upload(c));
    const uint64_t total = n_ctg ? h_ctg_off[n_ctg] - h_ctg_off[0] : 0;
    if (!total)
        return AGC_HIP_OK;
    if (!pk->d_words || !pk->d_esc_index || h_ctg_off[n_ctg] > pk->n_symbols)
        return AGC_HIP_EINVAL;
    CHK(sbloom_upload(c, k));
    std::vector<ScanRange> ranges;
    CHK(packed_ranges(h_ctg_off, n_ctg, k, total, ranges));
    if (ranges.empty())
        return AGC_HIP_OK;
    if (ranges.size() > 0x7fffffffULL)
        return AGC_HIP_EINVAL;
    CHK(ensure(c, c->d_ranges, ranges.size() * sizeof(ScanRange)));
    CHK(ensure(c, c->d_counter, 64));
    CHK(upload(c, c->d_ranges.p, ranges.data(), ranges.size() * sizeof(ScanRange), c->stream));
    const PackedView pv = {pk->d_words, pk->d_esc_index, pk->d_esc_bytes, pk->n_symbols};
    uint32_t dev_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(total / 2000 + 4096, c->d_hits.cap / sizeof(ScanHit)), 1u << 30);
    uint32_t n_found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) { // (more hits than the list held: once more, with room for as many as were counted)
        CHK(ensure(c, c->d_hits, (size_t)dev_cap * sizeof(ScanHit)));
        HIPCHK(c, hipMemsetAsync(c->d_counter.p, 0, 4, c->stream));
        CHK(launch_packed_scan(c, pv, c->d_ranges, (uint32_t)ranges.size(), k, c->d_hits, c->d_counter, dev_cap, c->stream, AGC_HIP_K_SCAN));
        HIPCHK(c, hipMemcpyAsync(&n_found, c->d_counter.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (n_found <= dev_cap)
            break;
        dev_cap = n_found;
    }
    *n_found_out = n_found;
    return AGC_HIP_OK;
}

// The prefetch of this very sample, collected: AGC_HIP_EINVAL when nothing, or something else, was prefetched; otherwise its stream
// is waited for and its time booked on the scan row.  Then c->pf.scanned, *h_count, dev_cap and d_hits say what it found.
static int collect_prefetch(agc_hip_ctx *c, const agc_hip_packed *pk, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k)
{
    agc_hip_ctx::Prefetch &pf = c->pf;
    if (!pf.valid || pf.words != pk->d_words || pf.n_symbols != pk->n_symbols || pf.k != k || pf.n_ctg != n_ctg || pf.first_off != h_ctg_off[0] ||
        pf.last_off != h_ctg_off[n_ctg])
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(pf.stream));
    if (pf.timed) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, pf.e0, pf.e1);
        c->ms[AGC_HIP_K_SCAN] += ms;
        c->launches[AGC_HIP_K_SCAN] += 1;
        pf.timed = false;
    }
    return AGC_HIP_OK;
}

extern "C" {

int agc_hip_scan_packed_dev(agc_hip_ctx *c, const agc_hip_packed *pk, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k, uint64_t cap,
                            uint64_t *h_n_hits, uint32_t *h_hit_ctg, uint64_t *h_hit_pos, uint64_t *h_hit_dir, uint64_t *h_hit_rc)
{
    if (!c || !pk || !h_ctg_off || !h_n_hits || k < 16 || k > 32)
        return AGC_HIP_EINVAL; // (k < 16: the last-16-symbols filter does not apply; expand and use agc_hip_scan_contigs_dev)
    if (cap && (!h_hit_ctg || !h_hit_pos || !h_hit_dir || !h_hit_rc))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    *h_n_hits = 0;
    uint32_t n_found = 0;
    CHK(packed_scan_raw(c, pk, h_ctg_off, n_ctg, k, &n_found));
    if (!n_found)
        return AGC_HIP_OK;
    return deliver_hits(c, n_found, h_ctg_off, n_ctg, k, cap, h_n_hits, h_hit_ctg, h_hit_pos, h_hit_dir, h_hit_rc);
}

// The next sample ahead of its turn (include/agc_hip.h): its packed scan queued on the prefetch stream, nothing waited for.
int agc_hip_prefetch_packed_dev(agc_hip_ctx *c, const agc_hip_packed *pk, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k)
{
    if (!c || !pk || !h_ctg_off || !n_ctg || k < 16 || k > 32 || !pk->d_words || !pk->d_esc_index || !pk->n_symbols ||
        h_ctg_off[n_ctg] > pk->n_symbols)
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    agc_hip_ctx::Prefetch &pf = c->pf;
    if (!pf.stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&pf.stream.h, hipStreamNonBlocking));
        CHK(ensure_pinned(c, pf.h_count, 64, 64));
        HIPCHK(c, hipEventCreate(&pf.e0.h));
        HIPCHK(c, hipEventCreate(&pf.e1.h));
    }
    HIPCHK(c, hipStreamSynchronize(pf.stream)); // (a prefetch nobody asked for again: its kernels must be done before its buffers go)
    pf.valid = false;
    if (!c->d_table.p)
        CHK(splitters_upload(c));
    CHK(sbloom_upload(c, k));
    const PackedView pv = {pk->d_words, pk->d_esc_index, pk->d_esc_bytes, pk->n_symbols};
    pf.timed = c->timing;
    if (pf.timed)
        HIPCHK(c, hipEventRecord(pf.e0, pf.stream));
    // the scan: as packed_scan_raw, own scratch, nothing waited for -- and one attempt: a hit list that overflows (it has twice the
    // ordinary room per symbol) is found out by whoever collects the prefetch, who scans again the ordinary way
    const uint64_t total = h_ctg_off[n_ctg] - h_ctg_off[0];
    std::vector<ScanRange> ranges;
    CHK(packed_ranges(h_ctg_off, n_ctg, k, total, ranges));
    pf.scanned = !ranges.empty() && ranges.size() <= 0x7fffffffULL;
    *pf.h_count.as<uint32_t>() = 0;
    if (pf.scanned) {
        CHK(ensure(c, pf.d_ranges, ranges.size() * sizeof(ScanRange), pf.stream));
        CHK(ensure(c, pf.d_counter, 64, pf.stream));
        pf.dev_cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(total / 1000 + 4096, pf.d_hits.cap / sizeof(ScanHit)), 1u << 30);
        CHK(ensure(c, pf.d_hits, (size_t)pf.dev_cap * sizeof(ScanHit), pf.stream));
        CHK(upload(c, pf.d_ranges.p, ranges.data(), ranges.size() * sizeof(ScanRange), pf.stream));
        HIPCHK(c, hipMemsetAsync(pf.d_counter.p, 0, 4, pf.stream));
        CHK(launch_packed_scan(c, pv, pf.d_ranges, (uint32_t)ranges.size(), k, pf.d_hits, pf.d_counter, pf.dev_cap, pf.stream, -1));
        HIPCHK(c, hipMemcpyAsync(pf.h_count.p, pf.d_counter.p, 4, hipMemcpyDeviceToHost, pf.stream));
    }
    if (pf.timed)
        HIPCHK(c, hipEventRecord(pf.e1, pf.stream));
    pf.words = pk->d_words;
    pf.n_symbols = pk->n_symbols;
    pf.k = k;
    pf.n_ctg = n_ctg;
    pf.first_off = h_ctg_off[0];
    pf.last_off = h_ctg_off[n_ctg];
    pf.valid = true;
    return AGC_HIP_OK;
}

int agc_hip_scan_prefetched(agc_hip_ctx *c, const agc_hip_packed *pk, const uint64_t *h_ctg_off, uint32_t n_ctg, uint32_t k, uint64_t cap,
                            uint64_t *h_n_hits, uint32_t *h_hit_ctg, uint64_t *h_hit_pos, uint64_t *h_hit_dir, uint64_t *h_hit_rc)
{
    if (!c || !pk || !h_ctg_off || !h_n_hits)
        return AGC_HIP_EINVAL;
    CHK(collect_prefetch(c, pk, h_ctg_off, n_ctg, k));
    const agc_hip_ctx::Prefetch &pf = c->pf;
    *h_n_hits = 0;
    if (!pf.scanned)
        return AGC_HIP_OK;
    const uint32_t n_found = *pf.h_count.as<uint32_t>();
    if (n_found > pf.dev_cap) // (more hits than the list held: the scan again, the ordinary way)
        return agc_hip_scan_packed_dev(c, pk, h_ctg_off, n_ctg, k, cap, h_n_hits, h_hit_ctg, h_hit_pos, h_hit_dir, h_hit_rc);
    return deliver_hits(c, n_found, h_ctg_off, n_ctg, k, cap, h_n_hits, h_hit_ctg, h_hit_pos, h_hit_dir, h_hit_rc, pf.d_hits.p, pf.stream);
}

// ---------------------------------------------------------------------------
// references
// ---------------------------------------------------------------------------
} // extern "C"

// new references out of a packed buffer: stored form (2-bit words from bit 0, escape blocks where needed), index, key filter
static int ref_register_impl(agc_hip_ctx *c, uint32_t n_refs, const uint32_t *h_gid, const PackedSrc &src, const uint64_t *h_off,
                             const uint32_t *h_len, const uint8_t *h_rc, uint32_t min_match_len)
{
    if (min_match_len < HASHING_STEP + 4 || min_match_len > 32)
        return AGC_HIP_EINVAL; // key_len = mml-3 must fit 2 bits x key_len <= 58 and the wave's 64 lanes
    if (!n_refs)
        return AGC_HIP_OK;
    const uint32_t key_len = min_match_len - HASHING_STEP + 1;
    uint32_t max_gid = 0;
    for (uint32_t i = 0; i < n_refs; ++i) {
        max_gid = std::max(max_gid, h_gid[i]);
        if (h_gid[i] < c->refs.size() && c->refs[h_gid[i]].valid) {
            c->err = "group " + std::to_string(h_gid[i]) + " already has a reference";
            return AGC_HIP_EINVAL;
        }
    }
    {
        std::vector<uint32_t> g(h_gid, h_gid + n_refs);
        std::sort(g.begin(), g.end());
        if (std::adjacent_find(g.begin(), g.end()) != g.end())
            return AGC_HIP_EINVAL;
    }

    // 1. the stored forms, back to back (lz_plan.h: stored_bytes)
    std::vector<IdxBuild> jobs(n_refs);
    std::vector<uint64_t> roff(n_refs), toff(n_refs), boff(n_refs);
    uint8_t *rbase = nullptr, *tbase = nullptr, *bbase = nullptr;
    CHK(arena_alloc(c, lp::prefix(n_refs, roff.data(), [&](uint32_t i) { return lp::stored_bytes(h_len[i]); }), &rbase));
    for (uint32_t i = 0; i < n_refs; ++i) {
        IdxBuild &j = jobs[i] = IdxBuild(); // (escape blocks, table and filter: null until step 2 places them)
        j.src = {src.words, src.esc_index, src.esc_bytes, h_off[i], h_len[i], h_rc ? (uint32_t)(h_rc[i] != 0) : 0u};
        j.words = (uint32_t *)(rbase + roff[i]);
        j.ref_size = h_len[i];
        j.key_len = key_len;
        j.is_short = lp::is_short(h_len[i]);
    }
    CHK(ensure(c, c->d_jobs, (size_t)n_refs * sizeof(IdxBuild)));
    CHK(ensure(c, c->d_counts, (size_t)n_refs * 4));
    CHK(ensure(c, c->d_flags, (size_t)n_refs * 4));
    CHK(upload(c, c->d_jobs.p, jobs.data(), (size_t)n_refs * sizeof(IdxBuild), c->stream));
    const uint32_t split = lp::split_factor(n_refs);
    HIPCHK(c, hipMemsetAsync(c->d_flags.p, 0, (size_t)n_refs * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_counts.p, 0, (size_t)n_refs * 4, c->stream));
    {
        KTimer t(c, AGC_HIP_K_REFSTORE);
        hipLaunchKernelGGL(ref_pack_kernel, dim3(n_refs * split), dim3(256), 0, c->stream, (const IdxBuild *)c->d_jobs.p, (uint32_t *)c->d_flags.p, split);
    }
    // 2. count keys -> table sizes (lz_plan.h: ht_size), tables pre-set to all ones
    std::vector<uint32_t> counts(n_refs), flags(n_refs);
    {
        KTimer t(c, AGC_HIP_K_INDEX);
        hipLaunchKernelGGL(idx_count_kernel, dim3(n_refs * split), dim3(256), 0, c->stream, (const IdxBuild *)c->d_jobs.p,
                           (uint32_t *)c->d_counts.p, split);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(counts.data(), c->d_counts.p, (size_t)n_refs * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(flags.data(), c->d_flags.p, (size_t)n_refs * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t tab_bytes = lp::prefix(n_refs, toff.data(), [&](uint32_t i) { return lp::table_bytes(h_len[i], counts[i]); });
    CHK(arena_alloc(c, tab_bytes, &tbase));
    HIPCHK(c, hipMemsetAsync(tbase, 0xFF, tab_bytes, c->stream));
    // key filters (two per reference, sized by its length: dev_common.h; zeroed; the insert kernel sets the bits)
    const uint64_t bloom_bytes = lp::prefix(n_refs, boff.data(), [&](uint32_t i) { return lp::filter_bytes(h_len[i]); });
    CHK(arena_alloc(c, bloom_bytes, &bbase));
    HIPCHK(c, hipMemsetAsync(bbase, 0, bloom_bytes, c->stream));
    // references that hold a symbol outside ACGT: escape index + one byte per symbol for the blocks that need it
    std::vector<EscJob> ejobs;
    for (uint32_t i = 0; i < n_refs; ++i) {
        jobs[i].ht_mask = (uint32_t)(lp::ht_size(counts[i]) - 1);
        jobs[i].table = tbase + toff[i];
        jobs[i].bloom = (unsigned long long *)(bbase + boff[i]);
        if (flags[i]) {
            const uint32_t nb = lp::esc_blocks(h_len[i]);
            uint8_t *eb = nullptr;
            CHK(arena_alloc(c, lp::esc_alloc_bytes(nb), &eb));
            jobs[i].esc_index = (int32_t *)eb;
            jobs[i].esc_bytes = eb + lp::esc_bytes_at(nb);
            lp::push_esc_jobs(ejobs, jobs[i].src, jobs[i].esc_index, jobs[i].esc_bytes);
        }
    }
    if (!ejobs.empty()) {
        CHK(ensure(c, c->d_esc_jobs, ejobs.size() * sizeof(EscJob)));
        CHK(upload(c, c->d_esc_jobs.p, ejobs.data(), ejobs.size() * sizeof(EscJob), c->stream));
        KTimer t(c, AGC_HIP_K_REFSTORE);
        hipLaunchKernelGGL(ref_esc_kernel, dim3((uint32_t)ejobs.size()), dim3(256), 0, c->stream, (const EscJob *)c->d_esc_jobs.p);
    }
    CHK(upload(c, c->d_jobs.p, jobs.data(), (size_t)n_refs * sizeof(IdxBuild), c->stream));
    {
        KTimer t(c, AGC_HIP_K_INDEX);
        hipLaunchKernelGGL(idx_insert_kernel, dim3(n_refs * split), dim3(256), 0, c->stream, (const IdxBuild *)c->d_jobs.p, split);
    }
    HIPCHK(c, hipGetLastError());
    // (whatever parses against these tables is ordered behind the insert -- the steps' stream itself, or a lane through the `ready`
    // event its begin records there -- so this wait is not needed for them; without it the step measured the same, twice: round 6)
    HIPCHK(c, hipStreamSynchronize(c->stream));

    if (c->refs.size() <= max_gid)
        c->refs.resize((size_t)max_gid + 1, RefDesc{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0});
    for (uint32_t i = 0; i < n_refs; ++i) {
        RefDesc &r = c->refs[h_gid[i]];
        r.words = jobs[i].words;
        r.esc_index = jobs[i].esc_index;
        r.esc_bytes = jobs[i].esc_bytes;
        r.table = jobs[i].table;
        r.bloom = jobs[i].bloom;
        r.ref_size = h_len[i];
        r.ht_mask = jobs[i].ht_mask;
        r.key_len = key_len;
        r.min_match_len = min_match_len;
        r.is_short = jobs[i].is_short;
        r.valid = 1;
    }
    const lp::DirtyRange dr = lp::widen_dirty(c->refs_dirty, {c->refs_dirty_lo, c->refs_dirty_hi}, c->refs_on_dev, *std::min_element(h_gid, h_gid + n_refs), max_gid);
    c->refs_dirty_lo = dr.lo, c->refs_dirty_hi = dr.hi;
    c->refs_dirty = true;
    return AGC_HIP_OK;
}

extern "C" {

int agc_hip_ref_register_batch_packed(agc_hip_ctx *c, uint32_t n_refs, const uint32_t *h_gid, const agc_hip_packed *pk, const uint64_t *h_off,
                                      const uint32_t *h_len, const uint8_t *h_rc, uint32_t min_match_len)
{
    if (!c || (n_refs && (!h_gid || !h_off || !h_len || !pk || !pk->d_words)))
        return AGC_HIP_EINVAL;
    if (!n_refs)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const PackedSrc src = src_of(pk);
    if (!slices_inside(src, n_refs, h_off, h_len))
        return AGC_HIP_EINVAL;
    return ref_register_impl(c, n_refs, h_gid, src, h_off, h_len, h_rc, min_match_len);
}

int agc_hip_ref_register_batch_dev(agc_hip_ctx *c, uint32_t n_refs, const uint32_t *h_gid, const uint8_t *d_base,
                                   const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc, uint32_t min_match_len)
{
    if (!c || (n_refs && (!h_gid || !h_off || !h_len || !d_base)))
        return AGC_HIP_EINVAL;
    if (!n_refs)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n_refs, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return ref_register_impl(c, n_refs, h_gid, src, off2, h_len, h_rc, min_match_len);
    });
}

int agc_hip_ref_register(agc_hip_ctx *c, uint32_t gid, const uint8_t *h_ref, uint32_t n, uint32_t min_match_len)
{
    if (!c || (n && !h_ref))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure(c, c->d_in, (size_t)n + 64));
    if (n)
        HIPCHK(c, hipMemcpyAsync(c->d_in.p, h_ref, n, hipMemcpyHostToDevice, c->stream));
    const uint64_t off = 0;
    const uint8_t rc = 0;
    return agc_hip_ref_register_batch_dev(c, 1, &gid, (const uint8_t *)c->d_in.p, &off, &n, &rc, min_match_len);
}

int agc_hip_ref_get(agc_hip_ctx *c, uint32_t gid, uint8_t *h_ref, uint32_t cap, uint32_t *h_n)
{
    if (!c || !h_n)
        return AGC_HIP_EINVAL;
    if (gid >= c->refs.size() || !c->refs[gid].valid)
        return AGC_HIP_ENOREF;
    HIPCHK(c, hipSetDevice(c->device));
    const RefDesc &r = c->refs[gid];
    *h_n = r.ref_size;
    if (cap < r.ref_size)
        return AGC_HIP_ECAP;
    if (r.ref_size) { // the stored 2-bit form back as one byte per symbol
        const SliceBufs B = slice_bufs(c);
        const PackedSrc stored = {r.words, r.esc_index, r.esc_bytes, r.ref_size};
        const uint64_t off = 0, out_off[2] = {0, r.ref_size};
        CHK(put_view_jobs(c, B, c->stream, 1, stored, &off, &r.ref_size, nullptr, out_off));
        CHK(queue_expand(c, B, c->stream, 1, h_ref, r.ref_size, -1));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return AGC_HIP_OK;
}

int agc_hip_ref_index_get(agc_hip_ctx *c, uint32_t gid, uint32_t *h_table, uint64_t cap, uint64_t *h_ht_size, int *h_is16)
{
    if (!c || !h_ht_size || !h_is16)
        return AGC_HIP_EINVAL;
    if (gid >= c->refs.size() || !c->refs[gid].valid)
        return AGC_HIP_ENOREF;
    HIPCHK(c, hipSetDevice(c->device));
    const RefDesc &r = c->refs[gid];
    const uint64_t hs = (uint64_t)r.ht_mask + 1;
    *h_ht_size = hs;
    *h_is16 = r.is_short;
    if (cap < hs)
        return AGC_HIP_ECAP;
    HIPCHK(c, hipStreamSynchronize(c->stream)); // (the insert of the registration may still be running)
    if (r.is_short) {
        std::vector<uint32_t> t(hs);
        HIPCHK(c, hipMemcpy(t.data(), r.table, hs * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < hs; ++i)
            h_table[i] = t[i] == 0xFFFFFFFFu ? 0xFFFFu : (t[i] >> 16);
    } else {
        std::vector<uint64_t> t(hs);
        HIPCHK(c, hipMemcpy(t.data(), r.table, hs * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < hs; ++i)
            h_table[i] = t[i] == ~0ULL ? 0xFFFFFFFFu : (uint32_t)(t[i] >> 32);
    }
    return AGC_HIP_OK;
}

// ---------------------------------------------------------------------------
// parse batches
// ---------------------------------------------------------------------------
} // extern "C"

namespace {

using LzLane = agc_hip_ctx::LzLane;

struct Batch {
    std::vector<SegDesc> segs; // processing order (longest first); SegDesc.idx = original index
    uint64_t out_total = 0;    // scratch units (bytes or cost_t)
    uint64_t text_total = 0;   // symbols of all texts
};

// Builds the descriptors of a parse on lane L: every text is a view into the packed buffer (either orientation -- nothing is copied or
// staged).  (An encode lane: encode only -- no filter bitmaps.)
int prepare_batch(agc_hip_ctx *c, LzLane &L, int mode, uint32_t n, const uint32_t *h_gid, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len,
                  const uint8_t *h_rc, const uint8_t *h_prefix, Batch &b)
{
    Laps LAP("prepare_batch", n);
    for (uint32_t i = 0; i < n; ++i)
        if (h_gid[i] >= c->refs.size() || !c->refs[h_gid[i]].valid) {
            c->err = "group " + std::to_string(h_gid[i]) + " has no registered reference";
            return AGC_HIP_ENOREF;
        }
    if (!slices_inside(src, n, h_off, h_len)) {
        c->err = "a sequence runs past the end of its buffer";
        return AGC_HIP_EINVAL;
    }
    LAP("valid");
    CHK(upload_refs(c));
    const std::vector<uint32_t> order = lp::longest_first(n, h_len);
    LAP("sort");
    b.text_total = std::accumulate(h_len, h_len + n, (uint64_t)0);
    if (Laps::enabled() && mode == MODE_COSTVEC && n)
        fprintf(stderr, "    cost-vector batch: %u parses, %.1f Mb of text, longest %u %u %u %u, median %u\n", n, b.text_total / 1e6, h_len[order[0]],
                h_len[order[n > 1 ? 1 : 0]], h_len[order[n > 2 ? 2 : 0]], h_len[order[n > 3 ? 3 : 0]], h_len[order[n / 2]]);
    std::vector<uint64_t> ooff(n), moff(n, 0);
    b.out_total = lp::out_offsets(mode, n, h_len, ooff.data());
    // estimate / cost vector: one "may match" bit per text position (key_filter_kernel) lets the parse skip literal runs
    if (mode != MODE_ENCODE)
        CHK(ensure(c, c->d_maybe, lp::filter_word_offsets(n, h_len, moff.data()) * 8 + 64));
    std::vector<FilterJob> fjobs;
    b.segs.resize(n);
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t i = order[p];
        SegDesc &s = b.segs[p];
        s = SegDesc();
        s.text = {src.words, src.esc_index, src.esc_bytes, h_off[i], h_len[i], (h_rc && h_rc[i]) ? 1u : 0u};
        s.out_off = ooff[i];
        s.ref_slot = h_gid[i];
        s.flags = (h_prefix && h_prefix[i]) ? 1u : 0u;
        s.idx = i;
        const RefDesc &rd = c->refs[h_gid[i]];
        if (mode != MODE_ENCODE && rd.bloom && h_len[i] > 4 * WAVE) { // (short texts: not worth a block)
            unsigned long long *maybe = (unsigned long long *)c->d_maybe.p + moff[i];
            s.maybe = maybe;
            lp::push_filter_jobs(fjobs, s.text, rd.bloom, maybe, rd.key_len, rd.ref_size);
        }
    }
    if (!fjobs.empty()) {
        CHK(ensure(c, c->d_fjobs, fjobs.size() * sizeof(FilterJob)));
        CHK(upload(c, c->d_fjobs.p, fjobs.data(), fjobs.size() * sizeof(FilterJob), L.s));
        {
            KTimer t(c, AGC_HIP_K_FILTER);
            hipLaunchKernelGGL(key_filter_kernel, dim3((uint32_t)fjobs.size()), dim3(FILTER_THREADS), 0, L.s, (const FilterJob *)c->d_fjobs.p);
        }
        HIPCHK(c, hipGetLastError());
    }
    LAP("descriptors");
    CHK(ensure(c, L.d_segs, (size_t)n * sizeof(SegDesc), L.s));
    CHK(upload(c, L.d_segs.p, b.segs.data(), (size_t)n * sizeof(SegDesc), L.s));
    CHK(ensure(c, L.d_resv, (size_t)n * 4, L.s));
    CHK(ensure(c, L.d_resp, (size_t)n * 4, L.s));
    LAP("upload");
    return AGC_HIP_OK;
}

// The chunk list of a launch in chunks of chunk_len, its logs and (encode) its per-chunk output in the lane's chunk buffers -> pl;
// pl.n_jobs stays 0 when there would be too many chunks (lz_plan.h): the launch then parses whole texts
int place_chunks(agc_hip_ctx *c, LzLane &L, const Batch &b, uint32_t chunk_len, bool encode, ChunkPlan &pl)
{
    std::vector<ChunkJob> jobs;
    std::vector<uint32_t> seg0;
    if (!lp::plan_chunks(b.segs.data(), (uint32_t)b.segs.size(), chunk_len, encode, jobs, seg0, pl))
        return AGC_HIP_OK;
    LzLane::Chunks &cb = L.chunks;
    CHK(ensure(c, cb.d_jobs, jobs.size() * sizeof(ChunkJob), L.s));
    CHK(ensure(c, cb.d_seg0, seg0.size() * 4, L.s));
    if (cb.logs_ahead.valid()) { // (allocated ahead by a helper thread: see LzLane::Chunks)
        DevBuf ahead = cb.logs_ahead.get();
        if (ahead.p && ahead.cap > cb.d_logs.cap) { // (otherwise it goes back as `ahead` goes)
            if (cb.d_logs.p)
                HIPCHK(c, hipStreamSynchronize(L.s));
            cb.d_logs = std::move(ahead);
        }
    }
    CHK(ensure(c, cb.d_logs, jobs.size() * (size_t)pl.cap * sizeof(ChunkState), L.s));
    CHK(ensure(c, cb.d_logn, jobs.size() * 4, L.s));
    if (encode)
        CHK(ensure(c, cb.d_out, jobs.size() * (size_t)pl.chunk_stride + 64, L.s));
    CHK(upload(c, cb.d_jobs.p, jobs.data(), jobs.size() * sizeof(ChunkJob), L.s)); // (a window of diverged genomes has a few 10 k chunks)
    CHK(upload(c, cb.d_seg0.p, seg0.data(), seg0.size() * 4, L.s));
    pl.jobs = (const ChunkJob *)cb.d_jobs.p;
    pl.seg_chunk0 = (const uint32_t *)cb.d_seg0.p;
    pl.logs = (ChunkState *)cb.d_logs.p;
    pl.log_n = (uint32_t *)cb.d_logn.p;
    pl.chunk_out = (uint8_t *)cb.d_out.p;
    return AGC_HIP_OK;
}

// a big batch that was not worth chunks: the next one may be -- a helper thread has the logs ready (once per lane)
void ask_logs_ahead(agc_hip_ctx *c, LzLane::Chunks &cb, bool encode, uint32_t n, uint64_t text_total)
{
    const size_t want = cb.logs_asked ? 0 : (size_t)lp::logs_ahead_bytes(encode, n, text_total, cb.d_logs.cap, sizeof(ChunkState));
    if (!want)
        return;
    cb.logs_asked = true;
    cb.logs_ahead = std::async(std::launch::async, [want, dev = c->device] {
        DevBuf d;
        if (hipSetDevice(dev) == hipSuccess && hipMalloc(&d.p, want) == hipSuccess)
            d.cap = want;
        else
            d.p = nullptr;
        return d;
    });
}

// AGC_HIP_CHUNK_LOG (a measuring aid): every parse launch the host has descriptors of on stderr, timed by events of its own
struct ChunkLog {
    Event ev[3];
    int marks = 0;
    bool on;
    explicit ChunkLog(bool has_batch)
    {
        static const bool asked = getenv("AGC_HIP_CHUNK_LOG") != nullptr;
        on = asked && has_batch;
        for (int i = 0; on && i < 3; ++i)
            on = hipEventCreate(&ev[i].h) == hipSuccess;
    }
    void mark(hipStream_t st)
    {
        if (on)
            (void)hipEventRecord(ev[marks++], st);
    }
    // pl.n_jobs == 0: a whole-text launch (two marks); otherwise the chunk kernel and the hop kernel (three)
    void print(const agc_hip_ctx *c, int mode, const Batch &b, const ChunkPlan &pl, const uint32_t *d_resp)
    {
        if (!on)
            return;
        const uint32_t n = (uint32_t)b.segs.size(), longest = n ? b.segs[0].text.len : 0u;
        (void)hipEventSynchronize(ev[marks - 1]);
        float t1 = 0, t2 = 0;
        (void)hipEventElapsedTime(&t1, ev[0], ev[1]);
        if (!pl.n_jobs) {
            fprintf(stderr, "    whole-text launch mode %d: %u texts, %.2f Mb, longest %u: %.3f ms\n", mode, n, b.text_total / 1e6, longest, t1);
            return;
        }
        (void)hipEventElapsedTime(&t2, ev[1], ev[2]);
        fprintf(stderr, "    chunked launch mode %d: %u texts, %.2f Mb, longest %u, %u chunks of %u: chunk kernel %.3f ms, hop kernel %.3f ms\n", mode, n, b.text_total / 1e6,
                longest, pl.n_jobs, pl.chunk_len, t1, t2);
        if (mode == MODE_ESTIMATE) // (elsewhere the hop parser left its counters where an estimate's peak goes)
            return;
        std::vector<uint32_t> dbg(n);
        (void)hipMemcpy(dbg.data(), d_resp, (size_t)n * 4, hipMemcpyDeviceToHost);
        uint32_t shown = 0;
        for (uint32_t i = 0; i < n && shown < 16; ++i) {
            const SegDesc &sd = b.segs[i];
            const uint32_t nch = (sd.text.len + pl.chunk_len - 1) / pl.chunk_len, hops = dbg[sd.idx] >> 16;
            if (i >= 4 && (hops * 2 >= nch || nch < 4))
                continue; // (the first few, and every text the hop wavefront had to parse mostly by itself)
            ++shown;
            fprintf(stderr, "        text %u: %u symbols (rc %u), %u chunks, ref %u (gid %u): %u chunks taken over, %u matches parsed by the hop wavefront\n", i, sd.text.len,
                    sd.text.rc, nch, c->refs[sd.ref_slot].ref_size, sd.ref_slot, hops, dbg[sd.idx] & 0xFFFFu);
        }
    }
};

// The parse of the n descriptors in L.d_segs, on the lane's stream.  n_dev: their number was made on the device (n is an upper bound);
// b: the batch the host made them from.  A launch with few, long texts is a handful of dependent chains on an empty GPU: such batches
// are parsed in chunks (lz_kernels.hip: ChunkCtl) -- a wavefront per 4096-symbol chunk, then a wavefront per text that joins them.
// AGC_HIP_LZ_CHUNK=<symbols> forces a chunk length for every launch the host has descriptors of (the tests run the whole LZ suite
// that way), 0 switches the path off.
template <int MODE>
int launch_parse(agc_hip_ctx *c, LzLane &L, uint32_t n, uint8_t *out_bytes, uint32_t *out_u32, const uint32_t *n_dev = nullptr, const Batch *b = nullptr)
{
    static const int forced = getenv("AGC_HIP_LZ_CHUNK") ? atoi(getenv("AGC_HIP_LZ_CHUNK")) : -1;
    const bool has_batch = b && !n_dev && b->segs.size() == n;
    const RefDesc *d_refs = (const RefDesc *)c->d_refs.p;
    const SegDesc *d_segs = (const SegDesc *)L.d_segs.p;
    uint32_t *d_resv = (uint32_t *)L.d_resv.p, *d_resp = (uint32_t *)L.d_resp.p;
    ChunkPlan pl{};
    if (const uint32_t chunk_len = lp::chunk_len_for(forced, has_batch, n, has_batch && n ? b->segs[0].text.len : 0u, has_batch ? b->text_total : 0))
        CHK(place_chunks(c, L, *b, chunk_len, MODE == MODE_ENCODE, pl));
    if (!pl.n_jobs && has_batch && forced != 0)
        ask_logs_ahead(c, L.chunks, MODE == MODE_ENCODE, n, b->text_total);
    ChunkLog log(has_batch);
    {
        // (KTimer records on the steps' stream: an encode lane times its launch with its own events)
        KTimer t(c, L.s != c->stream ? -1 : MODE == MODE_ENCODE ? AGC_HIP_K_ENCODE : MODE == MODE_ESTIMATE ? AGC_HIP_K_ESTIMATE : AGC_HIP_K_COSTVEC);
        const uint32_t grid = (n + 3) / 4; // one wave per segment, 4 waves per block
        log.mark(L.s);
        if (pl.n_jobs) {
            hipLaunchKernelGGL(lz_chunk_kernel<MODE>, dim3((pl.n_jobs + 3) / 4), dim3(256), 0, L.s, d_refs, d_segs, pl, out_u32);
            log.mark(L.s);
            hipLaunchKernelGGL(lz_hop_kernel<MODE>, dim3(grid), dim3(256), 0, L.s, d_refs, d_segs, n, pl, out_bytes, out_u32, d_resv, d_resp);
        } else
            hipLaunchKernelGGL(lz_parse_kernel<MODE>, dim3(grid), dim3(256), 0, L.s, d_refs, d_segs, n, out_bytes, out_u32, d_resv, d_resp, n_dev);
        log.mark(L.s);
    }
    HIPCHK(c, hipGetLastError());
    if (has_batch)
        log.print(c, MODE, *b, pl, d_resp);
    return AGC_HIP_OK;
}

// The deltas of a batch parsed on lane L, back to back on the host: offsets from their lengths, one gather, one copy, waited for on
// the lane's stream.  direct: a pinned h_enc (agc_hip_host_alloc) is written by the gather itself, over the link -- no second
// buffer, no copy engine; anything else, and every result of the one-call encode, gets the deltas compacted in HBM and copied.
int collect_deltas(agc_hip_ctx *c, LzLane &L, uint32_t n, const uint32_t *lens, bool direct, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off, Laps LAP)
{
    for (uint32_t i = 0; i < n; ++i)
        h_enc_off[i + 1] = h_enc_off[i] + lens[i];
    const uint64_t tot = h_enc_off[n];
    if (tot > enc_cap)
        return AGC_HIP_ECAP;
    LAP("offsets");
    if (!tot)
        return AGC_HIP_OK;
    if (!h_enc)
        return AGC_HIP_EINVAL;
    CHK(ensure(c, L.d_dstoff, (size_t)n * 8, L.s));
    CHK(upload(c, L.d_dstoff.p, h_enc_off, (size_t)n * 8, L.s));
    void *d_host = nullptr;
    if (direct && hipHostGetDevicePointer(&d_host, h_enc, 0) != hipSuccess) {
        (void)hipGetLastError();
        d_host = nullptr;
    }
    if (!d_host)
        CHK(ensure(c, L.d_compact, tot, L.s));
    hipLaunchKernelGGL(gather_bytes_kernel, dim3(grid_for(n, 1, 8192)), dim3(256), 0, L.s, (const uint8_t *)L.d_scratch.p, (const SegDesc *)L.d_segs.p,
                       (const uint32_t *)L.d_resv.p, (const uint64_t *)L.d_dstoff.p, n, d_host ? (uint8_t *)d_host : (uint8_t *)L.d_compact.p);
    HIPCHK(c, hipGetLastError());
    if (!d_host)
        HIPCHK(c, hipMemcpyAsync(h_enc, L.d_compact.p, tot, hipMemcpyDeviceToHost, L.s));
    LAP("queued");
    HIPCHK(c, hipStreamSynchronize(L.s));
    LAP("deltas on the host");
    return AGC_HIP_OK;
}

} // namespace

static int lz_encode_impl(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len,
                          const uint8_t *h_rc, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off)
{
    LzLane &L = c->lane(0);
    Batch b;
    CHK(prepare_batch(c, L, MODE_ENCODE, n, h_gid, src, h_off, h_len, h_rc, nullptr, b));
    CHK(ensure(c, L.d_scratch, b.out_total + 64));
    CHK(launch_parse<MODE_ENCODE>(c, L, n, (uint8_t *)L.d_scratch.p, nullptr, nullptr, &b));
    std::vector<uint32_t> lens(n);
    HIPCHK(c, hipMemcpyAsync(lens.data(), L.d_resv.p, (size_t)n * 4, hipMemcpyDeviceToHost, L.s));
    HIPCHK(c, hipStreamSynchronize(L.s));
    return collect_deltas(c, L, n, lens.data(), false, h_enc, enc_cap, h_enc_off, Laps("", 0));
}

// The encode in two halves (include/agc_hip.h): begin queues the parse and the copy of the delta lengths on an encode lane's
// stream and returns; end waits, lays the deltas out back to back and brings them over.  Between the two the caller may use every
// other entry point (they run on the first stream with their own scratch).
static int lz_encode_begin_impl(agc_hip_ctx *c, LzLane &L, uint32_t n, const uint32_t *h_gid, const PackedSrc &src, const uint64_t *h_off,
                                const uint32_t *h_len, const uint8_t *h_rc)
{
    Batch b;
    CHK(prepare_batch(c, L, MODE_ENCODE, n, h_gid, src, h_off, h_len, h_rc, nullptr, b));
    CHK(ensure(c, L.d_scratch, b.out_total + 64, L.s));
    CHK(ensure_pinned(c, L.h_lens, (size_t)n * 4, ((size_t)n + n / 4 + 1024) * 4));
    L.timed = c->timing;
    if (L.timed)
        (void)hipEventRecord(L.e0, L.s);
    CHK(launch_parse<MODE_ENCODE>(c, L, n, (uint8_t *)L.d_scratch.p, nullptr, nullptr, &b));
    if (L.timed)
        (void)hipEventRecord(L.e1, L.s);
    HIPCHK(c, hipEventRecord(L.done, L.s));
    L.done_valid = true;
    HIPCHK(c, hipMemcpyAsync(L.h_lens.p, L.d_resv.p, (size_t)n * 4, hipMemcpyDeviceToHost, L.s));
    L.pending = true;
    return AGC_HIP_OK;
}

// common start of the two begin entry points: an abandoned encode is dropped, the first stream's work so far comes first
static int lz_encode_begin_enter(agc_hip_ctx *c, LzLane &L, uint32_t n)
{
    if (L.pending) { // (an abandoned encode: a caller that failed between the two halves) -- dropped
        HIPCHK(c, hipStreamSynchronize(L.s));
        L.pending = false;
    }
    L.n = n;
    if (!n) {
        L.pending = true;
        return 1; // nothing to launch
    }
    HIPCHK(c, hipSetDevice(c->device));
    // the group descriptors of references registered a moment ago travel on the first stream: their copy has to be queued BEFORE the
    // event the lane waits for, or the lane's parse could read a table the copy has not reached yet (prepare_batch would queue it
    // behind the event)
    CHK(upload_refs(c));
    // everything queued on the first stream so far (index builds, a sample being packed) comes first
    HIPCHK(c, hipEventRecord(L.ready, c->stream));
    HIPCHK(c, hipStreamWaitEvent(L.s, L.ready, 0));
    return AGC_HIP_OK;
}

extern "C" {

int agc_hip_lz_encode_batch_packed(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const agc_hip_packed *pk, const uint64_t *h_off,
                                   const uint32_t *h_len, const uint8_t *h_rc, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off)
{
    if (!c || !h_enc_off || (n && (!h_gid || !h_off || !h_len || !pk || !pk->d_words)))
        return AGC_HIP_EINVAL;
    h_enc_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return lz_encode_impl(c, n, h_gid, src_of(pk), h_off, h_len, h_rc, h_enc, enc_cap, h_enc_off);
}

int agc_hip_lz_encode_batch_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *d_base, const uint64_t *h_off,
                                const uint32_t *h_len, const uint8_t *h_rc, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off)
{
    if (!c || !h_enc_off || (n && (!h_gid || !h_off || !h_len || !d_base)))
        return AGC_HIP_EINVAL;
    h_enc_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return lz_encode_impl(c, n, h_gid, src, off2, h_len, h_rc, h_enc, enc_cap, h_enc_off);
    });
}

int agc_hip_lz_encode_begin_packed_on(agc_hip_ctx *c, uint32_t lane, uint32_t n, const uint32_t *h_gid, const agc_hip_packed *pk, const uint64_t *h_off,
                                      const uint32_t *h_len, const uint8_t *h_rc)
{
    if (!c || lane >= AGC_HIP_ENCODE_LANES || (n && (!h_gid || !h_off || !h_len || !pk || !pk->d_words)))
        return AGC_HIP_EINVAL;
    LzLane &L = c->lane((int)lane + 1);
    const int e = lz_encode_begin_enter(c, L, n);
    if (e)
        return e > 0 ? AGC_HIP_OK : e;
    return lz_encode_begin_impl(c, L, n, h_gid, src_of(pk), h_off, h_len, h_rc);
}

int agc_hip_lz_encode_begin_packed(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const agc_hip_packed *pk, const uint64_t *h_off,
                                   const uint32_t *h_len, const uint8_t *h_rc)
{
    return agc_hip_lz_encode_begin_packed_on(c, 0, n, h_gid, pk, h_off, h_len, h_rc);
}

int agc_hip_lz_encode_begin_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *d_base, const uint64_t *h_off,
                                const uint32_t *h_len, const uint8_t *h_rc)
{
    if (!c || (n && (!h_gid || !h_off || !h_len || !d_base)))
        return AGC_HIP_EINVAL;
    LzLane &L = c->lane(1); // (the lane's own packed copy: it lives until end)
    const int e = lz_encode_begin_enter(c, L, n);
    if (e)
        return e > 0 ? AGC_HIP_OK : e;
    return with_packed_bytes(c, d_base, n, h_off, h_len, L.pk, L.s, [&](const PackedSrc &src, const uint64_t *off2) {
        return lz_encode_begin_impl(c, L, n, h_gid, src, off2, h_len, h_rc);
    });
}

int agc_hip_lz_encode_pending(agc_hip_ctx *c, uint32_t *h_n) { return agc_hip_lz_encode_pending_on(c, 0, h_n); }

int agc_hip_lz_encode_pending_on(agc_hip_ctx *c, uint32_t lane, uint32_t *h_n)
{
    if (!c || !h_n || lane >= AGC_HIP_ENCODE_LANES)
        return AGC_HIP_EINVAL;
    LzLane &L = c->lane((int)lane + 1);
    *h_n = 0;
    if (!L.pending)
        return AGC_HIP_OK;
    if (L.n_pinned) { // (launched from descriptors made on the device: the count was copied behind the parse)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(L.s));
        L.n = *L.n_pinned;
        L.n_pinned = nullptr;
    }
    *h_n = L.n;
    return AGC_HIP_OK;
}

int agc_hip_lz_encode_drop_on(agc_hip_ctx *c, uint32_t lane)
{
    if (!c || lane >= AGC_HIP_ENCODE_LANES)
        return AGC_HIP_EINVAL;
    LzLane &L = c->lane((int)lane + 1);
    if (L.pending) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(L.s));
    }
    L.pending = false;
    L.n_pinned = nullptr;
    L.timed = false;
    L.n = 0;
    return AGC_HIP_OK;
}

int agc_hip_lz_encode_end(agc_hip_ctx *c, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off)
{
    return agc_hip_lz_encode_end_on(c, 0, h_enc, enc_cap, h_enc_off);
}

int agc_hip_lz_encode_end_on(agc_hip_ctx *c, uint32_t lane, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off)
{
    if (!c || !h_enc_off || lane >= AGC_HIP_ENCODE_LANES)
        return AGC_HIP_EINVAL;
    LzLane &L = c->lane((int)lane + 1);
    if (!L.pending) {
        c->err = "lz_encode_end: no encode in flight";
        return AGC_HIP_EINVAL;
    }
    h_enc_off[0] = 0;
    if (L.n_pinned) { // (launched by agc_hip_segments_encode_known: the count was copied behind the parse)
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(L.s));
        L.n = *L.n_pinned;
        L.n_pinned = nullptr;
    }
    const uint32_t n = L.n;
    if (!n) {
        L.pending = false;
        return AGC_HIP_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(L.s));
    if (L.timed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, L.e0, L.e1) == hipSuccess) {
            c->ms[AGC_HIP_K_ENCODE] += ms;
            c->launches[AGC_HIP_K_ENCODE] += 1;
        }
        L.timed = false; // (a second call after AGC_HIP_ECAP must not count the launch twice)
    }
#ifdef AGC_PHASES
    {
        unsigned long long acc[8], cnt[8];
        (void)hipMemcpyFromSymbol(acc, HIP_SYMBOL(agc::g_phase_acc), sizeof acc);
        (void)hipMemcpyFromSymbol(cnt, HIP_SYMBOL(agc::g_phase_cnt), sizeof cnt);
        static const char *nm[5] = {"emit", "window", "probe", "literals", "verify"};
        unsigned long long tot = 0;
        for (int k = 0; k < 5; ++k)
            tot += acc[k];
        for (int k = 0; k < 5; ++k)
            fprintf(stderr, "phase %-8s %6.2f %%  %.0f cycles per visit (%llu visits)\n", nm[k], 100.0 * acc[k] / (tot ? tot : 1), cnt[k] ? (double)acc[k] / cnt[k] : 0.0, cnt[k]);
        fprintf(stderr, "phase total %.0f cycles per wave (%u waves)\n", (double)tot / n, n);
        (void)hipMemset((void *)nullptr, 0, 0);
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(agc::g_phase_acc), z, sizeof z);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(agc::g_phase_cnt), z, sizeof z);
    }
#endif
    // (AGC_HIP_ECAP: still in flight -- call again with a larger buffer)
    CHK(collect_deltas(c, L, n, L.h_lens.as<uint32_t>(), true, h_enc, enc_cap, h_enc_off, Laps("lz_encode_end", n)));
    L.pending = false;
    return AGC_HIP_OK;
}

// pinned host memory for the buffers results are copied into (a copy into pageable memory goes through a bounce buffer)
int agc_hip_host_alloc(agc_hip_ctx *c, uint64_t bytes, void **out)
{
    if (!c || !out)
        return AGC_HIP_EINVAL;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    void *p = nullptr;
    HIPCHK(c, hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault));
    {
        std::lock_guard<std::mutex> lk(c->host_alloc_mtx);
        c->host_allocs.emplace_back(p, (size_t)bytes);
    }
    *out = p;
    return AGC_HIP_OK;
}

int agc_hip_host_free(agc_hip_ctx *c, void *p)
{
    if (!c)
        return AGC_HIP_EINVAL;
    if (!p)
        return AGC_HIP_OK;
    PinnedBuf mine;
    {
        std::lock_guard<std::mutex> lk(c->host_alloc_mtx);
        auto it = std::find_if(c->host_allocs.begin(), c->host_allocs.end(), [p](const PinnedBuf &b) { return b.p == p; });
        if (it == c->host_allocs.end())
            return AGC_HIP_EINVAL;
        mine = std::move(*it);
        c->host_allocs.erase(it);
    }
    if (mine.release() != hipSuccess) // (no write to the shared error string: this may be the thread that collects an encode)
        return AGC_HIP_ENODEV;
    return AGC_HIP_OK;
}

} // extern "C"

static int lz_estimate_impl(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len,
                            const uint8_t *h_rc, uint32_t *h_cost, uint32_t *h_peak)
{
    LzLane &L = c->lane(0);
    Batch b;
    CHK(prepare_batch(c, L, MODE_ESTIMATE, n, h_gid, src, h_off, h_len, h_rc, nullptr, b));
    CHK(launch_parse<MODE_ESTIMATE>(c, L, n, nullptr, nullptr, nullptr, &b));
    HIPCHK(c, hipMemcpyAsync(h_cost, L.d_resv.p, (size_t)n * 4, hipMemcpyDeviceToHost, L.s));
    if (h_peak)
        HIPCHK(c, hipMemcpyAsync(h_peak, L.d_resp.p, (size_t)n * 4, hipMemcpyDeviceToHost, L.s));
    HIPCHK(c, hipStreamSynchronize(L.s));
    return AGC_HIP_OK;
}

static int lz_cost_vector_impl(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len,
                               const uint8_t *h_rc, const uint8_t *h_prefix_costs, uint32_t *h_costs)
{
    LzLane &L = c->lane(0);
    Batch b;
    CHK(prepare_batch(c, L, MODE_COSTVEC, n, h_gid, src, h_off, h_len, h_rc, h_prefix_costs, b));
    CHK(ensure(c, L.d_scratch, b.out_total + 64)); // (one byte per position on the device: lz_kernels.hip, cost_t)
    CHK(launch_parse<MODE_COSTVEC>(c, L, n, nullptr, (uint32_t *)L.d_scratch.p, nullptr, &b));
    std::vector<uint8_t> tmp(b.out_total);
    if (b.out_total)
        HIPCHK(c, hipMemcpyAsync(tmp.data(), L.d_scratch.p, b.out_total, hipMemcpyDeviceToHost, L.s));
    HIPCHK(c, hipStreamSynchronize(L.s));
    for (uint64_t i = 0; i < b.out_total; ++i)
        h_costs[i] = tmp[i];
    return AGC_HIP_OK;
}

static int lz_split_point_impl(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid1, const uint32_t *h_gid2, const PackedSrc &src, const uint64_t *h_off,
                               const uint32_t *h_len, const uint8_t *h_rc1, const uint8_t *h_prefix1, const uint8_t *h_rc2, const uint8_t *h_prefix2,
                               uint32_t *h_best_pos, uint32_t *h_best_sum)
{
    // 2n cost-vector parses: job 2s = (gid1, rc1, prefix1), job 2s+1 = (gid2, rc2, prefix2)
    const uint32_t m = 2 * n;
    std::vector<uint32_t> gid(m), len(m);
    std::vector<uint64_t> off(m);
    std::vector<uint8_t> rc(m), pf(m);
    for (uint32_t s = 0; s < n; ++s) {
        gid[2 * s] = h_gid1[s];
        gid[2 * s + 1] = h_gid2[s];
        off[2 * s] = off[2 * s + 1] = h_off[s];
        len[2 * s] = len[2 * s + 1] = h_len[s];
        rc[2 * s] = h_rc1[s];
        rc[2 * s + 1] = h_rc2[s];
        pf[2 * s] = h_prefix1[s];
        pf[2 * s + 1] = h_prefix2[s];
    }
    LzLane &L = c->lane(0); // (the split-point kernel reads the cost vectors out of the parse's scratch and answers into d_dstoff)
    Batch b;
    CHK(prepare_batch(c, L, MODE_COSTVEC, m, gid.data(), src, off.data(), len.data(), rc.data(), pf.data(), b));
    CHK(ensure(c, L.d_scratch, b.out_total + 64));
    CHK(launch_parse<MODE_COSTVEC>(c, L, m, nullptr, (uint32_t *)L.d_scratch.p, nullptr, &b));
    std::vector<SplitJob> jobs(n);
    uint64_t o = 0;
    for (uint32_t s = 0; s < n; ++s) {
        jobs[s].off1 = o;
        jobs[s].off2 = o + h_len[s];
        jobs[s].n = h_len[s];
        jobs[s].rev1 = h_prefix1[s] ? 0u : 1u;
        jobs[s].rev2 = h_prefix2[s] ? 1u : 0u;
        jobs[s].pad = 0;
        o += 2ULL * h_len[s];
    }
    CHK(ensure(c, c->d_jobs, (size_t)n * sizeof(SplitJob)));
    CHK(ensure(c, L.d_dstoff, (size_t)n * 8));
    CHK(upload(c, c->d_jobs.p, jobs.data(), (size_t)n * sizeof(SplitJob), c->stream));
    uint32_t *d_pos = (uint32_t *)L.d_dstoff.p, *d_sum = d_pos + n;
    {
        KTimer t(c, AGC_HIP_K_COSTVEC);
        hipLaunchKernelGGL(split_point_kernel, dim3(n), dim3(256), 0, c->stream, (const SplitJob *)c->d_jobs.p,
                           (const cost_t *)L.d_scratch.p, d_pos, d_sum);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_best_pos, d_pos, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_best_sum)
        HIPCHK(c, hipMemcpyAsync(h_best_sum, d_sum, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

static int fetch_slices_impl(agc_hip_ctx *c, uint32_t n, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc,
                             uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    for (uint32_t i = 0; i < n; ++i)
        h_out_off[i + 1] = h_out_off[i] + h_len[i];
    const uint64_t tot = h_out_off[n];
    if (tot > out_cap)
        return AGC_HIP_ECAP;
    if (!tot)
        return AGC_HIP_OK;
    if (!h_out)
        return AGC_HIP_EINVAL;
    const SliceBufs B = slice_bufs(c);
    CHK(put_view_jobs(c, B, c->stream, n, src, h_off, h_len, h_rc, h_out_off));
    CHK(queue_expand(c, B, c->stream, n, h_out, tot, AGC_HIP_K_REVCOMP));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

static int ref_lag_counts_impl(agc_hip_ctx *c, uint32_t n, const PackedSrc &src, const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc,
                               uint32_t *h_cnt, uint32_t *h_cur)
{
    const SliceBufs B = slice_bufs(c);
    CHK(put_view_jobs(c, B, c->stream, n, src, h_off, h_len, h_rc, nullptr));
    CHK(queue_lag_counts(c, B, c->stream, n, h_cnt, h_cur, AGC_HIP_K_REFSTORE));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

extern "C" {

// The new references (and raw items) of a registration in ONE submission that nobody on the steps' stream waits for: the
// repetitiveness counters of the first n_refs slices (agc_hip_ref_lag_counts_packed) and the symbols of all n slices
// (agc_hip_fetch_slices_packed), on a stream and in buffers of their own; _end waits for the slot (include/agc_hip.h).
int agc_hip_ref_store_begin_packed(agc_hip_ctx *c, uint32_t slot, uint32_t n_refs, uint32_t n, const agc_hip_packed *pk, const uint64_t *h_off, const uint32_t *h_len,
                                   const uint8_t *h_rc, uint32_t *h_cnt, uint32_t *h_cur, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    if (!c || slot >= 2 || n_refs > n || !h_out_off || (n && (!pk || !pk->d_words || !h_off || !h_len)) || (n_refs && (!h_cnt || !h_cur)))
        return AGC_HIP_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    agc_hip_ctx::RefStore &R = c->ref_store[slot];
    if (!c->ref_store_stream)
        HIPCHK(c, hipStreamCreateWithFlags(&c->ref_store_stream.h, hipStreamNonBlocking));
    if (!R.done)
        HIPCHK(c, hipEventCreateWithFlags(&R.done.h, hipEventDisableTiming));
    const hipStream_t st = c->ref_store_stream;
    if (R.pending) { // (a slot nobody collected: its copies must have landed before its buffers are written again)
        HIPCHK(c, hipEventSynchronize(R.done));
        R.pending = false;
    }
    h_out_off[0] = 0;
    for (uint32_t i = 0; i < n; ++i)
        h_out_off[i + 1] = h_out_off[i] + h_len[i];
    const uint64_t tot = h_out_off[n];
    if (tot > out_cap)
        return AGC_HIP_ECAP;
    if (!n)
        return AGC_HIP_OK;
    if (tot && !h_out)
        return AGC_HIP_EINVAL;
    const SliceBufs B = slice_bufs(R);
    CHK(put_view_jobs(c, B, st, n, src_of(pk), h_off, h_len, h_rc, h_out_off));
    if (n_refs)
        CHK(queue_lag_counts(c, B, st, n_refs, h_cnt, h_cur, -1));
    if (tot)
        CHK(queue_expand(c, B, st, n, h_out, tot, -1));
    HIPCHK(c, hipEventRecord(R.done, st));
    R.pending = true;
    return AGC_HIP_OK;
}

int agc_hip_ref_store_end(agc_hip_ctx *c, uint32_t slot)
{
    if (!c || slot >= 2)
        return AGC_HIP_EINVAL;
    agc_hip_ctx::RefStore &R = c->ref_store[slot];
    if (!R.pending)
        return AGC_HIP_OK;
    // (no hipSetDevice, no write to the shared error string: this may be the bookkeeping thread)
    if (hipEventSynchronize(R.done) != hipSuccess)
        return AGC_HIP_ENODEV;
    R.pending = false;
    return AGC_HIP_OK;
}

// ---- sequences in a 2-bit packed buffer -------------------------------------
int agc_hip_lz_estimate_batch_packed(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const agc_hip_packed *pk, const uint64_t *h_off,
                                     const uint32_t *h_len, const uint8_t *h_rc, uint32_t *h_cost, uint32_t *h_peak)
{
    if (!c || (n && (!h_gid || !h_off || !h_len || !pk || !pk->d_words || !h_cost)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return lz_estimate_impl(c, n, h_gid, src_of(pk), h_off, h_len, h_rc, h_cost, h_peak);
}

int agc_hip_lz_cost_vector_batch_packed(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const agc_hip_packed *pk, const uint64_t *h_off,
                                        const uint32_t *h_len, const uint8_t *h_rc, const uint8_t *h_prefix_costs, uint32_t *h_costs)
{
    if (!c || (n && (!h_gid || !h_off || !h_len || !pk || !pk->d_words || !h_costs)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return lz_cost_vector_impl(c, n, h_gid, src_of(pk), h_off, h_len, h_rc, h_prefix_costs, h_costs);
}

int agc_hip_lz_split_point_batch_packed(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid1, const uint32_t *h_gid2, const agc_hip_packed *pk,
                                        const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc1, const uint8_t *h_prefix1,
                                        const uint8_t *h_rc2, const uint8_t *h_prefix2, uint32_t *h_best_pos, uint32_t *h_best_sum)
{
    if (!c || (n && (!h_gid1 || !h_gid2 || !pk || !pk->d_words || !h_off || !h_len || !h_rc1 || !h_prefix1 || !h_rc2 || !h_prefix2 || !h_best_pos)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return lz_split_point_impl(c, n, h_gid1, h_gid2, src_of(pk), h_off, h_len, h_rc1, h_prefix1, h_rc2, h_prefix2, h_best_pos, h_best_sum);
}

int agc_hip_fetch_slices_packed(agc_hip_ctx *c, uint32_t n, const agc_hip_packed *pk, const uint64_t *h_off, const uint32_t *h_len,
                                const uint8_t *h_rc, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    if (!c || !h_out_off || (n && (!pk || !pk->d_words || !h_off || !h_len)))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return fetch_slices_impl(c, n, src_of(pk), h_off, h_len, h_rc, h_out, out_cap, h_out_off);
}

int agc_hip_ref_lag_counts_packed(agc_hip_ctx *c, uint32_t n, const agc_hip_packed *pk, const uint64_t *h_off, const uint32_t *h_len,
                                  const uint8_t *h_rc, uint32_t *h_cnt, uint32_t *h_cur)
{
    if (!c || (n && (!pk || !pk->d_words || !h_off || !h_len || !h_cnt || !h_cur)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return ref_lag_counts_impl(c, n, src_of(pk), h_off, h_len, h_rc, h_cnt, h_cur);
}

// ---- one byte per symbol (device): packed first -------------------------------
int agc_hip_lz_estimate_batch_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *d_base, const uint64_t *h_off,
                                  const uint32_t *h_len, const uint8_t *h_rc, uint32_t *h_cost, uint32_t *h_peak)
{
    if (!c || (n && (!h_gid || !h_off || !h_len || !d_base || !h_cost)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return lz_estimate_impl(c, n, h_gid, src, off2, h_len, h_rc, h_cost, h_peak);
    });
}

int agc_hip_lz_cost_vector_batch_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *d_base,
                                     const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc,
                                     const uint8_t *h_prefix_costs, uint32_t *h_costs)
{
    if (!c || (n && (!h_gid || !h_off || !h_len || !d_base || !h_costs)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return lz_cost_vector_impl(c, n, h_gid, src, off2, h_len, h_rc, h_prefix_costs, h_costs);
    });
}

// host-resident texts --------------------------------------------------------
int agc_hip_lz_encode_batch(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_text, const uint64_t *h_off,
                            const uint32_t *h_len, const uint8_t *h_rc, uint8_t *h_enc, uint64_t enc_cap, uint64_t *h_enc_off)
{
    if (!c || (n && (!h_text || !h_off || !h_len)))
        return AGC_HIP_EINVAL;
    return with_host_texts(c, n, h_text, h_off, h_len, [&](const uint8_t *d_base, const uint64_t *doff) {
        return agc_hip_lz_encode_batch_dev(c, n, h_gid, d_base, doff, h_len, h_rc, h_enc, enc_cap, h_enc_off);
    });
}

int agc_hip_lz_estimate_batch(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_text, const uint64_t *h_off,
                              const uint32_t *h_len, const uint8_t *h_rc, uint32_t *h_cost, uint32_t *h_peak)
{
    if (!c || (n && (!h_text || !h_off || !h_len)))
        return AGC_HIP_EINVAL;
    return with_host_texts(c, n, h_text, h_off, h_len, [&](const uint8_t *d_base, const uint64_t *doff) {
        return agc_hip_lz_estimate_batch_dev(c, n, h_gid, d_base, doff, h_len, h_rc, h_cost, h_peak);
    });
}

int agc_hip_lz_cost_vector_batch(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_text, const uint64_t *h_off,
                                 const uint32_t *h_len, const uint8_t *h_rc, const uint8_t *h_prefix_costs, uint32_t *h_costs)
{
    if (!c || (n && (!h_text || !h_off || !h_len)))
        return AGC_HIP_EINVAL;
    return with_host_texts(c, n, h_text, h_off, h_len, [&](const uint8_t *d_base, const uint64_t *doff) {
        return agc_hip_lz_cost_vector_batch_dev(c, n, h_gid, d_base, doff, h_len, h_rc, h_prefix_costs, h_costs);
    });
}

int agc_hip_lz_split_point_batch_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid1, const uint32_t *h_gid2,
                                     const uint8_t *d_base, const uint64_t *h_off, const uint32_t *h_len, const uint8_t *h_rc1,
                                     const uint8_t *h_prefix1, const uint8_t *h_rc2, const uint8_t *h_prefix2, uint32_t *h_best_pos,
                                     uint32_t *h_best_sum)
{
    if (!c || (n && (!h_gid1 || !h_gid2 || !d_base || !h_off || !h_len || !h_rc1 || !h_prefix1 || !h_rc2 || !h_prefix2 || !h_best_pos)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return lz_split_point_impl(c, n, h_gid1, h_gid2, src, off2, h_len, h_rc1, h_prefix1, h_rc2, h_prefix2, h_best_pos, h_best_sum);
    });
}

int agc_hip_fetch_slices_dev(agc_hip_ctx *c, uint32_t n, const uint8_t *d_base, const uint64_t *h_off, const uint32_t *h_len,
                             const uint8_t *h_rc, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    if (!c || !h_out_off || (n && (!d_base || !h_off || !h_len)))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return fetch_slices_impl(c, n, src, off2, h_len, h_rc, h_out, out_cap, h_out_off);
    });
}

int agc_hip_ref_lag_counts_dev(agc_hip_ctx *c, uint32_t n, const uint8_t *d_base, const uint64_t *h_off, const uint32_t *h_len,
                               const uint8_t *h_rc, uint32_t *h_cnt, uint32_t *h_cur)
{
    if (!c || (n && (!d_base || !h_off || !h_len || !h_cnt || !h_cur)))
        return AGC_HIP_EINVAL;
    if (!n)
        return AGC_HIP_OK;
    return with_packed_bytes(c, d_base, n, h_off, h_len, c->pk1, c->stream, [&](const PackedSrc &src, const uint64_t *off2) {
        return ref_lag_counts_impl(c, n, src, off2, h_len, h_rc, h_cnt, h_cur);
    });
}

// ---------------------------------------------------------------------------
// S3: zstd level-17 frames
// ---------------------------------------------------------------------------
uint32_t agc_hip_zstd17_max_input(void) { return zs::BLOCKSIZE_MAX; }

int agc_hip_zstd17_cparams(uint64_t src_size, uint32_t out7[7])
{
    if (!out7)
        return AGC_HIP_EINVAL;
    zs::level17Params(src_size, out7);
    return AGC_HIP_OK;
}

int agc_hip_zstd_cparams(int level, uint64_t src_size, uint32_t out7[7])
{
    if (!out7 || (level != 13 && level != 17 && level != 19))
        return AGC_HIP_EINVAL;
    zs::levelParams(level, src_size, out7);
    return AGC_HIP_OK;
}

uint32_t agc_hip_zstd17_resident_frames(agc_hip_ctx *c)
{
    if (!c)
        return 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0)
        return 0;
    // groups of 3 lanes: 21 frames per wave; 8 waves per CU (LDS: zgrp_lds_bytes(21, 3) = 20 328 of 160 KiB / 8; registers: 2 per SIMD)
    return (uint32_t)cus * 8u * 21u;
}

int agc_hip_zstd17_background(agc_hip_ctx *c, int on)
{
    if (!c)
        return AGC_HIP_EINVAL;
    c->zstd_background = on != 0;
    return AGC_HIP_OK;
}

// d_src_ext != nullptr: the inputs are in HBM already (input i = d_src_ext[h_src_off[i] .. h_src_off[i+1])); h_src is not looked at
static int zstd17_batch_impl(agc_hip_ctx *c, uint32_t n, const uint8_t *h_src, const uint8_t *d_src_ext, const uint64_t *h_src_off, uint8_t *h_dst,
                             uint64_t dst_cap, uint64_t *h_dst_off, const uint8_t *h_level = nullptr)
{
    if (!c || !h_dst_off || (n && (!h_src_off)))
        return AGC_HIP_EINVAL;
    h_dst_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const hipStream_t zs_ = c->zstream; // (this call shares no buffer, stream or event with the other entry points)
    const uint64_t src_total = h_src_off[n] - h_src_off[0];
    if (src_total && !h_src && !d_src_ext)
        return AGC_HIP_EINVAL;
    // per frame: parameters, workspace size; longest first so that the lanes of a wave finish together
    std::vector<ZFrameJob> jobs(n);
    std::vector<uint64_t> ws_need(n), dst_o(n);
    uint64_t dst_total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t len = h_src_off[i + 1] - h_src_off[i];
        if (h_src_off[i + 1] < h_src_off[i] || len > zs::BLOCKSIZE_MAX) {
            c->err = "zstd17_batch: input " + std::to_string(i) + " is larger than one block";
            return AGC_HIP_EINVAL;
        }
        const int level = h_level ? h_level[i] : 17;
        if (level != 13 && level != 17 && level != 19) {
            c->err = "zstd_batch: level " + std::to_string(level) + " (input " + std::to_string(i) + "): 13, 17 or 19";
            return AGC_HIP_EINVAL;
        }
        uint32_t p[7];
        zs::levelParams(level, len, p);
        const zs::CParams cp = {p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
        ws_need[i] = zs::wsLayout(cp, (uint32_t)len).total;
        dst_o[i] = dst_total;
        dst_total += (zs::frameBound((uint32_t)len) + 15) & ~15u;
        jobs[i].src = 0;
        jobs[i].dst = 0;
        jobs[i].ws = 0;
        jobs[i].src_size = (uint32_t)len;
        jobs[i].idx = i;
        jobs[i].cp = cp;
        jobs[i].pad = 0;
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return jobs[a].src_size > jobs[b].src_size; });

    if (!d_src_ext)
        CHK(ensure_z(c, c->d_zsrc, src_total + 64));
    const uint8_t *const d_src = d_src_ext ? d_src_ext + h_src_off[0] : (const uint8_t *)c->d_zsrc.p;
    CHK(ensure_z(c, c->d_zdst, dst_total + 64));
    CHK(ensure_z(c, c->d_zsize, (size_t)n * 4));
    CHK(ensure_z(c, c->d_zjobs, (size_t)n * sizeof(ZFrameJob)));
    if (src_total && !d_src_ext)
        HIPCHK(c, hipMemcpyAsync(c->d_zsrc.p, h_src + h_src_off[0], src_total, hipMemcpyHostToDevice, zs_));
    // workspace arena: as many frames per launch as the budget allows (a frame's tables must be zero at its start)
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    // (the call may run on a background thread beside the entry points that add samples: half of what is free, at most 32 GB --
    // one resident round of 43 008 frames of 16 KiB needs 19 GB -- leaves the other streams' buffers room to grow)
    uint64_t budget = std::min<uint64_t>(32ull << 30, (uint64_t)((free_b + c->d_zws.cap) * 0.5));
    if (const char *e = getenv("AGC_HIP_ZSTD_ARENA_MB"))
        budget = std::max<uint64_t>(1, strtoull(e, nullptr, 10)) << 20;
    budget = std::max<uint64_t>(budget, ws_need[order[0]]);
    std::vector<ZFrameJob> sorted(n);
    for (uint32_t done = 0; done < n;) {
        uint64_t used = 0;
        uint32_t m = 0;
        while (done + m < n && used + ws_need[order[done + m]] <= budget) {
            used += ws_need[order[done + m]];
            ++m;
        }
        CHK(ensure_z(c, c->d_zws, used));
        // the frames of this launch: first the ones the one-lane kernel takes, then the ones a group of lanes takes
        // (zstd/zs_opt_grp.h: inputs of the btultra2 class, <= 16 KiB -- every delta pack of a collection below ~35 samples)
        uint32_t grp_g = c->zstd_background ? 0u : 3u;
        if (const char *e = getenv("AGC_HIP_ZSTD_GROUP"))
            grp_g = (uint32_t)std::min(3, std::max(0, atoi(e)));
        if (grp_g == 1)
            grp_g = 0;
        // three classes: one-lane kernel (inputs the group parser does not take: < 8 bytes; everything in background mode), groups
        // with one-word records (inputs <= 16 KiB), groups with two-word records (the rest, up to one block)
        auto cls = [&](uint32_t i) -> int {
            if (!grp_g || !zs::grpEligible(jobs[i].cp, jobs[i].src_size))
                return 0;
            return zs::grpWide(jobs[i].cp, jobs[i].src_size) ? 2 : 1;
        };
        std::vector<uint32_t> part;
        part.reserve(m);
        uint32_t m_cls[3] = {0, 0, 0};
        for (int want = 0; want < 3; ++want)
            for (uint32_t t = 0; t < m; ++t) {
                const uint32_t i = order[done + t];
                if (cls(i) == want) {
                    part.push_back(i);
                    ++m_cls[want];
                }
            }
        const uint32_t m_one = m_cls[0], m_grp = m_cls[1], m_wide = m_cls[2];
        used = 0;
        for (uint32_t t = 0; t < m; ++t) {
            const uint32_t i = part[t];
            ZFrameJob jb = jobs[i];
            jb.src = h_src_off[i] - h_src_off[0];
            jb.dst = dst_o[i];
            jb.ws = used;
            used += ws_need[i];
            sorted[done + t] = jb;
        }
        HIPCHK(c, hipMemsetAsync(c->d_zws.p, 0, used, zs_));
        HIPCHK(c, hipMemcpyAsync((ZFrameJob *)c->d_zjobs.p + done, sorted.data() + done, (size_t)m * sizeof(ZFrameJob), hipMemcpyHostToDevice,
                                 zs_));
        {
            ZTimer t(c);
            const uint32_t dbg = 0; // (the kernels' trace word: a debugging build sets it)
            const dim3 block(64);
            if (m_one) {
                // frames per wave: fewer = fewer distinct parser states per trip of the micro-step loop, but every wave of the
                // launch must be resident at once (2 per SIMD = 2048 on 256 CUs) or the launch takes two rounds.  Measured per
                // 36 k frames of 13 KB: 24 lanes 1.31 s, 32 lanes 1.35 s, 48 lanes 1.38 s, 64 lanes 1.48 s, 16 lanes (two rounds) 1.82 s
                uint32_t lanes = 64; // (background launches: as few waves as possible, the other streams' kernels need the slots)
                if (!c->zstd_background)
                    for (uint32_t cand : {24u, 32u, 48u})
                        if ((m_one + cand - 1) / cand <= 1900) {
                            lanes = cand;
                            break;
                        }
                const dim3 grid((m_one + lanes - 1) / lanes);
                const ZFrameJob *dj = (const ZFrameJob *)c->d_zjobs.p + done;
                if (c->zstd_background)
                    hipLaunchKernelGGL((zstd_frames_kernel<2, false>), grid, block, 0, zs_, dj, m_one, (uint32_t *)c->d_zsize.p, lanes,
                                       d_src, (uint8_t *)c->d_zdst.p, (uint8_t *)c->d_zws.p, dbg);
                else // (frequency tables and the first matches of a request in LDS)
                    hipLaunchKernelGGL((zstd_frames_kernel<2, true, true>), grid, block, (size_t)lanes * zs::FAST_WORDS * 4, zs_, dj, m_one,
                                       (uint32_t *)c->d_zsize.p, lanes, d_src, (uint8_t *)c->d_zdst.p, (uint8_t *)c->d_zws.p, dbg);
            }
            // both group classes in one call: side by side on two streams (a launch lasts as long as its longest frame)
            const bool both = m_grp && m_wide;
            const hipStream_t zs_w = both ? c->zstream2 : zs_;
            if (both) {
                HIPCHK(c, hipEventRecord(c->zev_a, zs_));
                HIPCHK(c, hipStreamWaitEvent(c->zstream2, c->zev_a, 0));
            }
            const uint32_t gpw = grp_g ? 64 / grp_g : 1; // groups (= frames) per wave
            auto launch_grp = [&](uint32_t first, uint32_t count, bool wide, hipStream_t st) {
                const dim3 grid((count + gpw - 1) / gpw);
                const ZFrameJob *dj = (const ZFrameJob *)c->d_zjobs.p + done + first;
                const uint32_t stride = wide ? ZGRP_REC_STRIDE_WIDE : ZGRP_REC_STRIDE;
                if (grp_g == 2)
                    hipLaunchKernelGGL((zstd_frames_grp_kernel<2, 2>), grid, block, zgrp_lds_bytes(gpw, 2, wide), st, dj, count, (uint32_t *)c->d_zsize.p, gpw,
                                       d_src, (uint8_t *)c->d_zdst.p, (uint8_t *)c->d_zws.p, dbg, stride);
                else
                    hipLaunchKernelGGL((zstd_frames_grp_kernel<3, 2>), grid, block, zgrp_lds_bytes(gpw, 3, wide), st, dj, count, (uint32_t *)c->d_zsize.p, gpw,
                                       d_src, (uint8_t *)c->d_zdst.p, (uint8_t *)c->d_zws.p, dbg, stride);
            };
            if (m_wide)
                launch_grp(m_one + m_grp, m_wide, true, zs_w);
            if (m_grp)
                launch_grp(m_one, m_grp, false, zs_);
            if (both) {
                HIPCHK(c, hipEventRecord(c->zev_b, c->zstream2));
                HIPCHK(c, hipStreamWaitEvent(zs_, c->zev_b, 0));
            }
        }
        HIPCHK(c, hipGetLastError());
        done += m;
    }
    CHK(ensure_pinned(c, c->h_zsizes, (size_t)n * 4, ((size_t)n + n / 4 + 1024) * 4));
    uint32_t *sizes = c->h_zsizes.as<uint32_t>();
    HIPCHK(c, hipMemcpyAsync(sizes, c->d_zsize.p, (size_t)n * 4, hipMemcpyDeviceToHost, zs_));
    // (the launch lasts hundreds of ms and the host pool compresses its share of the packs meanwhile: this thread sleeps)
    HIPCHK(c, hipEventRecord(c->zev_wait, zs_));
    HIPCHK(c, hipEventSynchronize(c->zev_wait));
    for (uint32_t i = 0; i < n; ++i)
        h_dst_off[i + 1] = h_dst_off[i] + sizes[i];
    const uint64_t tot = h_dst_off[n];
    if (tot > dst_cap)
        return AGC_HIP_ECAP;
    if (!h_dst)
        return AGC_HIP_EINVAL;
    // compact the frames and bring them back in one copy
    CHK(ensure_z(c, c->d_zout, tot + 64));
    CHK(ensure_z(c, c->d_zdstoff, (size_t)(n + 1) * 8));
    HIPCHK(c, hipMemcpyAsync(c->d_zdstoff.p, h_dst_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, zs_));
    hipLaunchKernelGGL(zstd_gather_kernel, dim3(grid_for(n, 1, 16384)), dim3(256), 0, zs_, (const ZFrameJob *)c->d_zjobs.p, n,
                       (const uint64_t *)c->d_zdstoff.p, (const uint8_t *)c->d_zdst.p, (uint8_t *)c->d_zout.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_dst, c->d_zout.p, tot, hipMemcpyDeviceToHost, zs_));
    HIPCHK(c, hipStreamSynchronize(zs_));
    return AGC_HIP_OK;
}

int agc_hip_zstd_batch(agc_hip_ctx *c, uint32_t n, const uint8_t *h_src, const uint64_t *h_src_off, const uint8_t *h_level, uint8_t *h_dst,
                       uint64_t dst_cap, uint64_t *h_dst_off)
{
    return zstd17_batch_impl(c, n, h_src, nullptr, h_src_off, h_dst, dst_cap, h_dst_off, h_level);
}

int agc_hip_zstd17_batch(agc_hip_ctx *c, uint32_t n, const uint8_t *h_src, const uint64_t *h_src_off, uint8_t *h_dst, uint64_t dst_cap,
                         uint64_t *h_dst_off)
{
    return zstd17_batch_impl(c, n, h_src, nullptr, h_src_off, h_dst, dst_cap, h_dst_off);
}

int agc_hip_zstd17_batch_dev(agc_hip_ctx *c, uint32_t n, const uint8_t *d_src, const uint64_t *h_src_off, uint8_t *h_dst, uint64_t dst_cap,
                             uint64_t *h_dst_off)
{
    if (n && h_src_off && h_src_off[n] > h_src_off[0] && !d_src)
        return AGC_HIP_EINVAL;
    return zstd17_batch_impl(c, n, nullptr, d_src ? d_src : (const uint8_t *)1, h_src_off, h_dst, dst_cap, h_dst_off);
}

} // extern "C"

#include "splitters.hip"
#include "segments.hip"
#include "read_api.hip"
