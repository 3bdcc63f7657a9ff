// lz_plan.h -- the host arithmetic of the LZ write path (api.hip: prepare_batch, launch_parse, ref_register_impl): the order of a
// batch, where every text's output goes, when and how a launch is cut into chunks, how a reference is laid out in the arena.  Plain
// C++17 without HIP: api.hip uses it with the kernels' records, tests/lzplan_host with mirrors of them on the CPU.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cstring>
#include <vector>

#include "lz_consts.h"

namespace agc {
namespace lp {

// off[i] = the sizes in front of item i -> the sum of all n
template <class F> uint64_t prefix(uint32_t n, uint64_t *off, F size)
{
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        off[i] = tot;
        tot += size(i);
    }
    return tot;
}

// ---- a batch of parses ---------------------------------------------------------------------------------------------------------
// longest first, stable in the index: LSD radix sort on ~len (3 passes of 11 bits; a comparison sort of the 50 k segments of a human
// sample costs milliseconds of host time per call)
inline std::vector<uint32_t> longest_first(uint32_t n, const uint32_t *len)
{
    std::vector<uint32_t> order(n), tmp(n);
    for (uint32_t i = 0; i < n; ++i)
        order[i] = i;
    uint32_t *src = order.data(), *dst = tmp.data();
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = 11 * pass;
        uint32_t cnt[2049] = {0};
        for (uint32_t i = 0; i < n; ++i)
            ++cnt[((~len[src[i]] >> sh) & 2047u) + 1];
        for (int t = 0; t < 2048; ++t)
            cnt[t + 1] += cnt[t];
        for (uint32_t i = 0; i < n; ++i)
            dst[cnt[(~len[src[i]] >> sh) & 2047u]++] = src[i];
        std::swap(src, dst);
    }
    if (src != order.data()) // (an odd number of passes: the result is in tmp)
        std::memcpy(order.data(), src, (size_t)n * 4);
    return order;
}

// the bytes a text's delta may take: a >= 16-symbol match costs <= 21 bytes
inline uint64_t encode_bound(uint32_t len) { return (((uint64_t)len + 5ULL * len / 16 + 64) + 15) & ~15ULL; }

// where text i's output starts in the scratch buffer (encode: bytes; cost vector: one unit per symbol; estimate: none) -> the total
inline uint64_t out_offsets(int mode, uint32_t n, const uint32_t *len, uint64_t *off)
{
    return prefix(n, off, [&](uint32_t i) -> uint64_t { return mode == MODE_ENCODE ? encode_bound(len[i]) : mode == MODE_COSTVEC ? len[i] : 0; });
}

// ... and its "may match" bits (key_filter_kernel), in 64-bit words
inline uint64_t filter_word_offsets(uint32_t n, const uint32_t *len, uint64_t *off)
{
    return prefix(n, off, [&](uint32_t i) { return ((uint64_t)len[i] + 63) / 64 + 1; });
}

// one FilterJob per FILTER_CHUNK positions of a text
template <class FJ, class View> void push_filter_jobs(std::vector<FJ> &jobs, const View &text, const unsigned long long *bloom, unsigned long long *out, uint32_t key_len,
                                                      uint32_t ref_size)
{
    for (uint32_t ch = 0; ch < text.len; ch += FILTER_CHUNK)
        jobs.push_back({text, bloom, out, key_len, ch, key_bloom_shift(ref_size), 0u});
}

// ---- the parse in chunks -------------------------------------------------------------------------------------------------------
// The chunk length of a launch, 0: whole texts.  forced: AGC_HIP_LZ_CHUNK (< 0: not set, 0: never in chunks); has_batch: the host made
// the n descriptors (a count made on the device cannot be planned for); longest, total: symbols of the longest text and of all.
// Unforced, chunks are worth it when the longest text's chain outlasts the launch's work spread over the chip (~6 k wavefronts in
// flight): the diverged collections' few long texts, not the 3 000 cost-vector parses of a human sample
inline uint32_t chunk_len_for(int forced, bool has_batch, uint32_t n, uint32_t longest, uint64_t total)
{
    if (!has_batch || !n || forced == 0)
        return 0;
    if (forced > 0)
        return (uint32_t)std::max(64, forced);
    return longest >= 16384 && (uint64_t)longest * 6144 > 4 * total ? 4096 : 0;
}

inline bool chunks_fit(uint64_t n_jobs) { return n_jobs <= (1u << 22); } // more: the launch parses whole texts
inline uint32_t chunks_of(uint32_t len, uint32_t chunk_len) { return std::max<uint32_t>(1, (uint32_t)(((uint64_t)len + chunk_len - 1) / chunk_len)); }
template <class Seg> uint64_t count_chunk_jobs(const Seg *segs, uint32_t n, uint32_t chunk_len)
{
    uint64_t jobs = 0;
    for (uint32_t i = 0; i < n; ++i)
        jobs += chunks_of(segs[i].text.len, chunk_len);
    return jobs;
}

// The chunk list of n descriptors (jobs; seg0[i] = text i's first job, seg0[n] = their number) and the sizes in pl: `cap` log entries
// per chunk, encode: the bytes of a chunk's own output slot.  false: too many jobs -- nothing is built, pl is left alone
template <class Seg, class Job, class Plan>
bool plan_chunks(const Seg *segs, uint32_t n, uint32_t chunk_len, bool encode, std::vector<Job> &jobs, std::vector<uint32_t> &seg0, Plan &pl)
{
    const uint64_t n_jobs = count_chunk_jobs(segs, n, chunk_len);
    if (!chunks_fit(n_jobs))
        return false;
    jobs.reserve(n_jobs), seg0.resize((size_t)n + 1);
    for (uint32_t i = 0; i < n; ++i) {
        seg0[i] = (uint32_t)jobs.size();
        for (uint32_t ch = 0, nc = chunks_of(segs[i].text.len, chunk_len); ch < nc; ++ch)
            jobs.push_back({i, ch});
    }
    seg0[n] = pl.n_jobs = (uint32_t)n_jobs;
    pl.chunk_len = chunk_len;
    pl.cap = chunk_len / 8 + 4;
    pl.chunk_stride = encode ? ((chunk_len + 5 * chunk_len / 16 + 160 + 15) & ~15u) : 0;
    return true;
}

// A big batch that was not worth chunks: the next one may be.  The bytes of chunk logs to allocate ahead for it (this batch's text
// and a half, in 4096-symbol chunks of state_bytes per entry), 0: none -- an encode, a small batch, or `have` bytes are enough (the
// few-texts launches of every step leave a small buffer behind)
inline uint64_t logs_ahead_bytes(bool encode, uint32_t n, uint64_t total, uint64_t have, uint64_t state_bytes)
{
    if (encode || n < 1024 || total < (32u << 20))
        return 0;
    const uint64_t n_jobs = total / 4096 + n, want = (n_jobs + n_jobs / 2) * (4096 / 8 + 4) * state_bytes;
    return have < want ? want : 0;
}

// ---- a reference in the arena --------------------------------------------------------------------------------------------------
// stored form: ref_size symbols in 2-bit words + REF_TAIL_WORDS words of slack, 16-byte aligned
inline uint64_t stored_bytes(uint32_t len) { return ((((uint64_t)len + 15) / 16 + REF_TAIL_WORDS) * 4 + 15) & ~15ULL; }
inline uint32_t is_short(uint32_t len) { return (len / HASHING_STEP) < 65535u; } // 16-bit positions in the index: lz_diff.cpp:146
// entries of the index of n_keys keys (prepare_index, lz_diff.cpp:117-125): double division by 0.7, down to a power of two, doubled, >= 8
inline uint64_t ht_size(uint32_t n_keys)
{
    uint64_t hs = (uint64_t)((double)n_keys / 0.7);
    while (hs & (hs - 1))
        hs &= hs - 1;
    return std::max<uint64_t>(hs << 1, 8);
}
inline uint64_t table_bytes(uint32_t len, uint32_t n_keys) { return (ht_size(n_keys) * (is_short(len) ? 4 : 8) + 255) & ~255ULL; }
inline uint64_t filter_bytes(uint32_t len) { return (uint64_t)2 * key_bloom_half_words(key_bloom_shift(len)) * 8; } // two filters of 64-bit words
// a reference that holds a symbol outside ACGT: one block of esc_alloc_bytes -- the escape index, then (16-byte aligned) a byte per symbol
inline uint32_t esc_blocks(uint32_t len) { return (uint32_t)(((uint64_t)len + PACK_BLOCK - 1) / PACK_BLOCK); }
inline uint64_t esc_alloc_bytes(uint32_t nb) { return (uint64_t)nb * 4 + 64 + (uint64_t)nb * PACK_BLOCK; }
inline uint64_t esc_bytes_at(uint32_t nb) { return ((uint64_t)nb * 4 + 64 + 15) & ~15ULL; }
template <class EJ, class View> void push_esc_jobs(std::vector<EJ> &jobs, const View &src, int32_t *esc_index, uint8_t *esc_bytes)
{
    for (uint32_t b = 0, nb = esc_blocks(src.len); b < nb; ++b)
        jobs.push_back({src, esc_index, esc_bytes, b, 0u});
}
// few references per batch (steady state): each is spread over this many blocks to fill the chip
inline uint32_t split_factor(uint32_t n_refs) { return n_refs >= 2048 ? 1u : std::min<uint32_t>(16u, 2048u / n_refs); }

// The groups [lo, hi) whose descriptors have to go to the device, after a batch with these gids was registered on top of the old
// range (`dirty`: it holds something).  The descriptors a resize added between the old end and min_gid are invalid ones and go over
// too: lo never lies above on_dev, the number of descriptors the device has
struct DirtyRange {
    size_t lo, hi;
};
inline DirtyRange widen_dirty(bool dirty, DirtyRange old, size_t on_dev, uint32_t min_gid, uint32_t max_gid)
{
    DirtyRange r = {min_gid, (size_t)max_gid + 1};
    if (dirty && old.hi > old.lo)
        r = {std::min(old.lo, r.lo), std::max(old.hi, r.hi)};
    r.lo = std::min(r.lo, on_dev);
    return r;
}

} // namespace lp
} // namespace agc
