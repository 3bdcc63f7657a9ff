// lzplan_host.cpp -- agc_amd/csrc/lz_plan.h on the CPU: the host arithmetic of the LZ write path behind a C interface, with mirrors of
// the kernels' records in the places of SegDesc, ChunkJob, ChunkPlan, FilterJob and EscJob.  TEST INFRASTRUCTURE ONLY.
//   -DLZPLAN_MAIN: a stand-alone program (no Python): seeded random batches through every function against a plain re-computation;
//   built with -fsanitize=address,undefined it also shows that no batch makes them leave their arrays (exact-size heap blocks).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../agc_amd/csrc/lz_plan.h"
#include "../../agc_amd/csrc/sym_view.h"

using namespace agc;

namespace {
// mirrors of the records of dev_common.h / lz_kernels.hip: the same members in the same order
struct Seg {
    SymView text;
    const unsigned long long *maybe;
    uint64_t out_off;
    uint32_t ref_slot, flags, idx, pad;
};
struct Job {
    uint32_t seg, chunk;
};
struct Plan {
    const Job *jobs;
    const uint32_t *seg_chunk0;
    uint32_t n_jobs, chunk_len, cap;
    void *logs;
    uint32_t *log_n;
    uint8_t *chunk_out;
    uint32_t chunk_stride;
};
struct FJ {
    SymView text;
    const unsigned long long *bloom;
    unsigned long long *out;
    uint32_t key_len, chunk, bloom_shift, pad;
};
struct EJ {
    SymView src;
    int32_t *esc_index;
    uint8_t *esc_bytes;
    uint32_t block, pad;
};

std::vector<Seg> segs_of(uint32_t n, const uint32_t *len)
{
    std::vector<Seg> s(n);
    for (uint32_t i = 0; i < n; ++i)
        s[i] = {{nullptr, nullptr, nullptr, 0, len[i], 0}, nullptr, 0, 0, 0, i, 0};
    return s;
}
} // namespace

extern "C" {

void lp_order(uint32_t n, const uint32_t *len, uint32_t *order)
{
    const std::vector<uint32_t> o = lp::longest_first(n, len);
    if (n)
        memcpy(order, o.data(), (size_t)n * 4);
}
uint64_t lp_out_offsets(int mode, uint32_t n, const uint32_t *len, uint64_t *off) { return lp::out_offsets(mode, n, len, off); }
uint64_t lp_filter_word_offsets(uint32_t n, const uint32_t *len, uint64_t *off) { return lp::filter_word_offsets(n, len, off); }
// the chunk starts of a text's filter jobs -> their number (every job carries the same bloom_shift: *shift)
uint32_t lp_filter_jobs(uint32_t len, uint32_t ref_size, uint32_t *chunk, uint32_t cap, uint32_t *shift)
{
    std::vector<FJ> jobs;
    lp::push_filter_jobs(jobs, SymView{nullptr, nullptr, nullptr, 0, len, 0}, nullptr, nullptr, 7, ref_size);
    for (size_t j = 0; j < jobs.size() && j < cap; ++j)
        chunk[j] = jobs[j].chunk, *shift = jobs[j].bloom_shift;
    return (uint32_t)jobs.size();
}
uint32_t lp_chunk_len_for(int forced, int has_batch, uint32_t n, uint32_t longest, uint64_t total) { return lp::chunk_len_for(forced, has_batch != 0, n, longest, total); }
uint64_t lp_count_chunk_jobs(uint32_t n, const uint32_t *len, uint32_t chunk_len) { return lp::count_chunk_jobs(segs_of(n, len).data(), n, chunk_len); }
int lp_chunks_fit(uint64_t n_jobs) { return lp::chunks_fit(n_jobs) ? 1 : 0; }
// -> 1: planned -- sizes = n_jobs, chunk_len, cap, chunk_stride, jobs (when there is room for them: jobs_cap pairs) and seg0[n + 1];
// 0: refused -- *built = what plan_chunks had put into its lists all the same (must be 0)
int lp_plan_chunks(uint32_t n, const uint32_t *len, uint32_t chunk_len, int encode, uint32_t *sizes, uint32_t *jobs, uint64_t jobs_cap, uint32_t *seg0, uint64_t *built)
{
    std::vector<Job> j;
    std::vector<uint32_t> s0;
    Plan pl{};
    const bool ok = lp::plan_chunks(segs_of(n, len).data(), n, chunk_len, encode != 0, j, s0, pl);
    *built = j.capacity() + s0.capacity() + pl.n_jobs;
    if (!ok)
        return 0;
    sizes[0] = pl.n_jobs, sizes[1] = pl.chunk_len, sizes[2] = pl.cap, sizes[3] = pl.chunk_stride;
    if (j.size() <= jobs_cap && !j.empty())
        memcpy(jobs, j.data(), j.size() * sizeof(Job));
    memcpy(seg0, s0.data(), s0.size() * 4);
    return 1;
}
uint64_t lp_logs_ahead_bytes(int encode, uint32_t n, uint64_t total, uint64_t have, uint64_t state_bytes) { return lp::logs_ahead_bytes(encode != 0, n, total, have, state_bytes); }

uint64_t lp_ht_size(uint32_t n_keys) { return lp::ht_size(n_keys); }
uint32_t lp_is_short(uint32_t len) { return lp::is_short(len); }
uint32_t lp_split_factor(uint32_t n_refs) { return lp::split_factor(n_refs); }
// the three regions of a batch of references: offsets of every stored form, table and filter pair, and each region's bytes (tot[3]);
// for a reference with esc[i] != 0, esc_at[2 i], [2 i + 1] = where the byte-per-symbol part starts in its escape block and the block's bytes
void lp_ref_layout(uint32_t n, const uint32_t *len, const uint32_t *n_keys, const uint8_t *esc, uint64_t *roff, uint64_t *toff, uint64_t *boff, uint64_t *tot, uint64_t *esc_at)
{
    tot[0] = lp::prefix(n, roff, [&](uint32_t i) { return lp::stored_bytes(len[i]); });
    tot[1] = lp::prefix(n, toff, [&](uint32_t i) { return lp::table_bytes(len[i], n_keys[i]); });
    tot[2] = lp::prefix(n, boff, [&](uint32_t i) { return lp::filter_bytes(len[i]); });
    for (uint32_t i = 0; i < n; ++i)
        if (esc[i]) {
            std::vector<EJ> jobs;
            lp::push_esc_jobs(jobs, SymView{nullptr, nullptr, nullptr, 0, len[i], 0}, nullptr, nullptr);
            esc_at[2 * i] = lp::esc_bytes_at((uint32_t)jobs.size()), esc_at[2 * i + 1] = lp::esc_alloc_bytes(lp::esc_blocks(len[i]));
        }
}
void lp_widen_dirty(int dirty, uint64_t lo, uint64_t hi, uint64_t on_dev, uint32_t min_gid, uint32_t max_gid, uint64_t *out)
{
    const lp::DirtyRange r = lp::widen_dirty(dirty != 0, {(size_t)lo, (size_t)hi}, (size_t)on_dev, min_gid, max_gid);
    out[0] = r.lo, out[1] = r.hi;
}

} // extern "C"

#ifdef LZPLAN_MAIN
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}
// lengths with the edges in them: tiny, around the chunk lengths and 16384, the radix digits' borders, huge
uint32_t rnd_len()
{
    static const uint32_t edges[] = {0, 1, 15, 16, 17, 63, 64, 65, 2047, 2048, 4095, 4096, 4097, 16383, 16384, 262139, 262140, 1u << 22, (1u << 22) + 1, 0xFFFFFFFFu};
    switch (rnd(8)) {
    case 0: return edges[rnd(sizeof edges / sizeof *edges)];
    case 1: return rnd(1u << 20);
    case 2: return rnd(70);
    default: return rnd(40000);
    }
}

#define FAIL(...)                                                                                  \
    do {                                                                                           \
        fprintf(stderr, "round %d: ", it);                                                         \
        fprintf(stderr, __VA_ARGS__);                                                              \
        fprintf(stderr, "\n");                                                                     \
        return 1;                                                                                  \
    } while (0)

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1)
        rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ULL;
    const int rounds = argc > 2 ? atoi(argv[2]) : 3000;
    uint64_t texts = 0;
    for (int it = 0; it < rounds; ++it) {
        const uint32_t n = rnd(8) ? rnd(40) : rnd(3000);
        std::vector<uint32_t> len(n);
        for (uint32_t &l : len)
            l = rnd_len();
        len.shrink_to_fit(); // (exact-size heap blocks: the sanitizer sees one element too far)
        // order: against a stable comparison sort
        std::vector<uint32_t> want(n), got(n);
        for (uint32_t i = 0; i < n; ++i)
            want[i] = i;
        std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return len[a] > len[b]; });
        lp_order(n, len.data(), got.data());
        if (got != want)
            FAIL("longest_first disagrees with a stable sort of %u lengths", n);
        // offsets in every mode and the filter words
        std::vector<uint64_t> off(n);
        off.shrink_to_fit();
        for (int mode = 0; mode < 3; ++mode) {
            const uint64_t tot = lp_out_offsets(mode, n, len.data(), off.data());
            uint64_t t = 0;
            for (uint32_t i = 0; i < n; ++i) {
                if (off[i] != t)
                    FAIL("mode %d: text %u starts at %llu, not %llu", mode, i, (unsigned long long)off[i], (unsigned long long)t);
                const uint64_t l = len[i];
                t += mode == MODE_ENCODE ? (l + l * 5 / 16 + 64 + 15) / 16 * 16 : mode == MODE_COSTVEC ? l : 0;
            }
            if (tot != t)
                FAIL("mode %d: total %llu, not %llu", mode, (unsigned long long)tot, (unsigned long long)t);
        }
        {
            const uint64_t tot = lp_filter_word_offsets(n, len.data(), off.data());
            uint64_t t = 0;
            for (uint32_t i = 0; i < n; ++i) {
                if (off[i] != t)
                    FAIL("filter words of text %u start at %llu", i, (unsigned long long)off[i]);
                t += ((uint64_t)len[i] + 63) / 64 + 1;
            }
            if (tot != t)
                FAIL("filter words: total %llu", (unsigned long long)tot);
        }
        // the chunk decision and the plan
        uint64_t total = 0;
        uint32_t longest = 0;
        for (uint32_t l : len)
            total += l, longest = std::max(longest, l);
        static const int forceds[] = {-1, -1, 0, 1, 63, 64, 300, 1024};
        const int forced = forceds[rnd(8)], has_batch = rnd(8) != 0;
        const uint32_t cl = lp_chunk_len_for(forced, has_batch, n, longest, total);
        const uint32_t cl_want = !has_batch || !n || !forced ? 0 : forced > 0 ? (forced < 64 ? 64 : (uint32_t)forced) : longest >= 16384 && (unsigned __int128)longest * 6144 > (unsigned __int128)total * 4 ? 4096 : 0;
        if (cl != cl_want)
            FAIL("chunk_len_for(%d, %d, %u, %u, %llu) = %u, not %u", forced, has_batch, n, longest, (unsigned long long)total, cl, cl_want);
        const uint32_t chunk = cl ? cl : 64 + rnd(5000), encode = rnd(2);
        std::vector<Seg> sorted_segs(n); // (processing order: longest first)
        for (uint32_t p = 0; p < n; ++p)
            sorted_segs[p] = {{nullptr, nullptr, nullptr, 0, len[want[p]], 0}, nullptr, 0, 0, 0, want[p], 0};
        sorted_segs.shrink_to_fit();
        uint64_t n_jobs = 0;
        for (uint32_t p = 0; p < n; ++p)
            n_jobs += std::max<uint64_t>(1, ((uint64_t)sorted_segs[p].text.len + chunk - 1) / chunk);
        {
            std::vector<Job> jobs;
            std::vector<uint32_t> seg0;
            Plan pl{};
            const bool ok = lp::plan_chunks(sorted_segs.data(), n, chunk, encode != 0, jobs, seg0, pl);
            if (ok != (n_jobs <= (1u << 22)) || (!ok && (jobs.capacity() || seg0.capacity() || pl.n_jobs)))
                FAIL("plan_chunks: %llu jobs, accepted %d", (unsigned long long)n_jobs, (int)ok);
            if (ok) {
                if (pl.n_jobs != n_jobs || jobs.size() != n_jobs || seg0.size() != (size_t)n + 1 || seg0[n] != n_jobs || pl.chunk_len != chunk || pl.cap != chunk / 8 + 4 ||
                    pl.chunk_stride != (encode ? (chunk + 5 * chunk / 16 + 160 + 15) / 16 * 16 : 0))
                    FAIL("plan_chunks: sizes of %u texts in chunks of %u", n, chunk);
                size_t j = 0;
                for (uint32_t p = 0; p < n; ++p) {
                    if (seg0[p] != j)
                        FAIL("plan_chunks: text %u starts at job %u, not %llu", p, seg0[p], (unsigned long long)j);
                    for (uint32_t ch = 0; j < jobs.size() && jobs[j].seg == p; ++ch, ++j)
                        if (jobs[j].chunk != ch || (ch && (uint64_t)ch * chunk >= sorted_segs[p].text.len))
                            FAIL("plan_chunks: job %llu is chunk %u of text %u (%u symbols)", (unsigned long long)j, jobs[j].chunk, p, sorted_segs[p].text.len);
                }
                if (j != jobs.size())
                    FAIL("plan_chunks: jobs out of order");
            }
        }
        {
            const uint64_t have = rnd(2) ? 0 : (uint64_t)rnd(1u << 30) * 16, sb = 16, tot2 = rnd(2) ? total : total + ((uint64_t)rnd(64) << 20);
            const uint64_t jobs2 = tot2 / 4096 + n, w = (jobs2 + jobs2 / 2) * 516 * sb;
            const uint64_t want_b = encode || n < 1024 || tot2 < 33554432 || have >= w ? 0 : w;
            if (lp_logs_ahead_bytes(encode, n, tot2, have, sb) != want_b)
                FAIL("logs_ahead_bytes(%u, %u, %llu, %llu)", encode, n, (unsigned long long)tot2, (unsigned long long)have);
        }
        // references: sizes, alignment, nothing overlaps
        const uint32_t n_refs = 1 + rnd(20);
        std::vector<uint32_t> rlen(n_refs), keys(n_refs);
        std::vector<uint8_t> esc(n_refs);
        std::vector<uint64_t> roff(n_refs), toff(n_refs), boff(n_refs), esc_at(2 * (size_t)n_refs);
        for (uint32_t i = 0; i < n_refs; ++i)
            rlen[i] = rnd(4) ? rnd(300000) : rnd_len() >> rnd(4), keys[i] = rlen[i] / 4 ? rnd(rlen[i] / 4 + 1) : 0, esc[i] = !rnd(3);
        for (auto *v : {&roff, &toff, &boff, &esc_at})
            v->shrink_to_fit();
        uint64_t tot[3];
        lp_ref_layout(n_refs, rlen.data(), keys.data(), esc.data(), roff.data(), toff.data(), boff.data(), tot, esc_at.data());
        for (uint32_t i = 0; i < n_refs; ++i) {
            const uint64_t rend = i + 1 < n_refs ? roff[i + 1] : tot[0], tend = i + 1 < n_refs ? toff[i + 1] : tot[1], bend = i + 1 < n_refs ? boff[i + 1] : tot[2];
            uint64_t hs = (uint64_t)((double)keys[i] / 0.7), p2 = 1;
            while (p2 * 2 <= hs)
                p2 *= 2;
            hs = hs ? std::max<uint64_t>(8, p2 * 2) : 8;
            const bool sh = rlen[i] / 4 < 65535;
            if (lp_ht_size(keys[i]) != hs || lp_is_short(rlen[i]) != (uint32_t)sh)
                FAIL("ht_size(%u) = %llu (want %llu), is_short(%u) = %u", keys[i], (unsigned long long)lp_ht_size(keys[i]), (unsigned long long)hs, rlen[i], lp_is_short(rlen[i]));
            if (roff[i] % 16 || rend - roff[i] < (((uint64_t)rlen[i] + 15) / 16 + 4) * 4 || rend - roff[i] >= (((uint64_t)rlen[i] + 15) / 16 + 4) * 4 + 16)
                FAIL("stored form of reference %u (%u symbols) at %llu..%llu", i, rlen[i], (unsigned long long)roff[i], (unsigned long long)rend);
            if (toff[i] % 256 || tend % 256 || tend - toff[i] < hs * (sh ? 4 : 8) || tend - toff[i] >= hs * (sh ? 4 : 8) + 256)
                FAIL("table of reference %u at %llu..%llu", i, (unsigned long long)toff[i], (unsigned long long)tend);
            uint32_t kshift = 20;
            while (kshift > 8 && (1u << (32 - kshift)) < (rlen[i] / 4 + 1) / 4)
                --kshift;
            if (bend - boff[i] != (uint64_t)16 << (32 - kshift))
                FAIL("filters of reference %u (%u symbols): %llu bytes", i, rlen[i], (unsigned long long)(bend - boff[i]));
            const uint64_t nb = ((uint64_t)rlen[i] + 1023) / 1024;
            if (esc[i] && (esc_at[2 * i] % 16 || esc_at[2 * i] < nb * 4 + 64 || esc_at[2 * i] >= nb * 4 + 64 + 16 || esc_at[2 * i + 1] != nb * 1028 + 64))
                FAIL("escape block of reference %u", i);
        }
        {
            const uint32_t want_split = n_refs >= 2048 ? 1 : std::min(16u, 2048 / n_refs);
            if (lp_split_factor(n_refs) != want_split)
                FAIL("split_factor(%u)", n_refs);
            uint32_t chunks[8], shift = 0;
            const uint32_t flen = rnd(400000), nj = lp_filter_jobs(flen, rlen[0], chunks, 8, &shift);
            if (nj != (flen + 65535) / 65536)
                FAIL("filter jobs of %u positions: %u", flen, nj);
            for (uint32_t j = 0; j < nj && j < 8; ++j)
                if (chunks[j] != j * 65536 || shift != key_bloom_shift(rlen[0]))
                    FAIL("filter job %u of %u positions", j, flen);
        }
        // the dirty range holds the old one and the batch, and reaches down to what the device has
        {
            const uint64_t on_dev = rnd(100), lo = rnd(120), hi = rnd(3) ? lo + rnd(50) : rnd(120);
            const uint32_t a = rnd(200), b = a + rnd(60);
            const int dirty = rnd(2);
            uint64_t out[2];
            lp_widen_dirty(dirty, lo, hi, on_dev, a, b, out);
            const bool old = dirty && hi > lo;
            const uint64_t wlo = std::min<uint64_t>(on_dev, old ? std::min<uint64_t>(lo, a) : a), whi = old ? std::max<uint64_t>(hi, b + 1) : b + 1;
            if (out[0] != wlo || out[1] != whi)
                FAIL("widen_dirty(%d, [%llu, %llu), %llu, %u, %u) = [%llu, %llu)", dirty, (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)on_dev, a, b,
                     (unsigned long long)out[0], (unsigned long long)out[1]);
        }
        texts += n;
    }
    printf("ok %d batches, %llu texts\n", rounds, (unsigned long long)texts);
    return 0;
}
#endif
