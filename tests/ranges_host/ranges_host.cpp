// ranges_host.cpp -- agc_amd/csrc/range_clip.h and range_plan.h on the CPU.  The windowed decode runs in the order of
// lz_decode_window_kernel (range_kernels.hip): strips of 64 bytes, the scan of the Steps with the State carried between strips, every
// token cut to the window before it writes, the walk stopped at the first strip that starts at or behind the window.  TEST
// INFRASTRUCTURE ONLY.  The reference is a plain byte array here (the 2-bit accessors: tests/symview_host).  rp_layout runs the host
// arithmetic of agc_hip_ranges_parts (range_plan.h: lay_out_queries, lay_out_windows -- the output offsets, the windows' jobs, the
// first complaint) with mirrors of the kernels' job records; tables stand in for what the device finds in the packs and for the
// references' sizes.  The product (read_api.hip) calls the same two functions and only launches what they return.
//   -DRANGES_MAIN: a stand-alone program (no Python): random well-formed deltas, every window of a seeded sample against the plain
//   token-by-token decode, sliced, the output in a heap block of exactly the window's size -- built with -fsanitize=address,undefined
//   it also shows that no window makes the clipped walk write outside its output; random contigs through range_plan.h against
//   a position-by-position count; and random batches through rp_layout against a plain recomputation window by window.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../agc_amd/csrc/lz_decode.h"
#include "../../agc_amd/csrc/range_clip.h"
#include "../../agc_amd/csrc/range_plan.h"

using namespace agc::lzd;
namespace rw = agc::rw;
namespace rp = agc::rp;

namespace {

constexpr uint32_t LANES = STRIP;

// visit(tokens[64], states[64]) once per strip; false stops the walk (as tests/lzdec_host has it)
template <class F> State walk_delta(const uint8_t *enc, uint64_t enc_len, uint32_t ref_size, uint32_t min_match_len, F visit)
{
    State carry = {0, 0};
    uint32_t carry_end = 1;
    for (uint64_t base = 0; base < enc_len; base += STRIP) {
        uint64_t ends = 0, valid = 0;
        for (uint32_t lane = 0; lane < LANES; ++lane)
            if (base + lane < enc_len) {
                valid |= 1ULL << lane;
                ends |= (uint64_t)ends_token(enc[base + lane]) << lane;
            }
        const uint64_t starts = token_starts(ends, valid, carry_end);
        carry_end = starts_carry(ends);
        Token t[LANES];
        Step incl[LANES], up[LANES];
        State before[LANES];
        for (uint32_t lane = 0; lane < LANES; ++lane) {
            t[lane] = {NONE, 0, 0};
            if ((starts >> lane) & 1)
                t[lane] = parse_token(enc + base + lane, enc_len - (base + lane), min_match_len);
            incl[lane] = step_of(t[lane], ref_size);
        }
        for (uint32_t d = 1; d < LANES; d <<= 1) {
            for (uint32_t lane = d; lane < LANES; ++lane)
                up[lane] = incl[lane - d];
            for (uint32_t lane = d; lane < LANES; ++lane)
                incl[lane] = combine(up[lane], incl[lane]);
        }
        for (uint32_t lane = 0; lane < LANES; ++lane)
            before[lane] = apply(lane ? incl[lane - 1] : identity(), carry);
        if (!visit(t, before))
            break;
        carry = apply(incl[LANES - 1], carry);
    }
    return carry;
}

// the scan: status and length
uint32_t scan(uint32_t ref_size, uint32_t min_match_len, const uint8_t *enc, uint64_t enc_len, uint64_t *out_len)
{
    uint32_t status = OK;
    const State end = walk_delta(enc, enc_len, ref_size, min_match_len, [&](const Token *t, const State *before) {
        for (uint32_t lane = 0; lane < LANES; ++lane)
            if (t[lane].kind != NONE && (status = check_token(t[lane], before[lane], ref_size)) != OK)
                return false;
        return true;
    });
    if (status == OK)
        status = check_length(end.out);
    *out_len = end.out;
    return status;
}

// lz_decode_window_kernel's visit, lane after lane; -> the strips walked
uint32_t window_write(const uint8_t *ref, uint32_t ref_size, uint32_t min_match_len, const uint8_t *enc, uint64_t enc_len, uint32_t rc, uint32_t w_lo, uint32_t w_hi,
                      uint8_t *dst)
{
    uint32_t strips = 0;
    walk_delta(enc, enc_len, ref_size, min_match_len, [&](const Token *t, const State *before) {
        if (before[0].out >= w_hi)
            return false;
        ++strips;
        for (uint32_t lane = 0; lane < LANES; ++lane) {
            const Token &k = t[lane];
            const uint64_t at = before[lane].out;
            if ((k.kind == LITERAL || k.kind == LITERAL_REF) && rw::inside(at, w_lo, w_hi)) {
                const uint8_t c = k.kind == LITERAL ? (uint8_t)k.n : ref[before[lane].pred];
                dst[rw::dst_offset((uint32_t)at, 1, w_lo, w_hi, rc)] = rc ? complement(c) : c;
            }
            uint32_t lo = w_lo, cnt = 0;
            if (k.kind == NRUN || k.kind == MATCH || k.kind == MATCH_TO_END)
                rw::clip(at, match_symbols(k, before[lane], ref_size), w_lo, w_hi, lo, cnt);
            if (!cnt)
                continue;
            const uint64_t ref_pos = (uint64_t)match_ref_pos(k, before[lane]) + (lo - at);
            uint8_t *d = dst + rw::dst_offset(lo, cnt, w_lo, w_hi, rc);
            for (uint32_t q = 0; q < cnt; ++q) { // (wave_copy(rd, ref_pos, cnt, rc, d): the stretch, reverse-complemented on request)
                const uint8_t c = k.kind == NRUN ? 4 : ref[ref_pos + (rc ? cnt - 1 - q : q)];
                d[q] = rc ? complement(c) : c;
            }
        }
        return true;
    });
    return strips;
}

} // namespace

// the oriented window [win_from, win_from + win_len) of the delta's symbols -> out (win_len bytes).  -> 0, the delta's status when it
// is malformed, or 100 when the window does not fit its decoded length; *strips: the strips the clipped walk visited
extern "C" uint32_t ranges_decode_window(const uint8_t *ref, uint32_t ref_size, uint32_t min_match_len, const uint8_t *enc, uint64_t enc_len, int rc, uint32_t win_from,
                                         uint32_t win_len, uint8_t *out, uint32_t *strips)
{
    uint64_t len = 0;
    const uint32_t status = scan(ref_size, min_match_len, enc, enc_len, &len);
    if (status != OK)
        return status;
    if (!rp::window_fits(win_from, win_len, (uint32_t)len))
        return 100;
    uint32_t w_lo, w_hi;
    rw::decode_window(win_from, win_len, (uint32_t)len, rc ? 1 : 0, w_lo, w_hi);
    const uint32_t n = window_write(ref, ref_size, min_match_len, enc, enc_len, rc ? 1 : 0, w_lo, w_hi, out);
    if (strips)
        *strips = n;
    return 0;
}

// segment_window_kernel's RAW loop: the window of symbol bytes
extern "C" void ranges_raw_window(const uint8_t *src, uint32_t len, int rc, uint32_t win_from, uint32_t win_len, uint8_t *out)
{
    uint32_t w_lo, w_hi;
    rw::decode_window(win_from, win_len, len, rc ? 1 : 0, w_lo, w_hi);
    for (uint32_t q = 0; q < win_len; ++q)
        out[q] = rc ? complement(src[w_hi - 1 - q]) : src[w_lo + q];
}

// rw::decode_window itself (range_clip.h): the oriented window in decode order
extern "C" void ranges_window_in_decode_order(uint32_t win_from, uint32_t win_len, uint32_t len, int rc, uint32_t *w_lo, uint32_t *w_hi)
{
    rw::decode_window(win_from, win_len, len, rc ? 1 : 0, *w_lo, *w_hi);
}

// range_plan.h: the windows of [from, to] on a contig of n_seg segments -> their count (at most n_seg: the arrays' size); *n_sym:
// the symbols of the range
extern "C" uint64_t ranges_contig_windows(uint64_t n_seg, const uint32_t *lengths, uint32_t k, int64_t from, int64_t to, uint32_t *seg, uint32_t *win_from,
                                          uint32_t *win_len, uint64_t *n_sym)
{
    uint64_t n = 0;
    *n_sym = rp::contig_windows(
        n_seg, [&](uint64_t s) { return lengths[s]; }, k, from, to, [&](uint64_t s, uint32_t a, uint32_t len) {
            seg[n] = (uint32_t)s, win_from[n] = a, win_len[n] = len;
            ++n;
        });
    return n;
}

// ---- range_plan.h: the layout agc_hip_ranges_parts computes from a batch, behind tables in the device's and the context's place ------
namespace {
// mirrors of DecodeJob (lz_decode_kernels.hip), WindowJob and WindowCopyJob (range_kernels.hip): the same members in the same order
// (read_api.hip asserts the kernel records' sizes, these are asserted here)
struct DJ {
    uint64_t enc_off, enc_len, out_off;
    uint32_t out_len, ref_slot, rc, pad;
};
struct WJ {
    uint64_t enc_off, enc_len, out_off;
    uint32_t w_lo, w_hi, ref_slot, rc;
};
struct CJ {
    uint64_t src_off, out_off;
    uint32_t len, win_from, win_len, ref_slot, rc, is_ref;
};
static_assert(sizeof(DJ) == 40 && sizeof(WJ) == 40 && sizeof(CJ) == 40, "the mirrors have the kernel records' sizes");
typedef rp::WindowLayout<DJ, WJ, CJ> HostLayout;

// what the device found: pack p has pack_count[p] sequences, sequence q < min(count, seq_cap) of it is the bytes
// [seq_off[p * seq_cap + q], + seq_len[p * seq_cap + q]); ref_size[gid], gid < n_refs: a reference's symbols, new or registered (< 0: none)
struct Tables {
    const uint32_t *pack_count;
    uint32_t seq_cap;
    const uint64_t *seq_off;
    const uint32_t *seq_len;
    const int64_t *ref_size;
    uint32_t n_refs;
};

HostLayout lay_out(uint64_t n_win, const agc_hip_seg_win *win, const uint64_t *win_out, const Tables &T)
{
    return rp::lay_out_windows<DJ, WJ, CJ>(
        "ranges_parts", n_win, win, win_out,
        [&T](uint32_t part, uint32_t index, uint64_t &off, uint32_t &n, std::string &why) {
            if (index >= T.pack_count[part] || index >= T.seq_cap) {
                why = "sequence " + std::to_string(index) + " of part " + std::to_string(part) + ", which has " + std::to_string(T.pack_count[part]);
                return false;
            }
            off = T.seq_off[(size_t)part * T.seq_cap + index], n = T.seq_len[(size_t)part * T.seq_cap + index];
            return true;
        },
        [&T](uint32_t gid) { return gid < T.n_refs ? T.ref_size[gid] : (int64_t)-1; });
}
} // namespace

// Steps 1 and 4 of agc_hip_ranges_parts as the call runs them.  -> -1: step 1 refuses the ranges (out_off[0] = 0 is all that is
// written); otherwise step 4's code (0: no complaint; why: its message, cut to why_cap - 1 characters).  out_off: n_q + 1; win_out,
// dj, wj, cj: room for one row per window -- dj: the window, then the job's members (7 numbers), wj: 7, cj: 8; sizes: n_dj, n_wj, n_cj,
// the total
extern "C" int rp_layout(uint32_t n_q, const uint64_t *q_seg, const agc_hip_seg_win *win, const uint32_t *pack_count, uint32_t seq_cap, const uint64_t *seq_off,
                         const uint32_t *seq_len, const int64_t *ref_size, uint32_t n_refs, uint64_t *out_off, uint64_t *win_out, uint64_t *dj, uint64_t *wj, uint64_t *cj,
                         uint64_t *sizes, char *why, uint32_t why_cap)
{
    std::vector<uint64_t> at;
    uint64_t total = 0;
    out_off[0] = 0;
    if (!rp::lay_out_queries(n_q, q_seg, win, out_off, at, total))
        return -1;
    const HostLayout Y = lay_out(at.size(), win, at.data(), {pack_count, seq_cap, seq_off, seq_len, ref_size, n_refs});
    if (!at.empty())
        memcpy(win_out, at.data(), at.size() * sizeof(uint64_t));
    for (size_t i = 0; i < Y.dj.size(); ++i) {
        const DJ &j = Y.dj[i];
        const uint64_t row[7] = {Y.dj_win[i], j.enc_off, j.enc_len, j.out_off, j.out_len, j.ref_slot, j.rc};
        memcpy(dj + 7 * i, row, sizeof row);
    }
    for (size_t i = 0; i < Y.wj.size(); ++i) {
        const WJ &j = Y.wj[i];
        const uint64_t row[7] = {j.enc_off, j.enc_len, j.out_off, j.w_lo, j.w_hi, j.ref_slot, j.rc};
        memcpy(wj + 7 * i, row, sizeof row);
    }
    for (size_t i = 0; i < Y.cj.size(); ++i) {
        const CJ &j = Y.cj[i];
        const uint64_t row[8] = {j.src_off, j.out_off, j.len, j.win_from, j.win_len, j.ref_slot, j.rc, j.is_ref};
        memcpy(cj + 8 * i, row, sizeof row);
    }
    sizes[0] = Y.dj.size(), sizes[1] = Y.wj.size(), sizes[2] = Y.cj.size(), sizes[3] = total;
    if (why_cap)
        snprintf(why, why_cap, "%s", Y.why.c_str());
    return Y.code;
}

#ifdef RANGES_MAIN
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

void put_number(std::vector<uint8_t> &e, uint64_t v)
{
    char b[32];
    snprintf(b, sizeof b, "%llu", (unsigned long long)v);
    e.insert(e.end(), b, b + strlen(b));
}

// a well-formed delta and what it decodes to, token after token
void random_delta(const std::vector<uint8_t> &ref, uint32_t mml, std::vector<uint8_t> &enc, std::vector<uint8_t> &want)
{
    const uint32_t ref_size = (uint32_t)ref.size();
    int64_t pred = 0;
    for (uint32_t n_tok = rnd(120), t = 0; t < n_tok; ++t) {
        const uint32_t kind = rnd(100);
        if (kind < 50) {
            const bool bang = rnd(6) == 0 && pred < (int64_t)ref_size;
            const uint8_t c = (uint8_t)rnd(21);
            enc.push_back(bang ? '!' : 'A' + c);
            want.push_back(bang ? ref[pred] : c);
            ++pred;
        } else if (kind < 60) {
            const uint32_t n = rnd(90);
            enc.push_back(NRUN_FIRST);
            put_number(enc, n);
            enc.push_back(NRUN_LAST);
            want.insert(want.end(), n + NRUN_MIN, 4);
        } else {
            const int64_t ref_pos = rnd(ref_size + 1), diff = ref_pos - pred;
            const uint64_t room = ref_size - ref_pos;
            if (diff < 0)
                enc.push_back('-');
            put_number(enc, (uint64_t)(diff < 0 ? -diff : diff));
            uint64_t n = room;
            if (rnd(8) && room >= mml) {
                n = mml + rnd((uint32_t)(room - mml) + 1);
                enc.push_back(',');
                put_number(enc, n - mml);
            }
            enc.push_back('.');
            want.insert(want.end(), ref.begin() + ref_pos, ref.begin() + ref_pos + n);
            pred = ref_pos + (int64_t)n;
        }
    }
}

// A random batch through rp_layout -- some windows out of their pack's reach or of another size than their sequence or reference --
// against a plain recomputation window by window: the offsets, every job, the first complaint.  Inputs and outputs are heap blocks
// of exactly their size (the job arrays: of the rows the recomputation expects).
bool random_batch(int it)
{
    const uint32_t n_q = 1 + rnd(5), n_packs = 1 + rnd(3), seq_cap = 1 + rnd(6), n_refs = 1 + rnd(5);
    std::vector<uint64_t> q_seg{0}, seq_off((size_t)n_packs * seq_cap);
    std::vector<uint32_t> pack_count(n_packs), seq_len((size_t)n_packs * seq_cap);
    std::vector<int64_t> ref_size(n_refs);
    for (uint32_t q = 0; q < n_q; ++q)
        q_seg.push_back(q_seg.back() + rnd(4));
    uint64_t bytes = 0;
    for (uint32_t p = 0; p < n_packs; ++p) {
        pack_count[p] = rnd(seq_cap + 3); // (also more than are indexed)
        for (uint32_t q = 0; q < seq_cap; ++q) {
            seq_off[(size_t)p * seq_cap + q] = bytes, seq_len[(size_t)p * seq_cap + q] = 1 + rnd(200);
            bytes += seq_len[(size_t)p * seq_cap + q] + 1;
        }
    }
    for (auto &r : ref_size)
        r = rnd(5) ? 1 + (int64_t)rnd(300) : -1;
    const size_t n_win = (size_t)q_seg.back();
    std::vector<agc_hip_seg_win> win(n_win);
    std::vector<uint64_t> want_off, want_at, want_dj, want_wj, want_cj;
    int64_t bad = -1; // the first window the recomputation refuses
    for (size_t w = 0; w < n_win; ++w) {
        agc_hip_seg_win &g = win[w];
        g.kind = rnd(3), g.gid = rnd(n_refs), g.part = rnd(n_packs), g.index = rnd(seq_cap + 1), g.rc = rnd(2);
        const bool reach = g.index < pack_count[g.part] && g.index < seq_cap;
        const size_t row = (size_t)g.part * seq_cap + (reach ? g.index : 0);
        const int64_t have = g.kind == AGC_HIP_SEG_RAW ? (int64_t)seq_len[row] : ref_size[g.gid];
        g.length = g.kind != AGC_HIP_SEG_DELTA && have > 0 && rnd(8) ? (uint32_t)have : 1 + rnd(300);
        g.win_from = rnd(g.length), g.win_len = 1 + rnd(g.length - g.win_from);
        want_at.push_back(w ? want_at.back() + win[w - 1].win_len : 0);
        if (bad >= 0)
            continue;
        const uint64_t off = g.kind != AGC_HIP_SEG_REF ? seq_off[row] : 0, n = g.kind != AGC_HIP_SEG_REF ? seq_len[row] : 0;
        if ((g.kind != AGC_HIP_SEG_REF && !reach) || (g.kind != AGC_HIP_SEG_DELTA && have != (int64_t)g.length))
            bad = (int64_t)w;
        else if (g.kind == AGC_HIP_SEG_DELTA) {
            const uint32_t lo = g.rc ? g.length - g.win_from - g.win_len : g.win_from;
            want_dj.insert(want_dj.end(), {w, off, n, 0, g.length, g.gid, g.rc});
            want_wj.insert(want_wj.end(), {off, n, want_at[w], lo, lo + g.win_len, g.gid, g.rc});
        } else
            want_cj.insert(want_cj.end(), {off, want_at[w], g.length, g.win_from, g.win_len, g.gid, g.rc, g.kind == AGC_HIP_SEG_REF ? 1u : 0u});
    }
    const uint64_t total = n_win ? want_at.back() + win.back().win_len : 0;
    for (uint32_t q = 0; q <= n_q; ++q)
        want_off.push_back(q_seg[q] < n_win ? want_at[q_seg[q]] : total);
    q_seg.shrink_to_fit(), seq_off.shrink_to_fit(), pack_count.shrink_to_fit(), seq_len.shrink_to_fit(), ref_size.shrink_to_fit(), win.shrink_to_fit();
    uint64_t *out_off = (uint64_t *)malloc(((size_t)n_q + 1) * 8), *at = (uint64_t *)malloc(n_win * 8), *dj = (uint64_t *)malloc(want_dj.size() * 8),
             *wj = (uint64_t *)malloc(want_wj.size() * 8), *cj = (uint64_t *)malloc(want_cj.size() * 8), sizes[4];
    char why[200];
    const int code = rp_layout(n_q, q_seg.data(), win.data(), pack_count.data(), seq_cap, seq_off.data(), seq_len.data(), ref_size.data(), n_refs, out_off, at, dj, wj, cj, sizes,
                               why, sizeof why);
    char name[32];
    snprintf(name, sizeof name, "window %lld ", (long long)bad);
    auto same = [](const uint64_t *got, const std::vector<uint64_t> &want) { return want.empty() || !memcmp(got, want.data(), want.size() * 8); };
    const bool ok = code == (bad < 0 ? AGC_HIP_OK : AGC_HIP_EINVAL) && (bad < 0 || strstr(why, name)) && same(out_off, want_off) && same(at, want_at) &&
                    sizes[0] * 7 == want_dj.size() && sizes[1] * 7 == want_wj.size() && sizes[2] * 8 == want_cj.size() && sizes[3] == total && same(dj, want_dj) &&
                    same(wj, want_wj) && same(cj, want_cj);
    if (!ok)
        fprintf(stderr, "round %d: rp_layout of %llu windows in %u queries (first bad window %lld) gives code %d (%s) or other offsets or jobs than the plain recomputation\n", it,
                (unsigned long long)n_win, n_q, (long long)bad, code, why);
    free(out_off), free(at), free(dj), free(wj), free(cj);
    return ok;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1)
        rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ULL;
    const int rounds = argc > 2 ? atoi(argv[2]) : 2000;
    uint64_t n_win = 0, n_ctg = 0;
    for (int it = 0; it < rounds; ++it) {
        const uint32_t ref_size = 1 + rnd(it % 4 ? 300 : 3000), mml = 18 + rnd(4);
        std::vector<uint8_t> ref(ref_size), enc, want;
        for (auto &c : ref)
            c = rnd(40) ? rnd(4) : 4 + rnd(12);
        random_delta(ref, mml, enc, want);
        enc.shrink_to_fit(); // (exact-size heap blocks: the sanitizer sees one byte too far)
        const uint32_t len = (uint32_t)want.size();
        for (int w = 0; w < 12 && len; ++w) {
            const uint32_t a = w == 0 ? 0 : rnd(len), n = w == 0 ? len : 1 + rnd(w % 3 ? len - a : (len - a < 70 ? len - a : 70));
            for (int rc = 0; rc < 2; ++rc) {
                uint8_t *out = (uint8_t *)malloc(n);
                uint32_t strips = 0;
                const uint32_t st = ranges_decode_window(ref.data(), ref_size, mml, enc.data(), enc.size(), rc, a, n, out, &strips);
                if (st != 0) {
                    fprintf(stderr, "round %d: window [%u, +%u) of %u symbols is refused with %u\n", it, a, n, len, st);
                    return 1;
                }
                for (uint32_t q = 0; q < n; ++q) {
                    const uint8_t c = rc ? complement(want[len - 1 - (a + q)]) : want[a + q];
                    if (out[q] != c) {
                        fprintf(stderr, "round %d rc %d window [%u, +%u): symbol %u is %u, the plain walk has %u\n", it, rc, a, n, q, out[q], c);
                        return 1;
                    }
                }
                free(out);
                ++n_win;
            }
        }
        uint8_t one;
        if (ranges_decode_window(ref.data(), ref_size, mml, enc.data(), enc.size(), 0, len, 1, &one, nullptr) != 100) {
            fprintf(stderr, "round %d: a window one symbol past the delta's %u is not refused\n", it, len);
            return 1;
        }
        // a contig of random segments: the windows of a random range against a count position by position
        const uint32_t k = 1 + rnd(31), n_seg = 1 + rnd(6);
        std::vector<uint32_t> lengths(n_seg), seg(n_seg), wf(n_seg), wl(n_seg);
        std::vector<uint32_t> owner, inside; // per contig position: its segment, its offset in the oriented segment
        for (uint32_t s = 0; s < n_seg; ++s) {
            lengths[s] = (s ? k : 0) + rnd(4 * k);
            for (uint32_t i = s ? k : 0; i < lengths[s]; ++i)
                owner.push_back(s), inside.push_back(i);
        }
        const int64_t total = (int64_t)owner.size(), from = (int64_t)rnd((uint32_t)total + 8) - 3, to = (int64_t)rnd((uint32_t)total + 8) - 3;
        uint64_t n_sym = 0;
        const uint64_t n = ranges_contig_windows(n_seg, lengths.data(), k, from, to, seg.data(), wf.data(), wl.data(), &n_sym);
        int64_t lo = from < 0 ? 0 : from, hi = to < 0 ? total - 1 : to;
        if (to >= 0 && lo > hi)
            lo = 0, hi = total - 1;
        if (hi > total - 1)
            hi = total - 1;
        uint64_t p = (uint64_t)lo, sum = 0;
        for (uint64_t i = 0; i < n; ++i)
            for (uint32_t q = 0; q < (wl[i] ? wl[i] : 1); ++q, ++p, ++sum) // (an entry without symbols fails here too)
                if (!wl[i] || p >= owner.size() || owner[p] != seg[i] || inside[p] != wf[i] + q) {
                    fprintf(stderr, "round %d: window %llu of the range [%lld, %lld] is not the contig's positions\n", it, (unsigned long long)i, (long long)from, (long long)to);
                    return 1;
                }
        if (sum != n_sym || (int64_t)sum != (hi >= lo ? hi - lo + 1 : 0)) {
            fprintf(stderr, "round %d: the range [%lld, %lld] of %lld symbols yields %llu\n", it, (long long)from, (long long)to, (long long)total, (unsigned long long)sum);
            return 1;
        }
        ++n_ctg;
        if (!random_batch(it))
            return 1;
    }
    printf("ok %llu windows, %llu contigs, %d batches\n", (unsigned long long)n_win, (unsigned long long)n_ctg, rounds);
    return 0;
}
#endif
