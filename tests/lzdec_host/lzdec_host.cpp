// lzdec_host.cpp -- agc_amd/csrc/lz_decode.h on the CPU, in the order of the kernels of lz_decode_kernels.hip: strips of 64
// bytes, the token starts from the end bits with the carried bit, the scan of the Steps (the same doubling steps the wave makes)
// with the State carried between strips, pass 1 (length + status), then pass 2 (write by index).  TEST INFRASTRUCTURE ONLY.
// The reference is a plain byte array here: the 2-bit accessors pass 2 reads it through on the device are checked by
// tests/symview_host.
//   -DLZDEC_MAIN: a stand-alone program (no Python): random deltas over the grammar's bytes, the scan against a plain
//   token-by-token walk; built with -fsanitize=address,undefined it also shows that no delta makes the walk leave its buffers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../agc_amd/csrc/lz_decode.h"

using namespace agc::lzd;

namespace {

constexpr uint32_t LANES = STRIP;

// visit(tokens[64], states[64]) once per strip; false stops the walk
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

uint32_t pass1(uint32_t ref_size, uint32_t min_match_len, const uint8_t *enc, uint64_t enc_len, uint64_t *out_len)
{
    uint32_t status = OK;
    const State end = walk_delta(enc, enc_len, ref_size, min_match_len, [&](const Token *t, const State *before) {
        for (uint32_t lane = 0; lane < LANES; ++lane)
            if (t[lane].kind != NONE && (status = check_token(t[lane], before[lane], ref_size)) != OK)
                return false; // the first bad token's
        return true;
    });
    if (status == OK)
        status = check_length(end.out);
    *out_len = end.out;
    return status;
}

void pass2(const uint8_t *ref, uint32_t ref_size, uint32_t min_match_len, const uint8_t *enc, uint64_t enc_len, int rc, uint8_t *out, uint32_t total)
{
    walk_delta(enc, enc_len, ref_size, min_match_len, [&](const Token *t, const State *before) {
        for (uint32_t lane = 0; lane < LANES; ++lane) {
            const Token &k = t[lane];
            const uint32_t at = (uint32_t)before[lane].out;
            if (k.kind == LITERAL || k.kind == LITERAL_REF) {
                const uint8_t c = k.kind == LITERAL ? (uint8_t)k.n : ref[before[lane].pred];
                out[rc ? total - 1 - at : at] = rc ? complement(c) : c;
            } else if (k.kind == NRUN || k.kind == MATCH || k.kind == MATCH_TO_END) {
                const uint32_t n = (uint32_t)match_symbols(k, before[lane], ref_size);
                const uint64_t ref_pos = (uint64_t)match_ref_pos(k, before[lane]);
                for (uint32_t q = 0; q < n; ++q) {
                    const uint8_t c = k.kind == NRUN ? 4 : ref[ref_pos + q];
                    out[rc ? total - 1 - (at + q) : at + q] = rc ? complement(c) : c;
                }
            }
        }
        return true;
    });
}

} // namespace

// -> the delta's status (0: well formed); *out_len = the decoded length; the symbols go to out when it is well formed and cap holds them
extern "C" uint32_t lzdec_decode(const uint8_t *ref, uint32_t ref_size, uint32_t min_match_len, const uint8_t *enc, uint64_t enc_len, int rc, uint8_t *out,
                                 uint64_t cap, uint64_t *out_len)
{
    const uint32_t status = pass1(ref_size, min_match_len, enc, enc_len, out_len);
    if (status == OK && *out_len <= cap)
        pass2(ref, ref_size, min_match_len, enc, enc_len, rc, out, (uint32_t)*out_len);
    return status;
}

#ifdef LZDEC_MAIN
namespace {

// the plain walk: token after token, every check where Decode (lz_diff.cpp:801-836) would step outside
uint32_t plain_decode(const std::vector<uint8_t> &ref, uint32_t mml, const std::vector<uint8_t> &enc, std::vector<uint8_t> &out)
{
    out.clear();
    int64_t pred = 0;
    for (size_t p = 0; p < enc.size();) {
        const Token t = parse_token(enc.data() + p, enc.size() - p, mml);
        if (t.kind == BAD)
            return BAD_TOKEN;
        size_t e = p;
        while (!ends_token(enc[e]))
            ++e; // (a token that parsed has its end byte)
        p = e + 1;
        if (t.kind == LITERAL || t.kind == LITERAL_REF) {
            if (t.kind == LITERAL_REF && pred >= (int64_t)ref.size())
                return BAD_LITERAL_REF;
            out.push_back(t.kind == LITERAL ? (uint8_t)t.n : ref[pred]);
            ++pred;
        } else if (t.kind == NRUN) {
            if ((out.size() + t.n) >> 32)
                return TOO_LONG;
            out.insert(out.end(), t.n, 4);
        } else {
            const int64_t ref_pos = pred + t.diff;
            if (ref_pos < 0 || ref_pos > (int64_t)ref.size())
                return BAD_MATCH;
            const uint64_t n = t.kind == MATCH ? t.n : ref.size() - ref_pos;
            if (n > ref.size() - ref_pos)
                return BAD_MATCH;
            out.insert(out.end(), ref.begin() + ref_pos, ref.begin() + ref_pos + n);
            pred = ref_pos + n;
        }
    }
    return out.size() >> 32 ? TOO_LONG : OK;
}

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

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1)
        rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ULL;
    const int rounds = argc > 2 ? atoi(argv[2]) : 20000;
    uint64_t n_ok = 0, n_bad = 0;
    for (int it = 0; it < rounds; ++it) {
        const uint32_t ref_size = 1 + rnd(it % 4 ? 300 : 3000), mml = rnd(4) ? 18 + rnd(4) : rnd(3);
        std::vector<uint8_t> ref(ref_size);
        for (auto &c : ref)
            c = rnd(40) ? rnd(4) : 4 + rnd(12);
        // mostly well-formed tokens that stay inside the reference, now and then one that does not, or a stray byte
        std::vector<uint8_t> enc;
        int64_t pred = 0;
        const uint32_t n_tok = rnd(it % 3 ? 40 : 200);
        for (uint32_t k = 0; k < n_tok; ++k) {
            const uint32_t kind = rnd(100);
            if (kind < 45) {
                enc.push_back(rnd(6) ? 'A' + rnd(21) : '!');
                ++pred;
            } else if (kind < 55) {
                enc.push_back(NRUN_FIRST);
                put_number(enc, rnd(50));
                enc.push_back(NRUN_LAST);
            } else if (kind < 95) {
                const bool wild = rnd(60) == 0;
                const int64_t ref_pos = wild ? (int64_t)rnd(2 * ref_size) - (int64_t)(ref_size / 2) : (int64_t)rnd(ref_size + 1);
                const int64_t diff = ref_pos - pred;
                if (diff < 0)
                    enc.push_back('-');
                put_number(enc, (uint64_t)(diff < 0 ? -diff : diff));
                const uint64_t room = ref_pos >= 0 && ref_pos <= (int64_t)ref_size ? ref_size - ref_pos : 0;
                if (rnd(8) && room >= mml) {
                    const uint64_t n = mml + rnd((uint32_t)(room - mml) + (wild ? 3 : 1));
                    enc.push_back(',');
                    put_number(enc, n - mml);
                    pred = ref_pos + (int64_t)n;
                } else
                    pred = ref_size;
                enc.push_back('.');
            } else {
                static const uint8_t stray[] = {'Z', 0, ',', '.', '-', '7', NRUN_FIRST, NRUN_LAST, '!', 200};
                enc.push_back(stray[rnd(sizeof stray)]);
            }
        }
        if (rnd(10) == 0 && !enc.empty())
            enc.resize(rnd((uint32_t)enc.size())); // truncated
        if (rnd(50) == 0)
            for (int d = 0; d < 12; ++d)
                enc.push_back('0' + rnd(10)); // a number too long, and no end
        std::vector<uint8_t> want, enc_exact(enc); // (exact-size heap blocks: the sanitizer sees one byte too far)
        enc_exact.shrink_to_fit();
        const uint32_t st_want = plain_decode(ref, mml, enc_exact, want);
        for (int rc = 0; rc < 2; ++rc) {
            uint64_t len = 0;
            uint32_t st = lzdec_decode(ref.data(), ref_size, mml, enc_exact.data(), enc_exact.size(), rc, nullptr, 0, &len);
            if (st != st_want || (st == OK && len != want.size())) {
                fprintf(stderr, "round %d: status %u (plain walk: %u), length %llu (%zu)\n", it, st, st_want, (unsigned long long)len, want.size());
                return 1;
            }
            if (st != OK)
                continue;
            uint8_t *out = (uint8_t *)malloc(len ? len : 1);
            st = lzdec_decode(ref.data(), ref_size, mml, enc_exact.data(), enc_exact.size(), rc, out, len, &len);
            for (uint64_t q = 0; q < len; ++q) {
                const uint8_t c = rc ? complement(want[len - 1 - q]) : want[q];
                if (out[q] != c) {
                    fprintf(stderr, "round %d rc %d: symbol %llu is %u, the plain walk has %u\n", it, rc, (unsigned long long)q, out[q], c);
                    return 1;
                }
            }
            free(out);
        }
        (st_want == OK ? n_ok : n_bad)++;
    }
    printf("ok %llu well-formed, %llu rejected\n", (unsigned long long)n_ok, (unsigned long long)n_bad);
    return 0;
}
#endif
