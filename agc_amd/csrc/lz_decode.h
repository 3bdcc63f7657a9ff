// lz_decode.h -- the LZ-diff delta grammar and the scan that decodes it without a sequential walk (CLZDiff_V2::Decode,
// src/common/lz_diff.cpp:801-836).  The same source compiles for gfx950 (lz_decode_kernels.hip) and for the host
// (tests/lzdec_host emulates the kernels' order on the CPU and compares with the oracle).
//
// A delta is a sequence of tokens:
//   literal   one byte 'A' .. 'A' + 20 (the symbol code + 'A') or '!' (the symbol is ref[pred_pos])        -> 1 symbol
//   N-run     30, decimal digits v, 4                                                                     -> v + 4 symbols of code 4
//   match     [-]digits (diff), optionally ',' digits (l), '.'                                            -> ref[ref_pos, ref_pos + len)
//             ref_pos = pred_pos + diff; len = l + min_match_len, without ",l" the match runs to the end of the reference
// pred_pos starts at 0; a literal adds 1 to it, an N-run leaves it alone, a match sets it to ref_pos + len.
//
// Token starts: a byte starts a token iff it is byte 0 or the byte before it ends a token, and whether a byte ends a token is
// a property of that byte alone (a literal byte, '.', or the 4 that closes an N-run: none of them occurs inside a number).  One
// ballot per 64-byte strip gives the end bits, shifted by one with a bit carried from the strip before they are the start bits.
//
// pred_pos and the output offset in front of every token are a prefix "sum" over the tokens' Steps: a Step maps
// (pred_pos, out) to (pred_pos, out) of the next token, Steps compose (combine) associatively, so a wave scan over a strip's
// tokens plus the state carried from the strip before replaces the walk.
#pragma once
#include <stdint.h>
#include "sym_view.h"

namespace agc {
namespace lzd {

constexpr uint32_t STRIP = 64;      // delta bytes per step of a wave: one per lane
constexpr uint8_t NRUN_FIRST = 30;  // N_run_starter_code, lz_diff.h:35
constexpr uint8_t NRUN_LAST = 4;    // N_code closes the run's number
constexpr uint32_t NRUN_MIN = 4;    // min_Nrun_len, lz_diff.h:36
constexpr uint32_t MAX_DIGITS = 10; // of one number (a 32-bit position has at most 10)

enum Kind : uint32_t {
    NONE = 0,     // the byte starts no token
    LITERAL,      // n = the symbol
    LITERAL_REF,  // '!'
    NRUN,         // n = symbols
    MATCH,        // diff, n = symbols
    MATCH_TO_END, // diff
    BAD           // truncated, a number too long, or a byte that cannot stand where it stands
};

// status of a delta (pass 1)
enum Status : uint32_t { OK = 0, BAD_TOKEN = 1, BAD_LITERAL_REF = 2, BAD_MATCH = 3, TOO_LONG = 4 };

SV_HD bool is_literal(uint8_t c) { return (c >= 'A' && c <= 'A' + 20) || c == '!'; } // lz_diff.h:193-196
SV_HD bool ends_token(uint8_t c) { return is_literal(c) || c == '.' || c == NRUN_LAST; }

// start bits of a strip: ends = bit j set where byte j ends a token, valid = bit j set where byte j is inside the delta,
// carry = 1 when the byte in front of the strip ends a token (or the strip is the delta's first)
SV_HD uint64_t token_starts(uint64_t ends, uint64_t valid, uint32_t carry) { return ((ends << 1) | carry) & valid; }
SV_HD uint32_t starts_carry(uint64_t ends) { return (uint32_t)(ends >> (STRIP - 1)); }

struct Token {
    uint32_t kind;
    int64_t diff; // MATCH, MATCH_TO_END
    uint64_t n;   // LITERAL: the symbol; NRUN, MATCH: symbols
};

// decimal digits at p[i ...), at most MAX_DIGITS of them (none: 0, as read_int has it, lz_diff.h:264-280); false: too many
template <class P> SV_HD bool parse_number(P p, uint64_t avail, uint64_t &i, uint64_t &v)
{
    v = 0;
    for (uint32_t digits = 0; i < avail && p[i] >= '0' && p[i] <= '9'; ++i) {
        if (++digits > MAX_DIGITS)
            return false;
        v = v * 10 + (uint64_t)(p[i] - '0');
    }
    return true;
}

// the token that starts at p; reads p[0, avail) only (avail >= 1: the bytes left in the delta).  P: a pointer to bytes (a kernel
// passes one that names the global address space, as with the sym_view.h accessors)
template <class P> SV_HD Token parse_token(P p, uint64_t avail, uint32_t min_match_len)
{
    const Token bad = {BAD, 0, 0};
    const uint8_t c = p[0];
    if (c == '!')
        return {LITERAL_REF, 0, 0};
    if (is_literal(c))
        return {LITERAL, 0, (uint64_t)(c - 'A')};
    uint64_t i = 0, v;
    if (c == NRUN_FIRST) {
        i = 1;
        if (!parse_number(p, avail, i, v) || i >= avail || p[i] != NRUN_LAST)
            return bad;
        return {NRUN, 0, v + NRUN_MIN};
    }
    const bool neg = c == '-';
    i = neg ? 1 : 0;
    if (!parse_number(p, avail, i, v) || i >= avail)
        return bad;
    const int64_t diff = neg ? -(int64_t)v : (int64_t)v;
    if (p[i] == '.')
        return {MATCH_TO_END, diff, 0};
    if (p[i] != ',')
        return bad;
    ++i;
    if (!parse_number(p, avail, i, v) || i >= avail || p[i] != '.')
        return bad;
    return {MATCH, diff, v + min_match_len};
}

// (pred_pos, out) in front of a token
struct State {
    int64_t pred;
    uint64_t out;
};

// what a run of tokens does to a State.  set == 0: pred += p, out += o.  set == 1 (the run holds a match to the end of the
// reference, whose length depends on where it starts): pred = p, out += o - pred (the pred it was applied to).
// All arithmetic wraps (unsigned): the first bad token of a delta is found from exact values -- every token in front of it is
// valid, so pred_pos there is at most ref_size + the tokens so far -- and what wraps behind it is never used.
struct Step {
    uint32_t set;
    uint64_t p, o;
};

SV_HD Step identity() { return {0, 0, 0}; }

SV_HD Step step_of(const Token &t, uint32_t ref_size)
{
    switch (t.kind) {
    case LITERAL:
    case LITERAL_REF:
        return {0, 1, 1};
    case NRUN:
        return {0, 0, t.n};
    case MATCH:
        return {0, (uint64_t)t.diff + t.n, t.n};
    case MATCH_TO_END: // ref_pos = pred + diff, symbols = ref_size - ref_pos
        return {1, ref_size, (uint64_t)ref_size - (uint64_t)t.diff};
    default:
        return identity();
    }
}

// first a, then b
SV_HD Step combine(const Step &a, const Step &b)
{
    if (!b.set)
        return {a.set, a.p + b.p, a.o + b.o};
    return {1, b.p, a.o + b.o - a.p};
}

SV_HD State apply(const Step &s, const State &x)
{
    return {(int64_t)(s.set ? s.p : (uint64_t)x.pred + s.p), x.out + s.o - (s.set ? (uint64_t)x.pred : 0)};
}

// where a copying token reads the reference
SV_HD int64_t match_ref_pos(const Token &t, const State &before) { return (int64_t)((uint64_t)before.pred + (uint64_t)t.diff); }
SV_HD uint64_t match_symbols(const Token &t, const State &before, uint32_t ref_size)
{
    return t.kind == MATCH_TO_END ? (uint64_t)ref_size - (uint64_t)match_ref_pos(t, before) : t.n;
}

// a token against the State in front of it: OK, or why the delta is rejected
SV_HD uint32_t check_token(const Token &t, const State &before, uint32_t ref_size)
{
    if (t.kind == BAD)
        return BAD_TOKEN;
    if (t.kind == LITERAL_REF)
        return before.pred >= 0 && before.pred < (int64_t)ref_size ? OK : BAD_LITERAL_REF;
    if (t.kind == MATCH || t.kind == MATCH_TO_END) {
        const int64_t ref_pos = match_ref_pos(t, before);
        if (ref_pos < 0 || ref_pos > (int64_t)ref_size)
            return BAD_MATCH;
        return t.kind == MATCH && t.n > (uint64_t)ref_size - (uint64_t)ref_pos ? BAD_MATCH : OK;
    }
    return OK;
}

// the decoded length as a whole: it must fit 32 bits
SV_HD uint32_t check_length(uint64_t out) { return out >> 32 ? TOO_LONG : OK; }

// reverse_complement_copy (src/common/agc_basic.cpp:282-315) of one symbol
SV_HD uint8_t complement(uint8_t c) { return c < 4 ? (uint8_t)(3 - c) : c; }

} // namespace lzd
} // namespace agc
