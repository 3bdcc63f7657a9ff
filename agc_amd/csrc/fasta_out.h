// fasta_out.h -- the layout of a sample's FASTA text and the walk that fills 16 bytes of it (decompress_contig's stitching and the
// FASTA writer, src/common/agc_decompressor_lib.cpp:172-286, as arithmetic on offsets).  The same source compiles for gfx950
// (fasta_out_kernels.hip: one lane per 16-byte chunk of the text) and for the host (tests/fastaout_host runs the chunks in the
// kernel's order on the CPU and compares with text built independently).  No HIP calls.
//
// Text of one contig, as the host reader's append_fasta writes it:
//   '>' name '\n'                                                    the header: name_len + 2 bytes
//   the symbols in lines of L symbols, every line -- a last partial one too -- followed by '\n'
//   L = line_length, or the contig's symbol count when line_length == 0 (one line); a contig of 0 symbols is its header only.
// Body byte t (from 0 behind the header) lies in row t / (L + 1) at column t % (L + 1): column L is the line end, any other
// column holds symbol row * L + column -- unless that is the symbol count: then t is the line end of the last, partial line.
//
// Symbols: a contig is its segments back to back, every segment but the first without its first k symbols (the overlap with the
// segment in front).  In the sample's symbol buffer the segments lie whole, oriented; segment s of a contig starts at contig
// position seg_start[s] (the position of its first KEPT symbol), so contig position p inside it is
// sym[seg_off[s] + skip[s] + (p - seg_start[s])], skip = 0 for the contig's first segment and k for the others.  A segment that keeps
// nothing (exactly k symbols) has the seg_start of the segment behind it: the segment holding p is the LAST one whose start is <= p.
//
// All offsets are 64-bit: a human sample's text is more than 4 GiB.
#pragma once
#include <stdint.h>
#include "sym_view.h"

namespace agc {
namespace fo {

constexpr uint32_t CHUNK = 16; // text bytes per lane: one 16-byte store

// CNumAlphaConverter, agc_decompressor_lib.h:24-34 (codes >= 16 -> ' ')
SV_HD uint8_t letter(uint8_t c)
{
    // "ACGTNRYSWKMBDHVU", four letters per word (no table in memory: a kernel would read it through the constant cache per byte)
    const uint32_t w = c < 4 ? 0x54474341u : c < 8 ? 0x5359524Eu : c < 12 ? 0x424D4B57u : 0x55564844u;
    return c < 16 ? (uint8_t)(w >> (8 * (c & 3))) : (uint8_t)' ';
}

SV_HD uint64_t line_symbols(uint64_t n_sym, uint32_t line_length) { return line_length ? line_length : n_sym; }

// bytes of a contig's body: its symbols and one line end per line
SV_HD uint64_t body_bytes(uint64_t n_sym, uint32_t line_length)
{
    if (!n_sym)
        return 0;
    const uint64_t L = line_symbols(n_sym, line_length);
    return n_sym + (n_sym + L - 1) / L;
}

SV_HD uint64_t header_bytes(uint64_t name_len) { return name_len + 2; }

SV_HD uint64_t contig_text_bytes(uint64_t name_len, uint64_t n_sym, uint32_t line_length) { return header_bytes(name_len) + body_bytes(n_sym, line_length); }

// body byte t (< body_bytes) of a contig: true = a line end; false = it holds symbol `next`.  col / next: the byte's column and the
// symbol the walk is at (the symbol itself, or the first one of the next line), for a caller that goes on byte by byte
SV_HD bool body_locate(uint64_t t, uint64_t n_sym, uint64_t L, uint64_t &col, uint64_t &next)
{
    const uint64_t row = t / (L + 1);
    col = t % (L + 1);
    next = row * L + col;
    return col == L || next == n_sym;
}

// the inverse: body offset of symbol i
SV_HD uint64_t body_offset_of(uint64_t i, uint64_t L) { return i + i / L; }

// what the text kernel reads (P64 / P32 / P8: pointers to const uint64_t / uint32_t / uint8_t -- a kernel passes pointers that name
// the global address space, as with the sym_view.h accessors)
template <class P64, class P32, class P8> struct PlanT {
    P64 ctg_text;  // n_ctg + 1: text offset of every contig's '>', [n_ctg] = the text's size
    P64 ctg_seg;   // n_ctg + 1: contig c = segments [ctg_seg[c], ctg_seg[c + 1])
    P64 ctg_sym;   // n_ctg: symbols of the contig
    P64 name_off;  // n_ctg + 1: contig c's name = names[name_off[c], name_off[c + 1])
    P8 names;
    P64 seg_start; // per segment: contig position of its first kept symbol
    P64 seg_off;   // per segment: where it lies in sym
    P32 skip;      // per segment: 0 (a contig's first) or k
    P8 sym;        // the sample's symbol buffer
    uint32_t n_ctg;
    uint32_t line_length;
};

// last index i in [lo, hi) with a[i] <= x (a ascending, a[lo] <= x)
template <class P64> SV_HD uint64_t last_not_above(P64 a, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// text bytes [lo, lo + n), 1 <= n <= CHUNK, inside the text: byte i at bits [8 i, +7] of w0 (i < 8) or [8 (i - 8), +7] of w1.
// The contig is searched once, the segment once per contig the chunk touches; everything else walks forward.
template <class Plan> SV_HD void chunk_bytes(const Plan &P, uint64_t lo, uint32_t n, uint64_t &w0, uint64_t &w1)
{
    w0 = w1 = 0;
    uint64_t c = last_not_above(P.ctg_text, 0, P.n_ctg, lo);
    uint64_t rel = lo - P.ctg_text[c]; // offset inside the contig's text
    bool fresh = true;                 // the contig's numbers below have not been loaded yet
    uint64_t hdr = 0, end = 0, n_sym = 0, L = 0, name0 = 0, col = 0, p = 0, s = 0, s_end = 0, s_next = 0, src = 0;
    bool in_body = false, seg_known = false;
    for (uint32_t i = 0; i < n; ++i, ++rel) {
        if (!fresh && rel == end) { // the contig's text ends here: every contig has >= 2 bytes
            ++c;
            rel = 0;
            fresh = true;
        }
        if (fresh) {
            name0 = P.name_off[c];
            hdr = header_bytes(P.name_off[c + 1] - name0);
            n_sym = P.ctg_sym[c];
            L = line_symbols(n_sym, P.line_length);
            end = hdr + body_bytes(n_sym, P.line_length);
            in_body = seg_known = false;
            fresh = false;
        }
        uint8_t b;
        if (rel < hdr)
            b = rel == 0 ? (uint8_t)'>' : rel == hdr - 1 ? (uint8_t)'\n' : (uint8_t)P.names[name0 + rel - 1];
        else {
            bool line_end;
            if (!in_body) {
                line_end = body_locate(rel - hdr, n_sym, L, col, p);
                in_body = true;
            } else
                line_end = col == L || p == n_sym;
            if (line_end) {
                b = (uint8_t)'\n';
                col = 0;
            } else {
                if (!seg_known) {
                    s_end = P.ctg_seg[c + 1];
                    s = last_not_above(P.seg_start, P.ctg_seg[c], s_end, p);
                    seg_known = true;
                    s_next = s + 1 < s_end ? P.seg_start[s + 1] : ~(uint64_t)0;
                    src = P.seg_off[s] + P.skip[s] - P.seg_start[s];
                } else if (p >= s_next) {
                    while (s + 1 < s_end && P.seg_start[s + 1] <= p) // (segments that keep nothing are stepped over)
                        ++s;
                    s_next = s + 1 < s_end ? P.seg_start[s + 1] : ~(uint64_t)0;
                    src = P.seg_off[s] + P.skip[s] - P.seg_start[s];
                }
                b = letter(P.sym[src + p]);
                ++p;
                ++col;
            }
        }
        if (i < 8)
            w0 |= (uint64_t)b << (8 * i);
        else
            w1 |= (uint64_t)b << (8 * (i - 8));
    }
}

// chunk j of a text whose first byte lies at an address with (address & 15) == a: the text bytes [begin, begin + n) it covers
// (chunk 0 is short when a != 0, the last one when the text ends inside it)
SV_HD void chunk_range(uint64_t j, uint32_t a, uint64_t total, uint64_t &begin, uint32_t &n)
{
    const uint64_t b = j * CHUNK, lo = b < a ? 0 : b - a, hi = b + CHUNK - a < total ? b + CHUNK - a : total;
    begin = lo;
    n = (uint32_t)(hi - lo);
}
SV_HD uint64_t chunk_count(uint32_t a, uint64_t total) { return total ? (total + a + CHUNK - 1) / CHUNK : 0; }

} // namespace fo
} // namespace agc
