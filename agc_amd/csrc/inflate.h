// inflate.h -- a BGZF stream back into its bytes: the inverse of bgzf.h, and of every other writer of the format (`bgzip`, htslib).
// BGZF (SAM specification, 4.1) is multi-member gzip (RFC 1952) whose members stand alone and say how large they are: the extra
// subfield 'B' 'C' holds BSIZE = member size - 1, the trailer the CRC-32 and the size (ISIZE <= 65536) of the member's bytes.  So the
// host finds every member without inflating anything (walk), and every member is inflated (RFC 1951) by one wavefront
// (inflate_member).  One source for the host (g++, tests only: tests/inflate_host) and the device (hipcc: inflate_kernels.hip).  No
// HIP calls.
//
// (a) walk(): host arithmetic.  From byte 0, member by member: ID1 ID2, CM, FLG, the extra field subfield by subfield up to 'B' 'C'
// with SLEN 2, FNAME / FCOMMENT / FHCRC skipped when set, BSIZE, the trailer -> Job {payload offset, payload bytes, text offset,
// ISIZE, CRC}; the text offsets are the prefix sums of ISIZE.  The first complaint stops the walk:
//   UNSUPPORTED  CM != 8; reserved FLG bits; no FEXTRA or no 'B' 'C' subfield (plain gzip: the member's size is unknown)
//   MALFORMED    fewer bytes than a header / the extra field / a name's terminator / FHCRC need (this is also what bytes left over
//                behind the last member are); ID1 ID2 not 1f 8b; a subfield past the end of the extra field; BSIZE + 1 smaller than
//                header + trailer; BSIZE + 1 past the input; ISIZE > 65536
// The 28-byte EOF member is a member like any other (ISIZE 0); a stream without it is a stream (`gzip -d` reads it), and so is every
// slice of a stream that begins and ends on member boundaries.
//
// (b) inflate_member(): one wavefront of LANES lanes, written as one program every lane runs (as zstd/zs_decode.h is):
//   - what only READS the payload (block headers, the symbol chain, lengths and distances) is computed by all lanes alike;
//   - a code's tables are built by lane 0 alone (`if (ln.lane == 0)`) and left in the fast memory (Work: the LDS), for a dynamic
//     block after lane 0 has read the code lengths; INF_WAVE_SYNC() stands between that and the lanes that read it;
//   - the bytes move on all lanes: a stored block and a match are copies in strips of LANES bytes, a match whose distance is below
//     LANES the periodic copy dst[i] = period[i % distance]; decoded literals gather in a strip of registers (lane i keeps literal
//     i; the host build: an array) that is flushed across the lanes when it is full and in front of every match, stored block and
//     the end;
//   - the CRC-32 of the output: lane i takes slice i of LANES, moves its value to the end by x^(8 * bytes behind it) mod P and the
//     values are xor-ed (bgzf.h's mulmod; the powers by square-and-multiply, that header's xpow8 reading a table inside its Work).
// The host build runs the same program with one "lane 0" and the lane sections as loops over the 64 lanes.
//
// Tables: canonical codes (RFC 1951, 3.2.2) as count[16] + the symbols sorted by (length, symbol), in front of them a first-level
// look-up of LIT_FAST = 9 / DIST_FAST = 8 bits (entry: symbol | length << 9, 0: not in it) that resolves every code up to that
// length in one read; longer codes walk count[] bit by bit.  Work is 3 932 bytes a wave.
//
// Bounded memory access: a member is (src, n), (dst, isize), (Work).  load64() is the only reader of src at a computed offset and
// pads with zeros behind n.  Every index formed from payload bits is checked against the array it goes into first: a symbol is < the
// size of its alphabet by construction of the tables (sym[] holds only symbols < n), a run of code lengths is checked against HLIT +
// HDIST, a distance is checked against the bytes this member has produced and a length against isize before any address is formed.
// A member that fails has written nothing outside dst[0, isize).  Every loop names its bound.
//
// What is refused (MALFORMED; Why names the check):
//   block type 3; a stored block's LEN != ~NLEN; HLIT > 286 or HDIST > 30 (as zlib refuses them); a repeat code 16 with no length in
//   front of it; a run of lengths past HLIT + HDIST; no code for end-of-block; an over-subscribed code; an incomplete code -- except,
//   as in zlib, a distance code that is one code of length 1, and a distance code without any code (a match that then follows is
//   refused: bits that are no code); bits that are no code of an incomplete distance code; literal/length symbol 286 / 287 or distance
//   symbol 30 / 31 decoded; a distance beyond the bytes produced; output past ISIZE; output short of ISIZE; the payload exhausted (a
//   bit read behind its end); payload left over (more than the 7 padding bits); CRC-32 mismatch.
// Stricter than zlib: an incomplete literal/length code of a single one-bit code, and a code-length code without any code, pass
// zlib's table builder (the second is refused later, for the missing end-of-block); here both are incomplete codes.  zlib checks
// neither ISIZE nor the CRC nor that the payload ends (gzip's framing does).  Whatever this decoder accepts, zlib decodes to the
// same bytes (tests/test_inflate_host.py, and the sanitizer harness against zlib's inflate).
//
// The includer may define, before including this header (the kernel does; the host needs none):
//   INF_WAVE_SYNC()   orders a lane's stores (Work, dst) before the other lanes' loads of them
#pragma once
#include <stdint.h>

#include "bgzf.h"

#ifndef INF_WAVE_SYNC
#define INF_WAVE_SYNC() ((void)0)
#endif
// a section every lane runs with its own lane number l (host: a loop over the lanes)
#if defined(__HIP_DEVICE_COMPILE__)
#define INF_EACH_LANE(ln, l)                                                                                                                \
    {                                                                                                                                       \
        const uint32_t l = (ln).lane;                                                                                                       \
        {
#else
#define INF_EACH_LANE(ln, l)                                                                                                                \
    {                                                                                                                                       \
        for (uint32_t l = 0; l < LANES; ++l) {
#endif
#define INF_END_LANES                                                                                                                       \
    }                                                                                                                                       \
    }
#define INF_FN BGZF_FN

namespace agc {
namespace inflate {

// per member; 0 = inflated.  (include/agc_hip.h: AGC_HIP_INF_*)
enum Status : uint32_t { OK = 0, UNSUPPORTED = 1, MALFORMED = 2 };

// which check refused (the tests see it through tests/inflate_host; the device reports the Status alone)
enum Why : uint32_t {
    W_OK = 0,
    // the walk
    W_HEADER_TRUNCATED, W_MAGIC, W_METHOD, W_FLAGS, W_NO_BC, W_SUBFIELD, W_BSIZE_SMALL, W_BSIZE_PAST, W_ISIZE,
    // the member
    W_BLOCK_TYPE, W_STORED_LEN, W_HLIT, W_HDIST, W_REPEAT_FIRST, W_RUN_PAST, W_NO_EOB, W_OVERSUBSCRIBED, W_INCOMPLETE, W_NO_CODE, W_LITLEN_SYMBOL,
    W_DIST_SYMBOL, W_DISTANCE, W_OUT_PAST, W_OUT_SHORT, W_EXHAUSTED, W_LEFT_OVER, W_CRC,
};
INF_FN uint32_t status_of(uint32_t why) { return why == W_OK ? OK : why == W_METHOD || why == W_FLAGS || why == W_NO_BC ? UNSUPPORTED : MALFORMED; }

constexpr uint32_t LANES = 64;
constexpr uint32_t ISIZE_MAX = 65536;
constexpr uint32_t HEADER_MIN = 18, TRAILER = 8; // the fixed header with the BC subfield alone; CRC-32 + ISIZE
constexpr uint32_t LIT_FAST = 9, DIST_FAST = 8, CL_FAST = 7, MAX_BITS = 15;
constexpr uint32_t N_LITLEN = 288, N_DIST = 32, N_CL = 19; // the alphabets' sizes (fixed codes name 286 / 287 and 30 / 31)
constexpr uint32_t NO_SYM = 0xFFFFu;

// ---- (a) the walk ---------------------------------------------------------------------------------------------------------------
struct Job {
    uint64_t src_off; // the deflate payload: in[src_off, src_off + src_len)
    uint64_t out_off; // its bytes: text[out_off, out_off + out_len)
    uint32_t src_len, out_len; // out_len = ISIZE
    uint32_t crc;     // of those bytes, as the trailer has it
    uint32_t pad;
};

struct Walk {
    uint32_t why;        // W_OK, or the first complaint: member n_members, the byte `at` of the stream
    uint64_t n_members;  // members walked without a complaint
    uint64_t text_bytes; // the sum of their ISIZE
    uint64_t at;
};

INF_FN uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
INF_FN uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }

// the member at in[p, n): its job (out_off left to the caller) and its size -> W_OK or the complaint
INF_FN uint32_t walk_member(const uint8_t *in, uint64_t n, uint64_t p, Job &jb, uint64_t &size)
{
    if (n - p < 12)
        return W_HEADER_TRUNCATED;
    if (in[p] != 0x1f || in[p + 1] != 0x8b)
        return W_MAGIC;
    if (in[p + 2] != 8)
        return W_METHOD;
    const uint32_t flg = in[p + 3];
    if (flg & 0xE0)
        return W_FLAGS;
    if (!(flg & 4))
        return W_NO_BC;
    const uint64_t xlen = le16(in + p + 10);
    uint64_t q = p + 12;
    if (n - q < xlen)
        return W_HEADER_TRUNCATED;
    const uint64_t xend = q + xlen;
    bool found = false;
    uint32_t bsize = 0;
    while (q < xend) { // (a subfield is 4 bytes at least: <= xlen / 4 rounds)
        if (xend - q < 4)
            return W_SUBFIELD;
        const uint32_t slen = le16(in + q + 2);
        if (xend - q - 4 < slen)
            return W_SUBFIELD;
        if (!found && in[q] == 'B' && in[q + 1] == 'C' && slen == 2) {
            found = true;
            bsize = le16(in + q + 4);
        }
        q += 4 + slen;
    }
    if (!found)
        return W_NO_BC;
    for (uint32_t name = 8; name <= 16; name <<= 1) // FNAME, FCOMMENT: zero-terminated
        if (flg & name) {
            while (q < n && in[q]) // (n - q)
                ++q;
            if (q == n)
                return W_HEADER_TRUNCATED;
            ++q;
        }
    if (flg & 2) { // FHCRC
        if (n - q < 2)
            return W_HEADER_TRUNCATED;
        q += 2;
    }
    size = (uint64_t)bsize + 1;
    if (size < q - p + TRAILER)
        return W_BSIZE_SMALL;
    if (n - p < size)
        return W_BSIZE_PAST;
    const uint8_t *t = in + p + size - TRAILER;
    if (le32(t + 4) > ISIZE_MAX)
        return W_ISIZE;
    jb.src_off = q;
    jb.out_off = 0;
    jb.src_len = (uint32_t)(size - (q - p) - TRAILER);
    jb.out_len = le32(t + 4);
    jb.crc = le32(t);
    jb.pad = 0;
    return W_OK;
}

// the stream in[0, n) -> W; jobs (NULL: only count) receives the first `cap` members' jobs
INF_FN void walk(const uint8_t *in, uint64_t n, Job *jobs, uint64_t cap, Walk &W)
{
    W.why = W_OK;
    W.n_members = W.text_bytes = W.at = 0;
    uint64_t p = 0;
    while (p < n) { // (a member is HEADER_MIN + TRAILER bytes at least: <= n / 26 rounds)
        Job jb;
        uint64_t size = 0;
        W.at = p;
        W.why = walk_member(in, n, p, jb, size);
        if (W.why != W_OK)
            return;
        jb.out_off = W.text_bytes;
        if (jobs && W.n_members < cap)
            jobs[W.n_members] = jb;
        W.n_members += 1;
        W.text_bytes += jb.out_len;
        p += size;
    }
    W.at = n;
}

// ---- (b) one member ---------------------------------------------------------------------------------------------------------------
struct Lane {
    uint32_t lane; // device: the lane's number in its wave; host: 0
};

// the fast memory of one member (device: the wave's LDS)
struct Work {
    uint16_t lfast[1u << LIT_FAST], lsym[N_LITLEN], lcount[16];  // the literal/length code (and, while a dynamic block's lengths are read, the code-length code)
    uint16_t dfast[1u << DIST_FAST], dsym[N_DIST], dcount[16];   // the distance code
    uint16_t offs[16], next[16];                                 // build_code: where a length's symbols go in sym[]; its next code
    uint8_t lens[N_LITLEN + N_DIST];                             // the code lengths of a block: HLIT, then HDIST
    uint8_t cl[N_CL + 1];
    uint32_t crc_tab[256];
    uint32_t part[LANES]; // the lanes' CRC parts
    uint32_t res[2];      // what lane 0 found, for every lane to read: Why, the bit position behind the block's header
};

// the little-endian bytes [off, off + 8) of p[0, size), zeros behind size
INF_FN uint64_t load64(const uint8_t *p, uint32_t size, uint32_t off)
{
    uint64_t w = 0;
    if ((uint64_t)off + 8 <= size) {
        __builtin_memcpy(&w, p + off, 8);
        return w;
    }
    for (uint32_t k = 0; k < 8; ++k) // (8)
        if ((uint64_t)off + k < size)
            w |= (uint64_t)p[off + k] << (8 * k);
    return w;
}
// the 57 bits or more from bit `pos` on (bit 0 of a byte first: deflate's order)
INF_FN uint64_t peek(const uint8_t *p, uint32_t size, uint32_t pos) { return load64(p, size, pos >> 3) >> (pos & 7); }

// lens[0, n) -> the code's count[], sym[] and first-level table of `fbits` bits (lane 0).  dist: the distance code's two exceptions.
INF_FN uint32_t build_code(Work &w, const uint8_t *lens, uint32_t n, uint16_t *fast, uint32_t fbits, uint16_t *count, uint16_t *sym, bool dist)
{
    for (uint32_t b = 0; b <= MAX_BITS; ++b) // (16)
        count[b] = 0;
    for (uint32_t s = 0; s < n; ++s) // (n <= 288; a length is <= 15: four bits of lens' writers, or a symbol < 16)
        count[lens[s]] += 1;
    for (uint32_t i = 0; i < (1u << fbits); ++i) // (512)
        fast[i] = 0;
    int left = 1;
    uint32_t code = 0, at = 0;
    for (uint32_t b = 1; b <= MAX_BITS; ++b) { // (15)
        left = (left << 1) - (int)count[b];
        if (left < 0)
            return W_OVERSUBSCRIBED;
        code = (code + (b > 1 ? count[b - 1] : 0)) << 1;
        w.next[b] = (uint16_t)code;
        w.offs[b] = (uint16_t)at;
        at += count[b];
    }
    if (left > 0 && !(dist && (at == 0 || (at == 1 && count[1] == 1))))
        return W_INCOMPLETE;
    for (uint32_t s = 0; s < n; ++s) { // (n)
        const uint32_t l = lens[s];
        if (!l)
            continue;
        sym[w.offs[l]++] = (uint16_t)s; // (offs[l] < at <= n: every symbol has one place)
        const uint32_t c = w.next[l]++;
        if (l <= fbits)
            for (uint32_t k = bgzf::bit_reverse(c, l); k < (1u << fbits); k += 1u << l) // (2^(fbits - l); over a code: <= 2^fbits)
                fast[k] = (uint16_t)(s | l << 9);
    }
    return W_OK;
}

// the symbol whose code the low bits of `bits` begin with, its length in `used` -> NO_SYM: no code of this (incomplete) code
INF_FN uint32_t decode_sym(const uint16_t *fast, uint32_t fbits, const uint16_t *count, const uint16_t *sym, uint64_t bits, uint32_t &used)
{
    const uint32_t e = fast[(uint32_t)bits & ((1u << fbits) - 1)];
    if (e) {
        used = e >> 9;
        return e & 511;
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t b = 1; b <= MAX_BITS; ++b) { // (15)
        code |= (uint32_t)(bits >> (b - 1)) & 1;
        const uint32_t cnt = count[b];
        if (code < first + cnt) {
            used = b;
            return sym[index + (code - first)]; // (index + code - first < the code's symbols)
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    used = 0;
    return NO_SYM;
}

// lane 0: the header of a dynamic block behind HLIT / HDIST / HCLEN (at bit `pos`) -> the two codes; pos behind the header
INF_FN uint32_t read_dynamic(Work &w, const uint8_t *src, uint32_t n, uint32_t &pos, uint32_t hlit, uint32_t hdist, uint32_t hclen)
{
    for (uint32_t i = 0; i < N_CL; ++i) // (19)
        w.cl[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i, pos += 3) // (hclen <= 19)
        w.cl[bgzf::cl_order(i)] = (uint8_t)(peek(src, n, pos) & 7);
    if (pos > 8 * n)
        return W_EXHAUSTED;
    uint32_t why = build_code(w, w.cl, N_CL, w.lfast, CL_FAST, w.lcount, w.lsym, false);
    if (why)
        return why;
    const uint32_t total = hlit + hdist;
    for (uint32_t i = 0; i < total;) { // (i grows in every round: <= total <= 316)
        if (pos > 8 * n)
            return W_EXHAUSTED;
        uint64_t bits = peek(src, n, pos);
        uint32_t used;
        const uint32_t s = decode_sym(w.lfast, CL_FAST, w.lcount, w.lsym, bits, used);
        if (s == NO_SYM)
            return W_NO_CODE; // (not reached: the code-length code is complete)
        bits >>= used;
        pos += used;
        if (s < 16) {
            w.lens[i++] = (uint8_t)s;
            continue;
        }
        uint32_t v = 0, rep;
        if (s == 16) {
            if (i == 0)
                return W_REPEAT_FIRST;
            v = w.lens[i - 1];
            rep = 3 + ((uint32_t)bits & 3);
            pos += 2;
        } else if (s == 17) {
            rep = 3 + ((uint32_t)bits & 7);
            pos += 3;
        } else {
            rep = 11 + ((uint32_t)bits & 127);
            pos += 7;
        }
        if (i + rep > total)
            return W_RUN_PAST;
        for (; rep; --rep) // (<= 138)
            w.lens[i++] = (uint8_t)v;
    }
    if (pos > 8 * n)
        return W_EXHAUSTED;
    if (w.lens[256] == 0)
        return W_NO_EOB;
    why = build_code(w, w.lens, hlit, w.lfast, LIT_FAST, w.lcount, w.lsym, false);
    return why ? why : build_code(w, w.lens + hlit, hdist, w.dfast, DIST_FAST, w.dcount, w.dsym, true);
}

// lane 0: the codes of a fixed block (RFC 1951, 3.2.6)
INF_FN uint32_t fixed_codes(Work &w)
{
    for (uint32_t s = 0; s < N_LITLEN; ++s) // (288)
        w.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = 0; s < N_DIST; ++s) // (32)
        w.lens[N_LITLEN + s] = 5;
    const uint32_t why = build_code(w, w.lens, N_LITLEN, w.lfast, LIT_FAST, w.lcount, w.lsym, false);
    return why ? why : build_code(w, w.lens + N_LITLEN, N_DIST, w.dfast, DIST_FAST, w.dcount, w.dsym, true);
}

// the decoded literals not yet written: literal i of the strip is lane i's
struct Strip {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t v;
#else
    uint8_t v[LANES];
#endif
    uint32_t n;
};
INF_FN void strip_put(const Lane &ln, Strip &s, uint32_t byte)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (ln.lane == s.n)
        s.v = byte;
#else
    (void)ln;
    s.v[s.n] = (uint8_t)byte;
#endif
    s.n += 1;
}
// the strip to dst[op, op + s.n) (the caller has checked op + s.n <= isize)
INF_FN void strip_flush(const Lane &ln, Strip &s, uint8_t *dst, uint32_t &op)
{
    INF_EACH_LANE(ln, l)
    if (l < s.n)
#if defined(__HIP_DEVICE_COMPILE__)
        dst[op + l] = (uint8_t)s.v;
#else
        dst[op + l] = s.v[l];
#endif
    INF_END_LANES
    op += s.n;
    s.n = 0;
}

// dst[i] = dst[i - dist], i = 0 .. n - 1, 1 <= dist <= the bytes in front of dst: a strip reads only bytes in front of itself (dist
// >= LANES), or the match is the period dst[-dist, 0) repeated (dist < LANES: lane i reads period[i % dist], all of it in front of dst)
INF_FN void wave_match(const Lane &ln, uint8_t *dst, uint32_t dist, uint32_t n)
{
    const uint8_t *const period = dst - dist;
    for (uint32_t c = 0; c < n; c += LANES) { // (n / LANES <= 5)
        INF_EACH_LANE(ln, l)
        const uint32_t i = c + l;
        if (i < n)
            dst[i] = dist >= LANES ? period[i] : period[i % dist];
        INF_END_LANES
        if (dist >= LANES)
            INF_WAVE_SYNC(); // (the next strip may read this one)
    }
}

// x^(8 m) mod P
INF_FN uint32_t xpow8(uint32_t m)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u; // x^0; x^8
    for (; m; m >>= 1) {                        // (<= 17 rounds: m <= 65536)
        if (m & 1)
            p = bgzf::mulmod(p, sq);
        sq = bgzf::mulmod(sq, sq);
    }
    return p;
}

// the member's payload src[0, n) -> dst[0, isize), whose CRC-32 is crc_want -> W_OK or the check that refused it
INF_FN uint32_t inflate_member(const Lane &ln, Work &w, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t isize, uint32_t crc_want)
{
    if (isize > ISIZE_MAX || n > (1u << 24))
        return W_ISIZE; // (the walk lets neither through; pos below stays far from 2^32)
    INF_EACH_LANE(ln, l)
    for (uint32_t k = 0; k < 4; ++k) { // (4)
        uint32_t c = 4 * l + k;
        for (uint32_t r = 0; r < 8; ++r) // (8)
            c = (c >> 1) ^ ((c & 1) ? bgzf::CRC_POLY : 0);
        w.crc_tab[4 * l + k] = c;
    }
    INF_END_LANES
    uint32_t pos = 0, op = 0, last = 0;
    Strip strip;
    strip.n = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    strip.v = 0;
#endif
    do { // (a block takes 3 bits at least and pos <= 8 n is checked: <= 8 n / 3 + 1 rounds)
        if (pos + 3 > 8 * n)
            return W_EXHAUSTED;
        const uint32_t head = (uint32_t)peek(src, n, pos) & 7, type = head >> 1;
        last = head & 1;
        pos += 3;
        if (type == 3)
            return W_BLOCK_TYPE;
        if (type == 0) {
            const uint32_t at = (pos + 7) >> 3;
            if (at + 4 > n)
                return W_EXHAUSTED;
            const uint32_t v = (uint32_t)load64(src, n, at), len = v & 0xFFFF;
            if (len != (~(v >> 16) & 0xFFFF))
                return W_STORED_LEN;
            if (at + 4 + len > n)
                return W_EXHAUSTED;
            if (op + strip.n + len > isize)
                return W_OUT_PAST;
            strip_flush(ln, strip, dst, op);
            for (uint32_t c = 0; c < len; c += LANES) // (len / LANES)
                INF_EACH_LANE(ln, l)
                if (c + l < len)
                    dst[op + c + l] = (uint8_t)load64(src, n, at + 4 + c + l);
                INF_END_LANES
            op += len;
            pos = 8 * (at + 4 + len);
            continue;
        }
        uint32_t hlit = 0, hdist = 0, hclen = 0;
        if (type == 2) {
            if (pos + 14 > 8 * n)
                return W_EXHAUSTED;
            const uint32_t h = (uint32_t)peek(src, n, pos);
            hlit = 257 + (h & 31);
            hdist = 1 + ((h >> 5) & 31);
            hclen = 4 + ((h >> 10) & 15);
            pos += 14;
            if (hlit > 286)
                return W_HLIT;
            if (hdist > 30)
                return W_HDIST;
        }
        INF_WAVE_SYNC(); // (the tables are read no more)
        if (ln.lane == 0) {
            uint32_t p = pos;
            w.res[0] = type == 1 ? fixed_codes(w) : read_dynamic(w, src, n, p, hlit, hdist, hclen);
            w.res[1] = p;
        }
        INF_WAVE_SYNC(); // (the two codes are in the fast memory)
        const uint32_t why = w.res[0];
        pos = w.res[1];
        if (why)
            return why;
        for (;;) { // (a round adds a byte or more to op + strip.n, which isize bounds, or ends the block: <= isize + 1 rounds)
            if (pos > 8 * n)
                return W_EXHAUSTED;
            uint64_t bits = peek(src, n, pos); // (57 bits: a code, 5 extra bits, a code, 13 extra bits are 48 at most)
            uint32_t used;
            const uint32_t s = decode_sym(w.lfast, LIT_FAST, w.lcount, w.lsym, bits, used);
            if (s == NO_SYM)
                return W_NO_CODE; // (not reached: a literal/length code is complete)
            bits >>= used;
            pos += used;
            if (s < 256) {
                if (op + strip.n >= isize)
                    return W_OUT_PAST;
                strip_put(ln, strip, s);
                if (strip.n == LANES)
                    strip_flush(ln, strip, dst, op);
                continue;
            }
            if (s == 256)
                break;
            if (s >= 286)
                return W_LITLEN_SYMBOL;
            uint32_t len, eb;
            if (s < 265) {
                len = s - 254;
                eb = 0;
            } else if (s == 285) {
                len = 258;
                eb = 0;
            } else {
                eb = (s - 261) >> 2;
                len = 3 + ((4 + ((s - 265) & 3)) << eb);
            }
            len += (uint32_t)bits & ((1u << eb) - 1); // (symbol 284 with all extra bits set is 258 as well: zlib takes it)
            bits >>= eb;
            pos += eb;
            const uint32_t ds = decode_sym(w.dfast, DIST_FAST, w.dcount, w.dsym, bits, used);
            if (ds == NO_SYM)
                return W_NO_CODE;
            if (ds >= 30)
                return W_DIST_SYMBOL;
            bits >>= used;
            pos += used;
            const uint32_t db = ds < 4 ? 0 : (ds >> 1) - 1;
            const uint32_t dist = (ds < 4 ? ds + 1 : 1 + ((2 + (ds & 1)) << db)) + ((uint32_t)bits & ((1u << db) - 1));
            pos += db;
            if (pos > 8 * n)
                return W_EXHAUSTED;
            if (dist > op + strip.n)
                return W_DISTANCE;
            if (op + strip.n + len > isize)
                return W_OUT_PAST;
            strip_flush(ln, strip, dst, op);
            INF_WAVE_SYNC(); // (what the match reads is written)
            wave_match(ln, dst + op, dist, len);
            op += len;
        }
    } while (!last);
    strip_flush(ln, strip, dst, op);
    if (op != isize)
        return W_OUT_SHORT;
    if (pos > 8 * n)
        return W_EXHAUSTED;
    if (((pos + 7) >> 3) != n)
        return W_LEFT_OVER;
    INF_WAVE_SYNC(); // (the output is written, the CRC's table too)
    const uint32_t slice = (isize + LANES - 1) / LANES;
    INF_EACH_LANE(ln, l)
    const uint32_t from = l * slice < isize ? l * slice : isize, to = from + slice < isize ? from + slice : isize;
    uint32_t c = 0;
    for (uint32_t i = from; i < to; ++i) // (slice <= 1024)
        c = w.crc_tab[(c ^ dst[i]) & 255] ^ (c >> 8);
    w.part[l] = to > from ? bgzf::mulmod(c, xpow8(isize - to)) : 0;
    INF_END_LANES
    INF_WAVE_SYNC();
    uint32_t crc = 0;
    for (uint32_t l = 0; l < LANES; ++l) // (64)
        crc ^= w.part[l];
    crc ^= bgzf::mulmod(0xFFFFFFFFu, xpow8(isize)) ^ 0xFFFFFFFFu; // (the register starts at all ones and is inverted at the end)
    return crc == crc_want ? W_OK : W_CRC;
}

} // namespace inflate
} // namespace agc
