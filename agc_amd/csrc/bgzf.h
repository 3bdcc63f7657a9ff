// bgzf.h -- bytes into BGZF (the blocked gzip of the SAM specification, 4.1; what `bgzip` writes): the input is cut into blocks of
// IN = 65280 bytes, every block becomes one gzip member that stands alone, and a fixed 28-byte EOF member ends the stream.  A member's
// payload is ONE deflate block of dynamic Huffman codes over literals and end-of-block -- no match search -- or, whenever that would
// not be smaller, a stored block.  The same source compiles for gfx950 (bgzf_kernels.hip: a workgroup of THREADS lanes per block)
// and for the host (tests/bgzf_host runs the lane sections as loops), and both write the same bytes.  No HIP calls.
//
// A block is one program every lane of the workgroup runs; between BGZF_EACH_LANE(t) and BGZF_END_LANES stands what lane t does,
// and BGZF_END_LANES is a barrier.  The includer may define, before including this header (the kernel does; the host needs none):
//   BGZF_EACH_LANE(t) / BGZF_END_LANES   one lane section; here: a loop over the THREADS lanes
//   BGZF_OR(p, v) / BGZF_ADD(p, v)       *p |= v / *p += v on a 32-bit word other lanes of the section may touch as well
//
// The member: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C', SLEN 2, BSIZE = member size - 1 (18 bytes); the deflate payload;
// CRC-32 and ISIZE of the block's input (8 bytes).  A stored payload is 5 + n bytes, so no member exceeds MEMBER_MAX = 65311 bytes.
//
// The dynamic block: BFINAL 1, BTYPE 2, HLIT 0 (257 literal/length codes: the bytes and end-of-block), HDIST 1 (two distance codes of
// one bit, never used -- what zlib sends for a block without matches: a complete code, which every inflate accepts), HCLEN, the
// code-length code's lengths, the 259 code lengths coded with it -- runs of zero lengths as symbols 17 (3-10) and 18 (11-138), runs of
// an equal length as symbol 16 (3-6 repeats) --, the literals, end-of-block.
//
// A code (code_lengths): the used symbols are ranked by (count, symbol); the Huffman tree is built from that order with two queues (of
// equal weights the leaf goes first, of two leaves or two inner nodes the earlier); the leaves' depths are clipped to the limit and
// the counts per length repaired as zlib's gen_bitlen does (one leaf of the deepest level below the limit becomes an inner node of two
// leaves, a leaf leaves the limit's level: the Kraft sum stays 1); then the lengths are dealt out along the ranking, the longest to the
// rarest.  The codes are canonical (RFC 1951, 3.2.2).  Counts are integer sums and every tie is broken by symbol value: nothing in the
// result depends on the order in which lanes run.
//
// Where the time goes on the device, per block: the input is read three times in 16-byte chunks, lane t chunk s * THREADS + t of step
// s (the first read from HBM, the others from L2) -- for the histogram and the CRC, for the chunks' bit counts, for the packing.  The
// CRC of a lane's chunks is carried across the 4080 bytes between them by one multiplication by x^(8 * 4080) mod P per step (CRC-32
// is linear: the lanes' values are xor-ed).  The packed bits are OR-ed into the zeroed member image in the LDS.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BGZF_FN __host__ __device__ inline
#else
#define BGZF_FN inline
#endif

#ifndef BGZF_EACH_LANE
#define BGZF_EACH_LANE(t)                                                                                                                   \
    {                                                                                                                                       \
        for (uint32_t t = 0; t < bgzf::THREADS; ++t) {
#define BGZF_END_LANES                                                                                                                      \
    }                                                                                                                                       \
    }
#define BGZF_OR(p, v) (*(p) |= (v))
#define BGZF_ADD(p, v) (*(p) += (v))
#endif

namespace agc {
namespace bgzf {

constexpr uint32_t IN = 65280;                       // input bytes of a block (0xFF00)
constexpr uint32_t THREADS = 256;                    // lanes of a block's workgroup
constexpr uint32_t CHUNK = 16;                       // input bytes a lane takes per step
constexpr uint32_t CHUNKS = 4096;                    // chunk slots of a block (IN / CHUNK = 4080 are used): 16 steps of THREADS
constexpr uint32_t HEADER = 18, TRAILER = 8, EOF_BYTES = 28;
constexpr uint32_t MEMBER_MAX = HEADER + 5 + IN + TRAILER; // 65311: a stored block
constexpr uint32_t SLOT = 65312;                     // a member's slot: MEMBER_MAX rounded up to 16-byte stores
constexpr uint32_t N_LIT = 257, N_LEN = 259, N_CL = 19; // bytes + end-of-block; + the two distance codes; the code-length alphabet
constexpr uint32_t CRC_POLY = 0xEDB88320u;

BGZF_FN uint64_t block_count(uint64_t n) { return n / IN + (n % IN ? 1 : 0); }
// what holds the stream of n input bytes, whatever they are: every capacity check uses this
BGZF_FN uint64_t bound(uint64_t n) { return n + 31 * block_count(n) + EOF_BYTES; }

// everything a block's lanes share: the LDS of the workgroup (79 888 bytes: two workgroups a CU)
struct Work {
    alignas(16) uint32_t stage[SLOT / 4]; // the member as it will lie in memory
    union {
        uint32_t hist[4][N_LIT]; // a histogram per 64 lanes: four letters would otherwise serialise on four counters
        struct {
            uint32_t weight[2 * N_LIT]; // code_lengths: a node's weight, then its depth
            uint16_t parent[2 * N_LIT];
        } tree;
    } u;
    uint32_t freq[264];
    uint16_t code[264], order[264];
    uint8_t len[264];         // [0, 257): the literal/length code; [257, 259): the two distance codes
    uint8_t chunkbits[CHUNKS]; // coded bits of every chunk (at most 16 * 15)
    uint32_t scan[2][THREADS]; // the lanes' CRC parts; then the bit totals of 16 chunks each and their prefix sums
    uint32_t crc_tab[256], xp[20]; // the CRC's byte table; x^(2^k) mod P
    uint32_t cl_freq[20];
    uint16_t cl_code[20], cl_seq[N_LEN + 1]; // the coded lengths: symbol | extra bits << 5
    uint8_t cl_len[20];
    uint32_t bl_count[16], next_code[16];
    uint32_t n_used, n_seq, hdr_bits, hclen, data_bits, payload, stored, member, crc, xgap;
};

// ---- CRC-32 as polynomial arithmetic mod P, bit-reflected as gzip has it: x^0 is bit 31 ----------------------------------------------
BGZF_FN uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m)
            p ^= b;
        b = (b >> 1) ^ ((b & 1) ? CRC_POLY : 0);
    }
    return p;
}

// x^(8 m) mod P, m < 2^17
BGZF_FN uint32_t xpow8(const Work &w, uint32_t m)
{
    uint32_t p = 0x80000000u;
    for (uint32_t k = 3; m; m >>= 1, ++k)
        if (m & 1)
            p = mulmod(w.xp[k], p);
    return p;
}

// ---- memory: 16 bytes at a time where the address allows ---------------------------------------------------------------------------------
struct V16 {
    uint32_t w[4];
};

// chunk c of the block's n bytes as four little-endian words, bytes past n as 0
BGZF_FN V16 load_chunk(const uint8_t *in, uint32_t n, uint32_t c)
{
    V16 v = {{0, 0, 0, 0}};
    const uint32_t off = c * CHUNK;
    const uint8_t *p = in + off;
    if (off + CHUNK <= n && ((uintptr_t)p & 15) == 0)
        __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    else
        for (uint32_t j = 0; j < CHUNK; ++j) // (constant bounds: the words stay registers)
            if (off + j < n)
                v.w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    return v;
}

BGZF_FN uint32_t chunk_bytes(uint32_t n, uint32_t c) { return c * CHUNK >= n ? 0 : n - c * CHUNK < CHUNK ? n - c * CHUNK : CHUNK; }
BGZF_FN uint32_t byte_of(const V16 &v, uint32_t j) { return (v.w[j >> 2] >> (8 * (j & 3))) & 255; }

// nb <= 32 bits of v at bit `pos` of the member image (least significant bit first: deflate's order, and a little-endian field's)
BGZF_FN void put_bits(Work &w, uint32_t pos, uint32_t v, uint32_t nb)
{
    (void)nb;
    const uint64_t x = (uint64_t)v << (pos & 31);
    if ((uint32_t)x)
        BGZF_OR(&w.stage[pos >> 5], (uint32_t)x);
    if (x >> 32)
        BGZF_OR(&w.stage[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

BGZF_FN uint32_t bit_reverse(uint32_t c, uint32_t nb)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < nb; ++i, c >>= 1)
        r = (r << 1) | (c & 1);
    return r;
}

// ---- a length-limited canonical Huffman code: freq[0, n_sym) -> len[], code[] (bit-reversed: ready for put_bits) ---------------------------
BGZF_FN void code_lengths(Work &w, const uint32_t *freq, uint32_t n_sym, uint32_t max_bits, uint8_t *len, uint16_t *code)
{
    // the used symbols in the order of (count, symbol): every symbol finds its own rank
    BGZF_EACH_LANE(t)
    for (uint32_t s = t; s < n_sym; s += THREADS) {
        len[s] = 0;
        const uint32_t f = freq[s];
        uint32_t rank = 0, used = 0;
        for (uint32_t o = 0; o < n_sym; ++o) {
            const uint32_t g = freq[o];
            used += g != 0;
            rank += g != 0 && (g < f || (g == f && o < s));
        }
        if (f)
            w.order[rank] = (uint16_t)s;
        if (s == 0)
            w.n_used = used;
    }
    BGZF_END_LANES
    BGZF_EACH_LANE(t)
    if (t == 0) {
        uint32_t m = w.n_used;
        if (m < 2) { // a code has two symbols at least: one that never occurs joins, in front as the rarer
            const uint16_t only = m ? w.order[0] : 1;
            w.order[0] = only ? 0 : 1;
            w.order[1] = only;
            m = 2;
        }
        uint32_t *wt = w.u.tree.weight;
        uint16_t *par = w.u.tree.parent;
        for (uint32_t i = 0; i < m; ++i)
            wt[i] = freq[w.order[i]];
        uint32_t leaf = 0, inner = m, made = m;
        for (uint32_t k = 0; k + 1 < m; ++k) {
            uint32_t pick[2];
            for (uint32_t j = 0; j < 2; ++j)
                pick[j] = leaf < m && (inner >= made || wt[leaf] <= wt[inner]) ? leaf++ : inner++;
            wt[made] = wt[pick[0]] + wt[pick[1]];
            par[pick[0]] = par[pick[1]] = (uint16_t)made;
            ++made;
        }
        wt[made - 1] = 0; // the root's depth; every node's parent lies behind it
        for (uint32_t j = made - 1; j-- > 0;)
            wt[j] = wt[par[j]] + 1;
        for (uint32_t b = 0; b < 16; ++b)
            w.bl_count[b] = 0;
        int overflow = 0;
        for (uint32_t i = 0; i < m; ++i) {
            overflow += wt[i] > max_bits;
            w.bl_count[wt[i] > max_bits ? max_bits : wt[i]] += 1;
        }
        while (overflow > 0) {
            uint32_t bits = max_bits - 1;
            while (w.bl_count[bits] == 0)
                --bits;
            w.bl_count[bits] -= 1;
            w.bl_count[bits + 1] += 2;
            w.bl_count[max_bits] -= 1;
            overflow -= 2;
        }
        uint32_t i = 0, next = 0;
        for (uint32_t bits = max_bits; bits >= 1; --bits)
            for (uint32_t k = 0; k < w.bl_count[bits]; ++k)
                len[w.order[i++]] = (uint8_t)bits;
        w.next_code[0] = 0;
        for (uint32_t bits = 1; bits <= max_bits; ++bits) {
            next = (next + w.bl_count[bits - 1]) << 1;
            w.next_code[bits] = next;
        }
    }
    BGZF_END_LANES
    // canonical codes: among the symbols of one length in symbol order
    BGZF_EACH_LANE(t)
    for (uint32_t s = t; s < n_sym; s += THREADS) {
        const uint32_t l = len[s];
        uint32_t before = 0;
        for (uint32_t o = 0; o < s; ++o)
            before += len[o] == l;
        code[s] = l ? (uint16_t)bit_reverse(w.next_code[l] + before, l) : 0;
    }
    BGZF_END_LANES
}

BGZF_FN void emit_length(Work &w, uint32_t sym, uint32_t extra)
{
    w.cl_seq[w.n_seq++] = (uint16_t)(sym | extra << 5);
    w.cl_freq[sym] += 1;
}

BGZF_FN uint32_t cl_order(uint32_t i)
{
    const uint8_t o[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

BGZF_FN uint32_t cl_extra_bits(uint32_t sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// ---- a block: in[0, n), 1 <= n <= IN -> its member in slot[0, SLOT) (16-byte aligned), the member's size in *size ------------------------
BGZF_FN void encode_block(Work &w, const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *size)
{
    const uint32_t n_chunks = (n + CHUNK - 1) / CHUNK;
    // the image and the histograms cleared, the CRC's tables made
    BGZF_EACH_LANE(t)
    for (uint32_t i = t; i < SLOT / 4; i += THREADS)
        w.stage[i] = 0;
    for (uint32_t i = t; i < 4 * N_LIT; i += THREADS)
        (&w.u.hist[0][0])[i] = 0;
    uint32_t c = t;
    for (uint32_t k = 0; k < 8; ++k)
        c = (c >> 1) ^ ((c & 1) ? CRC_POLY : 0);
    w.crc_tab[t] = c;
    if (t == 0) {
        w.xp[0] = 0x40000000u; // x^1
        for (uint32_t k = 1; k < 20; ++k)
            w.xp[k] = mulmod(w.xp[k - 1], w.xp[k - 1]);
    }
    BGZF_END_LANES
    BGZF_EACH_LANE(t)
    if (t == 0)
        w.xgap = xpow8(w, CHUNK * (THREADS - 1));
    BGZF_END_LANES
    // first read: the histogram, and the CRC of the bytes in this lane's chunks with zeros everywhere else
    BGZF_EACH_LANE(t)
    uint32_t crc = 0, end = 0;
    for (uint32_t c = t; c < n_chunks; c += THREADS) {
        const V16 v = load_chunk(in, n, c);
        const uint32_t nb = chunk_bytes(n, c);
        if (c != t)
            crc = mulmod(crc, w.xgap);
        for (uint32_t j = 0; j < CHUNK; ++j)
            if (j < nb) {
                const uint32_t b = byte_of(v, j);
                BGZF_ADD(&w.u.hist[t >> 6][b], 1u);
                crc = w.crc_tab[(crc ^ b) & 255] ^ (crc >> 8);
            }
        end = c * CHUNK + nb;
    }
    w.scan[0][t] = end ? mulmod(crc, xpow8(w, n - end)) : 0;
    BGZF_END_LANES
    BGZF_EACH_LANE(t)
    for (uint32_t s = t; s < N_LIT; s += THREADS)
        w.freq[s] = s == 256 ? 1 : w.u.hist[0][s] + w.u.hist[1][s] + w.u.hist[2][s] + w.u.hist[3][s];
    if (t == 0) {
        uint32_t crc = 0;
        for (uint32_t i = 0; i < THREADS; ++i)
            crc ^= w.scan[0][i];
        w.crc = crc ^ mulmod(0xFFFFFFFFu, xpow8(w, n)) ^ 0xFFFFFFFFu; // (the register starts at all ones and is inverted at the end)
    }
    BGZF_END_LANES
    code_lengths(w, w.freq, N_LIT, 15, w.len, w.code);
    // the 259 lengths as the code-length alphabet codes them
    BGZF_EACH_LANE(t)
    if (t == 0) {
        w.len[257] = w.len[258] = 1;
        w.n_seq = 0;
        for (uint32_t s = 0; s < 20; ++s)
            w.cl_freq[s] = 0;
        for (uint32_t i = 0; i < N_LEN;) {
            const uint32_t v = w.len[i];
            uint32_t run = 1;
            while (i + run < N_LEN && w.len[i + run] == v)
                ++run;
            i += run;
            if (v == 0) {
                for (; run >= 11; run -= run < 138 ? run : 138)
                    emit_length(w, 18, (run < 138 ? run : 138) - 11);
                if (run >= 3) {
                    emit_length(w, 17, run - 3);
                    run = 0;
                }
            } else {
                emit_length(w, v, 0);
                for (--run; run >= 3; run -= run < 6 ? run : 6)
                    emit_length(w, 16, (run < 6 ? run : 6) - 3);
            }
            for (; run; --run)
                emit_length(w, v, 0);
        }
    }
    BGZF_END_LANES
    code_lengths(w, w.cl_freq, N_CL, 7, w.cl_len, w.cl_code);
    // second read: every chunk's coded bits
    BGZF_EACH_LANE(t)
    for (uint32_t c = t; c < CHUNKS; c += THREADS) {
        uint32_t bits = 0;
        if (c < n_chunks) {
            const V16 v = load_chunk(in, n, c);
            const uint32_t nb = chunk_bytes(n, c);
            for (uint32_t j = 0; j < CHUNK; ++j)
                bits += j < nb ? w.len[byte_of(v, j)] : 0;
        }
        w.chunkbits[c] = (uint8_t)bits;
    }
    if (t == 0) {
        uint32_t hclen = N_CL;
        while (hclen > 4 && w.cl_len[cl_order(hclen - 1)] == 0)
            --hclen;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (uint32_t i = 0; i < w.n_seq; ++i)
            bits += w.cl_len[w.cl_seq[i] & 31] + cl_extra_bits(w.cl_seq[i] & 31);
        w.hclen = hclen;
        w.hdr_bits = bits;
    }
    BGZF_END_LANES
    // the bits of 16 chunks each, and their inclusive prefix sums (scan[0] again after eight steps)
    BGZF_EACH_LANE(t)
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 16; ++i)
        sum += w.chunkbits[16 * t + i];
    w.scan[0][t] = sum;
    BGZF_END_LANES
    for (uint32_t step = 0; step < 8; ++step) {
        BGZF_EACH_LANE(t)
        const uint32_t d = 1u << step;
        w.scan[(step + 1) & 1][t] = w.scan[step & 1][t] + (t >= d ? w.scan[step & 1][t - d] : 0);
        BGZF_END_LANES
    }
    // dynamic or stored; the gzip header, the block's header, the trailer
    BGZF_EACH_LANE(t)
    if (t == 0) {
        w.data_bits = w.scan[0][THREADS - 1];
        const uint32_t total = w.hdr_bits + w.data_bits + w.len[256];
        w.payload = (total + 7) / 8;
        w.stored = w.payload >= 5 + n;
        if (w.stored)
            w.payload = 5 + n;
        w.member = HEADER + w.payload + TRAILER;
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (uint32_t i = 0; i < 16; ++i)
            put_bits(w, 8 * i, head[i], 8);
        put_bits(w, 8 * 16, w.member - 1, 16);
        uint32_t pos = 8 * HEADER;
        if (w.stored) {
            put_bits(w, pos, 1, 8); // BFINAL 1, BTYPE 0, the rest of the byte
            put_bits(w, pos + 8, n, 16);
            put_bits(w, pos + 24, n ^ 0xFFFF, 16);
        } else {
            put_bits(w, pos, 1 | 2 << 1 | 0 << 3 | 1 << 8 | (w.hclen - 4) << 13, 17);
            pos += 17;
            for (uint32_t i = 0; i < w.hclen; ++i, pos += 3)
                put_bits(w, pos, w.cl_len[cl_order(i)], 3);
            for (uint32_t i = 0; i < w.n_seq; ++i) {
                const uint32_t sym = w.cl_seq[i] & 31;
                put_bits(w, pos, w.cl_code[sym], w.cl_len[sym]);
                pos += w.cl_len[sym];
                put_bits(w, pos, w.cl_seq[i] >> 5, cl_extra_bits(sym));
                pos += cl_extra_bits(sym);
            }
            put_bits(w, pos + w.data_bits, w.code[256], w.len[256]);
        }
        put_bits(w, 8 * (HEADER + w.payload), w.crc, 32);
        put_bits(w, 8 * (HEADER + w.payload) + 32, n, 32);
        *size = w.member;
    }
    BGZF_END_LANES
    // third read: the literals' codes, or the bytes as they are
    BGZF_EACH_LANE(t)
    for (uint32_t c = t; c < n_chunks; c += THREADS) {
        const V16 v = load_chunk(in, n, c);
        if (w.stored) {
            for (uint32_t k = 0; k < 4; ++k)
                put_bits(w, 8 * (HEADER + 5 + c * CHUNK + 4 * k), v.w[k], 32);
        } else {
            uint32_t pos = 8 * HEADER + w.hdr_bits + ((c >> 4) ? w.scan[0][(c >> 4) - 1] : 0);
            for (uint32_t i = c & ~15u; i < c; ++i)
                pos += w.chunkbits[i];
            const uint32_t nb = chunk_bytes(n, c);
            uint32_t word = pos >> 5, fill = pos & 31;
            uint64_t acc = 0;
            for (uint32_t j = 0; j < CHUNK; ++j)
                if (j < nb) {
                    const uint32_t b = byte_of(v, j);
                    acc |= (uint64_t)w.code[b] << fill;
                    fill += w.len[b];
                    if (fill >= 32) {
                        BGZF_OR(&w.stage[word++], (uint32_t)acc);
                        acc >>= 32;
                        fill -= 32;
                    }
                }
            if (fill && (uint32_t)acc)
                BGZF_OR(&w.stage[word], (uint32_t)acc);
        }
    }
    BGZF_END_LANES
    // the member to its slot, 16 bytes a lane
    BGZF_EACH_LANE(t)
    for (uint32_t i = t; i < (w.member + 15) / 16; i += THREADS)
        __builtin_memcpy(__builtin_assume_aligned(slot + 16 * i, 16), &w.stage[4 * i], 16);
    BGZF_END_LANES
}

// ---- placing: a member out of its slot (16-byte aligned) to dst, wherever that lies ------------------------------------------------------
// Bytes up to dst's first 16-byte boundary and behind its last are stored one at a time, what lies between as 16-byte stores whose
// words are put together from the slot's aligned words -- never a byte of dst outside [0, size) is written.
BGZF_FN void place_member(const uint8_t *slot, uint32_t size, uint8_t *dst)
{
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    head = head < size ? head : size;
    const uint32_t body = (size - head) / 16, tail = size - head - 16 * body;
    BGZF_EACH_LANE(t)
    if (t < head)
        dst[t] = slot[t];
    if (t < tail)
        dst[head + 16 * body + t] = slot[head + 16 * body + t];
    const uint32_t *words = (const uint32_t *)slot + (head >> 2);
    const uint32_t sh = 8 * (head & 3);
    for (uint32_t i = t; i < body; i += THREADS) {
        V16 v;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t lo = words[4 * i + k];
            v.w[k] = sh ? lo >> sh | words[4 * i + k + 1] << (32 - sh) : lo;
        }
        __builtin_memcpy(__builtin_assume_aligned(dst + head + 16 * i, 16), &v, 16);
    }
    BGZF_END_LANES
}

BGZF_FN void place_eof(uint8_t *dst)
{
    const uint8_t eof[EOF_BYTES] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    BGZF_EACH_LANE(t)
    if (t < EOF_BYTES)
        dst[t] = eof[t];
    BGZF_END_LANES
}

} // namespace bgzf
} // namespace agc
