// zs_decode.h -- one zstd frame back into its bytes: the inverse of zs_frame.h / zs_entropy.h (S3 of the read side:
// ZSTD_decompressDCtx as CSegment::get_raw / get call it, src/common/segment.cpp:136-400).  The format is the one the encoder
// headers of this directory write (RFC 8878); where the format leaves a decoder a choice -- what to do with bits that are not
// there -- libzstd 1.4.9's observable behaviour decides, and this decoder takes the strict side: whatever it accepts, libzstd
// decodes to the same bytes (tests/test_zstd_decode_host.py).
//
// One source for the host (gcc, tests only: tests/zsdec_host) and the device (hipcc: zstd_decode_kernels.hip).  No HIP calls.
//
// A frame is decoded by one wavefront of LANES lanes, written as one program every lane runs:
//   - everything that only READS the frame (headers, the FSE state chain of the sequences, the bit readers) is computed by all
//     lanes alike -- the same values in every lane, the cost of one;
//   - everything that builds a table is done by lane 0 alone (`if (ln.lane == 0)`), its result left in the fast memory, and a
//     ZSD_WAVE_SYNC() stands between it and the lanes that read it;
//   - the Huffman streams of a literals section go one to a lane (ZSD_EACH_LANE: lanes 0-3 of a 4-stream section);
//   - the bytes move on all lanes: literal runs, matches, raw and RLE blocks are copies in chunks of LANES bytes, a match whose
//     offset is below LANES a periodic one (lane i reads base[i % offset]).
// The host build runs the same program with one "lane 0" and the lane loops as loops over 64 lanes, so the periodic copy and the
// stream split are the code the CPU tests see.
//
// Bounded memory access: a frame is (src, srcSize), (dst, dstSize), (lit, litCap), (fast, FAST_WORDS); every index formed from
// frame bits is checked against the one of these it goes into before it is used.  load64() is the only reader of src that takes
// a computed offset and pads with zeros behind srcSize.
// Bounded loops: every loop below names its bound.
//
// The includer may define, before including this header (the kernel does; the host needs neither):
//   ZSD_WAVE_SYNC()   orders lane 0's stores (fast memory, lit, dst) before the other lanes' loads of them
//   ZSD_WAVE_ANY(x)   true in every lane when x is true in any
#pragma once
#include "zs_entropy.h"

#ifndef ZSD_WAVE_SYNC
#define ZSD_WAVE_SYNC() ((void)0)
#endif
#ifndef ZSD_WAVE_ANY
#define ZSD_WAVE_ANY(x) (x)
#endif
// a section every lane runs with its own lane number l (host: a loop over the lanes)
#if defined(__HIP_DEVICE_COMPILE__)
#define ZSD_EACH_LANE(ln, l)                                                                                                                \
    {                                                                                                                                       \
        const U32 l = (ln).lane;                                                                                                            \
        {
#else
#define ZSD_EACH_LANE(ln, l)                                                                                                                \
    {                                                                                                                                       \
        for (U32 l = 0; l < LANES; ++l) {
#endif
#define ZSD_END_LANES                                                                                                                       \
    }                                                                                                                                       \
    }

namespace zs {
namespace dec {

// per frame; 0 = decoded.  (include/agc_hip.h: AGC_HIP_ZD_*)
enum Status : U32 {
    OK = 0,
    UNSUPPORTED = 1, // a valid frame this decoder does not take: no content size, a dictionary id, a checksum, a skippable frame, >= 2^31 bytes
    MALFORMED = 2,   // not a frame: see the checks below
};

constexpr U32 LANES = 64;
constexpr U32 MAGIC = 0xFD2FB528u;
constexpr U32 HUF_LOG_MAX = 11; // Max_Number_of_Bits of the format (libzstd's own tables would take 12)
constexpr U32 WEIGHT_FSE_LOG_MAX = 6;
constexpr U32 MIN_CBLOCK = 3; // a compressed block below this size is refused by libzstd (MIN_CBLOCK_SIZE)

struct Lane {
    U32 lane; // device: the lane's number in its wave; host: 0
};

// ---- the frame header (host and device: the host sizes the output from it) ----
struct FrameHeader {
    U32 status;      // OK, or why the frame is refused (the other fields are 0 then)
    U32 headerSize;  // bytes in front of the first block
    U32 contentSize; // < 2^31
    U32 blockMax;    // min(128 KiB, window)
};

ZHD FrameHeader parseFrameHeader(const BYTE *src, U64 srcSize)
{
    const FrameHeader bad = {MALFORMED, 0, 0, 0}, unsup = {UNSUPPORTED, 0, 0, 0};
    if (srcSize < 4)
        return bad;
    const U32 magic = (U32)src[0] | ((U32)src[1] << 8) | ((U32)src[2] << 16) | ((U32)src[3] << 24);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u)
        return unsup; // a skippable frame
    if (magic != MAGIC || srcSize < 5)
        return bad;
    if (srcSize >> 32)
        return unsup;
    const U32 fhd = src[4];
    const U32 fcsFlag = fhd >> 6, single = (fhd >> 5) & 1, reserved = (fhd >> 3) & 1, checksum = (fhd >> 2) & 1, didFlag = fhd & 3;
    if (reserved)
        return bad;
    const U32 didBytes = didFlag == 3 ? 4 : didFlag;
    const U32 fcsBytes = fcsFlag == 0 ? single : fcsFlag == 1 ? 2 : fcsFlag == 2 ? 4 : 8;
    const U32 headerSize = 5 + !single + didBytes + fcsBytes;
    if (srcSize < headerSize)
        return bad;
    U32 pos = 5;
    U64 window = 0;
    if (!single) {
        const U32 wd = src[pos++], wlog = 10 + (wd >> 3);
        if (wlog > 31)
            return unsup; // (libzstd: frameParameter_windowTooLarge)
        window = (1ULL << wlog) + ((1ULL << wlog) >> 3) * (wd & 7);
    }
    U32 dictId = 0;
    for (U32 i = 0; i < didBytes; ++i) // (<= 4)
        dictId |= (U32)src[pos++] << (8 * i);
    if (dictId || checksum || !fcsBytes)
        return unsup;
    U64 content = 0;
    for (U32 i = 0; i < fcsBytes; ++i) // (<= 8)
        content |= (U64)src[pos++] << (8 * i);
    if (fcsBytes == 2)
        content += 256;
    if (content >> 31)
        return unsup;
    if (single)
        window = content;
    return {OK, headerSize, (U32)content, (U32)(window < BLOCKSIZE_MAX ? window : BLOCKSIZE_MAX)};
}

// ---- the fast memory of one frame (device: LDS), in 32-bit words ----
// Huffman entry: symbol | nbBits << 8.  FSE entry: symbol | nbBits << 8 | newStateBase << 16.
constexpr U32 F_HUF = 0;                                   // U16[1 << HUF_LOG_MAX]
constexpr U32 F_LL = F_HUF + (1u << HUF_LOG_MAX) / 2;      // U32[1 << LLFSELog]
constexpr U32 F_OF = F_LL + (1u << LLFSELog);              // U32[1 << OffFSELog]
constexpr U32 F_ML = F_OF + (1u << OffFSELog);             // U32[1 << MLFSELog]
constexpr U32 F_NORM = F_ML + (1u << MLFSELog);            // int16_t[256]: a distribution being read
constexpr U32 F_NEXT = F_NORM + 128;                       // U16[256]: symbolNext of the table being built
constexpr U32 F_WEIGHTS = F_NEXT + 128;                    // BYTE[256]: Huffman weights
constexpr U32 F_WFSE = F_WEIGHTS + 64;                     // U32[1 << WEIGHT_FSE_LOG_MAX]: the weights' FSE table
constexpr U32 F_RANK = F_WFSE + (1u << WEIGHT_FSE_LOG_MAX); // U32[16]
constexpr U32 F_RES = F_RANK + 16;                         // U32[4]: what lane 0 found, for every lane to read
constexpr U32 FAST_WORDS = F_RES + 4;                      // 2708 words = 10 832 bytes

ZFN U32 lowMask(U32 n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

// the little-endian bytes [off, off + 8) of p[0, size), zeros behind size
ZFN U64 load64(const BYTE *p, U32 size, U32 off)
{
    if ((U64)off + 8 <= size)
        return read64(p + off);
    U64 w = 0;
    for (U32 k = 0; k < 8; ++k) // (8)
        if ((U64)off + k < size)
            w |= (U64)p[off + k] << (8 * k);
    return w;
}

// ---- forward bit reader (FSE distributions): LSB first, zeros behind the end ----
struct FwdR {
    const BYTE *p;
    U32 size, pos; // pos: bits consumed
};
ZFN U32 fwPeek(const FwdR &f, U32 n) { return (U32)(load64(f.p, f.size, f.pos >> 3) >> (f.pos & 7)) & lowMask(n); } // n <= 16

// ---- backward bit reader (bitstream.h: BIT_DStream_t): the stream's bits are numbered from bit 0 of byte 0; the highest set bit
// of the last byte is the end marker, the bits below it are read from the top down.  hi = bits not yet read; a read of more
// than there are is padded with zeros below bit 0 (libzstd: the same, while its container is not exhausted) and leaves hi < 0.
struct BitR {
    const BYTE *p;
    U32 size;
    int hi, wlo; // w = the bits [wlo, wlo + 64)
    U64 w;
};
ZFN void brLoad(BitR &b)
{
    const U32 top = ((U32)b.hi + 7) >> 3, cb = top > 8 ? top - 8 : 0;
    b.w = load64(b.p, b.size, cb);
    b.wlo = (int)(cb * 8);
}
// false: an empty stream, or no end marker
ZFN bool brInit(BitR &b, const BYTE *p, U32 size)
{
    b.p = p;
    b.size = size;
    b.hi = b.wlo = 0;
    b.w = 0;
    if (size == 0 || size > (1u << 27))
        return false;
    const U32 last = p[size - 1];
    if (!last)
        return false;
    b.hi = (int)(8 * (size - 1) + highbit32(last));
    brLoad(b);
    return true;
}
ZFN U32 brPeek(BitR &b, U32 n) // n <= 32
{
    if (b.hi <= 0 || n == 0)
        return 0;
    const int lo = b.hi - (int)n;
    if (lo < b.wlo && b.wlo > 0)
        brLoad(b); // (then lo >= wlo: the window holds the 57 bits or more below hi, or starts at bit 0)
    if (lo >= b.wlo)
        return (U32)(b.w >> (lo - b.wlo)) & lowMask(n);
    return ((U32)b.w & lowMask((U32)b.hi)) << (n - (U32)b.hi); // (wlo == 0, hi < n: the last hi bits, zeros below)
}
ZFN void brSkip(BitR &b, U32 n) { b.hi -= (int)n; }
ZFN U32 brRead(BitR &b, U32 n)
{
    const U32 v = brPeek(b, n);
    brSkip(b, n);
    return v;
}

// ---- code -> value tables of the format as arithmetic (the inverses of LLcode / MLcode in zs_common.h) ----
ZHD U32 LLbase(U32 c) // LL_base[c], c <= 35
{
    return c < 16 ? c : c < 20 ? 16 + ((c - 16) << 1) : c < 22 ? 24 + ((c - 20) << 2) : c < 24 ? 32 + ((c - 22) << 3) : c == 24 ? 48 : 1u << (c - 19);
}
ZHD U32 MLbase(U32 c) // ML_base[c], c <= 52 (the match length, MINMATCH included)
{
    const U32 m = c < 32 ? c : c < 36 ? 32 + ((c - 32) << 1) : c < 38 ? 40 + ((c - 36) << 2) : c < 40 ? 48 + ((c - 38) << 3) : c < 42 ? 64 + ((c - 40) << 4)
                  : c == 42 ? 96 : 1u << (c - 36);
    return m + MINMATCH;
}

// ---- FSE distribution (fse_decompress.c: FSE_readNCount).  maxSym: in, the largest symbol allowed; out, the last one read.
// -> the bytes read, 0: malformed (does not sum to the table size, a symbol beyond maxSym, bits read behind the end)
ZFN U32 readNCount(int16_t *norm, U32 &maxSym, U32 &log, const BYTE *p, U32 size)
{
    FwdR f = {p, size, 0};
    U32 nbBits = fwPeek(f, 4) + FSE_MIN_TABLELOG;
    f.pos = 4;
    if (nbBits > 15)
        return 0;
    log = nbBits;
    int remaining = (1 << nbBits) + 1, threshold = 1 << nbBits;
    nbBits++;
    U32 charnum = 0;
    bool previous0 = false;
    while (remaining > 1 && charnum <= maxSym) { // (charnum grows in every round: <= maxSym + 1 <= 256 rounds)
        if (previous0) {
            U32 n0 = charnum;
            while (fwPeek(f, 16) == 0xFFFF) { // (n0 grows by 24: <= 11 rounds)
                n0 += 24;
                f.pos += 16;
                if (n0 > maxSym)
                    return 0;
            }
            while (fwPeek(f, 2) == 3) { // (n0 grows by 3: <= 86 rounds)
                n0 += 3;
                f.pos += 2;
                if (n0 > maxSym)
                    return 0;
            }
            n0 += fwPeek(f, 2);
            f.pos += 2;
            if (n0 > maxSym)
                return 0;
            while (charnum < n0) // (<= maxSym)
                norm[charnum++] = 0;
        }
        const int max = (2 * threshold - 1) - remaining;
        const U32 bits = fwPeek(f, nbBits); // (nbBits <= 16)
        int count;
        if ((int)(bits & (U32)(threshold - 1)) < max) {
            count = (int)(bits & (U32)(threshold - 1));
            f.pos += nbBits - 1;
        } else {
            count = (int)(bits & (U32)(2 * threshold - 1));
            if (count >= threshold)
                count -= max;
            f.pos += nbBits;
        }
        count--; // (-1: a "less than one" probability)
        remaining -= count < 0 ? -count : count;
        if (remaining < 1)
            return 0; // (cannot happen: count <= remaining - 1 by the coding; it bounds the loop below)
        norm[charnum++] = (int16_t)count;
        previous0 = !count;
        while (remaining < threshold) { // (threshold halves, remaining >= 1: <= 16 rounds)
            nbBits--;
            threshold >>= 1;
        }
    }
    if (remaining != 1)
        return 0;
    const U32 bytes = (f.pos + 7) >> 3;
    if (bytes > size)
        return 0;
    maxSym = charnum - 1;
    return bytes;
}

// ---- FSE decoding table (FSE_buildDTable / ZSTD_buildFSETable) from a distribution that sums to 1 << log ----
ZFN bool buildFseTable(U32 *tab, const int16_t *norm, U32 maxSym, U32 log, U16 *next)
{
    const U32 tableSize = 1u << log, mask = tableSize - 1, step = (tableSize >> 1) + (tableSize >> 3) + 3;
    U32 high = tableSize - 1;
    for (U32 s = 0; s <= maxSym; ++s) { // (<= 256)
        if (norm[s] == -1) {
            tab[high--] = s;
            next[s] = 1;
        } else
            next[s] = (U16)norm[s];
    }
    U32 position = 0, placed = 0;
    for (U32 s = 0; s <= maxSym; ++s)                    // (<= 256)
        for (int i = 0; i < norm[s]; ++i) {               // (all symbols together: the distribution's sum = tableSize)
            if (++placed > tableSize)
                return false;
            tab[position] = s;
            position = (position + step) & mask;
            for (U32 k = 0; position > high && k < tableSize; ++k) // (step is odd: every cell comes round within tableSize steps)
                position = (position + step) & mask;
        }
    if (position != 0)
        return false;
    for (U32 u = 0; u < tableSize; ++u) { // (<= 512)
        const U32 s = tab[u] & 0xFF, nextState = next[s]++;
        const U32 nb = log - highbit32(nextState);
        tab[u] = s | (nb << 8) | (((nextState << nb) - tableSize) << 16);
    }
    return true;
}

ZFN U32 fseSym(U32 e) { return e & 0xFF; }
ZFN U32 fseBits(U32 e) { return (e >> 8) & 0xFF; }
ZFN U32 fseBase(U32 e) { return e >> 16; }

// ---- Huffman tree description (huf_decompress.c: HUF_readStats + HUF_readDTableX1) at p[0, size) -> the decoding table.
// Lane 0's work.  -> bytes read | table log << 16; 0: malformed
ZFN U32 readHufTable(U32 *fast, const BYTE *p, U32 size)
{
    BYTE *const weights = (BYTE *)(fast + F_WEIGHTS);
    U16 *const huf = (U16 *)(fast + F_HUF);
    U32 *const rank = fast + F_RANK;
    if (size < 1)
        return 0;
    const U32 hb = p[0];
    U32 nW = 0, used;
    if (hb >= 128) { // weights as 4-bit fields
        nW = hb - 127;
        used = 1 + (nW + 1) / 2;
        if (used > size)
            return 0;
        for (U32 n = 0; n < nW; n += 2) { // (<= 128)
            weights[n] = p[1 + n / 2] >> 4;
            weights[n + 1] = p[1 + n / 2] & 15; // (nW odd: one entry past the last weight, inside the 256)
        }
    } else { // FSE-compressed weights, two interleaved states (fse_decompress.c: FSE_decompress_wksp, FSE_decompress_usingDTable)
        used = 1 + hb;
        if (used > size)
            return 0;
        int16_t *const norm = (int16_t *)(fast + F_NORM);
        U32 *const wfse = fast + F_WFSE;
        U32 maxSym = 255, log = 0;
        const U32 nc = readNCount(norm, maxSym, log, p + 1, hb);
        if (!nc || log > WEIGHT_FSE_LOG_MAX || !buildFseTable(wfse, norm, maxSym, log, (U16 *)(fast + F_NEXT)))
            return 0;
        BitR b;
        if (!brInit(b, p + 1 + nc, hb - nc) || b.hi < (int)(2 * log))
            return 0; // (two states that are not all there: libzstd goes on with what its container holds)
        U32 s1 = brRead(b, log), s2 = brRead(b, log);
        for (;;) { // (two weights a round, refused beyond 255: <= 128 rounds)
            if (nW > 253)
                return 0;
            U32 e = wfse[s1];
            weights[nW++] = (BYTE)fseSym(e);
            s1 = fseBase(e) + brRead(b, fseBits(e));
            if (b.hi < 0) {
                weights[nW++] = (BYTE)fseSym(wfse[s2]);
                break;
            }
            if (nW > 253)
                return 0;
            e = wfse[s2];
            weights[nW++] = (BYTE)fseSym(e);
            s2 = fseBase(e) + brRead(b, fseBits(e));
            if (b.hi < 0) {
                weights[nW++] = (BYTE)fseSym(wfse[s1]);
                break;
            }
        }
    }
    // HUF_readStats: the last weight is what completes the sum to a power of two
    for (U32 w = 0; w < 16; ++w) // (16)
        rank[w] = 0;
    U32 total = 0;
    for (U32 n = 0; n < nW; ++n) { // (<= 255)
        const U32 w = weights[n];
        if (w > HUF_LOG_MAX)
            return 0;
        rank[w]++;
        total += (1u << w) >> 1;
    }
    if (!total)
        return 0;
    const U32 log = highbit32(total) + 1;
    if (log > HUF_LOG_MAX)
        return 0;
    const U32 rest = (1u << log) - total, lastWeight = highbit32(rest) + 1;
    if ((1u << highbit32(rest)) != rest)
        return 0;
    weights[nW] = (BYTE)lastWeight;
    rank[lastWeight]++;
    nW++;
    if (rank[1] < 2 || (rank[1] & 1))
        return 0;
    // HUF_readDTableX1: the cells of a weight together, the symbols of a weight in their order
    U32 start = 0;
    for (U32 w = 1; w <= log; ++w) { // (<= 11)
        const U32 cur = start;
        start += rank[w] << (w - 1);
        rank[w] = cur;
    }
    for (U32 s = 0; s < nW; ++s) { // (<= 256 symbols; their cells together: 1 << log)
        const U32 w = weights[s];
        if (!w)
            continue;
        const U32 len = (1u << w) >> 1, e = s | ((log + 1 - w) << 8);
        for (U32 u = rank[w]; u < rank[w] + len; ++u)
            huf[u] = (U16)e;
        rank[w] += len;
    }
    return used | (log << 16);
}

// one Huffman stream p[0, size) -> n literals at out; true: malformed (no end marker, or not used up exactly)
ZFN bool hufDecodeStream(BYTE *out, U32 n, const BYTE *p, U32 size, const U16 *huf, U32 log)
{
    BitR b;
    if (!brInit(b, p, size))
        return true;
    for (U32 i = 0; i < n; ++i) { // (n <= the literals' size)
        if (b.hi < 0)
            return true;
        const U32 e = huf[brPeek(b, log)];
        brSkip(b, e >> 8);
        out[i] = (BYTE)e;
    }
    return b.hi != 0;
}

// ---- the bytes: chunks of LANES, a byte per lane ----
ZFN void waveCopy(const Lane &ln, BYTE *dst, const BYTE *src, U32 n)
{
    for (U32 c = 0; c < n; c += LANES) // (n / LANES)
        ZSD_EACH_LANE(ln, l)
        if (c + l < n)
            dst[c + l] = src[c + l];
        ZSD_END_LANES
}
ZFN void waveFill(const Lane &ln, BYTE *dst, BYTE v, U32 n)
{
    for (U32 c = 0; c < n; c += LANES) // (n / LANES)
        ZSD_EACH_LANE(ln, l)
        if (c + l < n)
            dst[c + l] = v;
        ZSD_END_LANES
}
// dst[i] = dst[i - off], i = 0 .. n - 1, 1 <= off <= the bytes in front of dst: a chunk reads only bytes in front of itself (off >=
// LANES), or the match is the period dst[-off, 0) repeated (off < LANES: lane i reads period[i % off], all of it in front of dst)
ZFN void waveMatch(const Lane &ln, BYTE *dst, U32 off, U32 n)
{
    const BYTE *const period = dst - off;
    for (U32 c = 0; c < n; c += LANES) { // (n / LANES)
        ZSD_EACH_LANE(ln, l)
        const U32 i = c + l;
        if (i < n)
            dst[i] = off >= LANES ? period[i] : period[i % off];
        ZSD_END_LANES
        if (off >= LANES)
            ZSD_WAVE_SYNC(); // (the next chunk may read this one)
    }
}

// what a frame carries from block to block
struct FrameState {
    U32 hufLog, llLog, ofLog, mlLog;
    bool hufValid, fseValid; // a table to reuse exists (treeless literals; repeat mode)
    U32 rep[3];
    U32 op; // bytes of the frame written so far
};

// one of the three sequence tables of a block.  mode: the block's choice for it; at p[0, size) what the mode needs.
// -> bytes read (0 is valid for predefined / repeat) or ~0u: malformed
ZFN U32 seqTable(const Lane &ln, U32 *fast, U32 *tab, U32 &log, U32 mode, const BYTE *p, U32 size, U32 maxSym, U32 maxLog, const int16_t *defNorm,
                 U32 defMax, U32 defLog, bool fseValid)
{
    if (mode == set_repeat)
        return fseValid ? 0 : ~0u;
    if (mode == set_rle) {
        if (size < 1 || p[0] > maxSym)
            return ~0u;
        if (ln.lane == 0)
            tab[0] = p[0]; // (0 bits, new state 0)
        log = 0;
        return 1;
    }
    if (mode == set_basic) {
        if (ln.lane == 0)
            buildFseTable(tab, defNorm, defMax, defLog, (U16 *)(fast + F_NEXT));
        log = defLog;
        return 0;
    }
    if (ln.lane == 0) {
        int16_t *const norm = (int16_t *)(fast + F_NORM);
        U32 ms = maxSym, lg = 0;
        const U32 nc = readNCount(norm, ms, lg, p, size);
        fast[F_RES] = nc && lg <= maxLog && buildFseTable(tab, norm, ms, lg, (U16 *)(fast + F_NEXT)) ? nc | (lg << 16) : 0;
    }
    ZSD_WAVE_SYNC();
    const U32 res = fast[F_RES];
    ZSD_WAVE_SYNC(); // (F_RES is written again by the next table)
    if (!res)
        return ~0u;
    log = res >> 16;
    return res & 0xFFFF;
}

// one compressed block src[0, n) (zstd_decompress_block.c: ZSTD_decompressBlock_internal) -> dst[st.op ...], st.op advanced
ZFN U32 decodeBlock(const Lane &ln, FrameState &st, const BYTE *src, U32 n, BYTE *dst, U32 dstSize, BYTE *lit, U32 litCap, U32 *fast)
{
    if (n < MIN_CBLOCK)
        return MALFORMED;
    // ---- literals (ZSTD_decodeLiteralsBlock) ----
    const U32 b0 = src[0], litType = b0 & 3, sf = (b0 >> 2) & 3;
    const BYTE *litPtr = lit;
    U32 litSize, used;
    if (litType < 2) { // raw, RLE
        const U32 lh = sf == 1 ? 2 : sf == 3 ? 3 : 1; // (n >= 3)
        litSize = sf == 1 ? ((U32)src[0] | ((U32)src[1] << 8)) >> 4 : sf == 3 ? ((U32)src[0] | ((U32)src[1] << 8) | ((U32)src[2] << 16)) >> 4 : b0 >> 3;
        if (litSize > BLOCKSIZE_MAX)
            return MALFORMED;
        if (litType == 0) {
            if (litSize > n - lh)
                return MALFORMED;
            litPtr = src + lh; // (read where they lie)
            used = lh + litSize;
        } else {
            if (n - lh < 1 || litSize > litCap)
                return MALFORMED;
            waveFill(ln, lit, src[lh], litSize);
            used = lh + 1;
        }
    } else { // Huffman: with its tree, or the frame's last one
        if (n < 5)
            return MALFORMED;
        const U32 lhc = read32(src);
        const U32 lh = sf < 2 ? 3 : sf == 2 ? 4 : 5, streams = sf == 0 ? 1 : 4;
        U32 cSize;
        if (sf < 2) {
            litSize = (lhc >> 4) & 0x3FF;
            cSize = (lhc >> 14) & 0x3FF;
        } else if (sf == 2) {
            litSize = (lhc >> 4) & 0x3FFF;
            cSize = lhc >> 18;
        } else {
            litSize = (lhc >> 4) & 0x3FFFF;
            cSize = (lhc >> 22) + ((U32)src[4] << 10);
        }
        if (litSize == 0 || litSize > BLOCKSIZE_MAX || litSize > litCap || cSize > n - lh)
            return MALFORMED;
        const BYTE *sp = src + lh;
        U32 sn = cSize;
        if (litType == 3) {
            if (!st.hufValid)
                return MALFORMED;
        } else {
            if (ln.lane == 0)
                fast[F_RES] = readHufTable(fast, sp, sn);
            ZSD_WAVE_SYNC();
            const U32 res = fast[F_RES];
            ZSD_WAVE_SYNC();
            if (!res)
                return MALFORMED;
            st.hufLog = res >> 16;
            st.hufValid = true;
            sp += res & 0xFFFF; // (<= sn: readHufTable stays inside)
            sn -= res & 0xFFFF;
        }
        U32 sOff[4] = {0, 0, 0, 0}, sLen[4] = {sn, 0, 0, 0}, seg = litSize;
        if (streams == 4) { // (huf_decompress.c: HUF_decompress4X1_usingDTable_internal)
            if (sn < 10)
                return MALFORMED;
            const U32 l1 = (U32)sp[0] | ((U32)sp[1] << 8), l2 = (U32)sp[2] | ((U32)sp[3] << 8), l3 = (U32)sp[4] | ((U32)sp[5] << 8);
            if (6 + l1 + l2 + l3 > sn)
                return MALFORMED;
            seg = (litSize + 3) / 4;
            if (3 * seg > litSize)
                return MALFORMED;
            sOff[0] = 6, sOff[1] = 6 + l1, sOff[2] = 6 + l1 + l2, sOff[3] = 6 + l1 + l2 + l3;
            sLen[0] = l1, sLen[1] = l2, sLen[2] = l3, sLen[3] = sn - sOff[3];
        }
        bool bad = false;
        ZSD_EACH_LANE(ln, l)
        if (l < streams) {
            // (selects, not indexing: the four descriptors stay in registers)
            const U32 o = l == 0 ? sOff[0] : l == 1 ? sOff[1] : l == 2 ? sOff[2] : sOff[3];
            const U32 sz = l == 0 ? sLen[0] : l == 1 ? sLen[1] : l == 2 ? sLen[2] : sLen[3];
            const U32 cnt = streams == 1 ? litSize : l < 3 ? seg : litSize - 3 * seg;
            if (hufDecodeStream(lit + l * seg, cnt, sp + o, sz, (const U16 *)(fast + F_HUF), st.hufLog))
                bad = true;
        }
        ZSD_END_LANES
        if (ZSD_WAVE_ANY(bad))
            return MALFORMED;
        used = lh + cSize;
    }
    ZSD_WAVE_SYNC(); // (the literals are in lit)

    // ---- sequences header (ZSTD_decodeSeqHeaders) ----
    const BYTE *sp = src + used;
    const U32 sn = n - used;
    if (sn < 1)
        return MALFORMED;
    U32 nbSeq = sp[0], k = 1;
    if (nbSeq == 0) {
        if (sn != 1)
            return MALFORMED;
    } else if (nbSeq >= 128) {
        if (nbSeq == 255) {
            if (sn < 3)
                return MALFORMED;
            nbSeq = ((U32)sp[1] | ((U32)sp[2] << 8)) + LONGNBSEQ;
            k = 3;
        } else {
            if (sn < 2)
                return MALFORMED;
            nbSeq = ((nbSeq - 128) << 8) + sp[1];
            k = 2;
        }
    }
    U32 litPos = 0;
    if (nbSeq) {
        if (sn < k + 1)
            return MALFORMED;
        const U32 modes = sp[k++];
        if (modes & 3)
            return MALFORMED;
        U32 *const tLL = fast + F_LL, *const tOF = fast + F_OF, *const tML = fast + F_ML;
        U32 r = seqTable(ln, fast, tLL, st.llLog, modes >> 6, sp + k, sn - k, MaxLL, LLFSELog, LL_defaultNorm, MaxLL, LL_defaultNormLog, st.fseValid);
        if (r == ~0u)
            return MALFORMED;
        k += r; // (<= sn: the table readers stay inside)
        r = seqTable(ln, fast, tOF, st.ofLog, (modes >> 4) & 3, sp + k, sn - k, MaxOff, OffFSELog, OF_defaultNorm, DefaultMaxOff, OF_defaultNormLog, st.fseValid);
        if (r == ~0u)
            return MALFORMED;
        k += r;
        r = seqTable(ln, fast, tML, st.mlLog, (modes >> 2) & 3, sp + k, sn - k, MaxML, MLFSELog, ML_defaultNorm, MaxML, ML_defaultNormLog, st.fseValid);
        if (r == ~0u)
            return MALFORMED;
        k += r;
        st.fseValid = true;
        ZSD_WAVE_SYNC(); // (the three tables are in the fast memory)

        // ---- the sequences (ZSTD_decompressSequences_body): one FSE state chain, the same in every lane ----
        BitR b;
        if (!brInit(b, sp + k, sn - k) || b.hi < (int)(st.llLog + st.ofLog + st.mlLog))
            return MALFORMED;
        U32 sLL = brRead(b, st.llLog), sOF = brRead(b, st.ofLog), sML = brRead(b, st.mlLog);
        U32 rep0 = st.rep[0], rep1 = st.rep[1], rep2 = st.rep[2];
        for (U32 i = 0; i < nbSeq; ++i) { // (nbSeq < 2^16 + LONGNBSEQ; a stream that runs out ends the loop at once)
            const U32 eLL = tLL[sLL], eOF = tOF[sOF], eML = tML[sML];
            const U32 llCode = fseSym(eLL), ofCode = fseSym(eOF), mlCode = fseSym(eML); // (<= MaxLL, MaxOff, MaxML: the tables hold nothing else)
            U32 offset;
            if (ofCode > 1) {
                offset = (1u << ofCode) - 3 + brRead(b, ofCode);
                rep2 = rep1, rep1 = rep0, rep0 = offset;
            } else {
                const U32 ll0 = llCode == 0;
                if (ofCode == 0) {
                    if (!ll0)
                        offset = rep0;
                    else {
                        offset = rep1;
                        rep1 = rep0, rep0 = offset;
                    }
                } else {
                    const U32 idx = 1 + ll0 + brRead(b, 1);
                    offset = idx == 3 ? rep0 - 1 : idx == 1 ? rep1 : rep2;
                    if (!offset)
                        return MALFORMED; // (libzstd decodes on with offset 1)
                    if (idx != 1)
                        rep2 = rep1;
                    rep1 = rep0, rep0 = offset;
                }
            }
            const U32 ml = MLbase(mlCode) + brRead(b, MLbits(mlCode));
            const U32 ll = LLbase(llCode) + brRead(b, LLbits(llCode));
            if (i + 1 < nbSeq) { // (the encoder wrote no bits for a state behind the last sequence)
                sLL = fseBase(eLL) + brRead(b, fseBits(eLL));
                sML = fseBase(eML) + brRead(b, fseBits(eML));
                sOF = fseBase(eOF) + brRead(b, fseBits(eOF));
            }
            if (b.hi < 0)
                return MALFORMED;
            if (ll > litSize - litPos || ll > dstSize - st.op || ml > dstSize - st.op - ll)
                return MALFORMED;
            waveCopy(ln, dst + st.op, litPtr + litPos, ll);
            litPos += ll;
            st.op += ll;
            if (offset > st.op)
                return MALFORMED; // (there is no dictionary in front of the frame)
            ZSD_WAVE_SYNC();
            waveMatch(ln, dst + st.op, offset, ml);
            st.op += ml;
            ZSD_WAVE_SYNC();
        }
        if (b.hi != 0)
            return MALFORMED;
        st.rep[0] = rep0, st.rep[1] = rep1, st.rep[2] = rep2;
    }
    const U32 rest = litSize - litPos;
    if (rest > dstSize - st.op)
        return MALFORMED;
    waveCopy(ln, dst + st.op, litPtr + litPos, rest);
    st.op += rest;
    ZSD_WAVE_SYNC();
    return OK;
}

// The frame src[0, srcSize) -> dst[0, dstSize), dstSize the content size parseFrameHeader found (the caller sized dst by it).
// lit: litCap bytes of the frame's own, litCap >= min(dstSize, 128 KiB); fast: FAST_WORDS words.  -> Status, the same in every lane
ZFN U32 decodeFrame(const Lane &ln, const BYTE *src, U32 srcSize, BYTE *dst, U32 dstSize, BYTE *lit, U32 litCap, U32 *fast)
{
    const FrameHeader h = parseFrameHeader(src, srcSize);
    if (h.status != OK)
        return h.status;
    if (h.contentSize != dstSize)
        return MALFORMED;
    FrameState st = {0, 0, 0, 0, false, false, {1, 4, 8}, 0};
    U32 ip = h.headerSize;
    for (;;) { // (a block takes 3 bytes of the input or more: <= srcSize / 3 rounds)
        if (srcSize - ip < 3)
            return MALFORMED;
        const U32 bh = (U32)src[ip] | ((U32)src[ip + 1] << 8) | ((U32)src[ip + 2] << 16);
        ip += 3;
        const U32 last = bh & 1, type = (bh >> 1) & 3, size = bh >> 3;
        if (type == 3 || size > h.blockMax)
            return MALFORMED;
        if (type == 0) {
            if (size > srcSize - ip || size > dstSize - st.op)
                return MALFORMED;
            waveCopy(ln, dst + st.op, src + ip, size);
            ip += size;
            st.op += size;
            ZSD_WAVE_SYNC();
        } else if (type == 1) {
            if (srcSize - ip < 1 || size > dstSize - st.op)
                return MALFORMED;
            waveFill(ln, dst + st.op, src[ip], size);
            ip += 1;
            st.op += size;
            ZSD_WAVE_SYNC();
        } else {
            if (size > srcSize - ip)
                return MALFORMED;
            const U32 s = decodeBlock(ln, st, src + ip, size, dst, dstSize, lit, litCap, fast);
            if (s != OK)
                return s;
            ip += size;
        }
        if (last)
            break;
    }
    if (ip != srcSize || st.op != dstSize)
        return MALFORMED;
    return OK;
}

} // namespace dec
} // namespace zs
