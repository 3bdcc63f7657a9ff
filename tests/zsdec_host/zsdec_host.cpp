// zsdec_host.cpp -- agc_amd/csrc/zstd/zs_decode.h on the CPU: the program a wave runs, with "lane 0" for everything one lane does
// and the lane sections as loops over 64 lanes (the periodic match copy and the split of the Huffman streams are the code the
// device runs).  TEST INFRASTRUCTURE ONLY.
//   -DZSDEC_MAIN: a stand-alone program (no Python).  It dlopen's libzstd the way agc_amd/csrc/host/host_support.h does, makes
//   frames from seeded inputs at the archive's levels, mutates them (single bytes at every header position and at random ones,
//   truncations, appended bytes) and runs every one through the decoder and through ZSTD_decompress.  Exit 1: a frame libzstd made
//   is refused or decodes to other bytes, or a mutated input both accept decodes to other bytes.  Every buffer is a heap block of
//   its exact size: built with -fsanitize=address,undefined the run also shows that no input makes the decoder leave them.
//   usage: zsdec_selftest SEED ROUNDS [DUMP]   DUMP: every input that was run, with the status found, for the device test
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../agc_amd/csrc/zstd/zs_decode.h"

using namespace zs;

extern "C" void zsdec_header(const uint8_t *src, uint64_t n, uint32_t out4[4])
{
    const dec::FrameHeader h = dec::parseFrameHeader(src, n);
    out4[0] = h.status, out4[1] = h.headerSize, out4[2] = h.contentSize, out4[3] = h.blockMax;
}

// -> the frame's status; *out_len = the content size its header declares (0 when the header is refused); the bytes go to dst
// when cap holds them (cap smaller: nothing is decoded, the status is the header's)
extern "C" uint32_t zsdec_decode(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap, uint64_t *out_len)
{
    const dec::FrameHeader h = dec::parseFrameHeader(src, n);
    *out_len = h.status == dec::OK ? h.contentSize : 0;
    if (h.status != dec::OK || h.contentSize > cap)
        return h.status;
    const uint32_t lit_cap = h.contentSize < BLOCKSIZE_MAX ? h.contentSize : BLOCKSIZE_MAX;
    uint8_t *lit = (uint8_t *)malloc(lit_cap ? lit_cap : 1); // (exact sizes: a sanitizer sees one byte too far)
    uint32_t *fast = (uint32_t *)malloc(dec::FAST_WORDS * 4);
    const dec::Lane ln = {0};
    const uint32_t st = dec::decodeFrame(ln, src, (uint32_t)n, dst, h.contentSize, lit, lit_cap, fast);
    free(lit);
    free(fast);
    return st;
}

// the code tables as the format lists them, against the arithmetic of zs_decode.h; -> 0 when they agree
extern "C" int zsdec_check_tables(void)
{
    for (uint32_t c = 0; c <= MaxLL; ++c)
        if (LLcode(dec::LLbase(c)) != c || (c < MaxLL && dec::LLbase(c) + (1u << LLbits(c)) != dec::LLbase(c + 1)))
            return 1;
    for (uint32_t c = 0; c <= MaxML; ++c)
        if (MLcode(dec::MLbase(c) - MINMATCH) != c || (c < MaxML && dec::MLbase(c) + (1u << MLbits(c)) != dec::MLbase(c + 1)))
            return 2;
    return 0;
}

#ifdef ZSDEC_MAIN
#include <dlfcn.h>
#include <string>

namespace {

struct Zstd {
    size_t (*compressBound)(size_t) = nullptr;
    size_t (*compress)(void *, size_t, const void *, size_t, int) = nullptr;
    size_t (*decompress)(void *, size_t, const void *, size_t) = nullptr;
    unsigned (*isError)(size_t) = nullptr;
    bool open()
    {
        const char *cands[] = {getenv("AGC_ZSTD_LIB"), "/opt/conda/lib/libzstd.so.1", "libzstd.so.1", "libzstd.so"};
        void *h = nullptr;
        for (const char *c : cands)
            if (c && *c && (h = dlopen(c, RTLD_NOW | RTLD_LOCAL))) // (no RTLD_DEEPBIND: the sanitizer runtime refuses it, and no other zstd is in this program)
                break;
        if (!h)
            return false;
        compressBound = (size_t(*)(size_t))dlsym(h, "ZSTD_compressBound");
        compress = (size_t(*)(void *, size_t, const void *, size_t, int))dlsym(h, "ZSTD_compress");
        decompress = (size_t(*)(void *, size_t, const void *, size_t))dlsym(h, "ZSTD_decompress");
        isError = (unsigned (*)(size_t))dlsym(h, "ZSTD_isError");
        return compressBound && compress && decompress && isError;
    }
} Z;

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

// inputs of the kinds the archive holds: delta-pack-like text, 2-bit tuples, symbol bytes, words, skewed bytes, mutated repeats
std::vector<uint8_t> make_input(uint32_t kind, uint32_t n)
{
    std::vector<uint8_t> v;
    v.reserve(n + 64);
    if (kind == 0) { // numbers, commas, letters, 0xFF between deltas
        while (v.size() < n) {
            const uint32_t t = rnd(10);
            if (t < 6) {
                char b[32];
                const int k = snprintf(b, sizeof b, "%u,%u.", rnd(60000), rnd(400));
                v.insert(v.end(), b, b + k);
            } else if (t < 9)
                v.push_back("ACGT"[rnd(4)]);
            else
                v.push_back(0xFF);
        }
    } else if (kind == 1) { // packed tuples: any byte, with long repeats
        std::vector<uint8_t> seg(200 + rnd(3000));
        for (auto &c : seg)
            c = (uint8_t)rnd(256);
        while (v.size() < n) {
            if (rnd(3))
                v.insert(v.end(), seg.begin(), seg.begin() + 1 + rnd((uint32_t)seg.size()));
            else
                for (uint32_t k = rnd(400); k; --k)
                    v.push_back((uint8_t)rnd(256));
        }
    } else if (kind == 2) { // symbol bytes 0..3, a few others
        while (v.size() < n)
            v.push_back(rnd(50) ? (uint8_t)rnd(4) : (uint8_t)(4 + rnd(12)));
    } else if (kind == 3) { // words
        std::vector<std::string> words(5 + rnd(150));
        for (auto &w : words)
            for (uint32_t k = 2 + rnd(7); k; --k)
                w.push_back((char)('a' + rnd(26)));
        while (v.size() < n) {
            const std::string &w = words[rnd((uint32_t)words.size())];
            v.insert(v.end(), w.begin(), w.end());
            v.push_back(' ');
        }
    } else if (kind == 4) { // skewed bytes
        const uint32_t k = 2 + rnd(30);
        while (v.size() < n)
            v.push_back((uint8_t)(32 + (rnd(k) * rnd(k)) / k));
    } else if (kind == 5) { // runs of one byte, short and very long
        while (v.size() < n)
            v.insert(v.end(), 1 + rnd(rnd(4) ? 100 : 200000), (uint8_t)rnd(256));
    } else // noise
        while (v.size() < n)
            v.push_back((uint8_t)rnd(256));
    v.resize(n);
    return v;
}

struct Tally {
    uint64_t valid = 0, mutated = 0, both = 0, neither = 0, only_zstd = 0, only_ours = 0;
} tally;
FILE *dump = nullptr;

// one input through both decoders; made_by_zstd: a frame the library wrote for `want`.  false: a disagreement (reported)
bool run_one(const std::vector<uint8_t> &in, const std::vector<uint8_t> *want, const char *what)
{
    uint8_t *src = (uint8_t *)malloc(in.size() ? in.size() : 1); // (exact size)
    if (!in.empty())
        memcpy(src, in.data(), in.size());
    uint64_t len = 0;
    uint32_t st = zsdec_decode(src, in.size(), nullptr, 0, &len);
    uint8_t *out = nullptr;
    const bool header_ok = st == dec::OK;
    if (header_ok) {
        out = (uint8_t *)malloc(len ? len : 1);
        st = zsdec_decode(src, in.size(), out, len, &len);
    }
    // libzstd gets room for what the header declares, or for a block when the header is refused here
    const size_t zcap = header_ok ? len : 1u << 17;
    uint8_t *zout = (uint8_t *)malloc(zcap ? zcap : 1);
    const size_t zr = Z.decompress(zout, zcap, src, in.size());
    const bool zok = !Z.isError(zr);
    bool ok = true;
    if (want) {
        ++tally.valid;
        if (st != dec::OK || len != want->size() || (len && memcmp(out, want->data(), len))) {
            fprintf(stderr, "%s: a frame libzstd made is %s (status %u, %llu bytes, %zu expected)\n", what, st ? "refused" : "decoded to other bytes", st,
                    (unsigned long long)len, want->size());
            ok = false;
        }
    } else {
        ++tally.mutated;
        if (st == dec::OK && zok) {
            ++tally.both;
            if (zr != len || (len && memcmp(out, zout, len))) {
                fprintf(stderr, "%s: both decoders accept, the bytes differ (%llu bytes here, %zu from libzstd)\n", what, (unsigned long long)len, zr);
                ok = false;
            }
        } else if (st == dec::OK)
            ++tally.only_ours;
        else if (zok)
            ++tally.only_zstd;
        else
            ++tally.neither;
    }
    if (dump) {
        const uint32_t n = (uint32_t)in.size();
        fwrite(&n, 4, 1, dump);
        fwrite(&st, 4, 1, dump);
        fwrite(src, 1, n, dump);
    }
    free(src);
    free(out);
    free(zout);
    return ok;
}

} // namespace

int main(int argc, char **argv)
{
    if (zsdec_check_tables()) {
        fprintf(stderr, "the code tables of zs_decode.h are not the inverse of zs_common.h's\n");
        return 1;
    }
    if (!Z.open()) {
        fprintf(stderr, "cannot dlopen libzstd (set AGC_ZSTD_LIB)\n");
        return 2;
    }
    if (argc > 1)
        rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ULL;
    const int rounds = argc > 2 ? atoi(argv[2]) : 40;
    if (argc > 3 && !(dump = fopen(argv[3], "wb"))) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 2;
    }
    static const int levels[] = {1, 3, 13, 17, 19};
    bool ok = true;
    for (int it = 0; it < rounds && ok; ++it) {
        // sizes: mostly small (every header form), some around the block size and beyond (several blocks, windowed headers)
        const uint32_t pick = rnd(16);
        const uint32_t n = pick < 2 ? rnd(300) : pick < 10 ? rnd(20000) : pick < 14 ? 100000 + rnd(80000) : 131000 + rnd(200000);
        const uint32_t kind = rnd(7);
        const int level = levels[rnd(5)];
        const std::vector<uint8_t> data = make_input(kind, n);
        std::vector<uint8_t> frame(Z.compressBound(n));
        const size_t k = Z.compress(frame.data(), frame.size(), data.data(), n, level);
        if (Z.isError(k)) {
            fprintf(stderr, "ZSTD_compress failed\n");
            return 2;
        }
        frame.resize(k);
        char what[96];
        snprintf(what, sizeof what, "round %d (kind %u, %u bytes, level %d)", it, kind, n, level);
        ok = run_one(frame, &data, what) && ok;
        // mutations: every position of the headers in front (frame, first block, literals, sequences), then random ones
        const uint32_t head = k < 24 ? (uint32_t)k : 24;
        std::vector<uint8_t> m;
        for (uint32_t p = 0; p < head && ok; ++p) {
            m = frame;
            m[p] ^= (uint8_t)(1 + rnd(255));
            ok = run_one(m, nullptr, what) && ok;
        }
        for (int r = 0; r < 24 && ok && k; ++r) {
            m = frame;
            const uint32_t t = rnd(8);
            if (t < 4)
                m[rnd((uint32_t)k)] ^= (uint8_t)(1u << rnd(8));
            else if (t < 6)
                m.resize(rnd((uint32_t)k)); // truncated
            else if (t == 6)
                for (uint32_t a = 1 + rnd(8); a; --a)
                    m.push_back((uint8_t)rnd(256)); // bytes behind the last block
            else
                for (uint32_t a = 1 + rnd(4); a; --a)
                    m[rnd((uint32_t)k)] = (uint8_t)rnd(256);
            ok = run_one(m, nullptr, what) && ok;
        }
    }
    if (dump)
        fclose(dump);
    printf("%s %llu frames of libzstd's, %llu mutated: %llu accepted by both, %llu by neither, %llu by libzstd alone, %llu by this decoder alone\n",
           ok ? "ok" : "FAILED", (unsigned long long)tally.valid, (unsigned long long)tally.mutated, (unsigned long long)tally.both,
           (unsigned long long)tally.neither, (unsigned long long)tally.only_zstd, (unsigned long long)tally.only_ours);
    return ok ? 0 : 1;
}
#endif
