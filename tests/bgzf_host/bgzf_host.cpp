// bgzf_host.cpp -- agc_amd/csrc/bgzf.h compiled for the HOST: the workgroup's program with its lane sections as loops, block by block,
// and the placing of the members as bgzf_place_kernel does it.  TEST INFRASTRUCTURE ONLY (tests/test_bgzf_host.py, and the byte-for-byte
// yardstick of tests/test_gpu_bgzf.py).  Every buffer the coder touches is a heap block of its exact size: a block's input, its slot,
// the stream.  With -DBGZF_MAIN: a stand-alone program for -fsanitize=address,undefined that runs seeded random inputs through the
// coder and through zlib's inflate.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../agc_amd/csrc/bgzf.h"

using namespace agc;

// -> 0, or -1 when cap < bound(n); *out_len: the stream's size (the bound when refused); block_off: n_blocks + 1 offsets or NULL
extern "C" int bgzf_host_encode(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len, uint64_t *block_off)
{
    const uint64_t n_blocks = bgzf::block_count(n);
    if (cap < bgzf::bound(n)) {
        *out_len = bgzf::bound(n);
        return -1;
    }
    std::unique_ptr<bgzf::Work> w(new bgzf::Work);
    std::vector<std::unique_ptr<uint8_t[]>> slots(n_blocks);
    std::vector<uint32_t> sizes(n_blocks);
    for (uint64_t b = 0; b < n_blocks; ++b) {
        const uint32_t len = (uint32_t)(n - b * bgzf::IN < bgzf::IN ? n - b * bgzf::IN : bgzf::IN);
        std::unique_ptr<uint8_t[]> blk(new uint8_t[len]); // (operator new: 16-byte aligned, like the device's blocks of an aligned input)
        std::memcpy(blk.get(), in + b * bgzf::IN, len);
        slots[b].reset(new uint8_t[bgzf::SLOT]);
        bgzf::encode_block(*w, blk.get(), len, slots[b].get(), &sizes[b]);
    }
    uint64_t at = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
        if (block_off)
            block_off[b] = at;
        bgzf::place_member(slots[b].get(), sizes[b], out + at);
        at += sizes[b];
    }
    if (block_off)
        block_off[n_blocks] = at;
    bgzf::place_eof(out + at);
    *out_len = at + bgzf::EOF_BYTES;
    return 0;
}

extern "C" uint64_t bgzf_host_bound(uint64_t n) { return bgzf::bound(n); }

// the same block from an input at an odd address: the byte loads of load_chunk (what the device does for an unaligned d_in)
extern "C" uint32_t bgzf_host_block_unaligned(const uint8_t *in, uint32_t n, uint8_t *member)
{
    std::unique_ptr<bgzf::Work> w(new bgzf::Work);
    std::unique_ptr<uint8_t[]> blk(new uint8_t[n + 1]), slot(new uint8_t[bgzf::SLOT]);
    std::memcpy(blk.get() + 1, in, n);
    uint32_t size = 0;
    bgzf::encode_block(*w, blk.get() + 1, n, slot.get(), &size);
    std::memcpy(member, slot.get(), size);
    return size;
}

#ifdef BGZF_MAIN
#include <zlib.h>

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static int check(const std::vector<uint8_t> &data, unsigned shift)
{
    const uint64_t n = data.size(), cap = bgzf::bound(n), n_blocks = bgzf::block_count(n);
    std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
    if (n)
        std::memcpy(in.get(), data.data(), n);
    // the stream at every alignment of its first byte: place_member's head / body / tail
    std::unique_ptr<uint8_t[]> out_mem(new uint8_t[cap + shift]);
    uint8_t *out = out_mem.get() + shift;
    std::vector<uint64_t> off(n_blocks + 1);
    uint64_t len = 0;
    if (bgzf_host_encode(in.get(), n, out, cap, &len, off.data()) != 0 || len > cap)
        return 1;
    uint64_t at = 0;
    for (uint64_t b = 0; b <= n_blocks; ++b) {
        if (at != off[b] || at + 18 > len)
            return 2;
        const uint32_t size = (out[at + 16] | out[at + 17] << 8) + 1u;
        if (at + size > len || size > bgzf::MEMBER_MAX)
            return 3;
        const uint32_t want = b < n_blocks ? (uint32_t)(n - b * bgzf::IN < bgzf::IN ? n - b * bgzf::IN : bgzf::IN) : 0;
        std::unique_ptr<uint8_t[]> dec(new uint8_t[want ? want : 1]);
        z_stream z;
        std::memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK)
            return 4;
        z.next_in = out + at + 18;
        z.avail_in = size - 26;
        z.next_out = dec.get();
        z.avail_out = want;
        const int rc = inflate(&z, Z_FINISH);
        const bool all = rc == Z_STREAM_END && z.avail_in == 0 && z.total_out == want;
        inflateEnd(&z);
        if (!all || (want && std::memcmp(dec.get(), data.data() + b * bgzf::IN, want)))
            return 5;
        uint32_t crc, isize;
        std::memcpy(&crc, out + at + size - 8, 4);
        std::memcpy(&isize, out + at + size - 4, 4);
        if (crc != crc32(0, dec.get(), want) || isize != want)
            return 6;
        at += size;
    }
    return at == len ? 0 : 7;
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 10;
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    static const uint32_t sizes[] = {0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 65279, 65280, 65281, 65280 + 17, 2 * 65280, 2 * 65280 + 1};
    int n_run = 0;
    for (int r = 0; r < rounds; ++r) {
        const uint32_t n = r < (int)(sizeof sizes / sizeof *sizes) ? sizes[r] : rnd() % 140000;
        const uint32_t alphabet = 1 + rnd() % 256, skew = rnd() % 4;
        uint8_t map[256];
        for (uint32_t i = 0; i < 256; ++i)
            map[i] = (uint8_t)(rnd() & 255);
        std::vector<uint8_t> data(n);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t x = rnd() % alphabet;
            for (uint32_t s = 0; s < skew; ++s) // skewed counts: the minimum of several draws (skew 3: deep codes)
                x = x < rnd() % alphabet ? x : rnd() % (x + 1);
            data[i] = map[x];
        }
        const int bad = check(data, (unsigned)(r % 17));
        if (bad) {
            printf("FAILED round %d: n %u alphabet %u skew %u: check %d\n", r, n, alphabet, skew, bad);
            return 1;
        }
        ++n_run;
    }
    printf("ok %d inputs\n", n_run);
    return 0;
}
#endif
