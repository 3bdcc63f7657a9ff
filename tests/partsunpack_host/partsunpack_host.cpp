// partsunpack_host.cpp -- agc_amd/csrc/parts_unpack.h compiled for the HOST and run in the order of parts_unpack_kernels.hip: a wave
// is a loop over 64 lanes, a ballot a loop that gathers one bit per lane, a launch a loop over chunks.  TEST INFRASTRUCTURE ONLY (the
// product compiles the same header with hipcc).  With -DPARTSUNPACK_MAIN: a stand-alone program that compares both routines with
// plain walks on seeded random packs and tuple streams, every buffer a heap block of its exact size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../agc_amd/csrc/fasta_out.h"
#include "../../agc_amd/csrc/parts_unpack.h"

using namespace agc;

// pack_index_kernel for one pack: the lanes' loads (only the bytes inside the pack: the kernel's load reaches into its buffer's
// padding, which `valid` masks off), the five ballots, the stores
static uint32_t pack_index(const uint8_t *pack, uint32_t len, uint32_t seq_cap, uint32_t *seq_end)
{
    uint32_t count = 0;
    for (uint64_t base = 0; base < len; base += pu::STRIP) {
        uint32_t mask[64];
        pu::CountBallots B = {};
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t o = base + (uint64_t)pu::LANE_BYTES * lane;
            uint64_t w[2] = {0, 0};
            uint32_t valid = 0;
            if (o < len) {
                valid = (uint32_t)(len - o < pu::LANE_BYTES ? len - o : pu::LANE_BYTES);
                uint8_t b[16] = {0};
                std::memcpy(b, pack + o, valid);
                std::memcpy(w, b, 16);
            }
            mask[lane] = pu::terminator_mask(w[0], w[1], valid);
            const uint32_t cnt = (uint32_t)__builtin_popcount(mask[lane]);
            for (uint32_t j = 0; j < 5; ++j)
                B.b[j] |= (uint64_t)(cnt >> j & 1) << lane;
        }
        for (uint32_t lane = 0; lane < 64; ++lane)
            pu::store_ends(seq_end, seq_cap, count + pu::terminators_in_front(B, lane), mask[lane], (uint32_t)(base + (uint64_t)pu::LANE_BYTES * lane));
        count += pu::terminators_of_the_strip(B);
    }
    return count;
}

// tuples_size_kernel + tuples_unpack_kernel for one stream whose output's first byte lies at an address with (address & 15) == a;
// out: exactly n bytes.  -> the shape's status; a refused stream writes nothing
static uint32_t tuples_unpack(const uint8_t *t, uint64_t size, uint32_t a, uint8_t *out, uint64_t out_cap, uint64_t *n_out)
{
    const pu::TupleShape sh = pu::tuple_shape(size, size ? t[size - 1] : (uint8_t)0);
    *n_out = sh.n;
    if (sh.status != pu::OK || sh.n > out_cap)
        return sh.status;
    const uint64_t n_chunks = fo::chunk_count(a, sh.n);
    for (uint64_t j = 0; j < n_chunks; ++j) {
        uint64_t begin, w0, w1;
        uint32_t n;
        fo::chunk_range(j, a, sh.n, begin, n);
        pu::chunk_symbols(t, sh.nb, sh.n, begin, n, w0, w1);
        for (uint32_t i = 0; i < n; ++i)
            out[begin + i] = (uint8_t)((i < 8 ? w0 : w1) >> (8 * (i & 7)));
    }
    return sh.status;
}

extern "C" {
uint32_t pu_pack_index(const uint8_t *pack, uint32_t len, uint32_t seq_cap, uint32_t *seq_end) { return pack_index(pack, len, seq_cap, seq_end); }
uint32_t pu_tuple_shape(uint64_t size, uint32_t marker, uint32_t *nb, uint64_t *n)
{
    const pu::TupleShape sh = pu::tuple_shape(size, (uint8_t)marker);
    *nb = sh.nb;
    *n = sh.n;
    return sh.status;
}
uint32_t pu_tuples_unpack(const uint8_t *t, uint64_t size, uint32_t a, uint8_t *out, uint64_t out_cap, uint64_t *n)
{
    return tuples_unpack(t, size, a, out, out_cap, n);
}
}

#ifdef PARTSUNPACK_MAIN
// the plain walks: nth_in_pack's loop, and tuples2bytes digit by digit with the checks it lacks
static uint32_t plain_index(const uint8_t *p, uint32_t len, std::vector<uint32_t> &ends)
{
    for (uint32_t i = 0; i < len; ++i)
        if (p[i] == 0xFF)
            ends.push_back(i);
    return (uint32_t)ends.size();
}

static bool plain_tuples(const uint8_t *t, uint64_t size, std::vector<uint8_t> &out)
{
    if (size < 2)
        return false;
    const uint32_t nb = t[size - 1] >> 4, last = t[size - 1] & 15;
    if (nb != 4 && nb != 3 && nb != 2) {
        out.assign(t, t + size - 1);
        return true;
    }
    if (last > nb)
        return false;
    const uint32_t base = nb == 4 ? 4 : nb == 3 ? 6 : 16;
    const uint64_t n = (size - 2) * nb + last;
    out.assign(n, 0);
    for (uint64_t q = 0; q * nb < n; ++q) {
        const uint32_t digits = (uint32_t)(n - q * nb < nb ? n - q * nb : nb);
        uint32_t c = t[q];
        for (int k = (int)digits - 1; k >= 0; --k, c /= base)
            out[q * nb + k] = (uint8_t)(c % base);
    }
    return true;
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1, rounds = argc > 2 ? (unsigned)atoi(argv[2]) : 2000;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    unsigned refused = 0;
    for (unsigned r = 0; r < rounds; ++r) {
        { // a pack: lengths around the strips' and lanes' edges, terminators rare, dense or in runs
            static const uint32_t edges[] = {0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2048, 3000};
            const uint32_t len = below(3) ? edges[below(13)] + below(3) : below(5000), density = 1 + below(40), seq_cap = below(4) ? below(60) : 0;
            std::unique_ptr<uint8_t[]> pack(new uint8_t[len]);
            for (uint32_t i = 0; i < len; ++i)
                pack[i] = below(density) == 0 || (i && pack[i - 1] == 0xFF && below(3) == 0) ? 0xFF : (uint8_t)below(255);
            std::vector<uint32_t> want;
            const uint32_t n = plain_index(pack.get(), len, want), kept = n < seq_cap ? n : seq_cap;
            std::unique_ptr<uint32_t[]> got(new uint32_t[seq_cap]);
            for (uint32_t i = 0; i < seq_cap; ++i)
                got[i] = 0xABABABABu;
            if (pack_index(pack.get(), len, seq_cap, got.get()) != n || (kept && std::memcmp(got.get(), want.data(), (size_t)kept * 4) != 0)) {
                printf("pack round %u: len %u cap %u\n", r, len, seq_cap);
                return 1;
            }
            for (uint32_t i = kept; i < seq_cap; ++i)
                if (got[i] != 0xABABABABu)
                    return 1;
        }
        { // a tuple stream: a third malformed
            const bool malformed = below(3) == 0, too_short = malformed && below(2);
            const uint32_t nbs[] = {2, 3, 4, 1, 0, 5, 15}, nb = nbs[below(malformed || below(2) ? 3 : 7)], packed = nb >= 2 && nb <= 4;
            const uint64_t size = too_short ? below(2) : 2 + (below(4) ? below(40) : below(3000));
            std::unique_ptr<uint8_t[]> t(new uint8_t[size]);
            for (uint64_t i = 0; i < size; ++i)
                t[i] = (uint8_t)below(256);
            if (size && !too_short) // (a malformed one: a last tuple byte with more symbols than a tuple byte has)
                t[size - 1] = (uint8_t)(nb << 4 | (malformed ? nb + 1 + below(15 - nb) : below(packed ? nb + 1 : 16)));
            std::vector<uint8_t> want;
            const bool ok = plain_tuples(t.get(), size, want);
            refused += !ok;
            const uint32_t a = below(16);
            uint64_t n = 0;
            std::unique_ptr<uint8_t[]> out(new uint8_t[want.size()]);
            const uint32_t st = tuples_unpack(t.get(), size, a, out.get(), want.size(), &n);
            if ((st == pu::OK) != ok || (ok && (n != want.size() || (n && std::memcmp(out.get(), want.data(), want.size()) != 0)))) {
                printf("tuples round %u: size %llu marker %02x a %u\n", r, (unsigned long long)size, size ? t[size - 1] : 0, a);
                return 1;
            }
        }
    }
    printf("ok %u rounds, %u tuple streams refused\n", rounds, refused);
    return 0;
}
#endif
