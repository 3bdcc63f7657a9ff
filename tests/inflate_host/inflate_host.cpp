// inflate_host.cpp -- agc_amd/csrc/inflate.h compiled for the HOST: the walk of a BGZF stream, and the wavefront's program with its
// lane sections as loops, member by member.  TEST INFRASTRUCTURE ONLY (tests/test_inflate_host.py, and the yardstick of
// tests/test_gpu_inflate.py).  Every buffer the decoder touches is a heap block of its exact size -- a member's payload -- or has guard
// bytes on both sides that are looked at afterwards -- a member's output.  With -DINF_MAIN: a stand-alone program for
// -fsanitize=address,undefined that runs seeded random members, most of them damaged, through the decoder and through zlib's inflate.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../agc_amd/csrc/inflate.h"

namespace inf = agc::inflate;

constexpr uint32_t GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xC7;

// one member's payload -> out[0, isize) -> Why; -1: a guard byte around the output was touched
static int member(const uint8_t *payload, uint32_t n, uint8_t *out, uint32_t isize, uint32_t crc)
{
    std::unique_ptr<uint8_t[]> src(new uint8_t[n ? n : 1]), dst(new uint8_t[isize + 2 * GUARD]);
    std::unique_ptr<inf::Work> w(new inf::Work);
    if (n)
        std::memcpy(src.get(), payload, n);
    std::memset(dst.get(), GUARD_BYTE, isize + 2 * GUARD);
    const inf::Lane ln = {0};
    const uint32_t why = inf::inflate_member(ln, *w, src.get(), n, dst.get() + GUARD, isize, crc);
    for (uint32_t i = 0; i < GUARD; ++i)
        if (dst[i] != GUARD_BYTE || dst[GUARD + isize + i] != GUARD_BYTE)
            return -1;
    if (isize)
        std::memcpy(out, dst.get() + GUARD, isize);
    return (int)why;
}

// the walk alone -> the Status of its first complaint (0: none); jobs: 4 x uint64 per member {src_off, out_off, src_len, out_len}, or NULL
extern "C" uint32_t inflate_host_walk(const uint8_t *in, uint64_t n, uint64_t *jobs4, uint32_t *crcs, uint64_t cap, uint64_t *n_members, uint64_t *text_bytes, uint32_t *why,
                                      uint64_t *at)
{
    std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]); // (exact size: the walk reads nothing behind n)
    if (n)
        std::memcpy(copy.get(), in, n);
    std::vector<inf::Job> jobs(cap);
    inf::Walk W;
    inf::walk(copy.get(), n, jobs4 ? jobs.data() : nullptr, cap, W);
    for (uint64_t m = 0; jobs4 && m < W.n_members && m < cap; ++m) {
        jobs4[4 * m] = jobs[m].src_off;
        jobs4[4 * m + 1] = jobs[m].out_off;
        jobs4[4 * m + 2] = jobs[m].src_len;
        jobs4[4 * m + 3] = jobs[m].out_len;
        crcs[m] = jobs[m].crc;
    }
    *n_members = W.n_members;
    *text_bytes = W.text_bytes;
    *why = W.why;
    *at = W.at;
    return inf::status_of(W.why);
}

// agc_hip_bgzf_inflate on the CPU, with its return codes (0, -2 EINVAL, -4 ECAP; -9: a guard byte was touched); why: a Why per member
extern "C" int inflate_host_stream(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *text_off, uint32_t *status, uint32_t *why)
{
    inf::Walk W;
    inf::walk(in, n, nullptr, 0, W);
    std::vector<inf::Job> jobs(W.n_members);
    inf::Walk W2;
    inf::walk(in, n, jobs.data(), jobs.size(), W2);
    *out_len = W.text_bytes;
    for (uint64_t m = 0; m < W.n_members; ++m) {
        text_off[m] = jobs[m].out_off;
        status[m] = why[m] = 0;
    }
    text_off[W.n_members] = W.text_bytes;
    if (W.why != inf::W_OK) {
        status[W.n_members] = inf::status_of(W.why);
        why[W.n_members] = W.why;
        return -2;
    }
    if (out_cap < W.text_bytes)
        return -4;
    int rc = 0;
    for (uint64_t m = 0; m < W.n_members; ++m) {
        const int y = member(in + jobs[m].src_off, jobs[m].src_len, out + jobs[m].out_off, jobs[m].out_len, jobs[m].crc);
        if (y < 0)
            return -9;
        why[m] = (uint32_t)y;
        status[m] = inf::status_of((uint32_t)y);
        if (y)
            rc = -2;
    }
    return rc;
}

extern "C" uint32_t inflate_host_work_bytes() { return (uint32_t)sizeof(inf::Work); }

#ifdef INF_MAIN
#include <zlib.h>

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static std::vector<uint8_t> make_text(uint32_t n)
{
    std::vector<uint8_t> d(n);
    const uint32_t kind = rnd() % 6;
    const uint32_t period = 1 + rnd() % 200;
    for (uint32_t i = 0; i < n; ++i) {
        switch (kind) {
        case 0: d[i] = "ACGT"[rnd() & 3]; break;                                       // uniform ACGT
        case 1: d[i] = (uint8_t)rnd(); break;                                          // random bytes
        case 2: d[i] = i < period ? "ACGTN"[rnd() % 5] : d[i - period]; break;         // one period repeated
        case 3: d[i] = (rnd() % 50) ? 'N' : "ACGT"[rnd() & 3]; break;                  // runs
        case 4: d[i] = i >= 2000 && (rnd() % 64) ? d[i - 1 - rnd() % 2000] : "ACGTacgtN\n"[rnd() % 10]; break; // near copies
        default: d[i] = (uint8_t)(40 + (rnd() % (1 + rnd() % 60))); break;             // skewed letters
        }
    }
    return d;
}

static std::vector<uint8_t> raw_deflate(const std::vector<uint8_t> &d)
{
    static const int strategies[] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (deflateInit2(&z, (int)(rnd() % 10), Z_DEFLATED, -15, 1 + (int)(rnd() % 9), strategies[rnd() % 5]) != Z_OK)
        abort();
    std::vector<uint8_t> out(deflateBound(&z, (uLong)d.size()) + 64);
    std::vector<uint8_t> none(1);
    z.next_in = d.empty() ? none.data() : const_cast<uint8_t *>(d.data());
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    const uint32_t cut = d.empty() ? 0 : rnd() % d.size();
    if (rnd() % 3 == 0) { // several blocks: a full flush in the middle
        z.avail_in = cut;
        deflate(&z, Z_FULL_FLUSH);
    }
    z.avail_in = (uInt)(d.size() - z.total_in);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END)
        abort();
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

// zlib's verdict on the payload as a member of `isize` bytes with that CRC: its bytes in dec
static bool zlib_takes(const std::vector<uint8_t> &payload, uint32_t isize, uint32_t crc, std::vector<uint8_t> &dec)
{
    dec.assign((size_t)isize + 1, 0);
    std::vector<uint8_t> none(1);
    z_stream z;
    std::memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK)
        abort();
    z.next_in = payload.empty() ? none.data() : const_cast<uint8_t *>(payload.data());
    z.avail_in = (uInt)payload.size();
    z.next_out = dec.data();
    z.avail_out = (uInt)dec.size();
    const int rc = inflate(&z, Z_FINISH);
    const bool all = rc == Z_STREAM_END && z.avail_in == 0 && z.total_out == isize;
    inflateEnd(&z);
    dec.resize(isize);
    return all && crc32(0, dec.data(), isize) == crc;
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int rounds = argc > 2 ? atoi(argv[2]) : 100;
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    static const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 4096, 65280, 65536};
    int n_ok = 0, n_refused = 0;
    for (int r = 0; r < rounds; ++r) {
        const uint32_t n = r < (int)(sizeof sizes / sizeof *sizes) ? sizes[r] : rnd() % 3 ? rnd() % 3000 : rnd() % 65537;
        const std::vector<uint8_t> text = make_text(n);
        std::vector<uint8_t> payload = raw_deflate(text);
        uint32_t isize = n, crc = (uint32_t)crc32(0, text.data(), n);
        const bool damage = r >= (int)(sizeof sizes / sizeof *sizes) && rnd() % 3 != 0;
        if (damage) {
            const uint32_t how = rnd() % 8;
            // (the first bytes hold the block's header and code lengths: damage there meets the table checks)
            const uint32_t at = payload.empty() ? 0 : rnd() % 2 ? rnd() % (uint32_t)payload.size() : rnd() % (payload.size() < 40 ? (uint32_t)payload.size() : 40);
            if (how < 3 && !payload.empty())
                payload[at] ^= (uint8_t)(1u << (rnd() & 7));
            else if (how == 3 && !payload.empty())
                payload[at] = (uint8_t)rnd();
            else if (how == 4 && !payload.empty())
                payload.resize(at);
            else if (how == 5)
                payload.push_back((uint8_t)rnd());
            else if (how == 6)
                isize = rnd() % 2 ? isize + 1 + rnd() % 3 : isize ? isize - 1 : 1;
            else
                crc ^= 1u << (rnd() & 31);
            if (isize > inf::ISIZE_MAX)
                isize = inf::ISIZE_MAX;
        }
        std::vector<uint8_t> got((size_t)isize + 1), dec;
        const int why = member(payload.data(), (uint32_t)payload.size(), got.data(), isize, crc);
        got.resize(isize);
        const bool zl = zlib_takes(payload, isize, crc, dec);
        if (why < 0) {
            printf("FAILED round %d: a guard byte was written\n", r);
            return 1;
        }
        if (why == 0 && (!zl || got != dec)) {
            printf("FAILED round %d: accepted, zlib %s\n", r, zl ? "decodes other bytes" : "refuses");
            return 1;
        }
        // (stricter than zlib in one place only: an incomplete literal/length code of a single one-bit code)
        if (why != 0 && zl && why != (int)inf::W_INCOMPLETE) {
            printf("FAILED round %d: refused (why %d), zlib accepts\n", r, why);
            return 1;
        }
        if (!damage && why != 0) {
            printf("FAILED round %d: an undamaged member of %u bytes is refused (why %d)\n", r, n, why);
            return 1;
        }
        ++(why ? n_refused : n_ok);
    }
    printf("ok %d accepted %d refused\n", n_ok, n_refused);
    return 0;
}
#endif
