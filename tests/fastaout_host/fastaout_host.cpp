// fastaout_host.cpp -- agc_amd/csrc/fasta_out.h on the CPU, in the order of fasta_text_kernel: chunk after chunk of 16 aligned
// bytes (the first and last one partial), each by fo::chunk_bytes exactly as a lane runs it.  TEST INFRASTRUCTURE ONLY.
//   -DFASTAOUT_MAIN: a stand-alone program (no Python): seeded random plans, the chunks against a plain contig-by-contig builder;
//   built with -fsanitize=address,undefined it also shows that no plan makes the walk leave its arrays (they are exact-size heap blocks).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../agc_amd/csrc/fasta_out.h"

using namespace agc;
typedef fo::PlanT<const uint64_t *, const uint32_t *, const uint8_t *> HostPlan;

// the text of a plan at alignment a (what the kernel's grid writes) -> out[0, total)
extern "C" void fo_text(uint32_t n_ctg, const uint64_t *ctg_text, const uint64_t *ctg_seg, const uint64_t *ctg_sym, const uint64_t *name_off, const uint8_t *names,
                        const uint64_t *seg_start, const uint64_t *seg_off, const uint32_t *skip, const uint8_t *sym, uint32_t line_length, uint32_t a,
                        uint64_t total, uint8_t *out)
{
    const HostPlan P = {ctg_text, ctg_seg, ctg_sym, name_off, names, seg_start, seg_off, skip, sym, n_ctg, line_length};
    const uint64_t n_chunks = fo::chunk_count(a, total);
    for (uint64_t j = 0; j < n_chunks; ++j) {
        uint64_t begin, w0, w1;
        uint32_t n;
        fo::chunk_range(j, a, total, begin, n);
        fo::chunk_bytes(P, begin, n, w0, w1);
        for (uint32_t i = 0; i < n; ++i)
            out[begin + i] = (uint8_t)((i < 8 ? w0 : w1) >> (8 * (i & 7)));
    }
}

// the layout arithmetic by itself
extern "C" uint64_t fo_contig_text_bytes(uint64_t name_len, uint64_t n_sym, uint32_t line_length) { return fo::contig_text_bytes(name_len, n_sym, line_length); }
extern "C" int fo_body_locate(uint64_t t, uint64_t n_sym, uint32_t line_length, uint64_t *sym)
{
    uint64_t col;
    return fo::body_locate(t, n_sym, fo::line_symbols(n_sym, line_length), col, *sym) ? 1 : 0;
}
extern "C" uint64_t fo_body_offset_of(uint64_t i, uint64_t n_sym, uint32_t line_length) { return fo::body_offset_of(i, fo::line_symbols(n_sym, line_length)); }
extern "C" uint32_t fo_letter(uint32_t c) { return fo::letter((uint8_t)c); }
extern "C" void fo_chunk_range(uint64_t j, uint32_t a, uint64_t total, uint64_t *begin, uint32_t *n) { fo::chunk_range(j, a, total, *begin, *n); }
extern "C" uint64_t fo_chunk_count(uint32_t a, uint64_t total) { return fo::chunk_count(a, total); }

#ifdef FASTAOUT_MAIN
namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

} // namespace

int main(int argc, char **argv)
{
    if (argc > 1)
        rng_state ^= strtoull(argv[1], nullptr, 10) * 0xD1342543DE82EF95ULL;
    const int rounds = argc > 2 ? atoi(argv[2]) : 4000;
    static const char ALPHA[] = "ACGTNRYSWKMBDHVU";
    uint64_t bytes = 0;
    for (int it = 0; it < rounds; ++it) {
        static const uint32_t lls[] = {0, 1, 2, 3, 15, 16, 17, 60, 80, 1000};
        const uint32_t k = rnd(3) ? 1 + rnd(40) : 0, line_length = lls[rnd(10)], n_ctg = 1 + rnd(it % 5 ? 6 : 60);
        std::vector<uint64_t> ctg_text, ctg_seg{0}, ctg_sym, name_off{0}, seg_start, seg_off;
        std::vector<uint32_t> skip;
        std::vector<uint8_t> names, sym, want;
        for (uint32_t c = 0; c < n_ctg; ++c) {
            const uint32_t name_len = rnd(8) ? rnd(20) : rnd(400), n_seg = rnd(6) ? rnd(6) : rnd(40);
            ctg_text.push_back(want.size());
            want.push_back('>');
            for (uint32_t i = 0; i < name_len; ++i) {
                names.push_back((uint8_t)(33 + rnd(90)));
                want.push_back(names.back());
            }
            want.push_back('\n');
            name_off.push_back(names.size());
            std::vector<uint8_t> ctg; // the contig's symbols, built the reader's way: append, without the first k
            for (uint32_t s = 0; s < n_seg; ++s) {
                const uint32_t sk = s ? k : 0;
                // a segment behind the first has at least k symbols; often exactly k (it keeps none)
                const uint32_t len = sk + (rnd(4) ? rnd(rnd(3) ? 70 : 700) : 0);
                seg_start.push_back(ctg.size());
                seg_off.push_back(sym.size());
                skip.push_back(sk);
                for (uint32_t i = 0; i < len; ++i) {
                    sym.push_back((uint8_t)(rnd(10) ? rnd(4) : rnd(3) ? rnd(16) : rnd(256)));
                    if (i >= sk)
                        ctg.push_back(sym.back());
                }
            }
            ctg_seg.push_back(seg_start.size());
            ctg_sym.push_back(ctg.size());
            const uint64_t L = line_length ? line_length : ctg.size();
            for (uint64_t i = 0; i < ctg.size(); ++i) {
                want.push_back(ctg[i] < 16 ? (uint8_t)ALPHA[ctg[i]] : (uint8_t)' ');
                if ((i + 1) % L == 0 || i + 1 == ctg.size())
                    want.push_back('\n');
            }
            if (want.size() - ctg_text.back() != fo::contig_text_bytes(name_len, ctg.size(), line_length)) {
                fprintf(stderr, "round %d contig %u: contig_text_bytes disagrees with the plain builder\n", it, c);
                return 1;
            }
        }
        ctg_text.push_back(want.size());
        // exact-size heap blocks: the sanitizer sees one element too far
        for (auto *v : {&ctg_text, &ctg_seg, &ctg_sym, &name_off, &seg_start, &seg_off})
            v->shrink_to_fit();
        skip.shrink_to_fit(), names.shrink_to_fit(), sym.shrink_to_fit();
        const uint32_t a = rnd(16);
        uint8_t *got = (uint8_t *)malloc(want.size());
        fo_text(n_ctg, ctg_text.data(), ctg_seg.data(), ctg_sym.data(), name_off.data(), names.data(), seg_start.data(), seg_off.data(), skip.data(), sym.data(),
                line_length, a, want.size(), got);
        for (uint64_t i = 0; i < want.size(); ++i)
            if (got[i] != want[i]) {
                fprintf(stderr, "round %d (k %u, line length %u, alignment %u): text byte %llu is %u, the plain builder has %u\n", it, k, line_length, a,
                        (unsigned long long)i, got[i], want[i]);
                return 1;
            }
        free(got);
        bytes += want.size();
    }
    printf("ok %d plans, %llu text bytes\n", rounds, (unsigned long long)bytes);
    return 0;
}
#endif
