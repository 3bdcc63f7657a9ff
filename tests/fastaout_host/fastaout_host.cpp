// fastaout_host.cpp -- agc_amd/csrc/fasta_out.h on the CPU, in the order of fasta_text_kernel: chunk after chunk of 16 aligned
// bytes (the first and last one partial), each by fo::chunk_bytes exactly as a lane runs it; and fasta_plan.h, the host arithmetic
// of agc_hip_sample_fasta, behind a table of reference sizes in the context's place.  TEST INFRASTRUCTURE ONLY.
//   -DFASTAOUT_MAIN: a stand-alone program (no Python): seeded random plans, the chunks against a plain contig-by-contig builder, and
//   fasta_plan.h's layout and packed block of the same plans against the arrays built by hand;
//   built with -fsanitize=address,undefined it also shows that no plan makes the walk leave its arrays (they are exact-size heap blocks).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../agc_amd/csrc/fasta_out.h"
#include "../../agc_amd/csrc/fasta_plan.h"

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

// ---- fasta_plan.h: the layout agc_hip_sample_fasta computes from a plan, and the block it uploads ------------------------------------
namespace {
// mirrors of DecodeJob (lz_decode_kernels.hip) and CopyJob (fasta_out_kernels.hip): the same members in the same order
struct DJ {
    uint64_t enc_off, enc_len, out_off;
    uint32_t out_len, ref_slot, rc, pad;
};
struct CJ {
    uint64_t src_off, out_off;
    uint32_t len, ref_slot, rc, is_ref;
};
typedef fp::SampleLayout<DJ, CJ> HostLayout;

// ref_size[gid], gid < n_refs: the size of the group's reference, < 0: not registered (the table stands in for the context)
HostLayout lay_out(uint32_t n_ctg, const uint64_t *ctg_seg, const agc_hip_seg_src *seg, uint64_t n_bytes, uint32_t k, uint32_t line_length, const uint64_t *name_off,
                   const int64_t *ref_size, uint32_t n_refs)
{
    return fp::lay_out_sample<DJ, CJ>(n_ctg, ctg_seg, seg, n_bytes, k, line_length, name_off, [=](uint32_t gid) { return gid < n_refs ? ref_size[gid] : (int64_t)-1; });
}

template <class T> void copy_out(const std::vector<T> &v, T *out)
{
    if (!v.empty())
        memcpy(out, v.data(), v.size() * sizeof(T));
}
} // namespace

// -> the complaint's code (0: none).  The arrays have room for the plan's counts (ctg_text: n_ctg + 1) and are left alone when the
// ranges do not ascend; dj / cj: one row per job -- the segment, then the job's members (7 and 6 numbers); sizes: n_dj, n_cj,
// sym_total, the text's size; why: the message, cut to why_cap - 1 characters
extern "C" int fp_layout(uint32_t n_ctg, const uint64_t *ctg_seg, const agc_hip_seg_src *seg, uint64_t n_bytes, uint32_t k, uint32_t line_length, const uint64_t *name_off,
                         const int64_t *ref_size, uint32_t n_refs, uint64_t *ctg_text, uint64_t *ctg_sym, uint64_t *seg_start, uint64_t *seg_off, uint32_t *skip,
                         uint64_t *dj, uint64_t *cj, uint64_t *sizes, char *why, uint32_t why_cap)
{
    const HostLayout Y = lay_out(n_ctg, ctg_seg, seg, n_bytes, k, line_length, name_off, ref_size, n_refs);
    copy_out(Y.ctg_text, ctg_text), copy_out(Y.ctg_sym, ctg_sym), copy_out(Y.seg_start, seg_start), copy_out(Y.seg_off, seg_off), copy_out(Y.skip, skip);
    for (size_t i = 0; i < Y.dj.size(); ++i) {
        const DJ &j = Y.dj[i];
        const uint64_t row[7] = {Y.dj_seg[i], j.enc_off, j.enc_len, j.out_off, j.out_len, j.ref_slot, j.rc};
        memcpy(dj + 7 * i, row, sizeof row);
    }
    for (size_t i = 0; i < Y.cj.size(); ++i) {
        const CJ &j = Y.cj[i];
        const uint64_t row[6] = {j.src_off, j.out_off, j.len, j.ref_slot, j.rc, j.is_ref};
        memcpy(cj + 6 * i, row, sizeof row);
    }
    sizes[0] = Y.dj.size(), sizes[1] = Y.cj.size(), sizes[2] = Y.sym_total, sizes[3] = Y.text;
    if (why_cap)
        snprintf(why, why_cap, "%s", Y.why.c_str());
    return Y.code;
}

// the block of a plan that lays out without complaint -> its size; block == nullptr: the size alone.  at[8]: the offsets of
// ctg_text, ctg_seg, ctg_sym, name_off, seg_start, seg_off, skip, names in it
extern "C" uint64_t fp_pack(uint32_t n_ctg, const uint64_t *ctg_seg, const agc_hip_seg_src *seg, uint64_t n_bytes, uint32_t k, uint32_t line_length, const char *names,
                            const uint64_t *name_off, const int64_t *ref_size, uint32_t n_refs, uint8_t *block, uint64_t *at)
{
    const fp::PlanBlock B = fp::pack_text_plan(lay_out(n_ctg, ctg_seg, seg, n_bytes, k, line_length, name_off, ref_size, n_refs), n_ctg, ctg_seg, names, name_off);
    const uint64_t a[8] = {B.ctg_text, B.ctg_seg, B.ctg_sym, B.name_off, B.seg_start, B.seg_off, B.skip, B.names};
    memcpy(at, a, sizeof a);
    if (block)
        copy_out(B.bytes, block);
    return B.bytes.size();
}

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
        std::vector<agc_hip_seg_src> segs; // the same sample as the plan agc_hip_sample_fasta is given: kinds at random
        std::vector<int64_t> ref_size;
        uint64_t n_bytes = 0;
        uint32_t n_delta = 0, n_copy = 0;
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
                const uint32_t kind = rnd(3), n_b = kind == AGC_HIP_SEG_RAW ? len : kind == AGC_HIP_SEG_DELTA ? rnd(50) : 0;
                if (kind != AGC_HIP_SEG_RAW)
                    ref_size.push_back(kind == AGC_HIP_SEG_REF ? (int64_t)len : (int64_t)rnd(1000)); // (a group of its own, or -1 slots in between)
                if (kind != AGC_HIP_SEG_RAW && !rnd(4))
                    ref_size.insert(ref_size.end() - 1, -1);
                segs.push_back({kind, kind == AGC_HIP_SEG_RAW ? rnd(9) : (uint32_t)ref_size.size() - 1, n_bytes, n_b, len, rnd(2), 0});
                n_bytes += n_b;
                n_delta += kind == AGC_HIP_SEG_DELTA;
                n_copy += kind != AGC_HIP_SEG_DELTA && len;
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
        // fasta_plan.h: the layout from the plan is the one built above; the block gives every array back (the names behind a prefix)
        segs.shrink_to_fit(), ref_size.shrink_to_fit();
        const HostLayout Y = lay_out(n_ctg, ctg_seg.data(), segs.data(), n_bytes, k, line_length, name_off.data(), ref_size.data(), (uint32_t)ref_size.size());
        if (Y.code || Y.ctg_text != ctg_text || Y.ctg_sym != ctg_sym || Y.seg_start != seg_start || Y.seg_off != seg_off || Y.skip != skip || Y.text != want.size() ||
            Y.sym_total != sym.size() || Y.dj.size() != n_delta || Y.dj_seg.size() != n_delta || Y.cj.size() != n_copy) {
            fprintf(stderr, "round %d: lay_out_sample disagrees with the plan built by hand (code %d: %s)\n", it, Y.code, Y.why.c_str());
            return 1;
        }
        const uint64_t shift = rnd(3) ? rnd(100) : 0;
        std::vector<uint64_t> name_off2(name_off);
        for (uint64_t &o : name_off2)
            o += shift;
        std::vector<char> names2(shift + names.size(), '#');
        if (!names.empty())
            memcpy(names2.data() + shift, names.data(), names.size());
        names2.shrink_to_fit(), name_off2.shrink_to_fit();
        const fp::PlanBlock B = fp::pack_text_plan(Y, n_ctg, ctg_seg.data(), names2.data(), name_off2.data());
        const struct {
            size_t at;
            const void *src;
            size_t n;
        } fields[] = {{B.ctg_text, ctg_text.data(), 8 * ctg_text.size()}, {B.ctg_seg, ctg_seg.data(), 8 * ctg_seg.size()}, {B.ctg_sym, ctg_sym.data(), 8 * ctg_sym.size()},
                      {B.name_off, name_off.data(), 8 * name_off.size()}, {B.seg_start, seg_start.data(), 8 * seg_start.size()}, {B.seg_off, seg_off.data(), 8 * seg_off.size()},
                      {B.skip, skip.data(), 4 * skip.size()},             {B.names, names.data(), names.size()}};
        size_t end = 0;
        for (const auto &f : fields) {
            if (f.at != end || f.at + f.n > B.bytes.size() || (f.n && memcmp(B.bytes.data() + f.at, f.src, f.n))) {
                fprintf(stderr, "round %d: pack_text_plan: the field at %llu is not its array\n", it, (unsigned long long)f.at);
                return 1;
            }
            end += f.n;
        }
        if (end != B.bytes.size()) {
            fprintf(stderr, "round %d: pack_text_plan: a block of %llu bytes, its fields have %llu\n", it, (unsigned long long)B.bytes.size(), (unsigned long long)end);
            return 1;
        }
        bytes += want.size();
    }
    printf("ok %d plans, %llu text bytes\n", rounds, (unsigned long long)bytes);
    return 0;
}
#endif
