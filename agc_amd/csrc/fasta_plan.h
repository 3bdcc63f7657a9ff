// fasta_plan.h -- the host arithmetic of agc_hip_sample_fasta (include/agc_hip.h): what a sample's plan says about the symbol buffer
// and the text (fasta_out.h's layout), which segments it refuses, and the block the text kernel's arrays travel in.  Plain C++17
// without HIP: read_api.hip uses it with the kernels' job records, tests/fastaout_host with mirrors of them on the CPU.
#pragma once
#include <stdint.h>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/agc_hip.h"
#include "fasta_out.h"

namespace agc {
namespace fp {

// Where everything lies -- the arrays of fo::PlanT the host makes, the sizes, the first complaint -- and the work that fills the symbol
// buffer.  DJ / CJ: DecodeJob (lz_decode_kernels.hip) and CopyJob (fasta_out_kernels.hip), made here member by member in their order.
template <class DJ, class CJ> struct SampleLayout {
    std::vector<uint64_t> ctg_text, ctg_sym, seg_start, seg_off;
    std::vector<uint32_t> skip;
    std::vector<DJ> dj;               // the DELTA segments ...
    std::vector<uint32_t> dj_seg;     // ... and the segment each is
    std::vector<CJ> cj;               // the RAW / REF segments that have symbols
    uint64_t sym_total = 0, text = 0; // symbols of all segments (each whole: the symbol buffer's size), bytes of the text
    int code = AGC_HIP_OK;            // the first complaint: AGC_HIP_EINVAL / AGC_HIP_ENOREF ...
    std::string why;                  // ... and its message
};

// The layout of a sample with n_ctg >= 1 contigs.  ref_size(gid): the size of the group's registered reference, < 0: it has none.
// The ranges and name offsets must ascend from 0, or nothing else is looked at (text stays 0).  Then every segment is visited, also
// behind a complaint -- the text's size is the plan's arithmetic alone; a segment that is refused gets no job.
template <class DJ, class CJ, class RefSize>
SampleLayout<DJ, CJ> lay_out_sample(uint32_t n_ctg, const uint64_t *h_ctg_seg, const agc_hip_seg_src *h_seg, uint64_t n_bytes, uint32_t k, uint32_t line_length,
                                    const uint64_t *h_name_off, RefSize ref_size)
{
    SampleLayout<DJ, CJ> Y;
    const uint64_t n_seg = h_ctg_seg[n_ctg];
    bool ascending = h_ctg_seg[0] == 0 && n_seg <= 0xFFFFFFFFull;
    for (uint32_t ci = 0; ci < n_ctg; ++ci)
        ascending = ascending && h_ctg_seg[ci] <= h_ctg_seg[ci + 1] && h_ctg_seg[ci + 1] <= n_seg && h_name_off[ci] <= h_name_off[ci + 1];
    if (!ascending) {
        Y.why = "sample_fasta: the contigs' segment ranges or name offsets do not ascend from 0";
        Y.code = AGC_HIP_EINVAL;
        return Y;
    }
    Y.ctg_text.resize((size_t)n_ctg + 1), Y.ctg_sym.resize(n_ctg), Y.seg_start.resize(n_seg), Y.seg_off.resize(n_seg), Y.skip.resize(n_seg);
    for (uint32_t ci = 0; ci < n_ctg; ++ci) {
        uint64_t pos = 0;
        for (uint64_t s = h_ctg_seg[ci]; s < h_ctg_seg[ci + 1]; ++s) {
            const agc_hip_seg_src &g = h_seg[s];
            const uint32_t sk = s == h_ctg_seg[ci] ? 0 : k;
            const char *why = nullptr;
            int code = AGC_HIP_EINVAL;
            if (g.kind > AGC_HIP_SEG_DELTA)
                why = "has an unknown kind";
            else if (g.kind != AGC_HIP_SEG_REF && (g.off > n_bytes || g.n_bytes > n_bytes - g.off))
                why = "names bytes outside the byte buffer";
            else if (g.kind == AGC_HIP_SEG_RAW && g.n_bytes != g.length)
                why = "is raw and its byte count differs from its length";
            else if (g.kind != AGC_HIP_SEG_RAW && ref_size(g.gid) < 0)
                why = "names a group without a registered reference", code = AGC_HIP_ENOREF;
            else if (g.kind == AGC_HIP_SEG_REF && (uint64_t)ref_size(g.gid) != g.length)
                why = "is a reference whose size differs from its length";
            else if (g.length < sk)
                why = "is shorter than the overlap with the segment in front of it";
            if (why && Y.code == AGC_HIP_OK) {
                Y.why = "sample_fasta: segment " + std::to_string(s) + " (contig " + std::to_string(ci) + ") " + why;
                Y.code = code;
            }
            Y.seg_start[s] = pos;
            Y.seg_off[s] = Y.sym_total;
            Y.skip[s] = sk;
            if (!why && g.kind == AGC_HIP_SEG_DELTA) {
                Y.dj.push_back({g.off, g.n_bytes, Y.sym_total, g.length, g.gid, g.rc ? 1u : 0u, 0});
                Y.dj_seg.push_back((uint32_t)s);
            } else if (!why && g.length)
                Y.cj.push_back({g.off, Y.sym_total, g.length, g.gid, g.rc ? 1u : 0u, g.kind == AGC_HIP_SEG_REF ? 1u : 0u});
            pos += g.length >= sk ? g.length - sk : 0;
            Y.sym_total += g.length;
        }
        Y.ctg_sym[ci] = pos;
        Y.ctg_text[ci] = Y.text;
        Y.text += fo::contig_text_bytes(h_name_off[ci + 1] - h_name_off[ci], pos, line_length);
    }
    Y.ctg_text[n_ctg] = Y.text;
    return Y;
}

// The text's size alone, for a caller that must know it before it has what lay_out_sample asks for (agc_hip_sample_fasta_parts:
// before the parts are unpacked): length(s) = segment s's symbols.  The same arithmetic, so the same number as SampleLayout::text;
// false: the ranges or name offsets do not ascend from 0.
template <class Length>
bool plan_text_bytes(uint32_t n_ctg, const uint64_t *h_ctg_seg, uint32_t k, uint32_t line_length, const uint64_t *h_name_off, Length length, uint64_t &text)
{
    const uint64_t n_seg = h_ctg_seg[n_ctg];
    bool ascending = h_ctg_seg[0] == 0 && n_seg <= 0xFFFFFFFFull;
    for (uint32_t ci = 0; ci < n_ctg; ++ci)
        ascending = ascending && h_ctg_seg[ci] <= h_ctg_seg[ci + 1] && h_ctg_seg[ci + 1] <= n_seg && h_name_off[ci] <= h_name_off[ci + 1];
    text = 0;
    if (!ascending)
        return false;
    for (uint32_t ci = 0; ci < n_ctg; ++ci) {
        uint64_t pos = 0;
        for (uint64_t s = h_ctg_seg[ci]; s < h_ctg_seg[ci + 1]; ++s) {
            const uint32_t sk = s == h_ctg_seg[ci] ? 0 : k, len = length(s);
            pos += len >= sk ? len - sk : 0;
        }
        text += fo::contig_text_bytes(h_name_off[ci + 1] - h_name_off[ci], pos, line_length);
    }
    return true;
}

// the text kernel's arrays in one block (one upload): the 64-bit arrays, the 32-bit one, the names; every member but `bytes` is
// the offset of that array of fo::PlanT in it
struct PlanBlock {
    std::vector<uint8_t> bytes;
    size_t ctg_text = 0, ctg_seg = 0, ctg_sym = 0, name_off = 0, seg_start = 0, seg_off = 0, skip = 0, names = 0;
};

// (name_off is rebased: the block holds names[h_name_off[0], h_name_off[n_ctg]) only)
template <class Layout> PlanBlock pack_text_plan(const Layout &Y, uint32_t n_ctg, const uint64_t *h_ctg_seg, const char *h_names, const uint64_t *h_name_off)
{
    const size_t n_seg = (size_t)h_ctg_seg[n_ctg];
    std::vector<uint64_t> name_off(h_name_off, h_name_off + n_ctg + 1);
    for (uint64_t &o : name_off)
        o -= h_name_off[0];
    const size_t names_bytes = (size_t)name_off[n_ctg];
    const struct {
        size_t PlanBlock::*at;
        const void *src;
        size_t n;
    } fields[] = {{&PlanBlock::ctg_text, Y.ctg_text.data(), 8 * ((size_t)n_ctg + 1)}, {&PlanBlock::ctg_seg, h_ctg_seg, 8 * ((size_t)n_ctg + 1)},
                  {&PlanBlock::ctg_sym, Y.ctg_sym.data(), 8 * (size_t)n_ctg},         {&PlanBlock::name_off, name_off.data(), 8 * ((size_t)n_ctg + 1)},
                  {&PlanBlock::seg_start, Y.seg_start.data(), 8 * n_seg},             {&PlanBlock::seg_off, Y.seg_off.data(), 8 * n_seg},
                  {&PlanBlock::skip, Y.skip.data(), 4 * n_seg},                       {&PlanBlock::names, names_bytes ? h_names + h_name_off[0] : nullptr, names_bytes}};
    PlanBlock B;
    size_t end = 0;
    for (const auto &f : fields) {
        B.*f.at = end;
        end += f.n;
    }
    B.bytes.resize(end);
    for (const auto &f : fields)
        if (f.n)
            std::memcpy(B.bytes.data() + B.*f.at, f.src, f.n);
    return B;
}

} // namespace fp
} // namespace agc
