// range_plan.h -- the host arithmetic of a contig range.  The window arithmetic: which segments of a contig a range [from, to] touches
// and which symbols of each (decompress_contig's range rules, src/common/agc_decompressor_lib.cpp:172-286, as arithmetic on the
// segments' lengths) -- the host reader (host/reader.cpp: GetRangeParts) makes its window entries with it.  And the layout of
// agc_hip_ranges_parts (include/agc_hip.h): where every query and window goes in the output (step 1), and the jobs of the windows
// with the first complaint about them (step 4) -- read_api.hip only calls these and launches.  Plain C++17 without HIP and without
// the archive: read_api.hip uses the layout with the kernels' job records, tests/ranges_host with mirrors of them on the CPU.
//
// A contig is its segments back to back, every segment but the first without its first k symbols (the overlap with the segment in
// front).  Segment s of length L keeps skip = (s ? k : 0) .. L of its ORIENTED symbols; they are the contig's positions
// [pos, pos + L - skip).  A window is the part of that stretch inside the range, in the oriented segment's own coordinates: it
// starts at skip + (range start - pos) or at skip, so behind a contig's first segment win_from >= k.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/agc_hip.h"
#include "range_clip.h"

namespace agc {
namespace rp {

// symbols of a contig of n_seg segments (length(s): segment s's symbols, overlap included)
template <class Length> inline uint64_t contig_symbols(uint64_t n_seg, Length length, uint32_t k)
{
    uint64_t pos = 0;
    for (uint64_t s = 0; s < n_seg; ++s) {
        const uint64_t len = length(s), skip = s ? k : 0;
        pos += len >= skip ? len - skip : 0;
    }
    return pos;
}

// The range [from, to] (inclusive) as the reference reads it, on a contig of ctg_len symbols -> the positions [lo, hi) it yields:
// from < 0 is 0, to < 0 is the contig's end, from > to is the whole contig, everything is clamped to the contig.  A range that
// starts at or behind the contig's end yields nothing (lo == hi).
inline void clamp_range(int64_t from, int64_t to, uint64_t ctg_len, uint64_t &lo, uint64_t &hi)
{
    const int64_t END = 0x7fffffffffffffffLL;
    if (from < 0)
        from = 0;
    if (to < 0)
        to = END;
    else if (from > to)
        from = 0, to = END;
    lo = (uint64_t)from < ctg_len ? (uint64_t)from : ctg_len;
    hi = to == END || (uint64_t)to + 1 > ctg_len ? ctg_len : (uint64_t)to + 1;
}

// The windows of the range on a contig, in segment order: emit(s, win_from, win_len) for every segment that contributes at least
// one symbol (win_len >= 1); the windows back to back are the range's symbols.  -> their count
template <class Length, class Emit> inline uint64_t contig_windows(uint64_t n_seg, Length length, uint32_t k, int64_t from, int64_t to, Emit emit)
{
    uint64_t lo, hi;
    clamp_range(from, to, contig_symbols(n_seg, length, k), lo, hi);
    uint64_t pos = 0;
    for (uint64_t s = 0; s < n_seg && pos < hi; ++s) {
        const uint64_t len = length(s), skip = s ? k : 0, kept = len >= skip ? len - skip : 0;
        const uint64_t a = pos > lo ? pos : lo, b = pos + kept < hi ? pos + kept : hi;
        if (a < b)
            emit(s, (uint32_t)(skip + (a - pos)), (uint32_t)(b - a));
        pos += kept;
    }
    return hi - lo;
}

// a window against the segment it is cut from: at least one symbol, all of them inside the segment
inline bool window_fits(uint32_t win_from, uint32_t win_len, uint32_t length) { return win_len >= 1 && win_from <= length && win_len <= length - win_from; }

// ---- the layout of agc_hip_ranges_parts ---------------------------------------------------------------------------------------------
// Step 1.  Query q is the windows h_win[h_q_seg[q], h_q_seg[q + 1]) back to back: h_out_off[0..n_q], win_out[w] = where window w
// goes, total = h_out_off[n_q].  false, with nothing written: h_q_seg does not ascend from 0 or names more than 2^32 - 1 windows.
inline bool lay_out_queries(uint32_t n_q, const uint64_t *h_q_seg, const agc_hip_seg_win *h_win, uint64_t *h_out_off, std::vector<uint64_t> &win_out, uint64_t &total)
{
    const uint64_t n_win = h_q_seg[n_q];
    bool ascending = h_q_seg[0] == 0 && n_win <= 0xFFFFFFFFull;
    for (uint32_t q = 0; q < n_q; ++q)
        ascending = ascending && h_q_seg[q] <= h_q_seg[q + 1] && h_q_seg[q + 1] <= n_win;
    if (!ascending)
        return false;
    win_out.resize(n_win);
    total = 0;
    for (uint32_t q = 0; q < n_q; ++q) {
        h_out_off[q] = total;
        for (uint64_t w = h_q_seg[q]; w < h_q_seg[q + 1]; ++w) {
            win_out[w] = total;
            total += h_win[w].win_len;
        }
    }
    h_out_off[n_q] = total;
    return true;
}

// The work that fills the output, and the first complaint in window order.  DJ / WJ / CJ: DecodeJob (lz_decode_kernels.hip),
// WindowJob and WindowCopyJob (range_kernels.hip), made here member by member in their order.
template <class DJ, class WJ, class CJ> struct WindowLayout {
    std::vector<DJ> dj;           // the DELTA windows' deltas, for the scan against their lengths ...
    std::vector<uint32_t> dj_win; // ... and the window each belongs to
    std::vector<WJ> wj;           // the DELTA windows, dj's order
    std::vector<CJ> cj;           // the RAW / REF windows
    int code = AGC_HIP_OK;
    std::string why;
};

// Step 4: the windows (each passed step 2: a known kind, window_fits) at their places win_out.  locate(part, index, off, n, why):
// sequence `index` of pack `part` is bytes [off, off + n) -- or false and why = what is out of reach ("sequence 5 of part 2, which
// has 3 ...").  ref_size(gid): the symbols of the group's reference, new or registered.  Nothing behind the first complaint is looked at.
template <class DJ, class WJ, class CJ, class Locate, class RefSize>
WindowLayout<DJ, WJ, CJ> lay_out_windows(const char *call, uint64_t n_win, const agc_hip_seg_win *h_win, const uint64_t *win_out, Locate locate, RefSize ref_size)
{
    WindowLayout<DJ, WJ, CJ> Y;
    for (uint64_t w = 0; w < n_win && Y.code == AGC_HIP_OK; ++w) {
        const agc_hip_seg_win &g = h_win[w];
        const uint32_t rc = g.rc ? 1u : 0u;
        uint64_t off = 0;
        uint32_t n = 0;
        std::string why;
        if (g.kind != AGC_HIP_SEG_REF && !locate(g.part, g.index, off, n, why))
            why = "is " + why;
        else if (g.kind == AGC_HIP_SEG_DELTA) {
            Y.dj.push_back({off, n, 0, g.length, g.gid, rc, 0});
            Y.dj_win.push_back((uint32_t)w);
            WJ j = {off, n, win_out[w], 0, 0, g.gid, rc};
            rw::decode_window(g.win_from, g.win_len, g.length, rc, j.w_lo, j.w_hi);
            Y.wj.push_back(j);
        } else {
            const int64_t have = g.kind == AGC_HIP_SEG_RAW ? (int64_t)n : (int64_t)ref_size(g.gid);
            if (have != (int64_t)g.length)
                why = std::string("is of a ") + (g.kind == AGC_HIP_SEG_RAW ? "raw sequence" : "reference") + " of " + std::to_string(have) + " symbols, its length says " +
                      std::to_string(g.length);
            else
                Y.cj.push_back({off, win_out[w], g.length, g.win_from, g.win_len, g.gid, rc, g.kind == AGC_HIP_SEG_REF ? 1u : 0u});
        }
        if (!why.empty()) {
            Y.why = std::string(call) + ": window " + std::to_string(w) + " " + why;
            Y.code = AGC_HIP_EINVAL;
        }
    }
    return Y;
}

} // namespace rp
} // namespace agc
