// range_plan.h -- the window arithmetic of a contig range: which segments of a contig a range [from, to] touches and which symbols of
// each (decompress_contig's range rules, src/common/agc_decompressor_lib.cpp:172-286, as arithmetic on the segments' lengths).
// Plain C++ without HIP and without the archive: the host reader (host/reader.cpp: GetRangeParts) makes its window entries with it,
// the device call's argument checks (read_api.hip: agc_hip_ranges_parts) and tests/ranges_host use the same functions.
//
// A contig is its segments back to back, every segment but the first without its first k symbols (the overlap with the segment in
// front).  Segment s of length L keeps skip = (s ? k : 0) .. L of its ORIENTED symbols; they are the contig's positions
// [pos, pos + L - skip).  A window is the part of that stretch inside the range, in the oriented segment's own coordinates: it
// starts at skip + (range start - pos) or at skip, so behind a contig's first segment win_from >= k.
#pragma once
#include <stdint.h>

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

} // namespace rp
} // namespace agc
