// range_clip.h -- the clip arithmetic of the windowed segment writers (range_kernels.hip): a window of a segment's ORIENTED symbols
// in the order the segment is decoded in, a token's stretch cut to it, and where the cut stretch lands in the window's compact
// output.  The same source compiles for gfx950 and for the host (tests/ranges_host walks the tokens in the kernel's order on the
// CPU and compares every window with the full decode, sliced).  No HIP calls.
//
// A segment of `len` symbols is decoded forward (decode-order position q = 0 .. len - 1); its oriented symbol i is decode-order
// symbol i, or -- reverse-complemented -- the complement of decode-order symbol len - 1 - i.  The oriented window [a, a + n) is
// therefore the decode-order stretch [w_lo, w_hi) = [a, a + n), or [len - a - n, len - a) for rc: the same symbols, mirrored.
// The output holds the window alone, oriented: decode-order position q of the window goes to byte q - w_lo, for rc to w_hi - 1 - q
// (the window is mirrored inside itself); a stretch [lo, lo + cnt) to the bytes from lo - w_lo, for rc from w_hi - lo - cnt.
#pragma once
#include <stdint.h>
#include "sym_view.h"

namespace agc {
namespace rw {

// the oriented window [win_from, win_from + win_len) of a segment of len symbols (it fits: win_from + win_len <= len) in decode order
SV_HD void decode_window(uint32_t win_from, uint32_t win_len, uint32_t len, uint32_t rc, uint32_t &w_lo, uint32_t &w_hi)
{
    w_lo = rc ? len - win_from - win_len : win_from;
    w_hi = w_lo + win_len;
}

// the stretch [at, at + n) of decode-order positions cut to the window: [lo, lo + cnt), cnt == 0 when nothing of it is inside
SV_HD void clip(uint64_t at, uint64_t n, uint32_t w_lo, uint32_t w_hi, uint32_t &lo, uint32_t &cnt)
{
    const uint64_t a = at > w_lo ? at : w_lo, b = at + n < w_hi ? at + n : w_hi;
    lo = (uint32_t)(a < b ? a : w_lo);
    cnt = (uint32_t)(a < b ? b - a : 0);
}

SV_HD bool inside(uint64_t at, uint32_t w_lo, uint32_t w_hi) { return at >= w_lo && at < w_hi; }

// where the cut stretch [lo, lo + cnt) (inside the window, cnt >= 1) begins in the window's output
SV_HD uint32_t dst_offset(uint32_t lo, uint32_t cnt, uint32_t w_lo, uint32_t w_hi, uint32_t rc) { return rc ? w_hi - lo - cnt : lo - w_lo; }

} // namespace rw
} // namespace agc
