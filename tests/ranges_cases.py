"""Windows and ranges for the range tests (tests/test_ranges_host.py and tests/test_range_parts_cpu.py on the CPU,
tests/test_gpu_ranges.py on the GPU): the windows of a delta at which a clipped decode can still go wrong, and the ranges of a contig
at which the window arithmetic can."""
from tests.lzdec_cases import MML


def token_starts(delta, ref_size, mml=MML):
    """the decode-order position every token of a WELL-FORMED delta starts at, and the decoded length behind the last -> (starts, length)"""
    b, i, pred, out, starts = bytes(delta), 0, 0, 0, []

    def number():
        nonlocal i
        j = i
        while i < len(b) and 48 <= b[i] <= 57:
            i += 1
        return int(b[j:i] or b"0")

    while i < len(b):
        starts.append(out)
        c = b[i]
        if c == ord("!") or ord("A") <= c <= ord("A") + 20:
            i, pred, out = i + 1, pred + 1, out + 1
        elif c == 30:
            i += 1
            out += number() + 4
            assert b[i] == 4
            i += 1
        else:
            neg = c == ord("-")
            i += neg
            diff = -number() if neg else number()
            pos = pred + diff
            if b[i] == ord(","):
                i += 1
                n = number() + mml
            else:
                n = ref_size - pos
            assert b[i] == ord(".")
            i += 1
            pred, out = pos + n, out + n
    return starts, out


def delta_windows(starts, length):
    """(win_from, win_len) in the ORIENTED coordinates of a segment of `length` >= 1 symbols whose tokens start at `starts` in either
    orientation's mirror: all of it, the first symbol, the last, [t - 1, t + 1) around every token boundary t, and 15 / 16 / 17 / 63 /
    64 / 65 symbols from offsets 0, 1 and 15 -- each cut to the segment, none empty, none twice"""
    w = [(0, length), (0, 1), (length - 1, 1)]
    for t in starts:
        w += [(t - 1, 2), (length - t - 1, 2)]  # (the same boundary as a reverse-complemented segment has it)
    w += [(o, n) for o in (0, 1, 15) for n in (15, 16, 17, 63, 64, 65)]
    out = []
    for a, n in w:
        lo, hi = max(a, 0), min(a + n, length)
        if lo < hi and (lo, hi - lo) not in out:
            out.append((lo, hi - lo))
    return out


def contig_ranges(seg_lengths, k):
    """(from, to) of a contig whose segments have these lengths (overlap included): the whole contig, from > to, [0, 0], the last
    symbol, a range starting at the contig's length and one behind it, `to` beyond the end, around every segment boundary b (the
    position of a segment's first kept symbol) [b - 1, b], [b, b], [b - k, b + k], and one range spanning three segments"""
    bounds, pos = [], 0
    for i, n in enumerate(seg_lengths):
        if i:
            bounds.append(pos)
        pos += n - (k if i else 0)
    r = [(-1, -1), (7, 3), (0, 0), (pos - 1, pos - 1), (pos, pos + 5), (pos + 3, pos + 9), (max(pos - 4, 0), pos + 1000), (-5, 2), (3, -1)]
    for b in bounds:
        r += [(b - 1, b), (b, b), (b - k, b + k)]
    if len(bounds) >= 2:
        r.append((bounds[0] - 2, bounds[1] + 2))
    return r
