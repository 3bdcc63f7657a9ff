// parts_unpack.h -- what lies between a decoded archive part and the read path's other stages: where the sequences of a pack end
// (CSegment::get_raw / get cut a pack at its 0xFF terminators, src/common/segment.cpp:150-165, 536-545) and the symbols of a
// reference stored as tuples (tuples2bytes, src/common/segment.h:92-138).  The same source compiles for gfx950
// (parts_unpack_kernels.hip) and for the host (tests/partsunpack_host runs the kernels' order on the CPU: a wave is a loop over 64
// lanes).  No HIP calls.
//
// A pack is a run of sequences, each FOLLOWED by one 0xFF; deltas and symbol codes never hold 0xFF.  Sequence i ends at the offset of
// terminator i, it begins behind terminator i - 1 (sequence 0 at offset 0).  Bytes behind the last terminator belong to no sequence.
// A wave reads a pack in strips of 1024 bytes, 16 per lane (one 16-byte load; measured against nothing here -- chosen because a
// strip of 64 single bytes would take sixteen times the loads for the same ballots).  A lane knows which of its bytes are 0xFF (a
// 16-bit mask) and how many (0 .. 16: five bits).  Five ballots, one per bit of that number, give every lane the terminators of the
// lanes in front of it (popcounts of the ballots below its own bit) and the wave the strip's total, carried to the next strip.  The
// ordinal of a terminator -- bounded by the caller's cap before it indexes anything -- is the only thing an address is made from.
//
// A tuple stream is tuple bytes, one marker byte at the end.  Marker >> 4 = nb: 4, 3 or 2 symbols per tuple byte, as digits of base
// 4, 6 or 16, the first symbol the most significant; any other nb: the stream without its marker is the symbols.  Marker & 15: the
// symbols of the LAST tuple byte (the byte in front of the marker), 0 .. nb; when it is below nb that byte holds only that many
// digits.  So n = (size - 2) * nb + (marker & 15) symbols, symbol j lies in tuple byte j / nb.
#pragma once
#include <stdint.h>
#include "sym_view.h"

namespace agc {
namespace pu {

constexpr uint32_t LANE_BYTES = 16;         // pack bytes per lane and strip: one 16-byte load
constexpr uint32_t STRIP = 64 * LANE_BYTES; // per wave
constexpr uint8_t TERMINATOR = 0xFF;

// status of a part: the zstd decoder's two refusals (zs::dec::UNSUPPORTED / MALFORMED) keep their numbers
enum Status : uint32_t { OK = 0, ZSTD_UNSUPPORTED = 1, ZSTD_MALFORMED = 2, BAD_TUPLES = 3 };

// ---- packs ---------------------------------------------------------------------------------------------------------------------------
// a lane's bytes (byte i at bits [8 i, +7] of w0, i < 8, or [8 (i - 8), +7] of w1): bit i set where byte i, i < valid, is a terminator
SV_HD uint32_t terminator_mask(uint64_t w0, uint64_t w1, uint32_t valid)
{
    uint32_t m = 0;
    for (uint32_t i = 0; i < LANE_BYTES; ++i) {
        const uint8_t b = (uint8_t)((i < 8 ? w0 : w1) >> (8 * (i & 7)));
        m |= (uint32_t)(b == TERMINATOR && i < valid) << i;
    }
    return m;
}

SV_HD uint32_t popcount64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}

// bit l of b[j]: bit j of lane l's terminator count
struct CountBallots {
    uint64_t b[5];
};

SV_HD uint32_t terminators_in_front(const CountBallots &B, uint32_t lane)
{
    const uint64_t below = lane ? ~(uint64_t)0 >> (64 - lane) : 0;
    uint32_t n = 0;
    for (uint32_t j = 0; j < 5; ++j)
        n += popcount64(B.b[j] & below) << j;
    return n;
}

SV_HD uint32_t terminators_of_the_strip(const CountBallots &B)
{
    uint32_t n = 0;
    for (uint32_t j = 0; j < 5; ++j)
        n += popcount64(B.b[j]) << j;
    return n;
}

// the lane's stores: its terminators have the ordinals first, first + 1, ...; byte0 = the pack offset of the lane's first byte.
// Ordinals at or above seq_cap are counted by the caller and stored nowhere.
template <class P32> SV_HD void store_ends(P32 seq_end, uint32_t seq_cap, uint32_t first, uint32_t mask, uint32_t byte0)
{
    for (uint32_t i = 0; i < LANE_BYTES && first < seq_cap; ++i)
        if (mask >> i & 1)
            seq_end[first++] = byte0 + i;
}

// ---- tuples --------------------------------------------------------------------------------------------------------------------------
struct TupleShape {
    uint32_t status; // OK or BAD_TUPLES: the host routine would read or write outside its buffers
    uint32_t nb;     // 4, 3, 2, or 0: the symbols are the stream's bytes as they are
    uint64_t n;      // symbols
};

// size: the bytes of the stream, marker included; marker: its last byte (only looked at when size >= 2)
SV_HD TupleShape tuple_shape(uint64_t size, uint8_t marker)
{
    if (size < 2)
        return {BAD_TUPLES, 0, 0};
    const uint32_t nb = marker >> 4, last = marker & 15;
    if (nb != 4 && nb != 3 && nb != 2)
        return {OK, 0, size - 1};
    if (last > nb) // (tuples2bytes does not look: it would read the marker as a tuple byte and write behind its output)
        return {BAD_TUPLES, 0, 0};
    return {OK, nb, (size - 2) * nb + last};
}

SV_HD uint32_t tuple_base(uint32_t nb) { return nb == 4 ? 4 : nb == 3 ? 6 : 16; }

// symbols [lo, lo + cnt), 1 <= cnt <= 16, lo + cnt <= n, of a stream of shape (nb, n): symbol lo + i at bits [8 i, +7] of w0 (i < 8)
// or [8 (i - 8), +7] of w1.  Reads the tuple bytes that hold them -- t[lo / nb .. (lo + cnt - 1) / nb] -- once each, nothing else.
template <class P8> SV_HD void chunk_symbols(P8 t, uint32_t nb, uint64_t n, uint64_t lo, uint32_t cnt, uint64_t &w0, uint64_t &w1)
{
    w0 = w1 = 0;
    if (!nb) {
        for (uint32_t i = 0; i < cnt; ++i)
            (i < 8 ? w0 : w1) |= (uint64_t)t[lo + i] << (8 * (i & 7));
        return;
    }
    const uint32_t base = tuple_base(nb), last_digits = (uint32_t)(n % nb);
    const uint64_t whole = n / nb; // tuple bytes with nb digits; the one behind them has last_digits
    uint64_t q = lo / nb;
    uint32_t k = (uint32_t)(lo - q * nb), digits = q < whole ? nb : last_digits, c = t[q];
    for (uint32_t i = 0; i < cnt; ++i) {
        uint32_t v = c;
        for (uint32_t d = digits - 1 - k; d; --d)
            v /= base;
        (i < 8 ? w0 : w1) |= (uint64_t)(v % base) << (8 * (i & 7));
        if (++k == digits && i + 1 < cnt) {
            ++q;
            k = 0;
            digits = q < whole ? nb : last_digits;
            c = t[q];
        }
    }
}

} // namespace pu
} // namespace agc
