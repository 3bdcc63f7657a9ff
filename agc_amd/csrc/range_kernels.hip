// range_kernels.hip -- windows of segments for gfx950 (wave64): what a batch of contig ranges needs of each segment it touches,
// written straight to its place in the output; the whole segment is never materialised (clip arithmetic: range_clip.h).
//   lz_decode_window_kernel  lz_decode_write_kernel's walk (lzd::walk_delta, one wave per job, four independent waves a block, no
//                            LDS, no barrier) with a window [w_lo, w_hi) of decode-order positions: every token is cut to the
//                            window before it writes -- a literal writes if its position is inside, an N-run or a match writes
//                            its cut stretch, a cut match reading the reference from ref_pos + (lo - at) -- and the walk stops at
//                            the first strip whose first token starts at or behind w_hi.  Launched only on deltas
//                            lz_decode_scan_kernel accepted, with windows inside the length it reported.
//   segment_window_kernel    the window of a reference as it is (lzd::wave_copy from the mirrored start) or of raw symbol bytes
//                            (segment_copy_kernel's byte loop over the window); one wave per job.
//   letters_kernel           symbol codes -> "ACGTNRYSWKMBDHVU" (fo::letter) in place: a lane owns 16 consecutive, 16-byte-aligned
//                            bytes, one load and one store; the unaligned head and the tail byte by byte.
#include "dev_common.h"
#include "fasta_out.h"
#include "lz_decode.h"
#include "range_clip.h"

namespace agc {

struct WindowJob {
    uint64_t enc_off; // the delta: enc[enc_off, enc_off + enc_len)
    uint64_t enc_len;
    uint64_t out_off; // the window's symbols go to out[out_off, out_off + w_hi - w_lo)
    uint32_t w_lo;    // the window in decode order (rw::decode_window)
    uint32_t w_hi;
    uint32_t ref_slot; // index into the RefDesc array
    uint32_t rc;
};

struct WindowCopyJob {
    uint64_t src_off; // raw: the segment's symbols are bytes[src_off, src_off + len)
    uint64_t out_off; // the window's symbols go to out[out_off, out_off + win_len)
    uint32_t len;     // the whole segment (a reference: ref_size)
    uint32_t win_from; // the window, in the oriented segment's coordinates
    uint32_t win_len;
    uint32_t ref_slot; // reference: index into the RefDesc array
    uint32_t rc;
    uint32_t is_ref;
};

__global__ void __launch_bounds__(256) lz_decode_window_kernel(const RefDesc *__restrict__ refs, const WindowJob *__restrict__ jobs, uint32_t n_jobs,
                                                              const uint8_t *__restrict__ enc, uint8_t *__restrict__ out)
{
    using namespace lzd;
    const uint32_t s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (s >= n_jobs)
        return;
    const WindowJob jb = jobs[s];
    const RefDesc rd = refs[jb.ref_slot];
    const SymViewG rv = {(g_u32 *)rd.words, (g_i32 *)rd.esc_index, (g_u8 *)rd.esc_bytes, 0, rd.ref_size, 0};
    uint8_t *dst = out + jb.out_off;
    const uint32_t w_lo = jb.w_lo, w_hi = jb.w_hi, rc = jb.rc;
    walk_delta((g_u8 *)enc + jb.enc_off, jb.enc_len, rd.ref_size, rd.min_match_len, [&](const Token &t, const State &before) {
        // lane 0 holds the State in front of the strip: where its first token starts.  Behind the window nothing is left to write
        if (shfl_u64(before.out, 0) >= w_hi)
            return false;
        const uint64_t at = before.out; // (< 2^32: the scan accepted the delta)
        if ((t.kind == LITERAL || t.kind == LITERAL_REF) && rw::inside(at, w_lo, w_hi)) {
            const uint8_t c = t.kind == LITERAL ? (uint8_t)t.n : (uint8_t)sv_buf_sym(rv, (uint64_t)before.pred, false);
            dst[rw::dst_offset((uint32_t)at, 1, w_lo, w_hi, rc)] = rc ? complement(c) : c;
        }
        uint32_t lo = w_lo, cnt = 0;
        if (t.kind == NRUN || t.kind == MATCH || t.kind == MATCH_TO_END)
            rw::clip(at, match_symbols(t, before, rd.ref_size), w_lo, w_hi, lo, cnt);
        const uint64_t ref_pos = (uint64_t)match_ref_pos(t, before) + (lo - at); // (of the cut stretch's first symbol)
        for (uint64_t todo = __ballot(cnt != 0); todo; todo &= todo - 1) {         // the strip's cut N-runs and matches, each by the whole wave
            const uint32_t l = ctz64(todo);
            const uint32_t cnt_l = __shfl(cnt, l), lo_l = __shfl(lo, l);
            uint8_t *d = dst + rw::dst_offset(lo_l, cnt_l, w_lo, w_hi, rc);
            if (__shfl(t.kind, l) == NRUN)
                for (uint32_t q = lane_id(); q < cnt_l; q += WAVE)
                    d[q] = N_CODE;
            else
                wave_copy(rd, shfl_u64(ref_pos, l), cnt_l, rc, d);
        }
        return true;
    });
}

// (only ever launched on windows the host checked against the segment's size: win_from + win_len <= len)
__global__ void __launch_bounds__(256) segment_window_kernel(const RefDesc *__restrict__ refs, const WindowCopyJob *__restrict__ jobs, uint32_t n_jobs,
                                                            const uint8_t *__restrict__ bytes, uint8_t *__restrict__ out)
{
    const uint32_t s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (s >= n_jobs)
        return;
    const WindowCopyJob jb = jobs[s];
    uint8_t *dst = out + jb.out_off;
    uint32_t w_lo, w_hi;
    rw::decode_window(jb.win_from, jb.win_len, jb.len, jb.rc, w_lo, w_hi);
    if (jb.is_ref) {
        const RefDesc rd = refs[jb.ref_slot];
        lzd::wave_copy(rd, w_lo, jb.win_len, jb.rc, dst);
        return;
    }
    g_u8 *src = (g_u8 *)bytes + jb.src_off;
    for (uint32_t q = lane_id(); q < jb.win_len; q += WAVE)
        dst[q] = jb.rc ? lzd::complement(src[w_hi - 1 - q]) : src[w_lo + q];
}

// sym: the first of `total` symbol codes, at an address with (address & 15) == a
__global__ void __launch_bounds__(256) letters_kernel(uint8_t *__restrict__ sym, uint32_t a, uint64_t total, uint64_t n_chunks)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_chunks)
        return;
    uint64_t begin;
    uint32_t n;
    fo::chunk_range(j, a, total, begin, n);
    if (n == fo::CHUNK) {
        uint4 v = *(const uint4 *)(sym + begin); // (begin + a is a multiple of 16)
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            w[i] = (uint32_t)fo::letter((uint8_t)w[i]) | (uint32_t)fo::letter((uint8_t)(w[i] >> 8)) << 8 | (uint32_t)fo::letter((uint8_t)(w[i] >> 16)) << 16 |
                   (uint32_t)fo::letter((uint8_t)(w[i] >> 24)) << 24;
        *(uint4 *)(sym + begin) = make_uint4(w[0], w[1], w[2], w[3]);
    } else
        for (uint32_t i = 0; i < n; ++i)
            sym[begin + i] = fo::letter(sym[begin + i]);
}

} // namespace agc
