// lz_decode_kernels.hip -- LZ-diff decode for gfx950 (wave64): CLZDiff_V2::Decode (src/common/lz_diff.cpp:801-836) for a batch of
// deltas against registered references, as two scans instead of a byte loop (grammar, token-start rule and scan: lz_decode.h).
//
// One wavefront per delta, a block is four independent waves (no LDS, no barrier).  A wave walks its delta in strips of 64
// bytes, one byte per lane: a ballot of the bytes that end a token gives the token starts, the lanes that start a token parse
// it, a wave scan of the tokens' Steps gives every token pred_pos and the output offset in front of it.
//   lz_decode_scan_kernel   walks once: decoded length and status per delta.  It reads the delta bytes and two scalars of the
//                           reference's descriptor, never the reference: the host launches the second kernel only when every
//                           delta of the batch is well formed, so no address is ever computed from a malformed delta.
//   lz_decode_write_kernel  walks again and writes: a literal by its lane, an N-run or a match by all 64 lanes (16 symbols a
//                           lane and step: two words of the 2-bit reference -> one 16-byte store; escaped blocks byte by byte).
//                           A reverse-complemented delta is written in place by index: symbol q goes to len - 1 - q.
#include "dev_common.h"
#include "lz_decode.h"

namespace agc {

struct DecodeJob {
    uint64_t enc_off; // the delta: enc[enc_off, enc_off + enc_len)
    uint64_t enc_len;
    uint64_t out_off; // write kernel: the decoded symbols go to out[out_off, out_off + out_len)
    uint32_t out_len;
    uint32_t ref_slot; // index into the RefDesc array
    uint32_t rc;
    uint32_t pad;
};

struct DecodeResult {
    uint32_t len;    // decoded symbols
    uint32_t status; // lzd::Status
};

namespace lzd {

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, uint32_t d)
{
    return ((uint64_t)__shfl_up((uint32_t)(v >> 32), d) << 32) | __shfl_up((uint32_t)v, d);
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t src)
{
    return ((uint64_t)__shfl((uint32_t)(v >> 32), src) << 32) | __shfl((uint32_t)v, src);
}
__device__ __forceinline__ Step shfl_up_step(const Step &s, uint32_t d) { return {__shfl_up(s.set, d), shfl_up_u64(s.p, d), shfl_up_u64(s.o, d)}; }
__device__ __forceinline__ Step shfl_step(const Step &s, uint32_t src) { return {__shfl(s.set, src), shfl_u64(s.p, src), shfl_u64(s.o, src)}; }

// The walk both kernels share: visit(token, state) is called by all 64 lanes once per strip with the token that starts at the
// lane's byte (kind NONE: none does) and the State in front of it; it returns false to stop the walk (wave-uniform).
// -> the State behind the last token visited.
template <class F> __device__ __forceinline__ State walk_delta(g_u8 *enc, uint64_t enc_len, uint32_t ref_size, uint32_t min_match_len, F visit)
{
    const uint32_t lane = lane_id();
    State carry = {0, 0};
    uint32_t carry_end = 1;
    for (uint64_t base = 0; base < enc_len; base += STRIP) {
        const uint64_t i = base + lane;
        const bool in = i < enc_len;
        const uint8_t c = in ? enc[i] : 0;
        const uint64_t ends = __ballot(in && ends_token(c));
        const uint64_t starts = token_starts(ends, __ballot(in), carry_end);
        carry_end = starts_carry(ends);
        Token t = {NONE, 0, 0};
        if ((starts >> lane) & 1)
            t = parse_token(enc + i, enc_len - i, min_match_len); // (reads on into the next strip, never past the delta)
        Step incl = step_of(t, ref_size);
#pragma unroll
        for (uint32_t d = 1; d < WAVE; d <<= 1) {
            const Step up = shfl_up_step(incl, d);
            if (lane >= d)
                incl = combine(up, incl);
        }
        Step excl = shfl_up_step(incl, 1);
        if (lane == 0)
            excl = identity();
        if (!visit(t, apply(excl, carry)))
            break;
        carry = apply(shfl_step(incl, WAVE - 1), carry);
    }
    return carry;
}

// n symbols of the reference from ref_pos as bytes at dst (whole wave); rc: the reverse complement of that stretch
__device__ __forceinline__ void wave_copy(const RefDesc &rd, uint64_t ref_pos, uint32_t n, uint32_t rc, uint8_t *__restrict__ dst)
{
    const SymViewG v = {(g_u32 *)rd.words, (g_i32 *)rd.esc_index, (g_u8 *)rd.esc_bytes, ref_pos, n, rc};
    for (uint64_t pos64 = (uint64_t)lane_id() * 16; pos64 < n; pos64 += WAVE * 16) {
        const uint32_t pos = (uint32_t)pos64, cnt = n - pos < 16 ? n - pos : 16;
        uint64_t P;
        uint32_t I;
        sv_fetch16(v, pos, cnt, false, P, I);
        if (cnt == 16 && I == 0) {
            const uint32_t lo = (uint32_t)P;
            const uint4 b = make_uint4(sv_expand4(lo), sv_expand4(lo >> 8), sv_expand4(lo >> 16), sv_expand4(lo >> 24));
            __builtin_memcpy(dst + pos64, &b, 16);
        } else
            for (uint32_t j = 0; j < cnt; ++j)
                dst[pos64 + j] = (uint8_t)(((I >> j) & 1u) ? sv_sym(v, pos + j) : (uint32_t)(P >> (2u * j)) & 3u);
    }
}

} // namespace lzd

__global__ void __launch_bounds__(256) lz_decode_scan_kernel(const RefDesc *__restrict__ refs, const DecodeJob *__restrict__ jobs, uint32_t n_jobs,
                                                            const uint8_t *__restrict__ enc, DecodeResult *__restrict__ res)
{
    using namespace lzd;
    const uint32_t s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (s >= n_jobs)
        return;
    const DecodeJob jb = jobs[s];
    const uint32_t ref_size = refs[jb.ref_slot].ref_size, min_match_len = refs[jb.ref_slot].min_match_len;
    uint32_t status = OK;
    const State end = walk_delta((g_u8 *)enc + jb.enc_off, jb.enc_len, ref_size, min_match_len, [&](const Token &t, const State &before) {
        const uint32_t st = t.kind == NONE ? (uint32_t)OK : check_token(t, before, ref_size);
        const uint64_t bad = __ballot(st != OK);
        if (bad)
            status = __shfl(st, ctz64(bad)); // the first bad token's
        return bad == 0;
    });
    if (status == OK)
        status = check_length(end.out);
    if (lane_id() == 0)
        res[s] = {(uint32_t)end.out, status};
}

// (only ever launched on deltas lz_decode_scan_kernel accepted, with out_len the length it reported)
__global__ void __launch_bounds__(256) lz_decode_write_kernel(const RefDesc *__restrict__ refs, const DecodeJob *__restrict__ jobs, uint32_t n_jobs,
                                                             const uint8_t *__restrict__ enc, uint8_t *__restrict__ out)
{
    using namespace lzd;
    const uint32_t s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (s >= n_jobs)
        return;
    const DecodeJob jb = jobs[s];
    const RefDesc rd = refs[jb.ref_slot];
    const SymViewG rv = {(g_u32 *)rd.words, (g_i32 *)rd.esc_index, (g_u8 *)rd.esc_bytes, 0, rd.ref_size, 0};
    uint8_t *dst = out + jb.out_off;
    const uint32_t total = jb.out_len, rc = jb.rc;
    walk_delta((g_u8 *)enc + jb.enc_off, jb.enc_len, rd.ref_size, rd.min_match_len, [&](const Token &t, const State &before) {
        const uint32_t at = (uint32_t)before.out; // (< total <= 2^32 - 1)
        if (t.kind == LITERAL || t.kind == LITERAL_REF) {
            const uint8_t c = t.kind == LITERAL ? (uint8_t)t.n : (uint8_t)sv_buf_sym(rv, (uint64_t)before.pred, false);
            dst[rc ? total - 1 - at : at] = rc ? complement(c) : c;
        }
        const uint32_t n = t.kind == NRUN || t.kind == MATCH || t.kind == MATCH_TO_END ? (uint32_t)match_symbols(t, before, rd.ref_size) : 0;
        const uint64_t ref_pos = (uint64_t)match_ref_pos(t, before);
        for (uint64_t todo = __ballot(n != 0); todo; todo &= todo - 1) { // the strip's N-runs and matches, each by the whole wave
            const uint32_t l = ctz64(todo);
            const uint32_t n_l = __shfl(n, l), at_l = __shfl(at, l);
            uint8_t *d = dst + (rc ? total - at_l - n_l : at_l);
            if (__shfl(t.kind, l) == NRUN)
                for (uint64_t q = lane_id(); q < n_l; q += WAVE)
                    d[q] = N_CODE;
            else
                wave_copy(rd, shfl_u64(ref_pos, l), n_l, rc, d);
        }
        return true;
    });
}

} // namespace agc
