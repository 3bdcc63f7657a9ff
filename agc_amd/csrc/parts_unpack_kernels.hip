// parts_unpack_kernels.hip -- archive parts, zstd-decoded in HBM, into what the read path's other stages take, for gfx950 (wave64):
// a pack cut at its terminators, a reference stored as tuples into its symbols (arithmetic and formats: parts_unpack.h).
//
//   pack_index_kernel      one wavefront per pack: strips of 1024 bytes (16 per lane, one load), five ballots per strip; the lane that
//                          owns terminator i < seq_cap stores its offset in the pack's row of seq_end, the exact count goes to the host
//   tuples_size_kernel     one lane per reference part: the shape its marker byte declares, or why it is refused
//   tuples_unpack_kernel   output-driven like fasta_text_kernel: a lane owns 16 consecutive, 16-byte-aligned output bytes, reads the
//                          tuple bytes that cover them and issues one 16-byte store (a part's first and last chunk, when partial, byte
//                          by byte); a job with nb == 0 copies -- a reference stored as bytes, or a pack a caller wants moved
// No LDS, no barrier.  Nothing here makes an address from a part's content: the index kernel indexes by an ordinal below the cap,
// the write kernel runs from sizes the host has checked against the size kernel's results.
#include "dev_common.h"
#include "fasta_out.h"
#include "parts_unpack.h"

namespace agc {

struct PartJob {
    uint64_t dec_off; // the part's decoded bytes: dec[dec_off, dec_off + dec_len), dec_off a multiple of 16
    uint32_t dec_len;
    uint32_t content; // AGC_HIP_PART_*
    uint32_t zd_slot; // its slot in the zstd stage's statuses, ~0u: it did not go through that stage
    uint32_t seq_row; // a pack: its row of seq_end
    uint32_t status;  // != 0: refused on the host -- nothing to do
    uint32_t pad;
};

struct PartInfo {
    uint32_t status; // pu::Status
    uint32_t count;  // a pack: its sequences (exact, also above the cap); a reference: nb of its tuples (0: bytes as they are)
    uint64_t n;      // a reference: its symbols
};

struct UnpackJob {
    uint64_t src_off;     // the tuple stream (or the bytes to copy) at dec[src_off ...)
    uint64_t out_off;     // the n symbols go to out[out_off, out_off + n)
    uint64_t n;
    uint64_t first_chunk; // the job's chunks are [first_chunk, next job's first_chunk) of the launch
    uint32_t nb;
    uint32_t a;           // (address of out[out_off]) & 15
};

__device__ __forceinline__ uint32_t part_status(const PartJob &jb, const uint32_t *__restrict__ zd_status)
{
    return jb.status != pu::OK || jb.zd_slot == ~0u ? jb.status : zd_status[jb.zd_slot];
}

__global__ void __launch_bounds__(256) pack_index_kernel(const PartJob *__restrict__ jobs, const uint32_t *__restrict__ ids, uint32_t n_ids,
                                                        const uint8_t *__restrict__ dec, const uint32_t *__restrict__ zd_status, uint32_t seq_cap,
                                                        uint32_t *__restrict__ seq_end, PartInfo *__restrict__ info)
{
    const uint32_t s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE, lane = lane_id();
    if (s >= n_ids)
        return;
    const uint32_t part = ids[s];
    const PartJob jb = jobs[part];
    const uint32_t st = part_status(jb, zd_status);
    uint32_t count = 0;
    if (st == pu::OK) {
        const uint8_t *p = dec + jb.dec_off;
        uint32_t *row = seq_end + (uint64_t)jb.seq_row * seq_cap;
        for (uint64_t base = 0; base < jb.dec_len; base += pu::STRIP) {
            const uint64_t o = base + (uint64_t)pu::LANE_BYTES * lane;
            uint64_t w0 = 0, w1 = 0;
            uint32_t valid = 0;
            if (o < jb.dec_len) { // (the load may reach 15 bytes behind the part: the buffer's padding, masked off by `valid`)
                const uint4 v = *(const uint4 *)(p + o);
                w0 = (uint64_t)v.x | (uint64_t)v.y << 32;
                w1 = (uint64_t)v.z | (uint64_t)v.w << 32;
                valid = (uint32_t)(jb.dec_len - o < pu::LANE_BYTES ? jb.dec_len - o : pu::LANE_BYTES);
            }
            const uint32_t m = pu::terminator_mask(w0, w1, valid), cnt = (uint32_t)__popc(m);
            pu::CountBallots B;
            for (uint32_t j = 0; j < 5; ++j)
                B.b[j] = __ballot(cnt >> j & 1);
            pu::store_ends(row, seq_cap, count + pu::terminators_in_front(B, lane), m, (uint32_t)o);
            count += pu::terminators_of_the_strip(B);
        }
    }
    if (lane == 0)
        info[part] = {st, count, 0};
}

__global__ void __launch_bounds__(256) tuples_size_kernel(const PartJob *__restrict__ jobs, const uint32_t *__restrict__ ids, uint32_t n_ids,
                                                         const uint8_t *__restrict__ dec, const uint32_t *__restrict__ zd_status, PartInfo *__restrict__ info)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_ids)
        return;
    const uint32_t part = ids[s];
    const PartJob jb = jobs[part];
    PartInfo r = {part_status(jb, zd_status), 0, 0};
    if (r.status == pu::OK) {
        if (jb.content == AGC_HIP_PART_REF_TUPLES) {
            const pu::TupleShape sh = pu::tuple_shape(jb.dec_len, jb.dec_len ? dec[jb.dec_off + jb.dec_len - 1] : (uint8_t)0);
            r = {sh.status, sh.nb, sh.n};
        } else
            r.n = jb.dec_len;
    }
    info[part] = r;
}

__global__ void __launch_bounds__(256) tuples_unpack_kernel(const UnpackJob *__restrict__ jobs, uint32_t n_jobs, uint64_t n_chunks, const uint8_t *__restrict__ dec,
                                                           uint8_t *__restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_chunks)
        return;
    uint32_t lo = 0, hi = n_jobs; // the last job whose first chunk is <= j (a job without symbols has no chunk: it shares its successor's first)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (jobs[mid].first_chunk <= j)
            lo = mid;
        else
            hi = mid;
    }
    const UnpackJob jb = jobs[lo];
    uint64_t begin, w0, w1;
    uint32_t n;
    fo::chunk_range(j - jb.first_chunk, jb.a, jb.n, begin, n);
    pu::chunk_symbols((g_u8 *)dec + jb.src_off, jb.nb, jb.n, begin, n, w0, w1);
    uint8_t *dst = out + jb.out_off + begin;
    if (n == fo::CHUNK)
        *(uint4 *)dst = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)); // (out_off + begin + a is a multiple of 16)
    else
        for (uint32_t i = 0; i < n; ++i)
            dst[i] = (uint8_t)((i < 8 ? w0 : w1) >> (8 * (i & 7)));
}

} // namespace agc
