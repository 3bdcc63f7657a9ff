// fasta_out_kernels.hip -- a sample's FASTA text for gfx950 (wave64): what follows zstd on the read path -- the segment sources,
// orientation, the k-symbol overlap, the alphabet and the line wrapping (decompress_contig and the FASTA writer,
// src/common/agc_decompressor_lib.cpp:172-286) -- in one submission (layout and the per-chunk walk: fasta_out.h).
//
// The segments of the sample first land back to back, whole and oriented, in one symbol buffer:
//   deltas            lz_decode_scan_kernel / lz_decode_write_kernel (lz_decode_kernels.hip), as they are
//   segment_copy_kernel   a group's reference as it is (in_group_id 0) out of the 2-bit layout with lzd::wave_copy, or symbol bytes
//                     the caller supplied (the raw groups); one wavefront per segment, reverse-complemented on request
// fasta_text_kernel then is output-driven: a lane owns 16 consecutive, 16-byte-aligned bytes of the text and writes them with one
// 16-byte store (the text's first and last chunk, when they are partial, byte by byte).  It finds its contig by binary search
// in the contigs' text offsets and its first symbol's segment by binary search in the contig's segment starts, once each, and
// walks forward from there.  No LDS, no barrier; it reads the symbol buffer byte by byte (in L2 right after the decode for small
// inputs) -- launched only after every segment of the plan has been checked, so no address comes from unchecked input.
#include "dev_common.h"
#include "fasta_out.h"
#include "lz_decode.h"

namespace agc {

struct CopyJob {
    uint64_t src_off; // raw: the symbols are bytes[src_off, src_off + len)
    uint64_t out_off; // they go to sym[out_off, out_off + len)
    uint32_t len;
    uint32_t ref_slot; // reference: index into the RefDesc array (the whole reference, ref_size == len)
    uint32_t rc;
    uint32_t is_ref;
};

typedef const __attribute__((address_space(1))) uint64_t g_u64;
using TextPlan = fo::PlanT<g_u64 *, g_u32 *, g_u8 *>;

__global__ void __launch_bounds__(256) segment_copy_kernel(const RefDesc *__restrict__ refs, const CopyJob *__restrict__ jobs, uint32_t n_jobs,
                                                          const uint8_t *__restrict__ bytes, uint8_t *__restrict__ sym)
{
    const uint32_t s = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    if (s >= n_jobs)
        return;
    const CopyJob jb = jobs[s];
    uint8_t *dst = sym + jb.out_off;
    if (jb.is_ref) {
        const RefDesc rd = refs[jb.ref_slot];
        lzd::wave_copy(rd, 0, jb.len, jb.rc, dst);
        return;
    }
    g_u8 *src = (g_u8 *)bytes + jb.src_off;
    for (uint32_t q = lane_id(); q < jb.len; q += WAVE) // reverse_complement, src/common/agc_basic.cpp:253-280
        dst[q] = jb.rc ? lzd::complement(src[jb.len - 1 - q]) : src[q];
}

// text: the text's first byte, at an address with (address & 15) == a; total: its size
__global__ void __launch_bounds__(256) fasta_text_kernel(TextPlan P, uint8_t *__restrict__ text, uint32_t a, uint64_t total, uint64_t n_chunks)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_chunks)
        return;
    uint64_t begin, w0, w1;
    uint32_t n;
    fo::chunk_range(j, a, total, begin, n);
    fo::chunk_bytes(P, begin, n, w0, w1);
    if (n == fo::CHUNK) {
        const uint4 v = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        *(uint4 *)(text + begin) = v; // (begin + a is a multiple of 16)
    } else
        for (uint32_t i = 0; i < n; ++i)
            text[begin + i] = (uint8_t)((i < 8 ? w0 : w1) >> (8 * (i & 7)));
}

} // namespace agc
