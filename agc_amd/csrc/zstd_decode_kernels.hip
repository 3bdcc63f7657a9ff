// zstd_decode_kernels.hip -- zstd frames back into their bytes on gfx950 (wave64): ZSTD_decompressDCtx as CSegment::get_raw / get
// call it (src/common/segment.cpp:136-400) for a batch of frames.  The decoder is zstd/zs_decode.h (one source with the CPU tests).
//
// One wavefront per frame, one wave per block (no barrier; the tables in the LDS are the wave's own).  What is serial in the
// format stays serial: the frame's headers and the FSE state chain of the sequences are computed by every lane alike (one lane's
// worth of work, nothing to broadcast), a table is built by lane 0, each Huffman stream of a literals section is one lane's (four
// lanes for a 4-stream section).  The bytes move on all 64 lanes: raw and RLE blocks, literal runs and matches are copies in
// chunks of 64 bytes, a match with an offset below 64 a periodic copy (lane i reads period[i % offset]).
//
// Tables: the Huffman table (2^11 x 2 bytes) and the three FSE tables (512 + 256 + 512 x 4 bytes) stay in the LDS from block to
// block (treeless literals and repeat mode reuse them), beside 1.6 KB of scratch for the table being built: 10 832 bytes a wave.
// That alone would allow 15 waves a CU (of 32); the registers bind first: the compiler reports 161 VGPRs (3 waves a SIMD, 12 a
// CU), 106 SGPRs with 66 more spilled to VGPR lanes, no scratch memory.  Keeping the tables in the LDS keeps every
// table lookup of the two serial chains out of HBM; it is not what limits the occupancy.
// Literals: a block's decoded literals go to the frame's slice of a workspace in HBM (min(content size, 128 KiB) bytes), written
// by the lanes that decode the streams, read back by the literal copies.
//
// Lanes of a wave hand bytes to each other through memory (lane 0's tables, the literals, the output a match reads): the wave's
// memory operations are issued in program order, ZSD_WAVE_SYNC keeps the compiler from moving them across the hand-over.
#include "dev_common.h"

#define ZSD_WAVE_SYNC()                                                                                                                     \
    do {                                                                                                                                    \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                                              \
        __builtin_amdgcn_wave_barrier();                                                                                                    \
    } while (0)
#define ZSD_WAVE_ANY(x) (__ballot(x) != 0)
#include "zstd/zs_decode.h"

namespace agc {

struct ZDecJob {
    uint64_t src_off; // the frame: src[src_off, src_off + src_len)
    uint64_t out_off; // its bytes: out[out_off, out_off + out_len), out_len the content size its header declares
    uint64_t ws_off;  // its literals workspace: ws[ws_off, ws_off + ws_len)
    uint32_t src_len, out_len, ws_len;
    uint32_t status; // != 0: the host refused the header -- nothing to do
};

__global__ void __launch_bounds__(64) zstd_decode_kernel(const ZDecJob *__restrict__ jobs, uint32_t n_jobs, const uint8_t *__restrict__ src,
                                                        uint8_t *__restrict__ out, uint8_t *__restrict__ ws, uint32_t *__restrict__ status)
{
    __shared__ uint32_t fast[zs::dec::FAST_WORDS];
    const uint32_t s = blockIdx.x;
    if (s >= n_jobs)
        return;
    const ZDecJob jb = jobs[s];
    uint32_t st = jb.status;
    if (st == zs::dec::OK) {
        const zs::dec::Lane ln = {threadIdx.x};
        st = zs::dec::decodeFrame(ln, src + jb.src_off, jb.src_len, out + jb.out_off, jb.out_len, ws + jb.ws_off, jb.ws_len, fast);
    }
    if (threadIdx.x == 0)
        status[s] = st;
}

} // namespace agc
