// bgzf_kernels.hip -- bytes into a BGZF stream on gfx950 (wave64).  The coder is bgzf.h (one source with the CPU tests).
//
// bgzf_block_kernel: a workgroup of 256 lanes per block of 65280 input bytes does the whole block -- three reads of the input in
// 16-byte chunks per lane (histogram + CRC; the chunks' bit counts; the packing), the two code constructions, the headers -- and leaves
// the finished member in the block's slot of 65312 bytes, its size beside it.  The member is put together in the LDS (the packed bits
// are OR-ed into a zeroed image with LDS atomics, a word being shared by the lanes whose chunks meet in it) and goes to the slot in
// 16-byte stores.  The other way considered, OR-ing into a zeroed slot in HBM, turns every one of those ORs into a read-modify-write
// at L2; the image costs 65 312 of the workgroup's 79 KB of LDS, which still lets two workgroups share a CU.
//
// bgzf_place_kernel: the compressed sizes depend on the data, so the members are placed by a second launch: the host has summed the
// sizes (one copy of 4 bytes per block) and says where every member begins; a workgroup copies its member there, at whatever
// alignment that is, and the workgroup behind the last block writes the EOF member.  No address is computed from anything but the
// host's offsets and the first launch's sizes, and no block waits for another.
#include "dev_common.h"

#define BGZF_EACH_LANE(t)                                                                                                                   \
    {                                                                                                                                       \
        const uint32_t t = threadIdx.x;                                                                                                     \
        {
#define BGZF_END_LANES                                                                                                                      \
    }                                                                                                                                       \
    }                                                                                                                                       \
    __syncthreads();
#define BGZF_OR(p, v) atomicOr((p), (v))
#define BGZF_ADD(p, v) atomicAdd((p), (v))
#include "bgzf.h"

namespace agc {

// block b: in[b * IN, min(n, (b + 1) * IN)) -> slots[b * SLOT, +sizes[b])
__global__ void __launch_bounds__(bgzf::THREADS, 2) bgzf_block_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t n_blocks, uint8_t *__restrict__ slots,
                                                                   uint32_t *__restrict__ sizes)
{
    __shared__ bgzf::Work w;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint64_t from = b * bgzf::IN;
        const uint32_t len = (uint32_t)(n - from < bgzf::IN ? n - from : bgzf::IN);
        bgzf::encode_block(w, in + from, len, slots + b * bgzf::SLOT, sizes + b);
    }
}

// block b < n_blocks: its member to out + off[b]; block n_blocks: the EOF member to out + off[n_blocks]
__global__ void __launch_bounds__(bgzf::THREADS) bgzf_place_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ off,
                                                                   uint64_t n_blocks, uint8_t *__restrict__ out)
{
    for (uint64_t b = blockIdx.x; b <= n_blocks; b += gridDim.x) {
        if (b < n_blocks)
            bgzf::place_member(slots + b * bgzf::SLOT, sizes[b], out + off[b]);
        else
            bgzf::place_eof(out + off[b]);
    }
}

} // namespace agc
