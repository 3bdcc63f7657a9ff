// inflate_kernels.hip -- a BGZF stream back into its bytes on gfx950 (wave64).  The decoder is inflate.h (one source with the CPU
// tests); the host has walked the stream and says where every member's payload lies and where its bytes go.
//
// bgzf_inflate_kernel: one wavefront per member, INF_WAVES waves to a workgroup (no barrier: the tables in the LDS are the wave's
// own, 3 932 bytes each).  What is serial in the format stays serial: the symbol chain of a member is computed by every lane alike
// (one lane's worth of work, nothing to broadcast), a block's codes are built by lane 0.  The bytes move on all 64 lanes: decoded
// literals gather in a strip of registers, a literal per lane, and are stored 64 at a time; stored blocks and matches are copies in
// strips of 64 bytes, a match with a distance below 64 a periodic copy; each lane takes a 64th of the output for the CRC-32.
//
// Lanes of a wave hand bytes to each other through memory (lane 0's tables, the output a match or the CRC reads): the wave's memory
// operations are issued in program order, INF_WAVE_SYNC keeps the compiler from moving them across the hand-over.
#include "dev_common.h"

#define INF_WAVE_SYNC()                                                                                                                     \
    do {                                                                                                                                    \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                                              \
        __builtin_amdgcn_wave_barrier();                                                                                                    \
    } while (0)
#include "inflate.h"

namespace agc {

constexpr uint32_t INF_WAVES = 4;

// member m: src[jobs[m].src_off, +src_len) -> out[jobs[m].out_off, +out_len); status[m] = inflate::OK or inflate::MALFORMED
__global__ void __launch_bounds__(INF_WAVES *WAVE) bgzf_inflate_kernel(const inflate::Job *__restrict__ jobs, uint32_t n_jobs, const uint8_t *__restrict__ src,
                                                                       uint8_t *__restrict__ out, uint32_t *__restrict__ status)
{
    __shared__ inflate::Work work[INF_WAVES];
    const uint32_t wave = threadIdx.x / WAVE, m = blockIdx.x * INF_WAVES + wave;
    if (m >= n_jobs)
        return;
    const inflate::Job jb = jobs[m];
    const inflate::Lane ln = {threadIdx.x % WAVE};
    const uint32_t why = inflate::inflate_member(ln, work[wave], src + jb.src_off, jb.src_len, out + jb.out_off, jb.out_len, jb.crc);
    if (ln.lane == 0)
        status[m] = inflate::status_of(why);
}

} // namespace agc
