// lz_consts.h -- the constants and sizing rules the LZ kernels share with the host's planning arithmetic (lz_plan.h).  No HIP needed:
// dev_common.h and lz_kernels.hip include it for the device, tests/lzplan_host compiles it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LZ_HD __host__ __device__ inline
#else
#define LZ_HD inline
#endif

namespace agc {

constexpr uint32_t HASHING_STEP = 4;     // lz_diff.h:38 (USE_SPARSE_HT)
constexpr uint32_t REF_TAIL_WORDS = 4;   // words of slack behind a reference's stored form (dev_common.h: RefDesc)
constexpr uint32_t PACK_BLOCK = 1024;    // symbols per block of the 2-bit layout (dev_common.h: PackedView)
constexpr uint32_t FILTER_CHUNK = 65536; // text positions per block of key_filter_kernel

enum { MODE_ENCODE = 0, MODE_ESTIMATE = 1, MODE_COSTVEC = 2 }; // what a parse produces (lz_kernels.hip)

// the key filters of a reference (dev_common.h): two of key_bloom_half_words(key_bloom_shift(ref_size)) 64-bit words each
constexpr uint32_t KEY_BLOOM_HALF = 4096;
constexpr uint32_t KEY_BLOOM_SHIFT0 = 20; // word index = 32 - shift bits of the hash: 12 bits for KEY_BLOOM_HALF words
LZ_HD uint32_t key_bloom_shift(uint32_t ref_size)
{
    const uint32_t keys = ref_size / HASHING_STEP + 1;
    uint32_t sh = KEY_BLOOM_SHIFT0;
    while (sh > 8 && (1u << (32 - sh)) < keys / 4)
        --sh;
    return sh;
}
LZ_HD uint32_t key_bloom_half_words(uint32_t shift) { return 1u << (32 - shift); }
#undef LZ_HD

} // namespace agc
