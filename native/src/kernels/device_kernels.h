// Device code shared by libvgpu_kernels.so (vgpu_kernels.hip) and the code object embedded in
// vgpu-validate (validate_kernels.hip): the CU census body and the pattern kernels of the
// memory conformance check (vgpu/pattern.h).
//
//  * pattern_fill   16 bytes per lane, grid-stride, non-temporal stores: word k of the buffer
//                   becomes w(base + k, seed).
//  * pattern_check  the same walk with non-temporal 16-byte loads; each lane counts its
//                   mismatching words and keeps the lowest mismatching index, the wave64
//                   reduces both with shuffles, and only a wave that saw a mismatch issues
//                   its one atomic add (out[0], count) and one atomic min (out[1], lowest
//                   word index of the buffer; the caller presets it to all-ones).
//  * pattern_poke   flips one bit in each listed word: proves that the checker can fail.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "vgpu/pattern.h"

namespace vgpu_dev {

constexpr unsigned kHwRegHwId = 4;
constexpr unsigned kHwRegXccId = 20;

// One single-wave workgroup: records where it runs, then spins `spin_ticks` (100 MHz).
__device__ inline void census_body(uint32_t* out, uint64_t spin_ticks) {
  if (threadIdx.x == 0) {
    // s_getreg_b32 immediate: id | offset << 6 | (size - 1) << 11
    uint32_t hw = __builtin_amdgcn_s_getreg(kHwRegHwId | (0u << 6) | (31u << 11));
    uint32_t xcc = __builtin_amdgcn_s_getreg(kHwRegXccId | (0u << 6) | (3u << 11));
    uint32_t cu = (hw >> 8) & 0xf;
    uint32_t sh = (hw >> 12) & 0x1;
    uint32_t se = (hw >> 13) & 0x7;
    out[blockIdx.x] = (xcc & 0xf) << 12 | se << 8 | sh << 4 | cu;
    uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < spin_ticks) __builtin_amdgcn_s_sleep(2);
  }
}

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

constexpr int kPatternBlock = 256;
constexpr int kPatternMaxBlocks = 256 * 16;  // as vgpu_stream_copy: >> 256 CUs x 8 waves

// Grid of a pattern kernel over n_vec 16-byte vectors.
inline unsigned pattern_blocks(uint64_t n_vec) {
  uint64_t b = (n_vec + kPatternBlock - 1) / kPatternBlock;
  if (b > (uint64_t)kPatternMaxBlocks) b = kPatternMaxBlocks;
  return b < 1 ? 1u : (unsigned)b;
}

// The four words from word index `idx` on. One hash when idx starts a pattern vector.
__device__ inline u32x4 pattern_vec(uint64_t idx, uint32_t seed) {
  u32x4 v;
  if ((idx & 3u) == 0) {
    const uint32_t h = vgpu_pattern_hash(idx >> 2, seed);
    v.x = vgpu_pattern_lane(h, 0);
    v.y = vgpu_pattern_lane(h, 1);
    v.z = vgpu_pattern_lane(h, 2);
    v.w = vgpu_pattern_lane(h, 3);
  } else {
    v.x = vgpu_pattern_word(idx, seed);
    v.y = vgpu_pattern_word(idx + 1, seed);
    v.z = vgpu_pattern_word(idx + 2, seed);
    v.w = vgpu_pattern_word(idx + 3, seed);
  }
  return v;
}

}  // namespace vgpu_dev

extern "C" __global__ void __launch_bounds__(256)
pattern_fill(vgpu_dev::u32x4* __restrict__ dst, uint64_t n_vec, uint64_t base, uint32_t seed) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n_vec; i += stride) __builtin_nontemporal_store(vgpu_dev::pattern_vec(base + 4 * i, seed), &dst[i]);
}

extern "C" __global__ void __launch_bounds__(256)
pattern_check(const vgpu_dev::u32x4* __restrict__ src, uint64_t n_vec, uint64_t base, uint32_t seed,
              unsigned long long* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long bad = 0, first = ~0ull;
  for (; i < n_vec; i += stride) {
    const vgpu_dev::u32x4 got = __builtin_nontemporal_load(&src[i]);
    const vgpu_dev::u32x4 want = vgpu_dev::pattern_vec(base + 4 * i, seed);
    const unsigned m = (got.x != want.x ? 1u : 0u) | (got.y != want.y ? 2u : 0u) | (got.z != want.z ? 4u : 0u) |
                       (got.w != want.w ? 8u : 0u);
    if (m) {
      bad += __builtin_popcount(m);
      // the lane walks upwards, so its first mismatch is its lowest
      if (first == ~0ull) first = 4 * i + (unsigned)__builtin_ctz(m);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    bad += __shfl_xor(bad, off, 64);
    const unsigned long long other = __shfl_xor(first, off, 64);
    first = other < first ? other : first;
  }
  if ((threadIdx.x & 63) == 0 && bad) {
    atomicAdd(&out[0], bad);
    atomicMin(&out[1], first);
  }
}

extern "C" __global__ void __launch_bounds__(64)
pattern_poke(uint32_t* __restrict__ dst, const unsigned long long* __restrict__ idx, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[idx[t]] ^= 0x00010000u;
}
