// Device code shared by libvgpu_kernels.so (vgpu_kernels.hip) and the code object embedded in
// vgpu-validate (validate_kernels.hip): the CU census body and the pattern kernels of the
// memory conformance check (vgpu/pattern.h), and the known-answer test of the compute
// conformance check (vgpu/selftest.h).
//
//  * pattern_fill   16 bytes per lane, grid-stride, non-temporal stores: word k of the buffer
//                   becomes w(base + k, seed).
//  * pattern_check  the same walk with non-temporal 16-byte loads; each lane counts its
//                   mismatching words and keeps the lowest mismatching index, the wave64
//                   reduces both with shuffles, and only a wave that saw a mismatch issues
//                   its one atomic add (out[0], count) and one atomic min (out[1], lowest
//                   word index of the buffer; the caller presets it to all-ones).
//  * pattern_poke   flips one bit in each listed word: proves that the checker can fail.
//  * cu_selftest    workgroups of four waves; every wave runs the whole known-answer test of
//                   vgpu/selftest.h on its own (VALU, LDS, the i8 and the f16 matrix core),
//                   reduces each unit's word with shuffles, and its lane 0 writes where it ran
//                   (census code plus SIMD id) and the four words. Then the wave holds its
//                   CU like the census does, so the grid spreads over every CU of the queue.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "vgpu/pattern.h"
#include "vgpu/selftest.h"

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

namespace vgpu_dev {

using i32x4 = int __attribute__((ext_vector_type(4)));
using i32x16 = int __attribute__((ext_vector_type(16)));
using f16x8 = _Float16 __attribute__((ext_vector_type(8)));
using f32x16 = float __attribute__((ext_vector_type(16)));

constexpr int kSelftestWaves = 4;   // waves of a cu_selftest workgroup
constexpr int kSelftestRecord = 8;  // words a wave writes: location, valu, lds, mfma_i8, mfma_f16, 0, 0, 0

__device__ inline uint32_t wave_sum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// fold() of a 32x32 accumulator in the C/D layout of the 32x32 MFMA shapes:
// col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
template <typename Acc>
__device__ inline uint32_t selftest_fold(const Acc& acc, uint32_t lane) {
  uint32_t f = 0;
#pragma unroll
  for (uint32_t reg = 0; reg < 16; reg++)
    f += vgpu_selftest_fold_term((uint32_t)(int32_t)acc[reg], (reg & 3u) + 8u * (reg >> 2) + 4u * (lane >> 5), lane & 31u);
  return wave_sum(f);
}

}  // namespace vgpu_dev

extern "C" __global__ void __launch_bounds__(256)
cu_selftest(uint32_t* __restrict__ out, uint32_t seed, uint32_t rounds, uint64_t hold_ticks,
            const uint32_t* __restrict__ bad, uint32_t n_bad) {
  using namespace vgpu_dev;
  __shared__ uint32_t lds[kSelftestWaves][64];
  const uint32_t lane = threadIdx.x & 63u, wave = (threadIdx.x >> 6) & (kSelftestWaves - 1);
  const uint32_t idx = lane & 31u, h = lane >> 5;  // the lane's A row and B column, and its half of k

  bool inject = false;  // wave 0 of a listed workgroup
  if (n_bad > VGPU_SELFTEST_MAX_BAD) n_bad = VGPU_SELFTEST_MAX_BAD;
  for (uint32_t k = 0; k < n_bad; k++) inject |= wave == 0 && bad[k] == blockIdx.x;

  // valu, then lds on its result
  const uint32_t x = vgpu_selftest_valu_lane(seed, lane, rounds);
  const uint32_t w_valu = wave_sum(vgpu_selftest_mix(x + lane));
  lds[wave][vgpu_selftest_lds_store(lane)] = x;
  __syncthreads();
  const uint32_t w_lds = wave_sum(vgpu_selftest_mix(lds[wave][vgpu_selftest_lds_load(lane)] + 0x9E3779B9u * lane));

  // mfma_i8: the lane holds words 4h .. 4h+3 of its A row and of its B column
  i32x16 ci = {};
  for (uint32_t r = 0; r < rounds; r++) {
    i32x4 a, b;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
      a[w] = (int)vgpu_selftest_i8_word(seed, r, 0, idx, 4u * h + w, inject);
      b[w] = (int)vgpu_selftest_i8_word(seed, r, 1, idx, 4u * h + w, 0);
    }
    ci = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, ci, 0, 0, 0);
  }
  const uint32_t w_i8 = selftest_fold(ci, lane);

  // mfma_f16: the lane holds k = 8h .. 8h+7 of its A row and of its B column
  f32x16 cf = {};
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t ba = vgpu_selftest_f16_bits(seed, r, 0, idx, h), bb = vgpu_selftest_f16_bits(seed, r, 1, idx, h);
    f16x8 a, b;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
      a[j] = (_Float16)vgpu_selftest_f16_elem(ba, j);
      b[j] = (_Float16)vgpu_selftest_f16_elem(bb, j);
    }
    cf = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, cf, 0, 0, 0);
  }
  const uint32_t w_f16 = selftest_fold(cf, lane);

  if (lane == 0) {
    uint32_t hw = __builtin_amdgcn_s_getreg(kHwRegHwId | (0u << 6) | (31u << 11));
    uint32_t xcc = __builtin_amdgcn_s_getreg(kHwRegXccId | (0u << 6) | (3u << 11));
    uint32_t* rec = out + ((size_t)blockIdx.x * kSelftestWaves + wave) * kSelftestRecord;
    rec[0] = ((hw >> 4) & 0x3) << 16 | (xcc & 0xf) << 12 | ((hw >> 13) & 0x7) << 8 | ((hw >> 12) & 0x1) << 4 | ((hw >> 8) & 0xf);
    rec[1 + VGPU_SELFTEST_VALU] = w_valu;
    rec[1 + VGPU_SELFTEST_LDS] = w_lds;
    rec[1 + VGPU_SELFTEST_MFMA_I8] = w_i8;
    rec[1 + VGPU_SELFTEST_MFMA_F16] = w_f16;
    rec[5] = rec[6] = rec[7] = 0;
  }
  uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < hold_ticks) __builtin_amdgcn_s_sleep(2);
}
