/* The test pattern of the memory conformance check: one definition for host C++ and the
 * gfx950 kernels (native/src/kernels/pattern_kernels.h), mirrored in numpy by
 * amdvgpu.ops.pattern_reference (tests/test_validate_conformance.py pins the two together).
 *
 * Word `index` (a 64-bit index of 32-bit words, counted from the start of the logical
 * buffer, never an address: promotion of a spilled buffer keeps the address, and a stuck or
 * aliased range must still show) under `seed` (a stale buffer of an earlier fill fails):
 *
 *   one hash per 16-byte vector (index >> 2), two 32-bit multiplies, and a rotate-and-add per
 *   word of the vector (index & 3) - the multiplies are quarter rate on CDNA, the rest is not.
 */
#ifndef VGPU_PATTERN_H
#define VGPU_PATTERN_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VGPU_PATTERN_FN __host__ __device__ inline
#else
#define VGPU_PATTERN_FN static inline
#endif

/* The hash of 16-byte vector `vec` (= word index >> 2). */
VGPU_PATTERN_FN uint32_t vgpu_pattern_hash(uint64_t vec, uint32_t seed) {
  uint32_t a = ((uint32_t)vec ^ seed) * 0x9E3779B1u;
  a ^= a >> 15;
  a += (uint32_t)(vec >> 32) * 0x85EBCA77u + seed;
  a *= 0xC2B2AE3Du;
  a ^= a >> 13;
  return a;
}

/* Word `lane` (0..3) of a vector whose hash is `h`. */
VGPU_PATTERN_FN uint32_t vgpu_pattern_lane(uint32_t h, uint32_t lane) {
  const uint32_t r = 8u * lane;
  return ((h << r) | (h >> ((32u - r) & 31u))) + lane * 0x9E3779B9u;
}

VGPU_PATTERN_FN uint32_t vgpu_pattern_word(uint64_t index, uint32_t seed) {
  return vgpu_pattern_lane(vgpu_pattern_hash(index >> 2, seed), (uint32_t)(index & 3u));
}

#endif
