/* The known-answer test of the compute conformance check: one definition for host C++, the
 * gfx950 kernel cu_selftest (native/src/kernels/device_kernels.h) and the fake runtime,
 * mirrored in numpy by amdvgpu.ops.selftest_reference (tests/test_selftest_reference.py pins
 * the two together).
 *
 * One wave64 runs the test under `seed` (32 bits) and `rounds` (1..1024) and produces four
 * 32-bit words, one per unit it exercised. All arithmetic is 32-bit and wraps.
 *
 *   H(q)    = vgpu_pattern_hash(q, seed)
 *   mix(x)  : x ^= x >> 15; x *= 0x85EBCA77; x ^= x >> 13
 *   fold(C) = sum over row, col of mix((uint32)C[row][col] + 0x9E3779B9 * (row * 32 + col))
 *             for a 32x32 matrix C: position-dependent, a transposed result differs.
 *
 *   mfma_i8   C = 0; every round r adds A.B, A and B 32x32 int8. Word w (0..7) of row i of A
 *             is H(((2r + 0) * 32 + i) * 8 + w), word w of column j of B is
 *             H(((2r + 1) * 32 + j) * 8 + w); byte t (little-endian) of word w, as int8, is
 *             element k = 4w + t. The word is fold(C). A round moves an element by at most
 *             32 * 128 * 128 = 2^19, so 1024 rounds stay below 2^29.
 *   mfma_f16  the same with 32x16 halves: A[i][8h + j] = ((H(0x10000 + ((2r + 0) * 32 + i) * 2
 *             + h) >> 4j) & 7) - 4 for h = 0..1, j = 0..7; B from 2r + 1 and its column.
 *             Values lie in [-4, 3], every partial sum is an integer below 2^24, so an f32
 *             accumulator is exact. The word is fold of the accumulator as int32.
 *   valu      per lane x = H(0x20000 + lane), then 16 * rounds steps (step = 0, 1, ...) of
 *             x = x * 0x9E3779B1 + step; x ^= x >> 15. The word is the sum over the 64 lanes
 *             of mix(x + lane).
 *   lds       lane l stores its final valu x at index (17l + 5) & 63 of a 64-word array and
 *             loads index l ^ 21; the word is the sum over lanes of mix(loaded + 0x9E3779B9 * l).
 *
 * `inject` flips bit 0 of word 0 of row 0 of A in round 0 of mfma_i8: only that word changes.
 */
#ifndef VGPU_SELFTEST_H
#define VGPU_SELFTEST_H

#include <stdint.h>

#include "vgpu/pattern.h"

#define VGPU_SELFTEST_MAX_ROUNDS 1024u
#define VGPU_SELFTEST_MAX_BAD 64u

/* Order of the four words, and of the unit names. */
enum { VGPU_SELFTEST_VALU = 0, VGPU_SELFTEST_LDS = 1, VGPU_SELFTEST_MFMA_I8 = 2, VGPU_SELFTEST_MFMA_F16 = 3 };

VGPU_PATTERN_FN uint32_t vgpu_selftest_mix(uint32_t x) {
  x ^= x >> 15;
  x *= 0x85EBCA77u;
  x ^= x >> 13;
  return x;
}

/* One term of fold(C). */
VGPU_PATTERN_FN uint32_t vgpu_selftest_fold_term(uint32_t c, uint32_t row, uint32_t col) {
  return vgpu_selftest_mix(c + 0x9E3779B9u * (row * 32u + col));
}

/* mfma_i8: word w (0..7) of row (ab = 0, A) or column (ab = 1, B) `idx` in round r. */
VGPU_PATTERN_FN uint32_t vgpu_selftest_i8_word(uint32_t seed, uint32_t r, uint32_t ab, uint32_t idx, uint32_t w,
                                               int inject) {
  const uint32_t v = vgpu_pattern_hash((uint64_t)(((2u * r + ab) * 32u + idx) * 8u + w), seed);
  return inject && !r && !ab && !idx && !w ? v ^ 1u : v;
}

/* mfma_f16: the eight 4-bit fields of half h (0..1) of row or column `idx` in round r. */
VGPU_PATTERN_FN uint32_t vgpu_selftest_f16_bits(uint32_t seed, uint32_t r, uint32_t ab, uint32_t idx, uint32_t h) {
  return vgpu_pattern_hash((uint64_t)(0x10000u + ((2u * r + ab) * 32u + idx) * 2u + h), seed);
}

/* Element j (0..7) of those fields: an integer in [-4, 3]. */
VGPU_PATTERN_FN int vgpu_selftest_f16_elem(uint32_t bits, uint32_t j) { return (int)((bits >> (4u * j)) & 7u) - 4; }

/* valu: the lane's x after 16 * rounds steps. */
VGPU_PATTERN_FN uint32_t vgpu_selftest_valu_lane(uint32_t seed, uint32_t lane, uint32_t rounds) {
  uint32_t x = vgpu_pattern_hash((uint64_t)(0x20000u + lane), seed);
  const uint32_t steps = 16u * rounds;
  for (uint32_t step = 0; step < steps; step++) {
    x = x * 0x9E3779B1u + step;
    x ^= x >> 15;
  }
  return x;
}

/* lds: where lane l stores and where it loads. */
VGPU_PATTERN_FN uint32_t vgpu_selftest_lds_store(uint32_t lane) { return (17u * lane + 5u) & 63u; }
VGPU_PATTERN_FN uint32_t vgpu_selftest_lds_load(uint32_t lane) { return lane ^ 21u; }

/* The four words on the host, with plain loops. Returns 0, or -1 on rounds outside 1..1024. */
static inline int vgpu_selftest_expected(uint32_t seed, uint32_t rounds, int inject, uint32_t out[4]) {
  int32_t c[32][32];
  uint32_t x[64], lds[64];
  if (rounds < 1 || rounds > VGPU_SELFTEST_MAX_ROUNDS) return -1;

  out[VGPU_SELFTEST_VALU] = out[VGPU_SELFTEST_LDS] = 0;
  for (uint32_t l = 0; l < 64; l++) {
    x[l] = vgpu_selftest_valu_lane(seed, l, rounds);
    out[VGPU_SELFTEST_VALU] += vgpu_selftest_mix(x[l] + l);
    lds[vgpu_selftest_lds_store(l)] = x[l];
  }
  for (uint32_t l = 0; l < 64; l++)
    out[VGPU_SELFTEST_LDS] += vgpu_selftest_mix(lds[vgpu_selftest_lds_load(l)] + 0x9E3779B9u * l);

  for (int pass = 0; pass < 2; pass++) { /* 0: mfma_i8 (K = 32), 1: mfma_f16 (K = 16) */
    const uint32_t depth = pass ? 16u : 32u;
    int8_t a[32][32], b[32][32]; /* b[col][k] */
    for (uint32_t i = 0; i < 32; i++)
      for (uint32_t j = 0; j < 32; j++) c[i][j] = 0;
    for (uint32_t r = 0; r < rounds; r++) {
      for (uint32_t i = 0; i < 32; i++) {
        if (!pass) {
          for (uint32_t w = 0; w < 8; w++) {
            const uint32_t wa = vgpu_selftest_i8_word(seed, r, 0, i, w, inject);
            const uint32_t wb = vgpu_selftest_i8_word(seed, r, 1, i, w, 0);
            for (uint32_t t = 0; t < 4; t++) {
              a[i][4 * w + t] = (int8_t)(uint8_t)(wa >> (8 * t));
              b[i][4 * w + t] = (int8_t)(uint8_t)(wb >> (8 * t));
            }
          }
        } else {
          for (uint32_t h = 0; h < 2; h++) {
            const uint32_t ba = vgpu_selftest_f16_bits(seed, r, 0, i, h);
            const uint32_t bb = vgpu_selftest_f16_bits(seed, r, 1, i, h);
            for (uint32_t j = 0; j < 8; j++) {
              a[i][8 * h + j] = (int8_t)vgpu_selftest_f16_elem(ba, j);
              b[i][8 * h + j] = (int8_t)vgpu_selftest_f16_elem(bb, j);
            }
          }
        }
      }
      for (uint32_t i = 0; i < 32; i++)
        for (uint32_t j = 0; j < 32; j++) {
          int32_t s = 0;
          for (uint32_t k = 0; k < depth; k++) s += (int32_t)a[i][k] * (int32_t)b[j][k];
          c[i][j] += s;
        }
    }
    uint32_t f = 0;
    for (uint32_t i = 0; i < 32; i++)
      for (uint32_t j = 0; j < 32; j++) f += vgpu_selftest_fold_term((uint32_t)c[i][j], i, j);
    out[pass ? VGPU_SELFTEST_MFMA_F16 : VGPU_SELFTEST_MFMA_I8] = f;
  }
  return 0;
}

#endif
