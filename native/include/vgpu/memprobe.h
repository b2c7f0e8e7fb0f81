/* The pointer-chase ring of the memory-system probe: one definition for host C++ and the gfx950
 * kernels ring_build and mem_chase (native/src/kernels/vgpu_kernels.hip), mirrored in numpy by
 * amdvgpu.ops.ring_reference and ring_jump (tests/test_memprobe_args.py pins them together).
 *
 * A ring has n = 2^L slots of 128 bytes (one L2 request), L in 1..25: 256 B to 4 GiB. Word 0 of
 * slot i is the slot that follows it,
 *
 *   next(i) = (A * i + C) mod n,  A = 0x9E3779B1 (= 1 mod 4),  C = vgpu_pattern_hash(0x30000, seed) | 1
 *
 * With C odd and A = 1 mod 4 the map is one cycle through all n slots for every L >= 1
 * (Hull-Dobell), so a chase of k steps touches min(k, n) distinct lines in an order no
 * prefetcher follows. Word 1 of slot i is i ^ seed; words 2..31 are never written.
 *
 * vgpu_ring_jump_slot(i, k) is the slot k steps after i: the affine map composed with itself by
 * squaring, 64 iterations for a 64-bit k. All arithmetic is mod 2^32 and the result is masked
 * to L bits, which is the same as arithmetic mod 2^L; k itself may have wrapped mod 2^64,
 * because the cycle's length 2^L divides 2^64.
 */
#ifndef VGPU_MEMPROBE_H
#define VGPU_MEMPROBE_H

#include <stdint.h>

#include "vgpu/pattern.h"

#define VGPU_RING_A 0x9E3779B1u
#define VGPU_RING_MIN_L 1
#define VGPU_RING_MAX_L 25
#define VGPU_RING_SLOT_WORDS 32u /* 128 bytes */

/* n - 1 for a ring of 2^L slots; L in 1..25. */
VGPU_PATTERN_FN uint32_t vgpu_ring_mask(uint32_t L) { return (1u << (L & 31u)) - 1u; }

VGPU_PATTERN_FN uint32_t vgpu_ring_c(uint32_t seed) { return vgpu_pattern_hash(0x30000u, seed) | 1u; }

VGPU_PATTERN_FN uint32_t vgpu_ring_next_slot(uint32_t i, uint32_t L, uint32_t seed) {
  return (VGPU_RING_A * i + vgpu_ring_c(seed)) & vgpu_ring_mask(L);
}

VGPU_PATTERN_FN uint32_t vgpu_ring_jump_slot(uint32_t i, uint64_t k, uint32_t L, uint32_t seed) {
  uint32_t ra = 1u, rc = 0u;                         /* the identity: next^0 */
  uint32_t pa = VGPU_RING_A, pc = vgpu_ring_c(seed); /* next^(2^bit) */
  for (int bit = 0; bit < 64; bit++) {
    if (k & 1u) {
      rc = pa * rc + pc;
      ra = pa * ra;
    }
    pc = pa * pc + pc;
    pa = pa * pa;
    k >>= 1;
  }
  return (ra * i + rc) & vgpu_ring_mask(L);
}

#endif
