// The host side of vgpu/memprobe.h and the memory probe's argument rules of vgpu/calib_args.h at
// their bound values, as a stand-alone program: the build compiles it with
// -fsanitize=address,undefined (no GPU, no HIP), and tests/test_memprobe_args.py runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vgpu/calib_args.h"
#include "vgpu/memprobe.h"

namespace calib = vgpu::calib;

static int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)

// One cycle through all n slots, and jump() against walking.
static void ring(uint32_t L, uint32_t seed) {
  const uint32_t n = 1u << L;
  std::vector<uint8_t> seen(n, 0);
  std::vector<uint32_t> order(n);
  uint32_t at = 0;
  for (uint32_t s = 0; s < n; s++) {
    CHECK(at < n && !seen[at]);
    seen[at] = 1;
    order[s] = at;
    at = vgpu_ring_next_slot(at, L, seed);
  }
  CHECK(at == 0);
  const uint64_t ks[] = {0, 1, 2, (uint64_t)n - 1, n, (uint64_t)n + 1, 1000, 1ull << 32, (1000ull << 40), ~0ull};
  for (uint64_t k : ks) {
    CHECK(vgpu_ring_jump_slot(0, k, L, seed) == order[k & (n - 1)]);
    CHECK(vgpu_ring_jump_slot(order[n - 1], k, L, seed) == order[(k + n - 1) & (n - 1)]);
  }
  // the product a chain's start is made of: chain 2^40 + 4095 * 64 + 63 times 2^18 steps wraps mod 2^64
  const uint64_t g = (1ull << 40) + 4095ull * 64 + 63, steps = 1ull << 18;
  CHECK(vgpu_ring_jump_slot(0, g * steps, L, seed) == order[(g * steps) & (n - 1)]);
}

int main() {
  const uint32_t seeds[] = {0u, 1u, 0xDEADBEEFu, 0xFFFFFFFFu};
  for (uint32_t seed : seeds) {
    CHECK(vgpu_ring_c(seed) & 1u);
    for (uint32_t L : {1u, 2u, 3u, 10u, 16u, 20u}) ring(L, seed);
  }
  CHECK(vgpu_ring_mask(1) == 1u && vgpu_ring_mask(25) == 0x1FFFFFFu);
  // the last slot of the largest ring, and jumps at the bound values of L
  CHECK(vgpu_ring_next_slot(0x1FFFFFFu, 25, 7) <= 0x1FFFFFFu);
  CHECK(vgpu_ring_jump_slot(0x1FFFFFFu, ~0ull, 25, 7) <= 0x1FFFFFFu);
  CHECK(vgpu_ring_jump_slot(1, ~0ull, 1, 7) <= 1u);
  CHECK(vgpu_ring_jump_slot(5, 1, 25, 7) == vgpu_ring_next_slot(5, 25, 7));

  alignas(128) static unsigned char buf[256];
  void *a = buf, *odd = buf + 16, *off = buf + 4;
  CHECK(calib::ring_build_args_ok(a, 1) && calib::ring_build_args_ok(a, 25));
  CHECK(!calib::ring_build_args_ok(a, 0) && !calib::ring_build_args_ok(a, 26) && !calib::ring_build_args_ok(a, -1));
  CHECK(!calib::ring_build_args_ok(nullptr, 1) && !calib::ring_build_args_ok(odd, 1));

  CHECK(calib::chase_args_ok(a, 1, 1, 1, 1, a) && calib::chase_args_ok(a, 25, 4096, 64, 1 << 18, a));
  CHECK(!calib::chase_args_ok(a, 0, 1, 1, 1, a) && !calib::chase_args_ok(a, 26, 1, 1, 1, a));
  CHECK(!calib::chase_args_ok(a, 1, 0, 1, 1, a) && !calib::chase_args_ok(a, 1, 4097, 1, 1, a));
  CHECK(!calib::chase_args_ok(a, 1, 1, 0, 1, a) && !calib::chase_args_ok(a, 1, 1, 65, 1, a));
  CHECK(!calib::chase_args_ok(a, 1, 1, 1, 0, a) && !calib::chase_args_ok(a, 1, 1, 1, (1 << 18) + 1, a));
  CHECK(!calib::chase_args_ok(nullptr, 1, 1, 1, 1, a) && !calib::chase_args_ok(a, 1, 1, 1, 1, nullptr));
  CHECK(!calib::chase_args_ok(a, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, a));
  CHECK(!calib::chase_args_ok(a, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, a));

  CHECK(calib::stream_args_ok(a, 4, 0, 4, 0, 1, a) && calib::stream_args_ok(a, ~0ull, 1, 16384, 1000000, 1 << 20, odd));
  CHECK(!calib::stream_args_ok(a, 4, 2, 4, 0, 1, a) && !calib::stream_args_ok(a, 4, -1, 4, 0, 1, a));
  CHECK(!calib::stream_args_ok(a, 4, 0, 0, 0, 1, a) && !calib::stream_args_ok(a, 4, 0, 3, 0, 1, a));
  CHECK(!calib::stream_args_ok(a, 1 << 20, 0, 16388, 0, 1, a) && !calib::stream_args_ok(a, 3, 0, 4, 0, 1, a));
  CHECK(!calib::stream_args_ok(a, 4, 0, 4, -1, 1, a) && !calib::stream_args_ok(a, 4, 0, 4, 1000001, 1, a));
  CHECK(!calib::stream_args_ok(a, 4, 0, 4, 0, 0, a) && !calib::stream_args_ok(a, 4, 0, 4, 0, (1 << 20) + 1, a));
  CHECK(!calib::stream_args_ok(nullptr, 4, 0, 4, 0, 1, a) && !calib::stream_args_ok(a, 4, 0, 4, 0, 1, nullptr));
  CHECK(!calib::stream_args_ok(off, 4, 0, 4, 0, 1, a) && !calib::stream_args_ok(a, 4, 0, 4, 0, 1, off));
  CHECK(!calib::stream_args_ok(a, 4, 0, INT32_MIN, INT32_MIN, INT32_MIN, a));
  // the ticks a stream gets hold whatever the check said
  CHECK(calib::spin_ticks(-1) == 0 && calib::spin_ticks(INT32_MAX) == 100000000ull && calib::spin_ticks(INT32_MIN) == 0);

  if (failures) {
    std::fprintf(stderr, "memprobe_host: %d checks failed\n", failures);
    return 1;
  }
  std::puts("memprobe_host ok");
  return 0;
}
