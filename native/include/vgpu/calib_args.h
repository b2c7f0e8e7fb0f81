// Argument rules of the calibration entry points of libvgpu_kernels.so (src/kernels/vgpu_kernels.hip).
//
// Plain host C++, no HIP: the entry points apply these before any HIP call and return -1 for
// whatever they refuse, and tests/core_tests.cpp checks them at both sides of every bound
// without a GPU. A spinning kernel with a wrong duration never returns on a GPU that others
// share, so the ticks a kernel gets are computed from the clamped value (spin_ticks): even a
// wrong check cannot produce an unbounded spin.
//
//   all          nblocks in 1 .. 2^20
//   census       spin_us in 0 .. 1 000 000; out non-null
//   spin         spin_us in 0 .. 1 000 000
//   spin_lds     spin_us in 0 .. 1 000 000; lds_bytes in 1 .. 163840 (a CU's whole LDS)
//   scratch_hog  stride odd and > 0; out non-null
//   stream_copy  bytes a multiple of 16; both pointers non-null and 16-byte aligned;
//                bytes == 0 is accepted and launches nothing
//   ring_build   L in 1 .. 25 (vgpu/memprobe.h); the ring non-null and 128-byte aligned
//   mem_chase    L in 1 .. 25; nblocks in 1 .. 4096; lanes in 1 .. 64; steps in 1 .. 2^18 (under
//                about a second even at a few us per load: a ring in spilled host memory, or
//                contention); ring and out non-null
//   mem_stream   mode 0 (read) or 1 (write); waves in 1 .. 16384 and a multiple of 4;
//                n_vec >= waves; duration_us in 0 .. 1 000 000 (its ticks are spin_ticks, clamped);
//                max_passes in 1 .. 2^20; buffer and out non-null and 16-byte aligned
#pragma once

#include <cstddef>
#include <cstdint>

namespace vgpu {
namespace calib {

constexpr int kMaxBlocks = 1 << 20;
constexpr int kMaxSpinUs = 1000000;
constexpr int kMaxLdsBytes = 160 * 1024;
constexpr uint64_t kTicksPerUs = 100;  // s_memrealtime counts at 100 MHz

inline bool blocks_ok(int nblocks) { return nblocks >= 1 && nblocks <= kMaxBlocks; }
inline bool spin_us_ok(int spin_us) { return spin_us >= 0 && spin_us <= kMaxSpinUs; }

// Ticks of the 100 MHz clock for `spin_us`, clamped to 0 .. kMaxSpinUs first: at most 10^8.
inline uint64_t spin_ticks(int spin_us) {
  const int us = spin_us < 0 ? 0 : spin_us > kMaxSpinUs ? kMaxSpinUs : spin_us;
  return (uint64_t)us * kTicksPerUs;
}

inline bool census_args_ok(const void* out, int nblocks, int spin_us) {
  return out && blocks_ok(nblocks) && spin_us_ok(spin_us);
}

inline bool spin_args_ok(int nblocks, int spin_us) { return blocks_ok(nblocks) && spin_us_ok(spin_us); }

inline bool spin_lds_args_ok(int nblocks, int spin_us, int lds_bytes) {
  return spin_args_ok(nblocks, spin_us) && lds_bytes >= 1 && lds_bytes <= kMaxLdsBytes;
}

inline bool scratch_args_ok(const void* out, int nblocks, int stride) {
  return out && blocks_ok(nblocks) && stride > 0 && (stride & 1);
}

enum CopyArgs { kCopyRefused = -1, kCopyNothing = 0, kCopyLaunch = 1 };

inline CopyArgs copy_args(const void* dst, const void* src, size_t bytes) {
  if (!dst || !src || ((uintptr_t)dst & 15) || ((uintptr_t)src & 15) || (bytes & 15)) return kCopyRefused;
  return bytes ? kCopyLaunch : kCopyNothing;
}

constexpr int kMinRingL = 1;
constexpr int kMaxRingL = 25;
constexpr int kMaxChaseBlocks = 4096;
constexpr int kMaxChaseLanes = 64;
constexpr int kMaxChaseSteps = 1 << 18;
constexpr int kMaxStreamWaves = 16384;
constexpr int kMaxStreamPasses = 1 << 20;

inline bool ring_l_ok(int L) { return L >= kMinRingL && L <= kMaxRingL; }

inline bool ring_build_args_ok(const void* ring, int L) { return ring && !((uintptr_t)ring & 127) && ring_l_ok(L); }

inline bool chase_args_ok(const void* ring, int L, int nblocks, int lanes, int steps, const void* out) {
  return ring && out && ring_l_ok(L) && nblocks >= 1 && nblocks <= kMaxChaseBlocks && lanes >= 1 &&
         lanes <= kMaxChaseLanes && steps >= 1 && steps <= kMaxChaseSteps;
}

inline bool stream_args_ok(const void* buf, uint64_t n_vec, int mode, int waves, int duration_us, int max_passes,
                           const void* out) {
  return buf && out && !((uintptr_t)buf & 15) && !((uintptr_t)out & 15) && (mode == 0 || mode == 1) && waves >= 1 &&
         waves <= kMaxStreamWaves && !(waves & 3) && n_vec >= (uint64_t)waves && spin_us_ok(duration_us) &&
         max_passes >= 1 && max_passes <= kMaxStreamPasses;
}

}  // namespace calib
}  // namespace vgpu
