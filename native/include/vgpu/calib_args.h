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

}  // namespace calib
}  // namespace vgpu
