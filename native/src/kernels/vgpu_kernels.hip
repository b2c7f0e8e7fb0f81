// gfx950 calibration kernels for the vGPU data plane (test instruments, SURVEY.md
// §2.8: "a calibration kernel that measures CU-mask / temporal-limit fidelity; a
// bandwidth probe for host-spill throughput").
//
//  * vgpu_cu_census   every workgroup records where it ran (XCC id from
//                     HW_REG_XCC_ID, SE/CU from HW_REG_HW_ID) while spinning long
//                     enough that the dispatcher has to spread the grid over every
//                     CU the queue may use: the number of distinct CUs observed is
//                     the spatial partition actually enforced.
//  * vgpu_spin        fixed-duration workgroups (s_memrealtime, 100 MHz) for
//                     duty-cycle / temporal-limit measurements; vgpu_spin_lds the
//                     same holding dynamic LDS (few workgroups per CU at a time). A spin
//                     lasts 0 .. 1 s: nothing longer, and nothing negative, is launched.
//  * vgpu_stream_copy 16-byte-per-lane grid-stride copy; with the source in spilled
//                     host memory it measures the oversubscription path's bandwidth.
//  * vgpu_scratch_hog a kernel with a 16 KiB-per-lane private segment (dynamically
//                     indexed, so it lives in scratch): makes ROCr allocate a large
//                     scratch backing store behind the allocation hooks' back, which the
//                     shim's context accounting has to pick up from KFD.
//  * vgpu_pattern_*   word-exact fill / verify at memory bandwidth (vgpu/pattern.h; the kernels
//                     are device_kernels.h, shared with the code object inside vgpu-validate):
//                     integrity of buffers the spill, promotion and demotion paths move.
//  * vgpu_cu_selftest four-wave workgroups whose every wave runs the known-answer test of
//                     vgpu/selftest.h (VALU, LDS, i8 and f16 MFMA) and records where it ran and
//                     its four words, then holds its CU like the census: which CU, and which
//                     unit of it, computes wrong (the kernel is device_kernels.h as well).
//
// C ABI, loaded with ctypes; pointers are device pointers (e.g. torch data_ptr()) and
// `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream). What each entry point
// accepts is vgpu/calib_args.h (host-only, tested in tests/core_tests.cpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_kernels.h"
#include "vgpu/calib_args.h"

namespace calib = vgpu::calib;

namespace {

__global__ void __launch_bounds__(64) census_kernel(uint32_t* out, uint64_t spin_ticks) {
  vgpu_dev::census_body(out, spin_ticks);
}

__global__ void __launch_bounds__(64) spin_kernel(uint64_t spin_ticks, uint64_t* done) {
  uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < spin_ticks) __builtin_amdgcn_s_sleep(1);
  if (threadIdx.x == 0 && done) atomicAdd(reinterpret_cast<unsigned long long*>(done), 1ull);
}

// Same spin, but each workgroup also holds `dynamic LDS` bytes, so only a few fit on a CU
// at once: the grid has to be dispatched over many rounds (like a GEMM kernel's), which
// exposes dispatcher-level interference between CU-masked queues.
__global__ void __launch_bounds__(64) spin_lds_kernel(uint64_t spin_ticks) {
  extern __shared__ unsigned char dyn_lds[];
  uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < spin_ticks) __builtin_amdgcn_s_sleep(1);
  if (threadIdx.x == 0) dyn_lds[0] = 1;
}

constexpr int kScratchWords = 4096;  // 16 KiB of private memory per lane

__global__ void __launch_bounds__(64) scratch_kernel(uint32_t* out, uint32_t stride) {
  uint32_t buf[kScratchWords];
  const uint32_t lane = threadIdx.x;
  // Data-dependent indices keep the array out of registers (stride comes from the host).
  for (int i = 0; i < kScratchWords; i++) buf[(i * stride + lane) % kScratchWords] = i ^ lane;
  uint32_t acc = 0;
  for (int i = 0; i < kScratchWords; i += 7) acc += buf[(i * stride) % kScratchWords];
  out[blockIdx.x * 64 + lane] = acc;
}

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) copy_kernel(u32x4* __restrict__ dst, const u32x4* __restrict__ src, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = __builtin_nontemporal_load(&src[i]);
}

}  // namespace

extern "C" {

// The argument rules are vgpu/calib_args.h: every entry point below returns -1, before any HIP
// call, for what they refuse (nblocks outside 1..2^20, spin_us outside 0..1000000, ...), 0 after
// a launch and -2 when the launch failed. The ticks a kernel spins come from the clamped spin_us.

// Launches `nblocks` single-wave workgroups that each spin `spin_us` microseconds and
// write their location code to out[block] (device buffer of nblocks uint32).
int vgpu_cu_census(uint32_t* out, int nblocks, int spin_us, void* stream) {
  if (!calib::census_args_ok(out, nblocks, spin_us)) return -1;
  hipLaunchKernelGGL(census_kernel, dim3(nblocks), dim3(64), 0, (hipStream_t)stream, out,
                     calib::spin_ticks(spin_us));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// `nblocks` single-wave workgroups spinning `spin_us` each; lane 0 of each then adds 1 to the
// device uint64 `done`, which may be null.
int vgpu_spin(int nblocks, int spin_us, uint64_t* done, void* stream) {
  if (!calib::spin_args_ok(nblocks, spin_us)) return -1;
  hipLaunchKernelGGL(spin_kernel, dim3(nblocks), dim3(64), 0, (hipStream_t)stream, calib::spin_ticks(spin_us), done);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// `nblocks` single-wave workgroups spinning `spin_us` each while holding `lds_bytes`
// (1..163840, a CU's whole LDS) of dynamic LDS.
int vgpu_spin_lds(int nblocks, int spin_us, int lds_bytes, void* stream) {
  if (!calib::spin_lds_args_ok(nblocks, spin_us, lds_bytes)) return -1;
  hipLaunchKernelGGL(spin_lds_kernel, dim3(nblocks), dim3(64), (size_t)lds_bytes, (hipStream_t)stream,
                     calib::spin_ticks(spin_us));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// `nblocks` single-wave workgroups, each lane with a 16 KiB private array; out holds
// nblocks * 64 uint32. `stride` must be odd and positive (any odd value gives a permutation).
int vgpu_scratch_hog(uint32_t* out, int nblocks, int stride, void* stream) {
  if (!calib::scratch_args_ok(out, nblocks, stride)) return -1;
  hipLaunchKernelGGL(scratch_kernel, dim3(nblocks), dim3(64), 0, (hipStream_t)stream, out, (uint32_t)stride);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Copies `bytes` (a multiple of 16) from src to dst: both 16-byte aligned, not overlapping.
// Zero bytes launch nothing.
int vgpu_stream_copy(void* dst, const void* src, size_t bytes, void* stream) {
  const calib::CopyArgs args = calib::copy_args(dst, src, bytes);
  if (args != calib::kCopyLaunch) return args;
  size_t n = bytes / 16;
  // >> 256 CUs x 8 waves: enough workgroups in flight to saturate HBM / the link.
  int blocks = (int)((n + 255) / 256);
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(copy_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (u32x4*)dst, (const u32x4*)src, n);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Fills `bytes` (multiple of 16) at dst: word k becomes w(base + k, seed) (vgpu/pattern.h).
int vgpu_pattern_fill(void* dst, size_t bytes, uint64_t base, uint32_t seed, void* stream) {
  if (!dst || !bytes || (bytes & 15)) return -1;
  const uint64_t n = bytes / 16;
  hipLaunchKernelGGL(pattern_fill, dim3(vgpu_dev::pattern_blocks(n)), dim3(vgpu_dev::kPatternBlock), 0,
                     (hipStream_t)stream, (vgpu_dev::u32x4*)dst, n, base, seed);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Verifies `bytes` (multiple of 16) at src against the same pattern. `out` is two device
// uint64 the caller preset to {0, ~0}: the mismatching words and the lowest such word index.
int vgpu_pattern_check(const void* src, size_t bytes, uint64_t base, uint32_t seed, uint64_t* out, void* stream) {
  if (!src || !out || !bytes || (bytes & 15)) return -1;
  const uint64_t n = bytes / 16;
  hipLaunchKernelGGL(pattern_check, dim3(vgpu_dev::pattern_blocks(n)), dim3(vgpu_dev::kPatternBlock), 0,
                     (hipStream_t)stream, (const vgpu_dev::u32x4*)src, n, base, seed, (unsigned long long*)out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Flips one bit in each of the `n` words of dst listed in idx (device array of word indices,
// which the caller keeps inside the buffer).
int vgpu_pattern_poke(void* dst, const uint64_t* idx, int n, void* stream) {
  if (!dst || !idx || n <= 0) return -1;
  hipLaunchKernelGGL(pattern_poke, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, (uint32_t*)dst,
                     (const unsigned long long*)idx, (uint32_t)n);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// `nblocks` workgroups of four waves; each wave runs the known-answer test of vgpu/selftest.h
// under (seed, rounds), writes eight words at out[(4 * block + wave) * 8] (location with SIMD,
// valu, lds, mfma_i8, mfma_f16, three zeros; out holds nblocks * 32 uint32) and then holds
// `hold_us`. `bad` is a device array of `n_bad` (at most 64) workgroup indices whose wave 0 runs
// the test with its injected input bit; it may be null when n_bad is 0.
int vgpu_cu_selftest(uint32_t* out, int nblocks, uint32_t seed, int rounds, int hold_us, const uint32_t* bad, int n_bad,
                     void* stream) {
  if (!out || nblocks <= 0 || nblocks > (1 << 20) || rounds < 1 || rounds > (int)VGPU_SELFTEST_MAX_ROUNDS ||
      hold_us < 0 || hold_us > 100000 || n_bad < 0 || n_bad > (int)VGPU_SELFTEST_MAX_BAD || (n_bad && !bad))
    return -1;
  hipLaunchKernelGGL(cu_selftest, dim3(nblocks), dim3(64 * vgpu_dev::kSelftestWaves), 0, (hipStream_t)stream, out, seed,
                     (uint32_t)rounds, (uint64_t)hold_us * 100, bad, (uint32_t)n_bad);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
