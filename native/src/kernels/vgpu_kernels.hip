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
//  * vgpu_ring_build / vgpu_mem_chase  a ring of 128-byte slots linked by a full-period affine
//                     map (vgpu/memprobe.h) and a pointer chase over it: dependent vector loads
//                     between s_memtime / s_memrealtime stamps, every chain's end slot known to
//                     the host. The latency of whichever level of the hierarchy the ring fits.
//  * vgpu_mem_stream  waves that read or write a chunk of their own for a fixed time with
//                     non-temporal 16-byte accesses: a controlled memory load, word-exact.
//
// C ABI, loaded with ctypes; pointers are device pointers (e.g. torch data_ptr()) and
// `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream). What each entry point
// accepts is vgpu/calib_args.h (host-only, tested in tests/core_tests.cpp and tests/memprobe_host.cpp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_kernels.h"
#include "vgpu/calib_args.h"
#include "vgpu/memprobe.h"

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

// ---- the memory-system probe (vgpu/memprobe.h)

using u32x2 = unsigned int __attribute__((ext_vector_type(2)));

constexpr unsigned kChaseRecord = 8;   // end slot, location, d(s_memtime) lo, hi, d(s_memrealtime), 0, 0, 0
constexpr unsigned kStreamRecord = 8;  // passes, sum, location, d(s_memrealtime) lo, hi, 0, 0, 0

// Census code plus SIMD id, as cu_selftest records it.
__device__ inline uint32_t location_with_simd() {
  const uint32_t hw = __builtin_amdgcn_s_getreg(vgpu_dev::kHwRegHwId | (0u << 6) | (31u << 11));
  const uint32_t xcc = __builtin_amdgcn_s_getreg(vgpu_dev::kHwRegXccId | (0u << 6) | (3u << 11));
  return ((hw >> 4) & 0x3) << 16 | (xcc & 0xf) << 12 | ((hw >> 13) & 0x7) << 8 | ((hw >> 12) & 0x1) << 4 | ((hw >> 8) & 0xf);
}

// Words 0 and 1 of every slot, one 8-byte store per slot; words 2..31 are left alone.
__global__ void __launch_bounds__(256) ring_build_kernel(uint32_t* __restrict__ ring, uint32_t L, uint32_t seed) {
  const uint64_t n = 1ull << L, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u32x2 v;
    v.x = vgpu_ring_next_slot((uint32_t)i, L, seed);
    v.y = (uint32_t)i ^ seed;
    *reinterpret_cast<u32x2*>(ring + i * VGPU_RING_SLOT_WORDS) = v;
  }
}

// Single-wave workgroups; lane l < lanes of block b walks chain g = chain_base + 64 b + l from
// next^(g * steps)(first). The start depends on threadIdx.x, so the address is not uniform and
// the loads are vector loads (global_load_dword, the vector L1 -> L2 path of a tenant's kernel)
// and not scalar ones. `& mask` keeps a corrupted ring inside the buffer.
__global__ void __launch_bounds__(64)
mem_chase_kernel(const uint32_t* ring, uint32_t L, uint32_t seed, uint32_t lanes, uint32_t steps, uint32_t first,
                 uint64_t chain_base, uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x;
  if (lane >= lanes) return;
  const uint64_t g = chain_base + 64ull * blockIdx.x + lane;
  const uint32_t mask = vgpu_ring_mask(L);
  uint32_t at = vgpu_ring_jump_slot(first & mask, g * steps, L, seed);
  // the start and the ring's address are there before the opening stamps (the pointer is an input
  // only: passed through the asm it would lose its address space, and the loads would be flat ones)
  asm volatile("" : "+v"(at) : "s"(ring));
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  for (uint32_t s = 0; s < steps; s++) at = ring[(uint64_t)at * VGPU_RING_SLOT_WORDS] & mask;
  // the closing stamps follow the last load's arrival: without this its wait may sink below them
  asm volatile("s_waitcnt vmcnt(0)" ::"v"(at) : "memory");
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  const uint64_t dc = c1 - c0;
  uint32_t* rec = out + ((uint64_t)blockIdx.x * 64 + lane) * kChaseRecord;
  rec[0] = at;
  rec[1] = location_with_simd();
  rec[2] = (uint32_t)dc;
  rec[3] = (uint32_t)(dc >> 32);
  rec[4] = (uint32_t)(r1 - r0);
  rec[5] = rec[6] = rec[7] = 0;
}

// The unit is the wave: wave w of `waves` owns n_vec / waves consecutive 16-byte vectors (the
// first n_vec % waves waves one more) and sweeps them, 16 bytes per lane, pass after pass until
// `ticks` of the 100 MHz clock have gone by or `max_passes` are done. Every wave reads the clock
// itself (a scalar read), so the loop condition is wave-uniform and needs no barrier; a pass
// once begun is finished, so ticks = 0 is exactly one pass.
__global__ void __launch_bounds__(256)
mem_stream_kernel(vgpu_dev::u32x4* buf, uint64_t n_vec, uint32_t waves, uint32_t mode, uint64_t ticks, uint32_t max_passes,
                  uint64_t base, uint32_t seed, uint32_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= waves) return;
  const uint64_t q = n_vec / waves, r = n_vec % waves;
  const uint64_t begin = w * q + (w < r ? w : r), len = q + (w < r ? 1 : 0);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint64_t dt;
  uint32_t passes = 0, sum = 0;
  do {
    asm volatile("" ::: "memory");  // every pass touches memory again
    if (mode == 0) {
#pragma unroll 4
      for (uint64_t i = lane; i < len; i += 64) {
        const vgpu_dev::u32x4 v = __builtin_nontemporal_load(&buf[begin + i]);
        sum += v.x + v.y + v.z + v.w;
      }
    } else {
      for (uint64_t i = lane; i < len; i += 64)
        __builtin_nontemporal_store(vgpu_dev::pattern_vec(base + 4 * (begin + i), seed), &buf[begin + i]);
    }
    passes++;
    dt = __builtin_amdgcn_s_memrealtime() - t0;
  } while (passes < max_passes && dt < ticks);
  sum = vgpu_dev::wave_sum(sum);
  asm volatile("s_waitcnt vmcnt(0)" ::"v"(sum) : "memory");  // the last loads and stores have landed
  dt =__builtin_amdgcn_s_memrealtime() - t0;
  if (lane == 0) {
    uint32_t* rec = out + w * kStreamRecord;
    rec[0] = passes;
    rec[1] = sum;
    rec[2] = location_with_simd();
    rec[3] = (uint32_t)dt;
    rec[4] = (uint32_t)(dt >> 32);
    rec[5] = rec[6] = rec[7] = 0;
  }
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

// The ring of vgpu/memprobe.h, on the host: no HIP call.
uint32_t vgpu_ring_next(uint32_t i, int L, uint32_t seed) {
  return calib::ring_l_ok(L) ? vgpu_ring_next_slot(i, (uint32_t)L, seed) : ~0u;
}

// The slot `k` steps after `i`; ~0 for an L outside 1..25.
uint32_t vgpu_ring_jump(uint32_t i, uint64_t k, int L, uint32_t seed) {
  return calib::ring_l_ok(L) ? vgpu_ring_jump_slot(i, k, (uint32_t)L, seed) : ~0u;
}

// Writes words 0 and 1 of the 2^L slots of 128 bytes at `ring` (128-byte aligned, L in 1..25).
int vgpu_ring_build(void* ring, int L, uint32_t seed, void* stream) {
  if (!calib::ring_build_args_ok(ring, L)) return -1;
  hipLaunchKernelGGL(ring_build_kernel, dim3(vgpu_dev::pattern_blocks(1ull << L)), dim3(vgpu_dev::kPatternBlock), 0,
                     (hipStream_t)stream, (uint32_t*)ring, (uint32_t)L, seed);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// `nblocks` (1..4096) single-wave workgroups; lane l < lanes (1..64) of block b makes `steps`
// (1..2^18) dependent loads from slot next^((chain_base + 64 b + l) * steps)(first) of a built
// ring and writes eight words at out[(64 b + l) * 8]: end slot, location with SIMD, the
// s_memtime difference (lo, hi), the s_memrealtime difference, three zeros. out holds
// nblocks * 512 uint32; lanes >= `lanes` write nothing.
int vgpu_mem_chase(const void* ring, int L, uint32_t seed, int nblocks, int lanes, int steps, uint32_t first,
                   uint64_t chain_base, uint32_t* out, void* stream) {
  if (!calib::chase_args_ok(ring, L, nblocks, lanes, steps, out)) return -1;
  hipLaunchKernelGGL(mem_chase_kernel, dim3(nblocks), dim3(64), 0, (hipStream_t)stream, (const uint32_t*)ring, (uint32_t)L,
                     seed, (uint32_t)lanes, (uint32_t)steps, first, chain_base, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// `waves` (1..16384, a multiple of 4) waves sweep the `n_vec` (>= waves) 16-byte vectors at buf
// for `duration_us` (0..1000000) or `max_passes` (1..2^20) passes, reading (mode 0) or writing
// the pattern of (base, seed) (mode 1). Wave w writes eight words at out[8 w]: passes, sum of all
// words read (0 in write mode), location with SIMD, the s_memrealtime difference (lo, hi), three zeros.
int vgpu_mem_stream(void* buf, uint64_t n_vec, int mode, int waves, int duration_us, int max_passes, uint64_t base,
                    uint32_t seed, uint32_t* out, void* stream) {
  if (!calib::stream_args_ok(buf, n_vec, mode, waves, duration_us, max_passes, out)) return -1;
  hipLaunchKernelGGL(mem_stream_kernel, dim3(waves / 4), dim3(256), 0, (hipStream_t)stream, (vgpu_dev::u32x4*)buf, n_vec,
                     (uint32_t)waves, (uint32_t)mode, calib::spin_ticks(duration_us), (uint32_t)max_passes, base, seed, out);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
