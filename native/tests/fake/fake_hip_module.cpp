// The module API of the fake libamdhip64.so: what vgpu-validate --conformance uses to run
// the kernels of its embedded gfx950 code object (hipModuleLoadData / hipModuleGetFunction /
// hipModuleLaunchKernel / hipModuleUnload).
//
// The fake's device memory is untouchable address space, so the kernels are emulated on what
// the launch says rather than on memory:
//   * pattern_fill / pattern_check / pattern_poke keep a shadow per destination pointer:
//     seed, base, length and the poked words; a check compares the pattern it is asked for
//     with the shadow's (vgpu/pattern.h) and writes count and lowest index to `out`, which is
//     pinned host memory (real memory here);
//   * census writes location codes for as many CUs as the stream's queue mask allows into
//     its pinned host output;
//   * cu_selftest writes, for every wave, a location on one of those CUs (SIMD 0..3 in turn)
//     and the four words of vgpu/selftest.h, with the injected words in wave 0 of the listed
//     workgroups. FAKE_HIP_SELFTEST_BAD=<census code>:<unit> makes every wave on that CU
//     return a wrong word for that unit (valu, lds, mfma_i8 or mfma_f16).
// Every launch then goes through the fake's timed-kernel path (fake_hip.cpp), so the GPU
// thread, the occupancy file and the shim's launch gate see it like any other kernel.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <hsa/hsa.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>

#include "vgpu/pattern.h"
#include "vgpu/selftest.h"

extern "C" {
void fake_hip_record(const char* name);
void fake_hip_priv_submit(hipStream_t stream, uint32_t us);
hsa_queue_t* fake_hip_priv_stream_queue(hipStream_t stream);
int fake_rocr_queue_state(const hsa_queue_t* queue, uint32_t* mask_words8, int* priority, int* device);
}

namespace {

enum Kind { kCensus, kFill, kCheck, kPoke, kSelftest };

struct FakeFunction {
  uint32_t us;  // first: a kernel of the fake is a pointer to its duration
  Kind kind;
};

struct FakeModule {
  FakeFunction fn[5] = {{2000, kCensus}, {100, kFill}, {100, kCheck}, {20, kPoke}, {2000, kSelftest}};
};

struct Shadow {
  uint32_t seed = 0;
  uint64_t base = 0, words = 0;
  std::set<uint64_t> poked;
};

std::mutex g_mu;
std::map<uintptr_t, Shadow> g_shadow;

template <typename T>
T arg(void** params, int i) {
  T v;
  memcpy(&v, params[i], sizeof(T));
  return v;
}

// The census codes of the CUs that the stream's queue mask allows.
int masked_cus(hipStream_t stream, uint32_t codes[256]) {
  uint32_t mask[8];
  memset(mask, 0xff, sizeof(mask));
  if (hsa_queue_t* q = fake_hip_priv_stream_queue(stream)) fake_rocr_queue_state(q, mask, nullptr, nullptr);
  int n = 0;
  for (int cu = 0; cu < 256; cu++)
    if ((mask[cu / 32] >> (cu % 32)) & 1u) codes[n++] = (uint32_t)(cu / 32) << 12 | (uint32_t)((cu % 32) / 8) << 8 | (cu % 8);
  return n;
}

void run_census(void** params, unsigned blocks, hipStream_t stream) {
  uint32_t* out = arg<uint32_t*>(params, 0);
  uint32_t codes[256];
  const int n = masked_cus(stream, codes);
  for (unsigned b = 0; n && b < blocks; b++) out[b] = codes[b % n];
}

void run_selftest(void** params, unsigned blocks, hipStream_t stream) {
  uint32_t* out = arg<uint32_t*>(params, 0);
  const uint32_t seed = arg<uint32_t>(params, 1), rounds = arg<uint32_t>(params, 2);
  const uint32_t* bad = arg<const uint32_t*>(params, 4);
  uint32_t n_bad = arg<uint32_t>(params, 5);
  if (n_bad > VGPU_SELFTEST_MAX_BAD) n_bad = VGPU_SELFTEST_MAX_BAD;
  uint32_t words[2][4], codes[256];
  if (vgpu_selftest_expected(seed, rounds, 0, words[0]) != 0 || vgpu_selftest_expected(seed, rounds, 1, words[1]) != 0) return;
  // FAKE_HIP_SELFTEST_BAD=<census code>:<unit>
  long bad_cu = -1;
  int bad_unit = -1;
  if (const char* e = getenv("FAKE_HIP_SELFTEST_BAD")) {
    char* colon = nullptr;
    const unsigned long code = strtoul(e, &colon, 0);
    const char* names[] = {"valu", "lds", "mfma_i8", "mfma_f16"};
    for (int u = 0; colon && *colon == ':' && u < 4; u++)
      if (!strcmp(colon + 1, names[u])) bad_cu = (long)code, bad_unit = u;
  }
  const int n = masked_cus(stream, codes);
  for (unsigned b = 0; n && b < blocks; b++) {
    bool listed = false;
    for (uint32_t k = 0; k < n_bad; k++) listed |= bad[k] == b;
    for (unsigned w = 0; w < 4; w++) {
      uint32_t* rec = out + ((size_t)b * 4 + w) * 8;
      // consecutive workgroups on consecutive CUs, and each CU's workgroups on its SIMDs in turn
      const uint32_t cu = codes[b % n], simd = (b / n + w) & 3u;
      rec[0] = simd << 16 | cu;
      memcpy(rec + 1, words[listed && w == 0], sizeof(words[0]));
      if ((long)cu == bad_cu) rec[1 + bad_unit] ^= 0x00010000u;
      rec[5] = rec[6] = rec[7] = 0;
    }
  }
}

void run_check(void** params) {
  const uintptr_t src = arg<uintptr_t>(params, 0);
  const uint64_t words = arg<uint64_t>(params, 1) * 4, base = arg<uint64_t>(params, 2);
  const uint32_t seed = arg<uint32_t>(params, 3);
  unsigned long long* out = arg<unsigned long long*>(params, 4);
  std::lock_guard<std::mutex> l(g_mu);
  auto it = g_shadow.find(src);
  uint64_t bad = 0, first = ~0ull;
  auto miss = [&](uint64_t k) {
    bad++;
    if (k < first) first = k;
  };
  if (it == g_shadow.end()) {  // never filled: nothing matches
    bad = words;
    first = 0;
  } else if (it->second.seed == seed && it->second.base == base) {
    for (uint64_t k : it->second.poked)
      if (k < words) miss(k);
    for (uint64_t k = it->second.words; k < words; k++) miss(k);
  } else {
    const Shadow& s = it->second;
    for (uint64_t k = 0; k < words; k++) {
      const uint32_t have = vgpu_pattern_word(s.base + k, s.seed) ^ (s.poked.count(k) ? 0x00010000u : 0u);
      if (k >= s.words || have != vgpu_pattern_word(base + k, seed)) miss(k);
    }
  }
  out[0] += bad;
  if (first < out[1]) out[1] = first;
}

}  // namespace

extern "C" {

hipError_t hipModuleLoadData(hipModule_t* module, const void* image) {
  if (!module || !image || memcmp(image, "\177ELF", 4) != 0) return hipErrorInvalidImage;
  *module = reinterpret_cast<hipModule_t>(new FakeModule());
  return hipSuccess;
}

hipError_t hipModuleUnload(hipModule_t module) {
  if (!module) return hipErrorInvalidResourceHandle;
  delete reinterpret_cast<FakeModule*>(module);
  return hipSuccess;
}

hipError_t hipModuleGetFunction(hipFunction_t* function, hipModule_t module, const char* name) {
  if (!function || !module || !name) return hipErrorInvalidValue;
  FakeModule* m = reinterpret_cast<FakeModule*>(module);
  const char* names[] = {"census", "pattern_fill", "pattern_check", "pattern_poke", "cu_selftest"};
  for (int i = 0; i < 5; i++)
    if (!strcmp(name, names[i])) {
      *function = reinterpret_cast<hipFunction_t>(&m->fn[i]);
      return hipSuccess;
    }
  return hipErrorNotFound;
}

hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned int gx, unsigned int gy, unsigned int gz, unsigned int bx,
                                 unsigned int by, unsigned int bz, unsigned int, hipStream_t stream, void** params,
                                 void**) {
  fake_hip_record("hipModuleLaunchKernel");
  if (!f || !params || !gx || !bx) return hipErrorInvalidValue;
  const FakeFunction* fn = reinterpret_cast<const FakeFunction*>(f);
  switch (fn->kind) {
    case kCensus: run_census(params, gx, stream); break;
    case kSelftest: run_selftest(params, gx, stream); break;
    case kFill: {
      std::lock_guard<std::mutex> l(g_mu);
      Shadow& s = g_shadow[arg<uintptr_t>(params, 0)];
      s.words = arg<uint64_t>(params, 1) * 4;
      s.base = arg<uint64_t>(params, 2);
      s.seed = arg<uint32_t>(params, 3);
      s.poked.clear();
      break;
    }
    case kCheck: run_check(params); break;
    case kPoke: {
      const unsigned long long* idx = arg<const unsigned long long*>(params, 1);
      const uint32_t n = arg<uint32_t>(params, 2);
      std::lock_guard<std::mutex> l(g_mu);
      Shadow& s = g_shadow[arg<uintptr_t>(params, 0)];
      for (uint32_t i = 0; i < n; i++)
        if (!s.poked.erase(idx[i])) s.poked.insert(idx[i]);
      break;
    }
  }
  fake_hip_priv_submit(stream, fn->us);
  return hipSuccess;
}

}  // extern "C"
