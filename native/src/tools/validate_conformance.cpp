// vgpu-validate --conformance: does this container really have the vGPU it was promised?
//
// The promise is the plugin's limits file (/vgpu/limits, falling back to the environment;
// names as in docs/ABI.md). The observation is what the HIP runtime answers in this process
// and what the shim published in the container's region (VGPU_SHARED_CACHE). The tool links
// no GPU library: libamdhip64 is loaded with dlopen, the gfx950 code object with the census,
// pattern and known-answer kernels (src/kernels/validate_kernels.hip) is embedded in the binary and
// loaded with hipModuleLoadData, and kernels are launched with hipModuleLaunchKernel, so
// inside a pod they pass the shim's launch gate like any tenant's. Every GPU wait is a
// stream synchronize after a bounded amount of work.
//
// Checks per visible HIP device: shim, quota, oom, cus, gate, memory, (--compute) compute and
// (--spill) spill;
// see usage() in vgpu_validate.cpp and docs/ABI.md.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <time.h>
#include <unistd.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "vgpu/config.h"
#include "vgpu/pattern.h"
#include "vgpu/region_api.h"
#include "vgpu/selftest.h"
#include "validate.h"

// src/tools/validate_blob.S: the gfx950 code object (a plain ELF)
extern "C" const unsigned char vgpu_validate_co[];

namespace {

// ---------------------------------------------------------------- the HIP runtime, by name

struct Hip {
  void* lib = nullptr;
  hipError_t (*Init)(unsigned) = nullptr;
  hipError_t (*GetDeviceCount)(int*) = nullptr;
  hipError_t (*SetDevice)(int) = nullptr;
  hipError_t (*DeviceGetAttribute)(int*, hipDeviceAttribute_t, int) = nullptr;
  hipError_t (*DeviceGetUuid)(hipUUID*, hipDevice_t) = nullptr;
  hipError_t (*MemGetInfo)(size_t*, size_t*) = nullptr;
  hipError_t (*DeviceTotalMem)(size_t*, hipDevice_t) = nullptr;
  hipError_t (*Malloc)(void**, size_t) = nullptr;
  hipError_t (*Free)(void*) = nullptr;
  hipError_t (*HostMalloc)(void**, size_t, unsigned) = nullptr;
  hipError_t (*HostFree)(void*) = nullptr;
  hipError_t (*StreamCreate)(hipStream_t*) = nullptr;
  hipError_t (*StreamDestroy)(hipStream_t) = nullptr;
  hipError_t (*StreamSynchronize)(hipStream_t) = nullptr;
  hipError_t (*ModuleLoadData)(hipModule_t*, const void*) = nullptr;
  hipError_t (*ModuleGetFunction)(hipFunction_t*, hipModule_t, const char*) = nullptr;
  hipError_t (*ModuleLaunchKernel)(hipFunction_t, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned,
                                   hipStream_t, void**, void**) = nullptr;
  hipError_t (*ModuleUnload)(hipModule_t) = nullptr;
};

template <typename F>
bool sym(void* lib, const char* name, F* out, std::string* err) {
  *out = reinterpret_cast<F>(dlsym(lib, name));
  if (!*out) *err = std::string("libamdhip64.so has no ") + name;
  return *out != nullptr;
}

bool load_hip(Hip* h, std::string* err) {
  h->lib = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h->lib) h->lib = dlopen("/opt/rocm/lib/libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h->lib) {
    const char* e = dlerror();
    *err = std::string("cannot load the HIP runtime: ") + (e ? e : "libamdhip64.so");
    return false;
  }
  void* l = h->lib;
  return sym(l, "hipInit", &h->Init, err) && sym(l, "hipGetDeviceCount", &h->GetDeviceCount, err) &&
         sym(l, "hipSetDevice", &h->SetDevice, err) && sym(l, "hipDeviceGetAttribute", &h->DeviceGetAttribute, err) &&
         sym(l, "hipDeviceGetUuid", &h->DeviceGetUuid, err) && sym(l, "hipMemGetInfo", &h->MemGetInfo, err) &&
         sym(l, "hipDeviceTotalMem", &h->DeviceTotalMem, err) && sym(l, "hipMalloc", &h->Malloc, err) &&
         sym(l, "hipFree", &h->Free, err) && sym(l, "hipHostMalloc", &h->HostMalloc, err) &&
         sym(l, "hipHostFree", &h->HostFree, err) && sym(l, "hipStreamCreate", &h->StreamCreate, err) &&
         sym(l, "hipStreamDestroy", &h->StreamDestroy, err) &&
         sym(l, "hipStreamSynchronize", &h->StreamSynchronize, err) &&
         sym(l, "hipModuleLoadData", &h->ModuleLoadData, err) &&
         sym(l, "hipModuleGetFunction", &h->ModuleGetFunction, err) &&
         sym(l, "hipModuleLaunchKernel", &h->ModuleLaunchKernel, err) &&
         sym(l, "hipModuleUnload", &h->ModuleUnload, err);
}

// ---------------------------------------------------------------- the promise

struct Promise {
  std::map<std::string, std::string> file;

  void load(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return;
    char line[4096];
    while (fgets(line, sizeof(line), f)) {
      char* eq = strchr(line, '=');
      if (!eq || line[0] == '#') continue;
      std::string k(line, eq), v(eq + 1);
      while (!v.empty() && isspace((unsigned char)v.back())) v.pop_back();
      file[k] = v;
    }
    fclose(f);
  }
  // The limits file first (the plugin's word), then the environment.
  const char* get(const std::string& key) const {
    auto it = file.find(key);
    if (it != file.end()) return it->second.c_str();
    return getenv(key.c_str());
  }
  const char* indexed(const char* name, int i) const {
    const char* v = get(std::string(name) + "_" + std::to_string(i));
    return v ? v : get(name);
  }
  bool truthy(const char* key) const {
    const char* v = get(key);
    return v && (*v == '1' || *v == 't' || *v == 'T' || *v == 'y' || *v == 'Y');
  }
};

// VGPU_DEVICE_MAP entries: (vGPU index, normalised UUID) in map order.
std::vector<std::pair<int, std::string>> parse_map(const char* s) {
  std::vector<std::pair<int, std::string>> out;
  while (s && *s) {
    while (*s && isspace((unsigned char)*s)) s++;
    const char* colon = strchr(s, ':');
    if (!colon) break;
    const char* end = colon + 1;
    while (*end && !isspace((unsigned char)*end)) end++;
    out.emplace_back(atoi(s), vgpu_validate::norm_uuid(std::string(colon + 1, end)));
    s = end;
  }
  return out;
}

// ---------------------------------------------------------------- results

struct Check {
  std::string name, status;
  std::vector<std::pair<std::string, std::string>> fields;  // values already rendered as JSON

  Check& num(const char* k, uint64_t v) {
    fields.emplace_back(k, std::to_string(v));
    return *this;
  }
  Check& real(const char* k, double v) {
    char b[64];
    snprintf(b, sizeof(b), "%.3f", v);
    fields.emplace_back(k, b);
    return *this;
  }
  Check& str(const char* k, const std::string& v) {
    std::string q = "\"";
    for (char c : v) {
      if (c == '"' || c == '\\') q += '\\';
      q += (unsigned char)c < 0x20 ? ' ' : c;
    }
    fields.emplace_back(k, q + "\"");
    return *this;
  }
  Check& null(const char* k) {
    fields.emplace_back(k, "null");
    return *this;
  }
  Check& raw(const char* k, const std::string& json) {
    fields.emplace_back(k, json);
    return *this;
  }
};

struct DeviceReport {
  int device = 0;
  std::string uuid;
  std::vector<Check> checks;
  Check& add(const char* name, const char* status) {
    checks.push_back(Check{name, status, {}});
    return checks.back();
  }
};

double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + ts.tv_nsec * 1e-9;
}

void sleep_ms(int ms) {
  timespec ts{ms / 1000, (ms % 1000) * 1000000L};
  nanosleep(&ts, nullptr);
}

// ---------------------------------------------------------------- the run

struct Run {
  Hip hip;
  vgpu_validate::Options opt;
  Promise promise;
  vgpu_region* region = nullptr;
  hipModule_t module = nullptr;
  hipFunction_t f_census = nullptr, f_fill = nullptr, f_check = nullptr, f_poke = nullptr, f_selftest = nullptr;
  uint64_t launched = 0;  // kernels this process launched (what the gate must have counted)
  int period_ms = 120;

  bool launch(hipFunction_t f, unsigned grid, unsigned block, hipStream_t s, void** args) {
    launched++;
    return hip.ModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, 0, s, args, nullptr) == hipSuccess;
  }
  static unsigned blocks(uint64_t n_vec) {
    uint64_t b = (n_vec + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    return b < 1 ? 1u : (unsigned)b;
  }
  bool fill(void* dst, uint64_t bytes, uint64_t base, uint32_t seed, hipStream_t s) {
    uint64_t n = bytes / 16;
    void* args[] = {&dst, &n, &base, &seed};
    return launch(f_fill, blocks(n), 256, s, args);
  }
  // res: two uint64 in pinned host memory.
  bool check(void* src, uint64_t bytes, uint64_t base, uint32_t seed, uint64_t* res, hipStream_t s) {
    uint64_t n = bytes / 16;
    res[0] = 0;
    res[1] = ~0ull;
    void* args[] = {&src, &n, &base, &seed, &res};
    return launch(f_check, blocks(n), 256, s, args) && hip.StreamSynchronize(s) == hipSuccess;
  }
  bool device_info(int slot, vgpu_device_info* di) const {
    return region && slot >= 0 && vgpu_region_device_info(region, slot, di) == 0;
  }
  bool self(vgpu_proc_info* out) const {
    static vgpu_proc_info procs[1024];
    const int n = region ? vgpu_region_procs(region, procs, 1024) : 0;
    for (int i = 0; i < n; i++)
      if (procs[i].pid == (int32_t)getpid()) {
        *out = procs[i];
        return true;
      }
    return false;
  }
};

// How HIP device `dev` maps onto the region and the promise.
struct Mapping {
  int compute_slot = -1;  // the GPU's region slot: CU share, mode, mask
  int memory_slot = -1;   // the slot holding this device's quota (a split vGPU's own)
  int vgpus_of_gpu = 1;   // HIP devices on this physical GPU
  int limit_index = 0;    // the <i> of VGPU_DEVICE_*_<i> that names this device
  uint64_t promised_mem = 0;
  bool has_promised_mem = false;
};

// Two UUIDs name one physical GPU: a split vGPU after the first reports byte 0 replaced by a
// character that is no hex digit (docs/ABI.md "Identity of a split vGPU").
bool same_gpu(const std::string& a, const std::string& b) {
  if (a.size() != b.size() || a.empty()) return false;
  const bool a0 = isxdigit((unsigned char)a[0]), b0 = isxdigit((unsigned char)b[0]);
  return a.compare(1, std::string::npos, b, 1, std::string::npos) == 0 && (!(a0 && b0) || a[0] == b[0]);
}

Mapping map_device(const Run& r, int dev, const std::vector<std::string>& uuids) {
  Mapping m;
  int k = 0;  // this device is the k-th HIP device of its GPU
  m.vgpus_of_gpu = 0;
  for (int i = 0; i < (int)uuids.size(); i++)
    if (same_gpu(uuids[i], uuids[dev])) {
      if (i < dev) k++;
      m.vgpus_of_gpu++;
    }
  if (r.region) {
    std::vector<int> slots;
    for (int s = 0; s < 16; s++) {
      vgpu_device_info di;
      if (vgpu_region_device_info(r.region, s, &di) == 0 && di.configured &&
          same_gpu(vgpu_validate::norm_uuid(di.uuid), uuids[dev]))
        slots.push_back(s);
    }
    if (!slots.empty()) {
      m.compute_slot = slots[0];
      // split vGPUs: their quota slots follow the agents', in map order, under the GPU's UUID
      m.memory_slot = m.vgpus_of_gpu > 1 && k + 1 < (int)slots.size() ? slots[k + 1] : slots[0];
    }
  }
  // The promise: the k-th map entry naming this GPU (split), all of them summed (merged), or
  // the device's own position when there is no map.
  m.limit_index = dev;
  uint64_t sum = 0;
  int entries = 0, seen = 0;
  const auto map = parse_map(r.promise.get("VGPU_DEVICE_MAP"));
  for (const auto& e : map) {
    if (!same_gpu(e.second, uuids[dev])) continue;
    entries++;
    const char* v = r.promise.indexed("VGPU_DEVICE_MEMORY_LIMIT", e.first);
    const int64_t b = v ? vgpu_parse_size(v) : -1;
    if (b > 0) sum += (uint64_t)b;
    if (seen++ == k) m.limit_index = e.first;
  }
  if (entries > 1 && m.vgpus_of_gpu == 1) {
    m.promised_mem = sum;
    m.has_promised_mem = sum > 0;
  } else {
    const char* v = r.promise.indexed("VGPU_DEVICE_MEMORY_LIMIT", m.limit_index);
    const int64_t b = v ? vgpu_parse_size(v) : -1;
    m.promised_mem = b > 0 ? (uint64_t)b : 0;
    m.has_promised_mem = b > 0;
  }
  return m;
}

const char* mode_name(int m) {
  switch (m) {
    case 1: return "spatial";
    case 2: return "temporal";
    case 3: return "both";
    default: return "off";
  }
}

void check_quota(Run& r, DeviceReport& rep, int dev, const Mapping& m) {
  size_t free_b = 0, total = 0, total2 = 0;
  vgpu_device_info di{};
  const bool ok = r.hip.MemGetInfo(&free_b, &total) == hipSuccess && r.hip.DeviceTotalMem(&total2, dev) == hipSuccess &&
                  r.device_info(m.memory_slot, &di);
  bool pass = ok && total == total2 && total == di.mem_limit && di.mem_limit != 0;
  if (m.has_promised_mem && total != m.promised_mem) pass = false;
  Check& c = rep.add("quota", pass ? "pass" : "fail");
  c.num("total", total).num("device_total", total2).num("region_limit", di.mem_limit).num("free", free_b);
  if (m.has_promised_mem) c.num("promised", m.promised_mem);
  else c.null("promised");
}

void check_oom(Run& r, DeviceReport& rep) {
  size_t free_b = 0, total = 0;
  (void)r.hip.MemGetInfo(&free_b, &total);
  void* p = nullptr;
  const hipError_t e = total ? r.hip.Malloc(&p, total) : hipErrorInvalidValue;
  const bool refused = e != hipSuccess || !p;
  if (!refused) (void)r.hip.Free(p);  // never touched
  rep.add("oom", total && refused ? "pass" : "fail").num("asked", total).num("error", (uint64_t)e);
}

void check_cus(Run& r, DeviceReport& rep, int dev, const Mapping& m, hipStream_t s) {
  constexpr int kBlocks = 8192, kSpinUs = 300;
  int reported = 0;
  (void)r.hip.DeviceGetAttribute(&reported, hipDeviceAttributeMultiprocessorCount, dev);
  uint32_t* out = nullptr;
  if (r.hip.HostMalloc((void**)&out, kBlocks * sizeof(uint32_t), 0) != hipSuccess || !out) {
    rep.add("cus", "fail").str("reason", "no pinned host memory for the census");
    return;
  }
  memset(out, 0xff, kBlocks * sizeof(uint32_t));
  uint64_t ticks = (uint64_t)kSpinUs * 100;
  void* args[] = {&out, &ticks};
  const bool ran = r.launch(r.f_census, kBlocks, 64, s, args) && r.hip.StreamSynchronize(s) == hipSuccess;
  std::set<uint32_t> distinct;
  for (int i = 0; ran && i < kBlocks; i++)
    if (out[i] != 0xffffffffu) distinct.insert(out[i]);
  (void)r.hip.HostFree(out);
  vgpu_device_info di{};
  r.device_info(m.compute_slot, &di);
  // The promised slice: the CU range's width, else the share of the GPU's CUs.
  int width = -1;
  if (m.vgpus_of_gpu == 1) {
    int b = -1, e = -1;
    const char* range = r.promise.get("VGPU_DEVICE_CU_RANGE_" + std::to_string(m.limit_index));
    const char* pct = r.promise.indexed("VGPU_DEVICE_CU_LIMIT", m.limit_index);
    if (range && vgpu::parse_range(range, &b, &e) && e > b) width = e - b;
    else if (!range && pct && atoi(pct) > 0 && atoi(pct) < 100 && di.cu_count > 0)
      width = vgpu_cu_share_count(di.cu_count, di.num_xcc > 0 ? di.num_xcc : 1, atoi(pct));
  }
  const bool enforced = di.cu_mode == 1 || di.cu_mode == 3;
  const char* status = "info";
  if (!ran) status = "fail";
  else if (enforced)
    status = (int)distinct.size() == reported && (width < 0 || (int)distinct.size() == width) ? "pass" : "fail";
  Check& c = rep.add("cus", status);
  c.num("census", distinct.size()).num("reported", (uint64_t)(reported > 0 ? reported : 0)).str("mode", mode_name(di.cu_mode));
  if (width >= 0) c.num("promised", (uint64_t)width);
  else c.null("promised");
  c.num("mask", (uint64_t)(di.cu_mask_count > 0 ? di.cu_mask_count : 0));
  c.fields.emplace_back("crowd", std::to_string(di.crowd));
}

void check_gate(Run& r, DeviceReport& rep, void* scratch, hipStream_t s) {
  constexpr int kLaunches = 32;
  bool ok = true;
  for (int i = 0; i < kLaunches && ok; i++) ok = r.fill(scratch, 4096, 0, 1u + i, s);
  ok = ok && r.hip.StreamSynchronize(s) == hipSuccess;
  // The shim publishes a process's launch counter once per maintenance period.
  vgpu_proc_info me{};
  const double deadline = now_s() + (2 * r.period_ms + 100) / 1000.0;
  bool found = false;
  do {
    found = r.self(&me);
    if (found && me.launches >= r.launched) break;
    sleep_ms(10);
  } while (now_s() < deadline);
  rep.add("gate", ok && found && me.launches >= r.launched ? "pass" : "fail")
      .num("launched", r.launched)
      .num("counted", found ? me.launches : 0);
}

// K distinct word indices spread over n_words.
bool poke(Run& r, void* buf, uint64_t n_words, int k, hipStream_t s) {
  unsigned long long* idx = nullptr;
  if (r.hip.HostMalloc((void**)&idx, (size_t)k * sizeof(*idx), 0) != hipSuccess || !idx) return false;
  const uint64_t step = n_words / (uint64_t)k;
  for (int j = 0; j < k; j++) idx[j] = (uint64_t)j * step + (j == k - 1 ? step - 1 : (uint64_t)j % step);
  uint32_t n = (uint32_t)k;
  void* args[] = {&buf, &idx, &n};
  const bool ok = r.launch(r.f_poke, (n + 63) / 64, 64, s, args) && r.hip.StreamSynchronize(s) == hipSuccess;
  (void)r.hip.HostFree(idx);
  return ok;
}

void check_memory(Run& r, DeviceReport& rep, uint64_t* res, hipStream_t s) {
  const uint64_t bytes = r.opt.bytes;
  void* buf = nullptr;
  if (r.hip.Malloc(&buf, bytes) != hipSuccess || !buf) {
    rep.add("memory", "fail").str("reason", "allocation refused").num("bytes", bytes);
    return;
  }
  const uint32_t seed = 0x5eed0000u ^ (uint32_t)getpid();
  double t0 = now_s();
  bool ok = r.fill(buf, bytes, 0, seed, s) && r.hip.StreamSynchronize(s) == hipSuccess;
  const double t_fill = now_s() - t0;
  if (ok && r.opt.inject > 0) ok = poke(r, buf, bytes / 4, r.opt.inject, s);
  t0 = now_s();
  ok = ok && r.check(buf, bytes, 0, seed, res, s);
  const double t_check = now_s() - t0;
  (void)r.hip.Free(buf);
  Check& c = rep.add("memory", ok && res[0] == 0 ? "pass" : "fail");
  c.num("bytes", bytes).num("mismatches", ok ? res[0] : 0);
  if (ok && res[0]) c.num("first_index", res[1]);
  else c.null("first_index");
  if (!ok) c.str("reason", "a kernel launch or wait failed");
  c.real("fill_gbps", t_fill > 0 ? bytes / t_fill / 1e9 : 0).real("check_gbps", t_check > 0 ? bytes / t_check / 1e9 : 0);
  if (r.opt.inject > 0) c.num("injected", (uint64_t)r.opt.inject);
}

// Does the slice compute? Every wave of 2048 four-wave workgroups runs the known-answer test
// of vgpu/selftest.h (VALU, LDS, i8 and f16 MFMA) and records the CU and SIMD it ran on; the
// waves hold their CU afterwards like the census's, so the grid covers the slice. Every
// wave's four words must equal the host definition's, and under an enforced CU mask the CUs
// covered must be the ones reported, as in `cus`.
void check_compute(Run& r, DeviceReport& rep, int dev, const Mapping& m, hipStream_t s) {
  constexpr uint32_t kBlocks = 2048, kWaves = 4 * kBlocks, kRecord = 8, kRounds = 64, kHoldUs = 300, kMaxListed = 16;
  static const char* const units[4] = {"valu", "lds", "mfma_i8", "mfma_f16"};
  int reported = 0;
  (void)r.hip.DeviceGetAttribute(&reported, hipDeviceAttributeMultiprocessorCount, dev);
  uint32_t* out = nullptr;
  uint32_t* bad = nullptr;
  if (r.hip.HostMalloc((void**)&out, kWaves * kRecord * sizeof(uint32_t), 0) != hipSuccess || !out ||
      r.hip.HostMalloc((void**)&bad, VGPU_SELFTEST_MAX_BAD * sizeof(uint32_t), 0) != hipSuccess || !bad) {
    if (out) (void)r.hip.HostFree(out);
    rep.add("compute", "fail").str("reason", "no pinned host memory for the known-answer test");
    return;
  }
  memset(out, 0xff, kWaves * kRecord * sizeof(uint32_t));
  // --inject-compute K: K distinct workgroups spread over the grid, the first and the last among them
  uint32_t n_bad = (uint32_t)r.opt.inject_compute;
  for (uint32_t j = 0; j < n_bad; j++) bad[j] = j && j + 1 == n_bad ? kBlocks - 1 : j * (kBlocks / n_bad);
  uint32_t seed = 0xc0de0000u ^ (uint32_t)getpid(), rounds = kRounds;
  uint64_t ticks = (uint64_t)kHoldUs * 100;
  uint32_t want[4];
  vgpu_selftest_expected(seed, rounds, 0, want);
  void* args[] = {&out, &seed, &rounds, &ticks, &bad, &n_bad};
  const double t0 = now_s();
  const bool ran = r.launch(r.f_selftest, kBlocks, 256, s, args) && r.hip.StreamSynchronize(s) == hipSuccess;
  const double ms = (now_s() - t0) * 1e3;
  std::set<uint32_t> cus, pairs, bad_cus;
  uint64_t waves = 0, bad_waves = 0;
  std::string listed;
  for (uint32_t w = 0; ran && w < kWaves; w++) {
    const uint32_t* rec = out + (size_t)w * kRecord;
    const bool wrote = rec[0] != 0xffffffffu;
    if (wrote) {
      waves++;
      cus.insert(rec[0] & 0xffffu);
      pairs.insert(rec[0]);
    }
    std::string which;
    for (int u = 0; u < 4; u++)
      if (rec[1 + u] != want[u]) which += std::string(which.empty() ? "" : ",") + "\"" + units[u] + "\"";
    if (which.empty()) continue;
    bad_waves++;
    if (wrote) bad_cus.insert(rec[0] & 0xffffu);
    if (bad_waves > kMaxListed) continue;
    char loc[64] = "none";
    if (wrote)
      snprintf(loc, sizeof(loc), "%u/%u/%u/%u/%u", (rec[0] >> 12) & 0xf, (rec[0] >> 8) & 0xf, (rec[0] >> 4) & 0xf,
               rec[0] & 0xf, (rec[0] >> 16) & 0x3);
    listed += std::string(listed.empty() ? "" : ",") + "{\"location\":\"" + loc + "\",\"units\":[" + which + "]}";
  }
  (void)r.hip.HostFree(bad);
  (void)r.hip.HostFree(out);
  vgpu_device_info di{};
  r.device_info(m.compute_slot, &di);
  const bool enforced = di.cu_mode == 1 || di.cu_mode == 3;
  const bool pass = ran && waves == kWaves && bad_waves == 0 && (!enforced || (int)cus.size() == reported);
  Check& c = rep.add("compute", pass ? "pass" : "fail");
  c.num("waves", waves).num("cus", cus.size()).num("reported", (uint64_t)(reported > 0 ? reported : 0));
  c.num("simd_pairs", pairs.size()).num("rounds", rounds).num("bad_waves", bad_waves).str("mode", mode_name(di.cu_mode));
  c.real("ms", ms);
  if (!ran) c.str("reason", "a kernel launch or wait failed");
  if (bad_waves) c.raw("bad", "[" + listed + "]").num("bad_cus", bad_cus.size());
  if (n_bad) c.num("injected", n_bad);
}

// Virtual device memory: a buffer that the shim placed in host memory holds the pattern,
// and still holds it after the shim promoted it into HBM at the same address.
void check_spill(Run& r, DeviceReport& rep, const Mapping& m, uint64_t* res, hipStream_t s) {
  vgpu_device_info di{};
  r.device_info(m.memory_slot, &di);
  if (!r.promise.truthy("VGPU_OVERSUBSCRIBE") || !di.hbm_limit || di.mem_limit <= di.hbm_limit) {
    rep.add("spill", "skip").str("reason", "no virtual device memory promised (quota within the HBM share)");
    return;
  }
  const uint64_t bytes = r.opt.bytes, chunk = 128ull << 20;
  std::vector<void*> ballast;
  void* buf = nullptr;
  uint64_t before = 0;
  // Untouched ballast fills the HBM share until the test buffer lands in host memory.
  for (int i = 0; i < 1024; i++) {
    r.device_info(m.memory_slot, &di);
    before = di.spilled;
    if (r.hip.Malloc(&buf, bytes) != hipSuccess) buf = nullptr;
    if (!buf) break;
    r.device_info(m.memory_slot, &di);
    if (di.spilled >= before + bytes) break;
    (void)r.hip.Free(buf);
    buf = nullptr;
    if (di.used + chunk + bytes > di.mem_limit) break;
    void* b = nullptr;
    if (r.hip.Malloc(&b, chunk) != hipSuccess || !b) break;
    ballast.push_back(b);
  }
  auto release = [&] {
    for (void* b : ballast) (void)r.hip.Free(b);
    ballast.clear();
  };
  if (!buf) {
    release();
    rep.add("spill", "skip").str("reason", "the test buffer never spilled").num("ballast", ballast.size() * chunk);
    return;
  }
  const uint64_t held = ballast.size() * chunk;
  const uint32_t seed = 0x51110000u ^ (uint32_t)getpid();
  bool ok = r.fill(buf, bytes, 0, seed, s) && r.check(buf, bytes, 0, seed, res, s);
  const uint64_t bad_spilled = res[0];
  release();
  // Promotion: checked by the shim every period and on every free; bounded wait.
  bool promoted = false;
  const double deadline = now_s() + 5.0 + 20 * r.period_ms / 1000.0;
  while (ok && !bad_spilled && now_s() < deadline) {
    r.device_info(m.memory_slot, &di);
    if (di.spilled <= before) {
      promoted = true;
      break;
    }
    sleep_ms(20);
  }
  uint64_t bad_promoted = 0;
  if (ok && promoted) {
    ok = r.check(buf, bytes, 0, seed, res, s);
    bad_promoted = res[0];
  }
  (void)r.hip.Free(buf);
  const char* status = !ok || bad_spilled || bad_promoted ? "fail" : promoted ? "pass" : "skip";
  Check& c = rep.add("spill", status);
  c.num("bytes", bytes).num("ballast", held).num("mismatches_spilled", bad_spilled).num("mismatches_promoted", bad_promoted);
  if (!ok) c.str("reason", "a kernel launch or wait failed");
  else if (!promoted && !bad_spilled) c.str("reason", "the buffer was not promoted within the bound");
}

void skip_rest(DeviceReport& rep, const vgpu_validate::Options& opt, const char* why) {
  for (const char* n : {"quota", "oom", "cus", "gate", "memory"}) rep.add(n, "skip").str("reason", why);
  if (opt.compute) rep.add("compute", "skip").str("reason", why);
  if (opt.spill) rep.add("spill", "skip").str("reason", why);
}

void run_device(Run& r, DeviceReport& rep, int dev, const std::vector<std::string>& uuids) {
  const Mapping m = map_device(r, dev, uuids);
  vgpu_device_info di{};
  vgpu_proc_info me{};
  const char* why = nullptr;
  if (!r.region) why = "no region (VGPU_SHARED_CACHE)";
  else if (!r.device_info(m.memory_slot, &di) || !di.configured) why = "the device is not configured in the region";
  else if (!r.self(&me)) why = "this process has no slot in the region";
  if (why) {
    rep.add("shim", "fail").str("reason", why);
    skip_rest(rep, r.opt, "the shim is not in effect");
    return;
  }
  rep.add("shim", "pass").num("slot", (uint64_t)m.memory_slot).num("pid", (uint64_t)me.pid);
  // Modules belong to the device that was current when they were loaded.
  if (r.hip.ModuleLoadData(&r.module, vgpu_validate_co) != hipSuccess ||
      r.hip.ModuleGetFunction(&r.f_census, r.module, "census") != hipSuccess ||
      r.hip.ModuleGetFunction(&r.f_fill, r.module, "pattern_fill") != hipSuccess ||
      r.hip.ModuleGetFunction(&r.f_check, r.module, "pattern_check") != hipSuccess ||
      r.hip.ModuleGetFunction(&r.f_poke, r.module, "pattern_poke") != hipSuccess ||
      r.hip.ModuleGetFunction(&r.f_selftest, r.module, "cu_selftest") != hipSuccess) {
    rep.add("runtime", "fail").str("reason", "the embedded gfx950 code object does not load on this GPU");
    skip_rest(rep, r.opt, "no kernels");
    return;
  }
  hipStream_t s = nullptr;
  uint64_t* res = nullptr;
  void* scratch = nullptr;
  if (r.hip.StreamCreate(&s) != hipSuccess || r.hip.HostMalloc((void**)&res, 2 * sizeof(uint64_t), 0) != hipSuccess ||
      r.hip.Malloc(&scratch, 4096) != hipSuccess) {
    skip_rest(rep, r.opt, "no stream or result buffer");
    rep.checks[0].status = "fail";
    return;
  }
  check_quota(r, rep, dev, m);
  check_oom(r, rep);
  check_cus(r, rep, dev, m, s);
  check_gate(r, rep, scratch, s);
  check_memory(r, rep, res, s);
  if (r.opt.compute) check_compute(r, rep, dev, m, s);
  if (r.opt.spill) check_spill(r, rep, m, res, s);
  (void)r.hip.Free(scratch);
  (void)r.hip.HostFree(res);
  (void)r.hip.StreamDestroy(s);
  (void)r.hip.ModuleUnload(r.module);
  r.module = nullptr;
}

void print(const std::vector<DeviceReport>& reps, bool ok, bool json, const std::string& runtime_error) {
  if (json) {
    printf("{\"version\":1,\"ok\":%s,", ok ? "true" : "false");
    if (!runtime_error.empty()) {
      Check c;
      c.str("reason", runtime_error);
      printf("\"runtime\":{\"status\":\"fail\",\"reason\":%s},", c.fields[0].second.c_str());
    }
    printf("\"devices\":[");
    for (size_t i = 0; i < reps.size(); i++) {
      printf("%s{\"device\":%d,\"uuid\":\"%s\",\"checks\":{", i ? "," : "", reps[i].device, reps[i].uuid.c_str());
      for (size_t j = 0; j < reps[i].checks.size(); j++) {
        const Check& c = reps[i].checks[j];
        printf("%s\"%s\":{\"status\":\"%s\"", j ? "," : "", c.name.c_str(), c.status.c_str());
        for (const auto& f : c.fields) printf(",\"%s\":%s", f.first.c_str(), f.second.c_str());
        printf("}");
      }
      printf("}}");
    }
    printf("]}\n");
    return;
  }
  if (!runtime_error.empty()) printf("runtime FAIL %s\n", runtime_error.c_str());
  for (const DeviceReport& d : reps)
    for (const Check& c : d.checks) {
      printf("device %d %s %s %s", d.device, d.uuid.c_str(), c.name.c_str(), c.status.c_str());
      for (const auto& f : c.fields) printf(" %s=%s", f.first.c_str(), f.second.c_str());
      printf("\n");
    }
}

}  // namespace

namespace vgpu_validate {

int conformance(const Options& opt) {
  Run r;
  r.opt = opt;
  r.promise.load(opt.limits);
  if (const char* p = r.promise.get("VGPU_UTIL_PERIOD_MS"))
    if (atoi(p) > 0) r.period_ms = atoi(p);
  std::vector<DeviceReport> reps;
  std::string err;
  int n = 0;
  if (!load_hip(&r.hip, &err)) {
  } else if (r.hip.Init(0) != hipSuccess || r.hip.GetDeviceCount(&n) != hipSuccess || n <= 0) {
    err = "no GPU visible to the HIP runtime";
  } else if (opt.device >= n) {
    err = "no HIP device " + std::to_string(opt.device);
  }
  if (!err.empty()) {
    print(reps, false, opt.json, err);
    return 1;
  }
  std::vector<std::string> uuids(n);
  for (int d = 0; d < n; d++) {
    hipUUID u{};
    if (r.hip.DeviceGetUuid(&u, d) == hipSuccess) uuids[d] = norm_uuid(std::string(u.bytes, strnlen(u.bytes, 16)));
  }
  if (const char* path = r.promise.get("VGPU_SHARED_CACHE")) {
    int e = 0;
    r.region = vgpu_region_open(path, 0, &e);
  }
  bool ok = true;
  for (int d = 0; d < n; d++) {
    if (opt.device >= 0 && d != opt.device) continue;
    DeviceReport rep;
    rep.device = d;
    rep.uuid = "GPU-" + uuids[d];
    if (r.hip.SetDevice(d) != hipSuccess) {
      rep.add("shim", "fail").str("reason", "hipSetDevice failed");
      skip_rest(rep, opt, "the device cannot be selected");
    } else {
      run_device(r, rep, d, uuids);
    }
    for (const Check& c : rep.checks) ok = ok && c.status != "fail";
    reps.push_back(rep);
  }
  if (r.region) vgpu_region_close(r.region);
  print(reps, ok, opt.json, "");
  return ok ? 0 : 1;
}

}  // namespace vgpu_validate
