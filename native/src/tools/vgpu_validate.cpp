// vgpu-validate: device-authorisation check for a vGPU container.
//
// Reference: vgpu/vgpuvalidator [validator.c:10-111] decrypts /vgpu/license and
// checks each visible device UUID against an authorised pool ("device %s
// authorized" / "uuid %s UNAUTHORIZED"); `--decode` dumps the list. The MI355X build
// keeps the authorisation capability and drops the commercial AES licensing: the
// plugin writes a plain allow-list of ROCr UUIDs (one per line) and this tool checks
// the GPUs ROCr exposes to the container against it. ROCr is loaded with dlopen so
// the tool has no build-time GPU dependency.
//
//   vgpu-validate [--allowlist FILE]   exit 0 iff every visible GPU is authorised
//   vgpu-validate --decode [FILE]      print the allow-list
//   vgpu-validate --list               print the visible GPU UUIDs
//   vgpu-validate --conformance [--json] [--device I] [--limits FILE] [--bytes N] [--spill] [--inject K]
//                 [--compute [--inject-compute K]]
//                                      check the vGPU's limits from inside the container
//                                      (validate_conformance.cpp): shim, quota, oom, cus, gate,
//                                      memory, compute, spill; exit 0 iff no check failed
//   vgpu-validate --pattern N SEED [BASE]  print N words of the memory test pattern (vgpu/pattern.h)
//   vgpu-validate --selftest-expected SEED ROUNDS [inject]
//                                      print the four words of the compute known-answer test (vgpu/selftest.h)
#include <dlfcn.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "vgpu/pattern.h"
#include "vgpu/region_api.h"
#include "vgpu/selftest.h"
#include "validate.h"

static std::string norm(std::string s) {
  while (!s.empty() && isspace((unsigned char)s.back())) s.pop_back();
  size_t i = 0;
  while (i < s.size() && isspace((unsigned char)s[i])) i++;
  s = s.substr(i);
  if (s.size() >= 4 && !strncasecmp(s.c_str(), "GPU-", 4)) s = s.substr(4);
  for (auto& c : s) c = (char)tolower((unsigned char)c);
  return s;
}

static bool read_allowlist(const char* path, std::vector<std::string>* out) {
  FILE* f = fopen(path, "r");
  if (!f) return false;
  char line[256];
  while (fgets(line, sizeof(line), f)) {
    std::string s = line;
    if (s.empty() || s[0] == '#') continue;
    s = norm(s);
    if (!s.empty()) out->push_back(s);
  }
  fclose(f);
  return true;
}

std::string vgpu_validate::norm_uuid(std::string s) { return norm(std::move(s)); }

using init_fn = hsa_status_t (*)();
using iter_fn = hsa_status_t (*)(hsa_status_t (*)(hsa_agent_t, void*), void*);
using info_fn = hsa_status_t (*)(hsa_agent_t, hsa_agent_info_t, void*);
static info_fn g_info;

static hsa_status_t agent_cb(hsa_agent_t a, void* data) {
  hsa_device_type_t t;
  if (g_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
  char uuid[64] = {0};
  g_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_UUID, uuid);
  static_cast<std::vector<std::string>*>(data)->push_back(uuid);
  return HSA_STATUS_SUCCESS;
}

static bool visible_gpus(std::vector<std::string>* out) {
  void* h = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) h = dlopen("/opt/rocm/lib/libhsa-runtime64.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    fprintf(stderr, "vgpu-validate: cannot load ROCr: %s\n", dlerror());
    return false;
  }
  auto init = (init_fn)dlsym(h, "hsa_init");
  auto iter = (iter_fn)dlsym(h, "hsa_iterate_agents");
  g_info = (info_fn)dlsym(h, "hsa_agent_get_info");
  if (!init || !iter || !g_info || init() != HSA_STATUS_SUCCESS) {
    fprintf(stderr, "vgpu-validate: ROCr initialisation failed\n");
    return false;
  }
  iter(agent_cb, out);
  return true;
}

static int usage() {
  fprintf(stderr,
          "usage: vgpu-validate [--allowlist FILE] | --decode [FILE] | --list\n"
          "       vgpu-validate --conformance [--json] [--device I] [--limits FILE] [--bytes N] [--spill] [--inject K]\n"
          "                     [--compute [--inject-compute K]]\n"
          "       vgpu-validate --pattern N SEED [BASE]\n"
          "       vgpu-validate --selftest-expected SEED ROUNDS [inject]\n");
  return 2;
}

static bool parse_u64(const char* s, uint64_t* out) {
  char* end = nullptr;
  if (!s || !isdigit((unsigned char)*s)) return false;
  *out = strtoull(s, &end, 0);
  return end && !*end;
}

// --pattern N SEED [BASE]: the host definition, one word per line (no GPU, no ROCm).
static int print_pattern(int argc, char** argv, int i) {
  uint64_t n = 0, seed = 0, base = 0;
  if (i + 2 >= argc || !parse_u64(argv[i + 1], &n) || !parse_u64(argv[i + 2], &seed) || seed > 0xffffffffull ||
      (i + 3 < argc && !parse_u64(argv[i + 3], &base)) || i + 4 < argc)
    return usage();
  for (uint64_t k = 0; k < n; k++) printf("%u\n", vgpu_pattern_word(base + k, (uint32_t)seed));
  return 0;
}

// --selftest-expected SEED ROUNDS [inject]: the host definition, one "unit word" line per unit
// (no GPU, no ROCm).
static int print_selftest(int argc, char** argv, int i) {
  static const char* const units[4] = {"valu", "lds", "mfma_i8", "mfma_f16"};
  uint64_t seed = 0, rounds = 0;
  uint32_t words[4];
  if (i + 2 >= argc || !parse_u64(argv[i + 1], &seed) || seed > 0xffffffffull || !parse_u64(argv[i + 2], &rounds) ||
      rounds > VGPU_SELFTEST_MAX_ROUNDS || (i + 3 < argc && strcmp(argv[i + 3], "inject")) || i + 4 < argc)
    return usage();
  if (vgpu_selftest_expected((uint32_t)seed, (uint32_t)rounds, i + 3 < argc, words) != 0) return usage();
  for (int u = 0; u < 4; u++) printf("%s %u\n", units[u], words[u]);
  return 0;
}

static int conformance_main(int argc, char** argv) {
  vgpu_validate::Options opt;
  for (int i = 1; i < argc; i++) {
    uint64_t v = 0;
    if (!strcmp(argv[i], "--conformance")) continue;
    if (!strcmp(argv[i], "--json")) opt.json = true;
    else if (!strcmp(argv[i], "--spill")) opt.spill = true;
    else if (!strcmp(argv[i], "--compute")) opt.compute = true;
    else if (!strcmp(argv[i], "--inject-compute") && i + 1 < argc && parse_u64(argv[i + 1], &v) && v >= 1 &&
             v <= VGPU_SELFTEST_MAX_BAD)
      opt.inject_compute = (int)v, i++;
    else if (!strcmp(argv[i], "--limits") && i + 1 < argc) opt.limits = argv[++i];
    else if (!strcmp(argv[i], "--device") && i + 1 < argc && parse_u64(argv[i + 1], &v) && v < 64) opt.device = (int)v, i++;
    else if (!strcmp(argv[i], "--inject") && i + 1 < argc && parse_u64(argv[i + 1], &v) && v >= 1 && v <= 4096)
      opt.inject = (int)v, i++;
    else if (!strcmp(argv[i], "--bytes") && i + 1 < argc) {
      const int64_t b = vgpu_parse_size(argv[++i]);
      if (b < 16 || (b & 15)) return usage();
      opt.bytes = (uint64_t)b;
    } else return usage();
  }
  if ((uint64_t)opt.inject * 8 > opt.bytes) return usage();  // the poked words are distinct
  if (opt.inject_compute && !opt.compute) return usage();
  return vgpu_validate::conformance(opt);
}

int main(int argc, char** argv) {
  const char* allow = "/vgpu/allowlist";
  bool decode = false, list = false;
  for (int i = 1; i < argc; i++)
    if (!strcmp(argv[i], "--conformance")) return conformance_main(argc, argv);
  if (argc > 1 && !strcmp(argv[1], "--pattern")) return print_pattern(argc, argv, 1);
  if (argc > 1 && !strcmp(argv[1], "--selftest-expected")) return print_selftest(argc, argv, 1);
  for (int i = 1; i < argc; i++) {
    if (!strcmp(argv[i], "--decode")) {
      decode = true;
      if (i + 1 < argc && argv[i + 1][0] != '-') allow = argv[++i];
    } else if (!strcmp(argv[i], "--allowlist") && i + 1 < argc) {
      allow = argv[++i];
    } else if (!strcmp(argv[i], "--list")) {
      list = true;
    } else {
      return usage();
    }
  }
  std::vector<std::string> allowed;
  if (decode) {
    if (!read_allowlist(allow, &allowed)) {
      fprintf(stderr, "vgpu-validate: cannot read %s\n", allow);
      return 1;
    }
    for (auto& a : allowed) printf("GPU-%s\n", a.c_str());
    return 0;
  }
  std::vector<std::string> gpus;
  if (!visible_gpus(&gpus)) return 1;
  if (list) {
    for (auto& g : gpus) printf("%s\n", g.c_str());
    return 0;
  }
  if (!read_allowlist(allow, &allowed)) {
    fprintf(stderr, "vgpu-validate: cannot read allow-list %s\n", allow);
    return 1;
  }
  std::set<std::string> ok(allowed.begin(), allowed.end());
  int bad = 0;
  for (auto& g : gpus) {
    if (ok.count(norm(g))) {
      printf("device %s authorized\n", g.c_str());
    } else {
      printf("uuid %s UNAUTHORIZED\n", g.c_str());
      bad++;
    }
  }
  return bad ? 1 : 0;
}
