// Driver for the CPU-only tests of split vGPUs' device identity (tests/test_vdev_identity.py):
// a multi-threaded "HIP application" linked against the fake HIP/ROCr and run with
// libvgpu_hip.so preloaded, like shim_harness. It executes the script on its command line, one
// JSON object per step. A step runs on host thread T0 unless prefixed "t1:" (or "t2:" ...):
// each thread keeps its own current device, as an application's threads do, and the steps
// still run one after the other.
//
//   dev=N             hipSetDevice(N)
//   count             hipGetDeviceCount / hipGetDevice -> {"count", "current"}
//   ids=D             who device D is: {"bus": hipDeviceGetPCIBusId, "uuid": its 16 bytes in hex,
//                     "prop": [pciDomainID, pciBusID, pciDeviceID] and "prop_uuid" of the
//                     properties, "attr": the same three as hipDeviceAttributePci*, "rc": [..]}
//   shortbus=D,LEN    hipDeviceGetPCIBusId into LEN bytes -> {"shortbus": rc}
//   bybus=ID          hipDeviceGetByPCIBusId -> {"bybus": device, "rc"}
//   meminfo           hipMemGetInfo -> {"free", "total"}
//   malloc=SIZE       hipMalloc -> {"malloc": "ok"|"oom", "idx", "addr"}; free=I frees the I-th
//   ptrdev=I,OFF      the device of pointer I + OFF by hipPointerGetAttributes, hipPointerGetAttribute
//                     and hipDrvPointerGetAttributes -> {"ptrdev": [a, b, c], "rc": [..]}
//   stream=KIND       a stream on the current device (create | flags | priority | cumask) -> {"stream": idx}
//   streamdev=I       hipStreamGetDevice of stream I (-1 the null stream)
//   sdestroy=I        hipStreamDestroy
//   amalloc=SIZE,S    hipMallocAsync on stream S -> {"amalloc": "ok"|"oom"|rc, "idx"}; pmalloc the same
//                     with hipMallocFromPoolAsync (the stream's device's default pool)
//   afree=I,S         hipFreeAsync of pointer I on stream S
//   ctxdev            hipCtxGetDevice -> {"ctxdev", "rc"}
//   advise=D / prefetch=D  hipMemAdvise_v2 / hipMemPrefetchAsync_v2 with Device location D ->
//                     {"advise": rc, "runtime_id": the device id the runtime got}
//   p2p=A,B           hipDeviceGetP2PAttribute -> {"p2p": [access, atomics, rank], "rc": [..]}
//   rccl=D            the fake librccl's view of device D -> {"rccl": rc, "bus", "uuid0", "bybus", "domain"}
//   ptrgates=I        each pointer entry point called on pointer I while the container is suspended
//                     (resumed after 40 ms by another thread) -> {"ptrgates": 3, "unrouted",
//                     "ungated", "unreached"} as the gates= step of shim_harness
#define __HIP_PLATFORM_AMD__ 1
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

extern "C" {
const char* fake_hip_last_call();
int fake_hip_last_location();
int fake_librccl_probe(int device, char* bus_id, int len, hipUUID* uuid, int* by_bus_id, int* domain);
}

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

long long parse_size(const char* s) {
  char* end = nullptr;
  long long v = strtoll(s, &end, 10);
  switch (end && *end ? *end : 0) {
    case 'k': case 'K': v <<= 10; break;
    case 'm': case 'M': v <<= 20; break;
    case 'g': case 'G': v <<= 30; break;
    default: break;
  }
  return v;
}

// A host thread that runs the steps given to it, one at a time.
class Worker {
 public:
  Worker() : th_([this] { loop(); }) {}
  ~Worker() {
    run(nullptr);
    th_.join();
  }
  void run(std::function<void()> f) {
    std::unique_lock<std::mutex> l(mu_);
    job_ = std::move(f);
    have_ = true;
    cv_.notify_all();
    if (!job_) return;
    cv_.wait(l, [&] { return !have_; });
  }

 private:
  void loop() {
    for (;;) {
      std::unique_lock<std::mutex> l(mu_);
      cv_.wait(l, [&] { return have_; });
      if (!job_) return;
      std::function<void()> f = job_;
      l.unlock();
      f();
      l.lock();
      have_ = false;
      cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::function<void()> job_;
  bool have_ = false;
  std::thread th_;
};

std::vector<void*> g_ptrs;
std::vector<hipStream_t> g_streams;

hipStream_t stream_at(int i) {
  return i >= 0 && i < (int)g_streams.size() ? g_streams[i] : nullptr;
}

void print_list(const char* key, const std::vector<std::string>& v, bool last) {
  printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); i++) printf("%s\"%s\"", i ? ", " : "", v[i].c_str());
  printf("]%s", last ? "" : ", ");
}

void ptr_gates(void* ptr) {
  using Ctl = int (*)();
  auto suspend = reinterpret_cast<Ctl>(dlsym(RTLD_DEFAULT, "vgpu_suspend_all"));
  auto resume = reinterpret_cast<Ctl>(dlsym(RTLD_DEFAULT, "vgpu_resume_all"));
  void* h = dlopen("libamdhip64.so", RTLD_NOLOAD | RTLD_LAZY);
  const char* names[3] = {"hipPointerGetAttributes", "hipPointerGetAttribute", "hipDrvPointerGetAttributes"};
  std::vector<std::string> unrouted, ungated, unreached;
  for (int i = 0; i < 3; i++) {
    // the linked call must be the shim's (not the runtime's own definition), like a lookup on the library
    void* linked = dlsym(RTLD_DEFAULT, names[i]);
    void* looked_up = h ? dlsym(h, names[i]) : nullptr;
    Dl_info a, b;
    if (!linked || !looked_up || linked != looked_up || !dladdr(linked, &a) || !dladdr((void*)&fake_hip_last_call, &b) ||
        a.dli_fbase == b.dli_fbase)
      unrouted.push_back(names[i]);
    if (!suspend || !resume || suspend() != 0) {
      ungated.push_back(names[i]);
      continue;
    }
    std::thread t([&] {
      std::this_thread::sleep_for(std::chrono::milliseconds(40));
      resume();
    });
    const double t0 = now_s();
    int dev = -1;
    hipPointerAttribute_t at;
    hipPointer_attribute which = HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL;
    void* data = &dev;
    hipError_t e = i == 0   ? hipPointerGetAttributes(&at, ptr)
                   : i == 1 ? hipPointerGetAttribute(&dev, which, ptr)
                            : hipDrvPointerGetAttributes(1, &which, &data, ptr);
    const double dt = now_s() - t0;
    t.join();
    if (dt < 0.030) ungated.push_back(names[i]);
    if (e != hipSuccess || std::string(names[i]) != fake_hip_last_call()) unreached.push_back(names[i]);
  }
  printf("{\"ptrgates\": 3, ");
  print_list("unrouted", unrouted, false);
  print_list("ungated", ungated, false);
  print_list("unreached", unreached, true);
  printf("}\n");
}

int step(const std::string& key, const std::string& val) {
  const int a = atoi(val.c_str());
  const int b = val.find(',') == std::string::npos ? 0 : atoi(val.substr(val.find(',') + 1).c_str());
  if (key == "dev") {
    printf("{\"dev\": %d, \"rc\": %d}\n", a, (int)hipSetDevice(a));
  } else if (key == "count") {
    int n = -1, cur = -1;
    hipError_t e = hipGetDeviceCount(&n);
    (void)hipGetDevice(&cur);
    printf("{\"count\": %d, \"rc\": %d, \"current\": %d}\n", n, (int)e, cur);
  } else if (key == "ids") {
    char bus[64] = {0};
    hipUUID u;
    memset(&u, 0, sizeof(u));
    hipDeviceProp_t p;
    memset(&p, 0, sizeof(p));
    int at[3] = {-1, -1, -1};
    const int rc[6] = {(int)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), a), (int)hipDeviceGetUuid(&u, a),
                       (int)hipGetDeviceProperties(&p, a),
                       (int)hipDeviceGetAttribute(&at[0], hipDeviceAttributePciDomainId, a),
                       (int)hipDeviceGetAttribute(&at[1], hipDeviceAttributePciBusId, a),
                       (int)hipDeviceGetAttribute(&at[2], hipDeviceAttributePciDeviceId, a)};
    char hex[33], phex[33];
    for (int i = 0; i < 16; i++) {
      snprintf(hex + 2 * i, 3, "%02x", (unsigned char)u.bytes[i]);
      snprintf(phex + 2 * i, 3, "%02x", (unsigned char)p.uuid.bytes[i]);
    }
    printf("{\"ids\": %d, \"bus\": \"%s\", \"uuid\": \"%s\", \"prop\": [%d, %d, %d], \"prop_uuid\": \"%s\", "
           "\"attr\": [%d, %d, %d], \"rc\": [%d, %d, %d, %d, %d, %d]}\n",
           a, bus, hex, p.pciDomainID, p.pciBusID, p.pciDeviceID, phex, at[0], at[1], at[2], rc[0], rc[1], rc[2], rc[3],
           rc[4], rc[5]);
  } else if (key == "shortbus") {
    char bus[64] = {0};
    printf("{\"shortbus\": %d}\n", (int)hipDeviceGetPCIBusId(bus, b < (int)sizeof(bus) ? b : (int)sizeof(bus), a));
  } else if (key == "bybus") {
    int d = -1;
    hipError_t e = hipDeviceGetByPCIBusId(&d, val.c_str());
    printf("{\"bybus\": %d, \"rc\": %d}\n", d, (int)e);
  } else if (key == "meminfo") {
    size_t f = 0, t = 0;
    (void)hipMemGetInfo(&f, &t);
    printf("{\"free\": %zu, \"total\": %zu}\n", f, t);
  } else if (key == "malloc") {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)parse_size(val.c_str()));
    g_ptrs.push_back(e == hipSuccess ? p : nullptr);
    printf("{\"malloc\": \"%s\", \"idx\": %zu, \"addr\": %llu}\n", e == hipSuccess ? "ok" : "oom", g_ptrs.size() - 1,
           (unsigned long long)reinterpret_cast<uintptr_t>(p));
  } else if (key == "free") {
    int rc = -1;
    if (a >= 0 && a < (int)g_ptrs.size() && g_ptrs[a]) {
      rc = (int)hipFree(g_ptrs[a]);
      g_ptrs[a] = nullptr;
    }
    printf("{\"free\": %d, \"rc\": %d}\n", a, rc);
  } else if (key == "ptrdev") {
    const long long off = parse_size(val.substr(val.find(',') == std::string::npos ? val.size() : val.find(',') + 1).c_str());
    char* p = a >= 0 && a < (int)g_ptrs.size() ? static_cast<char*>(g_ptrs[a]) + off : nullptr;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    at.device = -1;
    int d1 = -1, d2 = -1;
    hipPointer_attribute which = HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL;
    void* data = &d2;
    const int rc[3] = {(int)hipPointerGetAttributes(&at, p), (int)hipPointerGetAttribute(&d1, which, p),
                       (int)hipDrvPointerGetAttributes(1, &which, &data, p)};
    printf("{\"ptrdev\": [%d, %d, %d], \"rc\": [%d, %d, %d]}\n", at.device, d1, d2, rc[0], rc[1], rc[2]);
  } else if (key == "stream") {
    hipStream_t s = nullptr;
    const uint32_t mask[2] = {0xffffffffu, 0xffffffffu};
    hipError_t e = val == "flags"      ? hipStreamCreateWithFlags(&s, hipStreamNonBlocking)
                   : val == "priority" ? hipStreamCreateWithPriority(&s, hipStreamDefault, 0)
                   : val == "cumask"   ? hipExtStreamCreateWithCUMask(&s, 2, mask)
                                       : hipStreamCreate(&s);
    g_streams.push_back(s);
    printf("{\"stream\": %zu, \"rc\": %d}\n", g_streams.size() - 1, (int)e);
  } else if (key == "streamdev") {
    int d = -1;
    hipError_t e = hipStreamGetDevice(stream_at(a), &d);
    printf("{\"streamdev\": %d, \"rc\": %d}\n", d, (int)e);
  } else if (key == "sdestroy") {
    int rc = -1;
    if (a >= 0 && a < (int)g_streams.size() && g_streams[a]) {
      rc = (int)hipStreamDestroy(g_streams[a]);
      g_streams[a] = nullptr;
    }
    printf("{\"sdestroy\": %d, \"rc\": %d}\n", a, rc);
  } else if (key == "amalloc" || key == "pmalloc") {
    void* p = nullptr;
    hipError_t e;
    if (key == "amalloc") {
      e = hipMallocAsync(&p, (size_t)parse_size(val.c_str()), stream_at(b));
    } else {
      int d = 0;
      hipMemPool_t pool = nullptr;
      (void)hipStreamGetDevice(stream_at(b), &d);
      (void)hipDeviceGetDefaultMemPool(&pool, d);
      e = hipMallocFromPoolAsync(&p, (size_t)parse_size(val.c_str()), pool, stream_at(b));
    }
    g_ptrs.push_back(e == hipSuccess ? p : nullptr);
    printf("{\"%s\": \"%s\", \"rc\": %d, \"idx\": %zu}\n", key.c_str(),
           e == hipSuccess ? "ok" : e == hipErrorOutOfMemory ? "oom" : "error", (int)e, g_ptrs.size() - 1);
  } else if (key == "afree") {
    int rc = -1;
    if (a >= 0 && a < (int)g_ptrs.size() && g_ptrs[a]) {
      rc = (int)hipFreeAsync(g_ptrs[a], stream_at(b));
      g_ptrs[a] = nullptr;
    }
    printf("{\"afree\": %d, \"rc\": %d}\n", a, rc);
  } else if (key == "ctxdev") {
    int d = -1;
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wdeprecated-declarations"
    hipError_t e = hipCtxGetDevice(&d);
#pragma GCC diagnostic pop
    printf("{\"ctxdev\": %d, \"rc\": %d}\n", d, (int)e);
  } else if (key == "advise" || key == "prefetch") {
    static char* buf = static_cast<char*>(malloc(1 << 20));
    hipMemLocation loc;
    loc.type = hipMemLocationTypeDevice;
    loc.id = a;
    hipError_t e = key == "advise" ? hipMemAdvise_v2(buf, 1 << 20, hipMemAdviseSetPreferredLocation, loc)
                                   : hipMemPrefetchAsync_v2(buf, 1 << 20, loc, 0, nullptr);
    printf("{\"%s\": %d, \"runtime_id\": %d}\n", key.c_str(), (int)e, fake_hip_last_location());
  } else if (key == "p2p") {
    int v[3] = {-1, -1, -1};
    const int rc[3] = {(int)hipDeviceGetP2PAttribute(&v[0], hipDevP2PAttrAccessSupported, a, b),
                       (int)hipDeviceGetP2PAttribute(&v[1], hipDevP2PAttrNativeAtomicSupported, a, b),
                       (int)hipDeviceGetP2PAttribute(&v[2], hipDevP2PAttrPerformanceRank, a, b)};
    printf("{\"p2p\": [%d, %d, %d], \"rc\": [%d, %d, %d]}\n", v[0], v[1], v[2], rc[0], rc[1], rc[2]);
  } else if (key == "rccl") {
    char bus[64] = {0};
    hipUUID u;
    memset(&u, 0, sizeof(u));
    int by = -1, dom = -1;
    const int rc = fake_librccl_probe(a, bus, (int)sizeof(bus), &u, &by, &dom);
    printf("{\"rccl\": %d, \"bus\": \"%s\", \"uuid0\": %d, \"bybus\": %d, \"domain\": %d}\n", rc, bus,
           (int)(unsigned char)u.bytes[0], by, dom);
  } else if (key == "ptrgates") {
    ptr_gates(a >= 0 && a < (int)g_ptrs.size() ? g_ptrs[a] : nullptr);
  } else {
    fprintf(stderr, "unknown step %s\n", key.c_str());
    return 2;
  }
  fflush(stdout);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (hipInit(0) != hipSuccess) return 1;
  std::vector<std::unique_ptr<Worker>> workers;
  for (int i = 1; i < argc; i++) {
    std::string op(argv[i]);
    size_t t = 0;
    if (op.size() > 2 && op[0] == 't' && isdigit((unsigned char)op[1]) && op[2] == ':') {
      t = (size_t)(op[1] - '0');
      op = op.substr(3);
    }
    const std::string key = op.substr(0, op.find('='));
    const std::string val = op.find('=') == std::string::npos ? "" : op.substr(op.find('=') + 1);
    while (workers.size() <= t) workers.emplace_back(new Worker());
    int rc = 0;
    workers[t]->run([&] { rc = step(key, val); });
    if (rc) return rc;
  }
  return 0;
}
