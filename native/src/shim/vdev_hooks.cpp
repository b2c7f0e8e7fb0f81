// Split duplicate vGPUs: two vGPUs of one physical GPU as two HIP devices of the container.
//
// Reference: its shim keeps a container's duplicate vGPUs apart as separate virtual devices
// with virtual PCI bus ids (`assigning_virtual_pcibusID` [device.c:81-117], the device map
// [nvml/util.c:135-162], NVIDIA_DEVICE_MAP server.go:490,493) and disables cooperative launch
// on them [device.c:130-134]. ROCm enumerates one device per GPU agent, so with the plugin's
// default --duplicate-vgpus=split (VGPU_DUPLICATE_SPLIT=1) the shim presents them as separate
// devices at the HIP layer (=merge: one device, summed quota and CU share; docs/ABI.md
// "Duplicate vGPUs"):
//
//   * hipGetDeviceCount counts every vGPU; virtual device v is backed by physical device
//     phys(v) (the vGPUs of one GPU are consecutive, in VGPU_DEVICE_MAP order);
//   * hipSetDevice(v) selects phys(v) and remembers v for the thread (hipGetDevice returns
//     it), so torch.cuda.set_device(1), a cuda:1 tensor or one rank per visible device work;
//   * every entry point that takes a device ordinal maps it (hip_gates.def `device` rows for
//     the generic ones, the hooks below for those that return or virtualise something);
//   * each virtual device has its own quota: a region slot after the agents' (which keep the
//     summed quota as the physical guard), charged by the HSA allocation hook for the calling
//     thread's virtual device (hsa_hooks.cpp), reported by hipMemGetInfo / hipDeviceTotalMem /
//     the device properties;
//   * peer access between two virtual devices of one GPU is the same memory: reported
//     possible and enabled without a runtime call; cooperative launch stays as the runtime
//     reports it (one GPU).
//   * with VGPU_VIRTUAL_PCI_IDS (the plugin's --virtual-pci-ids, on by default) the k-th vGPU of
//     a GPU (k >= 1) has an identity of its own: PCI domain real + 0x1000 * k (same bus, device
//     and function) in hipDeviceGetPCIBusId, the device properties and the Pci* attributes,
//     accepted by hipDeviceGetByPCIBusId; byte 0 of its UUID is 'g' + k - 1 (no hex digit). A
//     pointer reports the vGPU it was allocated on (hipPointerGetAttribute(s),
//     hipDrvPointerGetAttributes; interior pointers too), a stream the vGPU it was created on
//     (hipStreamGetDevice), and a stream-ordered allocation is admitted against and charged to
//     its stream's vGPU.
// CU masks and the GPU-time limiter stay per physical GPU (HIP's hardware queues are shared by
// all streams of a device), with the vGPUs' shares summed as in merge mode.
// RCCL keeps seeing one physical GPU: a call of the bus id, UUID, lookup or property entry
// points from a loaded object named librccl* / libnccl* gets the physical values. RCCL between
// the virtual devices of one GPU therefore stays refused by RCCL itself ("Duplicate GPU
// detected": it compares bus ids); what it would do with a virtual id, whose sysfs path does
// not exist, has not been measured.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <hip/hip_deprecated.h>  // hipDeviceProp_tR0000: the hip_4.2 hipGetDeviceProperties

#include <dlfcn.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "real.h"
#include "shim.h"
#include "vgpu/devmap.h"
#include "vgpu/log.h"

using namespace vgpu;

namespace {

struct VirtDev {
  int phys = 0;    // HIP ordinal of the backing device
  int agent = 0;   // its agent (region device) index
  int slot = -1;   // region slot with this vGPU's quota (-1: the agent's own, no split)
  int k = 0;       // index among the vGPUs of its GPU (0 = the first)
  bool virt_id = false;  // reports a virtual PCI bus id and UUID (k >= 1, VGPU_VIRTUAL_PCI_IDS): the domain
                         // below, and byte 0 of the UUID 'g' + k - 1
  bool have_id = false;  // the runtime answered hipDeviceGetPCIBusId for the backing device
  int dom = 0, bus = 0, dev = 0, fn = 0;  // the PCI address this vGPU reports
};

std::atomic<int> g_state{0};  // 0 = not built, 1 = split active, 2 = off
VirtDev g_virt[kMaxDevices];
int g_nvirt = 0;
std::mutex g_build_mu;
thread_local int t_vdev = -1;  // the thread's current virtual device (-1 = none selected)
thread_local int t_charge_vdev = -1;  // VdevChargeScope: the vGPU allocations of this thread are charged to
bool g_ids = false;  // VGPU_VIRTUAL_PCI_IDS: virtual identities (set by build(), before g_state)
std::mutex g_stream_mu;
std::unordered_map<uintptr_t, int> g_streams;  // hipStream_t -> the vGPU it was created on

// "[dddd:]bb:dd.f", hex, either case (the runtime's own forms). False when malformed.
bool parse_bus_id(const char* s, int* dom, int* bus, int* dev, int* fn) {
  if (!s) return false;
  unsigned a = 0, b = 0, c = 0, d = 0;
  char tail = 0;
  if (sscanf(s, "%x:%x:%x.%x%c", &a, &b, &c, &d, &tail) == 4)
    return *dom = (int)a, *bus = (int)b, *dev = (int)c, *fn = (int)d, true;
  if (sscanf(s, "%x:%x.%x%c", &a, &b, &c, &tail) == 3) return *dom = 0, *bus = (int)a, *dev = (int)b, *fn = (int)c, true;
  return false;
}

// Whether the caller at `ret` is RCCL (a loaded object named librccl* / libnccl*): it keeps
// seeing the physical GPU's identity.
__attribute__((noinline)) bool caller_is_rccl(const void* ret) {
  Dl_info di;
  if (!ret || !dladdr(ret, &di) || !di.dli_fname) return false;
  const char* base = strrchr(di.dli_fname, '/');
  base = base ? base + 1 : di.dli_fname;
  return !strncmp(base, "librccl", 7) || !strncmp(base, "libnccl", 7);
}

int real_device_count() {
  VGPU_REAL_HIP(hipGetDeviceCount);
  int n = 0;
  if (!real_hipGetDeviceCount || real_hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

// Builds the virtual device table once the shim is initialised (the region holds the
// virtual slots' quotas). Off when the config asks for no split or has no duplicates.
bool build() {
  int st = g_state.load(std::memory_order_acquire);
  if (__builtin_expect(st != 0, 1)) return st == 1;
  // The shim's configuration is read when it initialises (with ROCr): a program whose first
  // HIP call takes a device ordinal (hipSetDevice(1), hipGetDeviceProperties) gets here first.
  ShimState& s = shim();
  if (s.phase.load(std::memory_order_acquire) == 0) (void)real_device_count();  // HIP (and the shim) initialise
  const int ph = s.phase.load(std::memory_order_acquire);
  if (ph == 3) {
    g_state.store(2, std::memory_order_release);  // inert shim: no limits, nothing to split
    return false;
  }
  if (ph != 2 || !s.active) return false;  // not yet: asked again on the next call
  const Config& cfg = config();
  if (!cfg.duplicate_split) {
    g_state.store(2, std::memory_order_release);
    return false;
  }
  std::lock_guard<std::mutex> g(g_build_mu);
  if ((st = g_state.load()) != 0) return st == 1;
  DeviceMap map;
  if (!parse_device_map(cfg.device_map.c_str(), &map) || map.duplicates == 0) {
    g_state.store(2, std::memory_order_release);
    return false;
  }
  const int np = real_device_count();
  if (np <= 0) return false;
  // Region slots of the virtual devices: after the agents, agent by agent, in map order
  // (shim.cpp assigns the same slots when it sets up the region: virtual_slots, devmap.h).
  const char* uu[kMaxDevices];
  for (int a = 0; a < s.n_agents; a++) uu[a] = s.agents[a].uuid;
  int first_slot[kMaxDevices], count[kMaxDevices];
  (void)virtual_slots(map, uu, s.n_agents, first_slot, count);  // (past the region's slots: shim.cpp warned)
  g_ids = cfg.virtual_pci_ids != 0;
  VGPU_REAL_HIP(hipDeviceGetPCIBusId);
  int n = 0;
  for (int h = 0; h < np && n < kMaxDevices; h++) {
    const int a = hip_device_agent(h);
    const int c = count[a] > 1 ? count[a] : 1;
    VirtDev base;
    base.phys = h;
    base.agent = a;
    char id[64] = {0};
    if (real_hipDeviceGetPCIBusId && real_hipDeviceGetPCIBusId(id, (int)sizeof(id), h) == hipSuccess)
      base.have_id = parse_bus_id(id, &base.dom, &base.bus, &base.dev, &base.fn);
    if (g_ids && c > 1 && base.have_id && base.dom >= 0x1000)
      VLOG_WARN("device %d: PCI domain %#x leaves no room for virtual ids; its vGPUs keep the physical id", h,
                base.dom);
    for (int k = 0; k < c && n < kMaxDevices; k++) {
      VirtDev v = base;
      v.k = k;
      v.slot = count[a] > 1 ? virtual_slot(first_slot[a], k) : -1;
      if (g_ids && k >= 1 && base.have_id && base.dom < 0x1000) {
        v.virt_id = true;
        v.dom = base.dom + 0x1000 * k;
      }
      g_virt[n++] = v;
    }
  }
  g_nvirt = n;
  VLOG_INFO("duplicate vGPUs split: %d HIP device(s) over %d physical", n, np);
  g_state.store(1, std::memory_order_release);
  return true;
}

inline bool split() {
  const int st = g_state.load(std::memory_order_relaxed);
  return st == 1 || (st == 0 && build());
}

// The virtual device a physical ordinal stands for in the calling thread: its current one
// when that is backed by `phys`, else the first one backed by it.
int virt_of(int phys) {
  if (t_vdev >= 0 && t_vdev < g_nvirt && g_virt[t_vdev].phys == phys) return t_vdev;
  for (int v = 0; v < g_nvirt; v++)
    if (g_virt[v].phys == phys) return v;
  return phys;
}

int current_virt() {
  VGPU_REAL_HIP(hipGetDevice);
  int p = 0;
  if (real_hipGetDevice) (void)real_hipGetDevice(&p);
  return virt_of(p);
}

// The quota of virtual device v: its slot's limit and usage (0 limit = none).
void slot_quota(int v, uint64_t* limit, uint64_t* used) {
  ShimState& s = shim();
  const int slot = g_virt[v].slot;
  if (slot < 0) {
    *limit = *used = 0;
    return;
  }
  *limit = s.region.limit(slot);
  *used = s.region.usage(slot);
}

// The vGPU the allocation holding `p` was made on (interior pointers too), or -1: no record
// (host or managed memory, another process's IPC mapping, memory from before the table).
int vdev_of_ptr(const void* p) {
  ShimState& s = shim();
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  std::lock_guard<std::mutex> g(s.alloc_mu);
  auto it = s.vcharge.upper_bound(a);
  if (it == s.vcharge.begin()) return -1;
  --it;
  return a - it->first < it->second.size ? it->second.vdev : -1;
}

// The device a pointer query reports: the recorded vGPU, else the calling thread's view of
// the physical ordinal the runtime answered.
int ptr_device(const void* p, int phys) {
  if (phys < 0) return phys;
  const int v = vdev_of_ptr(p);
  return v >= 0 && v < g_nvirt && g_virt[v].phys == phys ? v : virt_of(phys);
}

void remember_stream(hipStream_t stream) {
  if (!stream || !vdev_ids_active()) return;
  const int v = current_virt();
  std::lock_guard<std::mutex> g(g_stream_mu);
  g_streams[reinterpret_cast<uintptr_t>(stream)] = v;
}

// Writes vGPU v's bus id over the runtime's answer for its backing device, in the same
// format: the domain field (before the first of two colons) is replaced at its own width.
void print_virtual_bus_id(char* buf, int len, const VirtDev& v) {
  const char* c1 = strchr(buf, ':');
  if (!c1 || !strchr(c1 + 1, ':')) return;  // the short form has no domain field: left as it is
  bool upper = false;
  for (const char* q = buf; *q; q++) upper |= *q >= 'A' && *q <= 'F';
  char out[64];
  const int n = snprintf(out, sizeof(out), upper ? "%0*X%s" : "%0*x%s", (int)(c1 - buf), (unsigned)v.dom, c1);
  if (n > 0 && n < len && n < (int)sizeof(out)) memcpy(buf, out, (size_t)n + 1);
}

}  // namespace

namespace vgpu {

bool vdev_split_active() { return split(); }

int vdev_to_phys(int v) {
  if (v < 0 || !split() || v >= g_nvirt) return v;
  return g_virt[v].phys;
}

int vdev_charge_slot(int dev, int* vdev) {
  // Called from the HSA allocation hook, possibly inside the runtime's own initialisation:
  // only the table built already, and the thread's own record (no HIP call).
  if (vdev) *vdev = -1;
  if (g_state.load(std::memory_order_acquire) != 1) return -1;
  int v = t_charge_vdev;  // a stream-ordered allocation on another vGPU's stream (VdevChargeScope)
  if (v < 0 || v >= g_nvirt || g_virt[v].agent != dev) v = t_vdev;
  if (v < 0 || v >= g_nvirt || g_virt[v].agent != dev) {
    v = -1;
    for (int i = 0; i < g_nvirt && v < 0; i++)
      if (g_virt[i].agent == dev) v = i;
  }
  if (v < 0) return -1;
  if (vdev && g_ids) *vdev = v;  // recorded with the allocation for the pointer queries
  return g_virt[v].slot;
}

bool vdev_ids_active() { return split() && g_ids; }

int vdev_of_stream(void* stream_handle) {
  hipStream_t stream = static_cast<hipStream_t>(stream_handle);
  if (!split()) return -1;
  if (stream && stream != hipStreamPerThread && g_ids) {
    std::lock_guard<std::mutex> g(g_stream_mu);
    auto it = g_streams.find(reinterpret_cast<uintptr_t>(stream));
    if (it != g_streams.end()) return it->second;
  }
  if (!stream || stream == hipStreamPerThread || !g_ids) return current_virt();
  // not recorded (created before the table was built, or by an entry point the shim does not hook)
  VGPU_REAL_HIP(hipStreamGetDevice);
  int p = 0;
  if (real_hipStreamGetDevice && real_hipStreamGetDevice(stream, &p) == hipSuccess) return virt_of(p);
  return current_virt();
}

bool vdev_info(int v, int* phys, int* agent, int* slot) {
  if (v < 0 || !split() || v >= g_nvirt) return false;
  if (phys) *phys = g_virt[v].phys;
  if (agent) *agent = g_virt[v].agent;
  if (slot) *slot = g_virt[v].slot;
  return true;
}

VdevChargeScope::VdevChargeScope(int v) : prev_(t_charge_vdev) { t_charge_vdev = v; }
VdevChargeScope::~VdevChargeScope() { t_charge_vdev = prev_; }

void vdev_record_ptr(void* p, size_t size, int v) {
  if (!p || v < 0 || !vdev_ids_active()) return;
  ShimState& s = shim();
  std::lock_guard<std::mutex> g(s.alloc_mu);
  auto it = s.vcharge.find(reinterpret_cast<uintptr_t>(p));
  if (it != s.vcharge.end()) it->second.vdev = v;  // charged by the HSA hook inside the call: the charge stays
  else s.vcharge[reinterpret_cast<uintptr_t>(p)] = VChargeRec{size, -1, v};
}

void vdev_forget_ptr(void* p) {
  if (!p || g_state.load(std::memory_order_relaxed) != 1) return;
  ShimState& s = shim();
  std::lock_guard<std::mutex> g(s.alloc_mu);
  auto it = s.vcharge.find(reinterpret_cast<uintptr_t>(p));
  if (it != s.vcharge.end() && it->second.slot < 0) s.vcharge.erase(it);  // a charged one goes with its free (hsa_hooks.cpp)
}

}  // namespace vgpu

extern "C" {

hipError_t hipGetDeviceCount(int* count) {
  VGPU_REAL_HIP(hipGetDeviceCount);
  if (!real_hipGetDeviceCount) return hipErrorNotSupported;
  hipError_t e = real_hipGetDeviceCount(count);
  if (e == hipSuccess && count && split()) *count = g_nvirt;
  return e;
}

hipError_t hipSetDevice(int device) {
  VGPU_REAL_HIP(hipSetDevice);
  if (!real_hipSetDevice) return hipErrorNotSupported;
  if (!split()) return real_hipSetDevice(device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  hipError_t e = real_hipSetDevice(g_virt[device].phys);
  if (e == hipSuccess) t_vdev = device;
  return e;
}

hipError_t hipGetDevice(int* device) {
  VGPU_REAL_HIP(hipGetDevice);
  if (!real_hipGetDevice) return hipErrorNotSupported;
  hipError_t e = real_hipGetDevice(device);
  if (e == hipSuccess && device && split()) *device = virt_of(*device);
  return e;
}

hipError_t hipDeviceGet(hipDevice_t* device, int ordinal) {
  VGPU_REAL_HIP(hipDeviceGet);
  if (!real_hipDeviceGet) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceGet(device, ordinal);
  if (ordinal < 0 || ordinal >= g_nvirt) return hipErrorInvalidDevice;
  hipError_t e = real_hipDeviceGet(device, g_virt[ordinal].phys);
  if (e == hipSuccess && device) *device = ordinal;  // HIP's device handle is the ordinal
  return e;
}

hipError_t hipStreamGetDevice(hipStream_t stream, hipDevice_t* device) {
  VGPU_REAL_HIP(hipStreamGetDevice);
  if (!real_hipStreamGetDevice) return hipErrorNotSupported;
  hipError_t e = real_hipStreamGetDevice(stream, device);
  if (e != hipSuccess || !device || !split()) return e;
  int v = -1;
  if (g_ids && stream && stream != hipStreamPerThread) {
    std::lock_guard<std::mutex> g(g_stream_mu);
    auto it = g_streams.find(reinterpret_cast<uintptr_t>(stream));
    if (it != g_streams.end()) v = it->second;
  }
  *device = v >= 0 && v < g_nvirt && g_virt[v].phys == *device ? v : virt_of(*device);
  return e;
}

// Streams remember the vGPU they were created on (the creating thread's current one).
hipError_t hipStreamCreate(hipStream_t* stream) {
  VGPU_REAL_HIP(hipStreamCreate);
  if (!real_hipStreamCreate) return hipErrorNotSupported;
  hipError_t e = real_hipStreamCreate(stream);
  if (e == hipSuccess && stream) remember_stream(*stream);
  return e;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int flags) {
  VGPU_REAL_HIP(hipStreamCreateWithFlags);
  if (!real_hipStreamCreateWithFlags) return hipErrorNotSupported;
  hipError_t e = real_hipStreamCreateWithFlags(stream, flags);
  if (e == hipSuccess && stream) remember_stream(*stream);
  return e;
}

hipError_t hipStreamCreateWithPriority(hipStream_t* stream, unsigned int flags, int priority) {
  VGPU_REAL_HIP(hipStreamCreateWithPriority);
  if (!real_hipStreamCreateWithPriority) return hipErrorNotSupported;
  hipError_t e = real_hipStreamCreateWithPriority(stream, flags, priority);
  if (e == hipSuccess && stream) remember_stream(*stream);
  return e;
}

hipError_t hipExtStreamCreateWithCUMask(hipStream_t* stream, uint32_t cuMaskSize, const uint32_t* cuMask) {
  VGPU_REAL_HIP(hipExtStreamCreateWithCUMask);
  if (!real_hipExtStreamCreateWithCUMask) return hipErrorNotSupported;
  hipError_t e = real_hipExtStreamCreateWithCUMask(stream, cuMaskSize, cuMask);
  if (e == hipSuccess && stream) remember_stream(*stream);
  return e;
}

hipError_t hipStreamDestroy(hipStream_t stream) {
  VGPU_REAL_HIP(hipStreamDestroy);
  if (!real_hipStreamDestroy) return hipErrorNotSupported;
  if (stream && g_state.load(std::memory_order_relaxed) == 1) {
    // before the runtime frees the handle: another thread may get the same one at once
    std::lock_guard<std::mutex> g(g_stream_mu);
    g_streams.erase(reinterpret_cast<uintptr_t>(stream));
  }
  return real_hipStreamDestroy(stream);
}

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wdeprecated-declarations"  // the context API: deprecated, still exported
hipError_t hipCtxGetDevice(hipDevice_t* device) {
  VGPU_REAL_HIP(hipCtxGetDevice);
  if (!real_hipCtxGetDevice) return hipErrorNotSupported;
  hipError_t e = real_hipCtxGetDevice(device);
  if (e == hipSuccess && device && vdev_ids_active()) *device = virt_of(*device);
  return e;
}
#pragma GCC diagnostic pop

hipError_t hipDeviceGetPCIBusId(char* pci_bus_id, int len, int device) {
  VGPU_REAL_HIP(hipDeviceGetPCIBusId);
  if (!real_hipDeviceGetPCIBusId) return hipErrorNotSupported;
  gate_suspend();
  if (!split()) return real_hipDeviceGetPCIBusId(pci_bus_id, len, device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  const VirtDev& v = g_virt[device];
  hipError_t e = real_hipDeviceGetPCIBusId(pci_bus_id, len, v.phys);  // a short buffer fails as in the runtime
  if (e == hipSuccess && pci_bus_id && v.virt_id && !caller_is_rccl(__builtin_return_address(0)))
    print_virtual_bus_id(pci_bus_id, len, v);
  return e;
}

hipError_t hipDeviceGetUuid(hipUUID* uuid, hipDevice_t device) {
  VGPU_REAL_HIP(hipDeviceGetUuid);
  if (!real_hipDeviceGetUuid) return hipErrorNotSupported;
  gate_suspend();
  if (!split()) return real_hipDeviceGetUuid(uuid, device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  const VirtDev& v = g_virt[device];
  hipError_t e = real_hipDeviceGetUuid(uuid, v.phys);
  if (e == hipSuccess && uuid && v.virt_id && !caller_is_rccl(__builtin_return_address(0)))
    uuid->bytes[0] = (char)('g' + v.k - 1);
  return e;
}

hipError_t hipDeviceGetByPCIBusId(int* device, const char* pci_bus_id) {
  VGPU_REAL_HIP(hipDeviceGetByPCIBusId);
  if (!real_hipDeviceGetByPCIBusId) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceGetByPCIBusId(device, pci_bus_id);
  int dom = 0, bus = 0, dev = 0, fn = 0;
  const bool rccl = !g_ids || caller_is_rccl(__builtin_return_address(0));
  if (!rccl && device && parse_bus_id(pci_bus_id, &dom, &bus, &dev, &fn)) {
    // a virtual id names its vGPU; a physical one the GPU's first vGPU (the lowest ordinal)
    for (int v = 0; v < g_nvirt; v++) {
      const VirtDev& d = g_virt[v];
      if (d.have_id && d.dom == dom && d.bus == bus && d.dev == dev && d.fn == fn) return *device = v, hipSuccess;
    }
    if (dom >= 0x1000) return hipErrorInvalidValue;  // no such vGPU (the runtime: no such device)
  }
  hipError_t e = real_hipDeviceGetByPCIBusId(device, pci_bus_id);
  if (e == hipSuccess && device) *device = virt_of(*device);
  return e;
}

#undef hipGetDeviceProperties
hipError_t hipGetDeviceProperties(hipDeviceProp_tR0000* prop, int device) {
  using Fn = hipError_t (*)(hipDeviceProp_tR0000*, int);
  VGPU_REAL_AS(hipGetDeviceProperties, Fn, "libamdhip64", "hip_4.2");
  if (!real_hipGetDeviceProperties) return hipErrorNotSupported;
  if (!split()) return real_hipGetDeviceProperties(prop, device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  hipError_t e = real_hipGetDeviceProperties(prop, g_virt[device].phys);
  uint64_t lim = 0, used = 0;
  slot_quota(device, &lim, &used);
  if (e == hipSuccess && prop && lim) prop->totalGlobalMem = lim;
  if (e == hipSuccess && prop && g_virt[device].virt_id && !caller_is_rccl(__builtin_return_address(0)))
    prop->pciDomainID = g_virt[device].dom;
  return e;
}

hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* prop, int device) {
  VGPU_REAL_HIP(hipGetDevicePropertiesR0600);
  if (!real_hipGetDevicePropertiesR0600) return hipErrorNotSupported;
  if (!split()) return real_hipGetDevicePropertiesR0600(prop, device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  hipError_t e = real_hipGetDevicePropertiesR0600(prop, g_virt[device].phys);
  uint64_t lim = 0, used = 0;
  slot_quota(device, &lim, &used);
  if (e == hipSuccess && prop && lim) prop->totalGlobalMem = lim;
  if (e == hipSuccess && prop && g_virt[device].virt_id && !caller_is_rccl(__builtin_return_address(0))) {
    prop->pciDomainID = g_virt[device].dom;
    prop->uuid.bytes[0] = (char)('g' + g_virt[device].k - 1);
  }
  return e;
}

// Device attributes of virtual device v: the backing GPU's, except its global memory, which is
// v's own quota (hipDeviceAttributeTotalGlobalMem is an int: a quota past INT32_MAX saturates,
// as the runtime saturates the whole 288 GB GPU: profiles/r6y).
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t attr, int device) {
  VGPU_REAL_HIP(hipDeviceGetAttribute);
  if (!real_hipDeviceGetAttribute) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceGetAttribute(value, attr, device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  hipError_t e = real_hipDeviceGetAttribute(value, attr, g_virt[device].phys);
  if (e == hipSuccess && value && attr == hipDeviceAttributePciDomainId && g_virt[device].virt_id)
    *value = g_virt[device].dom;  // the virtual PCI bus id (bus and device stay the GPU's)
  if (e != hipSuccess || !value || attr != hipDeviceAttributeTotalGlobalMem) return e;
  uint64_t lim = 0, used = 0;
  slot_quota(device, &lim, &used);
  if (lim) *value = lim > (uint64_t)INT32_MAX ? INT32_MAX : (int)lim;
  return e;
}

hipError_t hipDeviceTotalMem(size_t* bytes, hipDevice_t device) {
  VGPU_REAL_HIP(hipDeviceTotalMem);
  if (!real_hipDeviceTotalMem) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceTotalMem(bytes, device);
  if (device < 0 || device >= g_nvirt) return hipErrorInvalidDevice;
  hipError_t e = real_hipDeviceTotalMem(bytes, g_virt[device].phys);
  uint64_t lim = 0, used = 0;
  slot_quota(device, &lim, &used);
  if (e == hipSuccess && bytes && lim) *bytes = lim;
  return e;
}

// The current device's free and total memory: the runtime's answer (the physical GPU, within
// the summed quota of its vGPUs: the HSA hook), narrowed to the current virtual device's own.
hipError_t hipMemGetInfo(size_t* free_bytes, size_t* total_bytes) {
  VGPU_REAL_HIP(hipMemGetInfo);
  if (!real_hipMemGetInfo) return hipErrorNotSupported;
  hipError_t e = real_hipMemGetInfo(free_bytes, total_bytes);
  if (e != hipSuccess || !split()) return e;
  const int v = current_virt();
  if (v < 0 || v >= g_nvirt) return e;
  uint64_t lim = 0, used = 0;
  slot_quota(v, &lim, &used);
  if (!lim) return e;
  const uint64_t left = lim > used ? lim - used : 0;
  if (free_bytes && *free_bytes > left) *free_bytes = left;
  if (total_bytes) *total_bytes = lim;
  return e;
}

hipError_t hipDeviceCanAccessPeer(int* can, int device, int peer) {
  VGPU_REAL_HIP(hipDeviceCanAccessPeer);
  if (!real_hipDeviceCanAccessPeer) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceCanAccessPeer(can, device, peer);
  if (device < 0 || device >= g_nvirt || peer < 0 || peer >= g_nvirt) return hipErrorInvalidDevice;
  if (g_virt[device].phys == g_virt[peer].phys) {
    if (can) *can = device != peer;  // one GPU's memory: always reachable (not from itself, as CUDA)
    return hipSuccess;
  }
  return real_hipDeviceCanAccessPeer(can, g_virt[device].phys, g_virt[peer].phys);
}

hipError_t hipDeviceEnablePeerAccess(int peer, unsigned int flags) {
  VGPU_REAL_HIP(hipDeviceEnablePeerAccess);
  if (!real_hipDeviceEnablePeerAccess) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceEnablePeerAccess(peer, flags);
  if (peer < 0 || peer >= g_nvirt) return hipErrorInvalidDevice;
  const int cur = current_virt();
  if (cur >= 0 && cur < g_nvirt && g_virt[cur].phys == g_virt[peer].phys) return hipSuccess;  // same memory
  return real_hipDeviceEnablePeerAccess(g_virt[peer].phys, flags);
}

hipError_t hipDeviceDisablePeerAccess(int peer) {
  VGPU_REAL_HIP(hipDeviceDisablePeerAccess);
  if (!real_hipDeviceDisablePeerAccess) return hipErrorNotSupported;
  if (!split()) return real_hipDeviceDisablePeerAccess(peer);
  if (peer < 0 || peer >= g_nvirt) return hipErrorInvalidDevice;
  const int cur = current_virt();
  if (cur >= 0 && cur < g_nvirt && g_virt[cur].phys == g_virt[peer].phys) return hipSuccess;
  return real_hipDeviceDisablePeerAccess(g_virt[peer].phys);
}

// Two vGPUs of one GPU are the same memory: the runtime would see src == dst and refuse.
hipError_t hipDeviceGetP2PAttribute(int* value, hipDeviceP2PAttr attr, int src, int dst) {
  VGPU_REAL_HIP(hipDeviceGetP2PAttribute);
  if (!real_hipDeviceGetP2PAttribute) return hipErrorNotSupported;
  gate_suspend();
  if (!split()) return real_hipDeviceGetP2PAttribute(value, attr, src, dst);
  if (src < 0 || src >= g_nvirt || dst < 0 || dst >= g_nvirt || src == dst) return hipErrorInvalidDevice;
  if (g_virt[src].phys != g_virt[dst].phys || !g_ids)
    return real_hipDeviceGetP2PAttribute(value, attr, g_virt[src].phys, g_virt[dst].phys);
  if (!value) return hipErrorInvalidValue;
  switch (attr) {
    case hipDevP2PAttrAccessSupported:
    case hipDevP2PAttrNativeAtomicSupported: *value = 1; return hipSuccess;
    case hipDevP2PAttrPerformanceRank: {
      // as the runtime ranks the GPU's best peer; 0 when it has none
      int best = 0;
      for (int v = 0; v < g_nvirt; v++) {
        int r = 0;
        if (g_virt[v].phys != g_virt[src].phys && g_virt[v].k == 0 &&
            real_hipDeviceGetP2PAttribute(&r, attr, g_virt[src].phys, g_virt[v].phys) == hipSuccess && r > best)
          best = r;
      }
      *value = best;
      return hipSuccess;
    }
    case hipDevP2PAttrHipArrayAccessSupported: *value = 1; return hipSuccess;
    default: return hipErrorInvalidValue;
  }
}

// hipMemLocation names a device by its (virtual) ordinal.
static bool map_location(hipMemLocation* loc) {
  if (loc->type != hipMemLocationTypeDevice || !split()) return true;
  if (loc->id < 0 || loc->id >= g_nvirt) return false;
  loc->id = g_virt[loc->id].phys;
  return true;
}

hipError_t hipMemAdvise_v2(const void* dev_ptr, size_t count, hipMemoryAdvise advice, hipMemLocation location) {
  VGPU_REAL_HIP(hipMemAdvise_v2);
  if (!real_hipMemAdvise_v2) return hipErrorNotSupported;
  gate_suspend();
  if (!map_location(&location)) return hipErrorInvalidDevice;
  return real_hipMemAdvise_v2(dev_ptr, count, advice, location);
}

hipError_t hipMemPrefetchAsync_v2(const void* dev_ptr, size_t count, hipMemLocation location, unsigned int flags,
                                  hipStream_t stream) {
  VGPU_REAL_HIP(hipMemPrefetchAsync_v2);
  if (!real_hipMemPrefetchAsync_v2) return hipErrorNotSupported;
  gate_suspend();
  if (!map_location(&location)) return hipErrorInvalidDevice;
  return real_hipMemPrefetchAsync_v2(dev_ptr, count, location, flags, stream);
}

// Pointer queries (suspend-gated, as the reference's): with split vGPUs the device they
// report is the vGPU the allocation was made on, not the physical ordinal. Without split
// they are one relaxed load, the gate and the runtime's call.
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attributes, const void* ptr) {
  VGPU_REAL_HIP(hipPointerGetAttributes);
  if (!real_hipPointerGetAttributes) return hipErrorNotSupported;
  gate_suspend();
  hipError_t e = real_hipPointerGetAttributes(attributes, ptr);
  if (__builtin_expect(g_state.load(std::memory_order_relaxed) == 2, 1) || e != hipSuccess) return e;
  if (attributes && vdev_ids_active()) attributes->device = ptr_device(ptr, attributes->device);
  return e;
}

hipError_t hipPointerGetAttribute(void* data, hipPointer_attribute attribute, hipDeviceptr_t ptr) {
  VGPU_REAL_HIP(hipPointerGetAttribute);
  if (!real_hipPointerGetAttribute) return hipErrorNotSupported;
  gate_suspend();
  hipError_t e = real_hipPointerGetAttribute(data, attribute, ptr);
  if (__builtin_expect(g_state.load(std::memory_order_relaxed) == 2, 1) || e != hipSuccess) return e;
  if (data && attribute == HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL && vdev_ids_active())
    *static_cast<int*>(data) = ptr_device(ptr, *static_cast<int*>(data));
  return e;
}

hipError_t hipDrvPointerGetAttributes(unsigned int numAttributes, hipPointer_attribute* attributes, void** data,
                                      hipDeviceptr_t ptr) {
  VGPU_REAL_HIP(hipDrvPointerGetAttributes);
  if (!real_hipDrvPointerGetAttributes) return hipErrorNotSupported;
  gate_suspend();
  hipError_t e = real_hipDrvPointerGetAttributes(numAttributes, attributes, data, ptr);
  if (__builtin_expect(g_state.load(std::memory_order_relaxed) == 2, 1) || e != hipSuccess) return e;
  if (attributes && data && vdev_ids_active())
    for (unsigned int i = 0; i < numAttributes; i++)
      if (attributes[i] == HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL && data[i])
        *static_cast<int*>(data[i]) = ptr_device(ptr, *static_cast<int*>(data[i]));
  return e;
}

}  // extern "C"
