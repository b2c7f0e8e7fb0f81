// The device-identity slice of the fake libamdhip64.so (fake_hip.cpp): PCI bus ids and UUIDs,
// pointer and stream queries, stream-ordered allocations and memory locations, as the shim's
// split-vGPU hooks (src/shim/vdev_hooks.cpp, hip_hooks.cpp) call them. Fake GPU g sits at
// 0000:(05 + 0x10 g):00.0 (the fake ROCr's BDF) and its UUID is the 16 characters after
// "GPU-" of the agent's, as CLR reports them. A stream-ordered allocation is one
// hsa_amd_memory_pool_allocate on the stream's device, so the shim's charges are exact.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstdio>
#include <cstring>
#include <mutex>

extern "C" {
void fake_hip_record(const char* name);
int fake_hip_priv_count();
int fake_hip_priv_current();
int fake_hip_priv_stream_device(hipStream_t stream);
uint64_t fake_hip_priv_agent(int d);
uint64_t fake_hip_priv_pool(int d);
int fake_hip_priv_device_of_rocr(int rocr);
hipError_t fake_hip_priv_new_stream(hipStream_t* stream);
int fake_rocr_pointer_info(const void* p, int* dev, void** base, uint64_t* size);
}

namespace {

std::mutex g_mu;
int g_last_location = -100;  // the device id of the last _v2 advise / prefetch as the runtime got it

void address_of(int d, unsigned* dom, unsigned* bus, unsigned* dev, unsigned* fn) {
  uint32_t bdf = 0, domain = 0;
  hsa_agent_t a{fake_hip_priv_agent(d)};
  hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf);
  hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &domain);
  *dom = domain;
  *bus = bdf >> 8;
  *dev = (bdf >> 3) & 0x1f;
  *fn = bdf & 7;
}

// The HIP device a pointer belongs to: -1 for host memory, -2 when it is in no allocation.
int pointer_device(const void* p) {
  int rocr = -1;
  if (!fake_rocr_pointer_info(p, &rocr, nullptr, nullptr)) return -2;
  return rocr < 0 ? -1 : fake_hip_priv_device_of_rocr(rocr);
}

hipError_t alloc_on(void** ptr, size_t size, hipStream_t stream) {
  if (!ptr) return hipErrorInvalidValue;
  hsa_amd_memory_pool_t pool{fake_hip_priv_pool(fake_hip_priv_stream_device(stream))};
  return hsa_amd_memory_pool_allocate(pool, size ? size : 1, 0, ptr) == HSA_STATUS_SUCCESS ? hipSuccess
                                                                                          : hipErrorOutOfMemory;
}

void note_location(hipMemLocation loc) {
  std::lock_guard<std::mutex> g(g_mu);
  g_last_location = loc.type == hipMemLocationTypeDevice ? loc.id : -1;
}

}  // namespace

extern "C" {

hipError_t hipDeviceGetPCIBusId(char* pci_bus_id, int len, int device) {
  fake_hip_record("hipDeviceGetPCIBusId");
  if (device < 0 || device >= fake_hip_priv_count()) return hipErrorInvalidDevice;
  if (!pci_bus_id || len <= 0) return hipErrorInvalidValue;
  unsigned dom, bus, dev, fn;
  address_of(device, &dom, &bus, &dev, &fn);
  const int n = snprintf(pci_bus_id, (size_t)len, "%04x:%02x:%02x.%01x", dom, bus, dev, fn);
  return n > 0 && n < len ? hipSuccess : hipErrorInvalidValue;  // CLR: a short buffer is an invalid value
}

hipError_t hipDeviceGetUuid(hipUUID* uuid, hipDevice_t device) {
  fake_hip_record("hipDeviceGetUuid");
  if (device < 0 || device >= fake_hip_priv_count()) return hipErrorInvalidDevice;
  if (!uuid) return hipErrorInvalidValue;
  char u[64] = {0};
  hsa_agent_get_info(hsa_agent_t{fake_hip_priv_agent(device)}, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_UUID, u);
  const char* hex = strncmp(u, "GPU-", 4) ? u : u + 4;
  memset(uuid->bytes, 0, sizeof(uuid->bytes));
  memcpy(uuid->bytes, hex, strnlen(hex, sizeof(uuid->bytes)));
  return hipSuccess;
}

hipError_t hipDeviceGetByPCIBusId(int* device, const char* pci_bus_id) {
  fake_hip_record("hipDeviceGetByPCIBusId");
  if (!device || !pci_bus_id) return hipErrorInvalidValue;
  unsigned dom = 0, bus = 0, dev = 0, fn = 0;
  char tail = 0;
  if (sscanf(pci_bus_id, "%x:%x:%x.%x%c", &dom, &bus, &dev, &fn, &tail) != 4) {
    dom = 0;
    if (sscanf(pci_bus_id, "%x:%x.%x%c", &bus, &dev, &fn, &tail) != 3) return hipErrorInvalidValue;
  }
  for (int d = 0; d < fake_hip_priv_count(); d++) {
    unsigned a, b, c, f;
    address_of(d, &a, &b, &c, &f);
    if (a == dom && b == bus && c == dev && f == fn) return *device = d, hipSuccess;
  }
  return hipErrorInvalidValue;
}

hipError_t hipDeviceGetP2PAttribute(int* value, hipDeviceP2PAttr attr, int src, int dst) {
  fake_hip_record("hipDeviceGetP2PAttribute");
  const int n = fake_hip_priv_count();
  if (src < 0 || src >= n || dst < 0 || dst >= n || src == dst) return hipErrorInvalidDevice;  // CLR: not itself
  if (!value) return hipErrorInvalidValue;
  *value = attr == hipDevP2PAttrPerformanceRank ? 3 : 1;
  return hipSuccess;
}

hipError_t hipCtxGetDevice(hipDevice_t* device) {
  fake_hip_record("hipCtxGetDevice");
  if (!device) return hipErrorInvalidValue;
  (void)fake_hip_priv_count();
  *device = fake_hip_priv_current();
  return hipSuccess;
}

hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attributes, const void* ptr) {
  fake_hip_record("hipPointerGetAttributes");
  const int d = pointer_device(ptr);
  if (!attributes || d == -2) return hipErrorInvalidValue;
  memset(attributes, 0, sizeof(*attributes));
  attributes->type = d >= 0 ? hipMemoryTypeDevice : hipMemoryTypeHost;
  attributes->device = d >= 0 ? d : fake_hip_priv_current();
  attributes->devicePointer = const_cast<void*>(ptr);
  return hipSuccess;
}

hipError_t hipPointerGetAttribute(void* data, hipPointer_attribute attribute, hipDeviceptr_t ptr) {
  fake_hip_record("hipPointerGetAttribute");
  const int d = pointer_device(ptr);
  if (!data || d == -2) return hipErrorInvalidValue;
  switch (attribute) {
    case HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL: *static_cast<int*>(data) = d >= 0 ? d : fake_hip_priv_current(); break;
    case HIP_POINTER_ATTRIBUTE_MEMORY_TYPE:
      *static_cast<unsigned*>(data) = d >= 0 ? hipMemoryTypeDevice : hipMemoryTypeHost;
      break;
    case HIP_POINTER_ATTRIBUTE_DEVICE_POINTER: *static_cast<void**>(data) = ptr; break;
    default: return hipErrorInvalidValue;
  }
  return hipSuccess;
}

hipError_t hipDrvPointerGetAttributes(unsigned int n, hipPointer_attribute* attributes, void** data,
                                      hipDeviceptr_t ptr) {
  hipError_t e = hipSuccess;
  if (!attributes || !data) e = hipErrorInvalidValue;
  for (unsigned int i = 0; e == hipSuccess && i < n; i++) {
    // (the fake's own definition: a call through the exported name would be the shim's hook)
    const int d = pointer_device(ptr);
    if (d == -2 || !data[i]) e = hipErrorInvalidValue;
    else if (attributes[i] == HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL)
      *static_cast<int*>(data[i]) = d >= 0 ? d : fake_hip_priv_current();
    else if (attributes[i] == HIP_POINTER_ATTRIBUTE_MEMORY_TYPE)
      *static_cast<unsigned*>(data[i]) = d >= 0 ? hipMemoryTypeDevice : hipMemoryTypeHost;
    else if (attributes[i] == HIP_POINTER_ATTRIBUTE_DEVICE_POINTER) *static_cast<void**>(data[i]) = ptr;
    else e = hipErrorInvalidValue;
  }
  fake_hip_record("hipDrvPointerGetAttributes");
  return e;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int) { return fake_hip_priv_new_stream(stream); }
hipError_t hipStreamCreateWithPriority(hipStream_t* stream, unsigned int, int) {
  return fake_hip_priv_new_stream(stream);
}
hipError_t hipExtStreamCreateWithCUMask(hipStream_t* stream, uint32_t, const uint32_t*) {
  return fake_hip_priv_new_stream(stream);
}

hipError_t hipMallocAsync(void** ptr, size_t size, hipStream_t stream) {
  fake_hip_record("hipMallocAsync");
  return alloc_on(ptr, size, stream);
}

hipError_t hipMallocFromPoolAsync(void** ptr, size_t size, hipMemPool_t, hipStream_t stream) {
  fake_hip_record("hipMallocFromPoolAsync");
  return alloc_on(ptr, size, stream);
}

hipError_t hipFreeAsync(void* ptr, hipStream_t) {
  fake_hip_record("hipFreeAsync");
  if (!ptr) return hipSuccess;
  return hsa_amd_memory_pool_free(ptr) == HSA_STATUS_SUCCESS ? hipSuccess : hipErrorInvalidValue;
}

hipError_t hipMemAdvise_v2(const void* ptr, size_t count, hipMemoryAdvise, hipMemLocation location) {
  fake_hip_record("hipMemAdvise_v2");
  if (!ptr || !count) return hipErrorInvalidValue;
  if (location.type == hipMemLocationTypeDevice && (location.id < 0 || location.id >= fake_hip_priv_count()))
    return hipErrorInvalidDevice;
  note_location(location);
  return hipSuccess;
}

hipError_t hipMemPrefetchAsync_v2(const void* ptr, size_t count, hipMemLocation location, unsigned int, hipStream_t) {
  fake_hip_record("hipMemPrefetchAsync_v2");
  if (!ptr || !count) return hipErrorInvalidValue;
  if (location.type == hipMemLocationTypeDevice && (location.id < 0 || location.id >= fake_hip_priv_count()))
    return hipErrorInvalidDevice;
  note_location(location);
  return hipSuccess;
}

// Test introspection: the device id the runtime got with the last _v2 advise / prefetch
// (-1 = not a device location, -100 = none yet).
int fake_hip_last_location() {
  std::lock_guard<std::mutex> g(g_mu);
  return g_last_location;
}

}  // extern "C"
