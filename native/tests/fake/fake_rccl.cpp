// A stand-in for librccl.so (CPU-only shim tests): asks the HIP runtime who device `device` is,
// the way RCCL does when it builds its topology, and hands back what it was told. The shim
// answers a caller in an object named librccl* with the physical GPU's identity.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

extern "C" int fake_librccl_probe(int device, char* bus_id, int len, hipUUID* uuid, int* by_bus_id, int* domain) {
  hipDeviceProp_t prop;
  if (hipDeviceGetPCIBusId(bus_id, len, device) != hipSuccess) return 1;
  if (hipDeviceGetUuid(uuid, device) != hipSuccess) return 2;
  if (hipDeviceGetByPCIBusId(by_bus_id, bus_id) != hipSuccess) return 3;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 4;
  *domain = prop.pciDomainID;
  return prop.uuid.bytes[0] == uuid->bytes[0] ? 0 : 5;
}
