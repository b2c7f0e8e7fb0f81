// The gfx950 code object embedded in vgpu-validate (a plain ELF, loaded with
// hipModuleLoadData): the CU census, the pattern kernels and
// the compute known-answer test (cu_selftest), the same device code as
// libvgpu_kernels.so (device_kernels.h).
#include "device_kernels.h"

extern "C" __global__ void __launch_bounds__(64) census(uint32_t* out, uint64_t spin_ticks) {
  vgpu_dev::census_body(out, spin_ticks);
}
