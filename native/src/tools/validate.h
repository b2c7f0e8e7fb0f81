// vgpu-validate: what vgpu_validate.cpp (command line, allow-list check) and
// validate_conformance.cpp (--conformance) share.
#pragma once

#include <cstdint>
#include <string>

namespace vgpu_validate {

struct Options {
  bool json = false;
  int device = -1;                      // --device I (-1: every visible HIP device)
  const char* limits = "/vgpu/limits";  // --limits FILE: the promise (then the environment)
  uint64_t bytes = 256ull << 20;        // --bytes N: size of the memory / spill test buffer
  bool spill = false;                   // --spill
  int inject = 0;                       // --inject K: poke K words between fill and check
  bool compute = false;                 // --compute: the per-CU known-answer test (vgpu/selftest.h)
  int inject_compute = 0;               // --inject-compute K: K workgroups run it with a flipped input bit
};

// Lower-case, no surrounding space, no "GPU-" prefix.
std::string norm_uuid(std::string s);

// Runs the conformance checks; the process exit code (0 no check failed, 1 otherwise).
int conformance(const Options& opt);

}  // namespace vgpu_validate
