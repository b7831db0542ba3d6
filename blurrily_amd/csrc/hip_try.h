// hip_try.h -- BLURRILY_HIP_TRY: a HIP call that fails is reported on stderr and ends the enclosing function with -1
// and errno (ENOMEM when the device is out of memory, EIO otherwise).
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdio>

#define BLURRILY_HIP_TRY(expr)                                                        \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      std::fprintf(stderr, "blurrily_hip: %s failed: %s\n", #expr, hipGetErrorString(e_)); \
      errno = (e_ == hipErrorOutOfMemory) ? ENOMEM : EIO;                             \
      return -1;                                                                      \
    }                                                                                 \
  } while (0)
