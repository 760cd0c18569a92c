// A host-only stand-in for <hip/hip_runtime.h>, found first by the stand-alone CPU programs of the tests that include a
// header of the kernels (tests/tools/serdeflate_hostcheck.cpp includes topowx_amd/csrc/twx_deflate.h): a plain C++ compiler
// then sees the __host__ __device__ functions as ordinary inline functions, and the kernels (#if defined(__HIPCC__)) not at all.
#pragma once
#include <stdint.h>

#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))

#ifndef __has_builtin
#define __has_builtin(x) 0
#endif
#if !__has_builtin(__builtin_bitreverse32)
static inline uint32_t twx_stub_bitreverse32(uint32_t v)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
#define __builtin_bitreverse32 twx_stub_bitreverse32
#endif
