/* A stand-in for <hip/hip_runtime.h> that runs a HIP kernel's text on the HOST, one lane after the other (tests/native/mix_kernel_check.cpp):
 * the qualifiers vanish, blockIdx / threadIdx / blockDim are globals, and hipLaunchKernelGGL loops over the grid.  Good for kernels whose
 * lanes do not talk to each other (no LDS, no barriers, no cross-lane operations): their indexing and bounds can then be checked under
 * AddressSanitizer on a CPU build. */
#pragma once
#include <cstdint>
#include <cstddef>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, blockDim;
typedef void *hipStream_t;
typedef int hipError_t;
static const hipError_t hipSuccess = 0;
static inline hipError_t hipGetLastError() { return 0; }
static int g_last_threads = 0;   /* geometry of the last launch, for the caller's messages */
static unsigned g_last_grid = 0;
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...)                       \
    do {                                                                              \
        blockDim = block; g_last_threads = block.x; g_last_grid = grid.x;             \
        for (unsigned b_ = 0; b_ < grid.x; b_++)                                      \
            for (unsigned t_ = 0; t_ < block.x; t_++) {                               \
                blockIdx = dim3(b_); threadIdx = dim3(t_);                            \
                kern(__VA_ARGS__);                                                    \
            }                                                                         \
    } while (0)
