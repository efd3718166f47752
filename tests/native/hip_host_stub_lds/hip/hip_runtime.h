/* A stand-in for <hip/hip_runtime.h> that runs a HIP kernel's text on the HOST for kernels whose lanes DO talk to each other through
 * LDS and barriers (tests/native/meter_kernel_check.cpp): the workgroups run one after the other, the lanes of a workgroup as threads
 * of their own (started once, woken for every launch), __shared__ arrays are statics they all see, and __syncthreads() is a barrier over the workgroup's lanes.  blockIdx and
 * threadIdx are thread-local.  A lane may return early only in a kernel that has no barrier.  Indexing and bounds can then be checked
 * under AddressSanitizer on a CPU build (hip_host_stub/ is the lighter one for kernels without LDS). */
#pragma once
#include <pthread.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static thread_local dim3 blockIdx, threadIdx;
static dim3 blockDim;
typedef void *hipStream_t;
typedef void *hipEvent_t;
typedef int hipError_t;
static const hipError_t hipSuccess = 0;
static inline hipError_t hipGetLastError() { return 0; }
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
static pthread_barrier_t g_group_barrier;
static inline void __syncthreads() { pthread_barrier_wait(&g_group_barrier); }
static unsigned long g_groups_run = 0; /* workgroups of all launches, for the caller's report */
/* the lanes: kHostLanesMax threads started once, woken for every launch (a thread a lane a launch costs seconds under a sanitizer) */
constexpr unsigned kHostLanesMax = 256;
struct HostLanes {
    pthread_barrier_t begin, end; /* the lanes and the launching thread */
    std::vector<std::thread> threads;
    const std::function<void()> *lane = nullptr;
    unsigned grid = 0, block = 0;
    bool quit = false;
    HostLanes() {
        pthread_barrier_init(&begin, nullptr, kHostLanesMax + 1);
        pthread_barrier_init(&end, nullptr, kHostLanesMax + 1);
        for (unsigned t = 0; t < kHostLanesMax; t++)
            threads.emplace_back([this, t]() {
                for (;;) {
                    pthread_barrier_wait(&begin);
                    if (quit) return;
                    for (unsigned b = 0; b < grid && t < block; b++) {
                        blockIdx = dim3(b);
                        threadIdx = dim3(t);
                        (*lane)();
                        pthread_barrier_wait(&g_group_barrier); /* (the next workgroup begins when every lane has left this one) */
                    }
                    pthread_barrier_wait(&end);
                }
            });
    }
    ~HostLanes() {
        quit = true;
        pthread_barrier_wait(&begin);
        for (auto &t : threads) t.join();
    }
};
static inline void host_launch(unsigned grid_, unsigned block_, const std::function<void()> &lane) {
    static HostLanes lanes;
    if (block_ > kHostLanesMax) abort();
    blockDim = dim3(block_);
    lanes.lane = &lane, lanes.grid = grid_, lanes.block = block_;
    pthread_barrier_init(&g_group_barrier, nullptr, block_);
    pthread_barrier_wait(&lanes.begin);
    pthread_barrier_wait(&lanes.end);
    pthread_barrier_destroy(&g_group_barrier);
    g_groups_run += grid_;
}
#define hipLaunchKernelGGL(kern, grid, block, shm, stream, ...) host_launch((grid).x, (block).x, [&]() { kern(__VA_ARGS__); })
