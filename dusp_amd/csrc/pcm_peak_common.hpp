// pcm_peak_common.hpp — one peak for every signal of a block (a call with stems: its signals are delivered under one gain).  Part of
// pcm_engine.hip, whose peak kernel writes the words this one reads; a header because, unlike the kernels there (LDS, cross-lane
// maxima, atomics), its text runs on the host under tests/native/hip_host_stub (score_stems_kernel_check.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dusp {

constexpr uint32_t kPeakCommonLanes = 64;  // one wavefront

// the n peak words the peak kernel wrote for the block's n instances -> n words, each the unsigned maximum of them all, which the encode
// kernels read as peaks[inst].  Every lane reads the n words (n is a dozen) and writes its own, so there is nothing to share and no atomic
__global__ void __launch_bounds__(kPeakCommonLanes) dusp_pcm_peak_common_kernel(const uint32_t *peaks, uint32_t *common, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < n; k++) {  // (wave-uniform addresses: every lane the same n words)
        const uint32_t w = peaks[k];
        m = w > m ? w : m;
    }
    for (uint32_t i = threadIdx.x; i < n; i += kPeakCommonLanes) common[i] = m;
}

// d_common[i] = the unsigned maximum of d_peaks[0 .. n) for every i < n (peak words are `bits & 0x7fffffff`, any NaN above infinity);
// n >= 1.  d_common is not d_peaks.  (Not inline: pcm_engine.hip is the one file of the library that includes this, and its object has it.)
hipError_t launch_pcm_peak_common(const float *d_peaks, float *d_common, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(dusp_pcm_peak_common_kernel, dim3(1), dim3(kPeakCommonLanes), 0, stream, (const uint32_t *)d_peaks, (uint32_t *)d_common, n);
    return hipGetLastError();
}

}  // namespace dusp
