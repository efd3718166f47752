// truepeak_engine.hip — the true peak of a delivery (dusp_amd/mix.py true_peak is the contract): for signals [S][C][n]
// f32 on the device, per (signal, channel) the largest |acc| of the row oversampled F times by a polyphase windowed sinc of 49 taps, in
// f64, -ffp-contract=off -fno-fast-math:
//
//     acc = 0.0;  acc = acc + h[p + F k] * f64(x[u - k]),  k = 0 .. K - 1 in that order        (no FMA; x is zero outside [0, n))
//
// for every output position u in [0, n + K - 1) — the filter's tail behind the last sample included — and every phase p in [0, F).  A
// phase whose last tap would lie behind h[48] multiplies by a zero tap like the rest.  One word a row comes out: the bits of the
// largest |acc|, sign cleared, which as UNSIGNED INTEGERS are monotone over the finite values; an accumulator that is not finite (a NaN
// or Inf sample, nothing else: 25 products of f32 values cannot overflow f64) makes the word the quiet NaN, which sorts above every
// finite value.  Integer maxima commute, so the result is exact and the same on every run: no floating-point atomic.
//
// MEMORY.  A workgroup of 256 lanes owns W = 256 x per_lane consecutive output positions [u0, u0 + W) of ONE row (truepeak_plan.hpp
// true_peak_grid picks per_lane).  It loads x[u0 - (K - 1) .. u0 + W) into LDS with 4-byte loads — consecutive lanes consecutive words,
// coalesced; not 16 bytes a lane: a row starts wherever n puts it, on no 16-byte boundary in general — zeros outside [0, n).  Lane l
// then takes u = u0 + l + 256 i, i < per_lane: its K reads for a position are of consecutive words across the lanes (no bank is asked
// twice), and every word read feeds all F phases, F multiply-adds in f64 a read.  The taps come BY VALUE with the kernel's arguments
// and are indexed by constants once the loops are unrolled: they live in scalar registers.  The maximum is kept a lane, then reduced
// in the wave by shuffles, across the four waves through LDS, and ONE 64-bit unsigned atomicMax a workgroup goes to the row's word.
// 8.3 KB of LDS a workgroup ((2048 + 24) floats and four words).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "truepeak_plan.hpp"

namespace dusp {

constexpr unsigned long long kTruePeakInfBits = 0x7ff0000000000000ull, kTruePeakNanBits = 0x7ff8000000000000ull;

// x: [rows][n] floats; workgroup b: tile b % tiles of row b / tiles.  words: [rows], zeroed by the launch
template <int F>
__global__ void __launch_bounds__(kTruePeakLanes) dusp_true_peak_kernel(const float *__restrict__ x, TruePeakTaps taps, uint64_t n, uint64_t tiles, uint32_t per_lane,
                                                                        unsigned long long *__restrict__ words) {
    constexpr uint32_t K = F == 1 ? 1 : (kTruePeakTaps + F - 1) / F;
    __shared__ float tile[kTruePeakLanes * kTruePeakPerLaneMax + kTruePeakHaloMax];
    __shared__ unsigned long long wave_max[kTruePeakLanes / 64];
    const uint32_t t = threadIdx.x, W = kTruePeakLanes * per_lane;
    const uint64_t row = blockIdx.x / tiles, u0 = (blockIdx.x - row * tiles) * W, n_out = n + K - 1;
    const float *r = x + row * n;
    for (uint32_t j = t; j < W + K - 1; j += kTruePeakLanes) {  // tile[j] = x[u0 - (K - 1) + j]
        const uint64_t at = u0 + j;                             // (... + (K - 1): no negative number is formed)
        tile[j] = at >= K - 1 && at - (K - 1) < n ? r[at - (K - 1)] : 0.0f;
    }
    __syncthreads();
    unsigned long long m = 0;
    for (uint32_t i = 0; i < per_lane; i++) {
        const uint32_t o = t + kTruePeakLanes * i;
        if (u0 + o >= n_out) break;  // (behind the tail: the row's last tile)
        double acc[F];
#pragma unroll
        for (int p = 0; p < F; p++) acc[p] = 0.0;
#pragma unroll
        for (uint32_t k = 0; k < K; k++) {
            const double v = (double)tile[o + (K - 1) - k];
#pragma unroll
            for (int p = 0; p < F; p++) {
                const uint32_t j = p + F * k;  // (a constant once unrolled; a padded phase's last tap is a zero)
                const double h = j < kTruePeakTaps ? taps.h[j] : 0.0;
                acc[p] = acc[p] + h * v;
            }
        }
#pragma unroll
        for (int p = 0; p < F; p++) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(acc[p]) & 0x7fffffffffffffffull;
            m = bits > m ? bits : m;
        }
    }
    if (m >= kTruePeakInfBits) m = kTruePeakNanBits;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(m, off);
        m = other > m ? other : m;
    }
    if ((t & 63) == 0) wave_max[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        for (uint32_t w = 1; w < kTruePeakLanes / 64; w++) m = wave_max[w] > m ? wave_max[w] : m;
        if (m) atomicMax(&words[row], m);
    }
}

// The true peaks of d_planar [rows][n] oversampled F times with `taps`: d_words [rows], one 8-byte word a row (true_peak_of_word).
// n >= 1; F is 1, 2 or 4.  The grid must fit 2^31 workgroups (the callers have checked the shapes)
hipError_t launch_true_peak(const float *d_planar, uint64_t rows, uint64_t n, uint32_t F, const TruePeakTaps &taps, int n_cus, uint64_t *d_words, hipStream_t stream) {
    const TruePeakGrid G = true_peak_grid(rows, n, true_peak_phase_taps(F), n_cus);
    if (G.groups > 0x7fffffffull || (F != 1 && F != 2 && F != 4)) return (hipError_t)1;  // (hipErrorInvalidValue)
    hipError_t e = hipMemsetAsync(d_words, 0, rows * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    unsigned long long *words = (unsigned long long *)d_words;
    if (F == 4)
        hipLaunchKernelGGL((dusp_true_peak_kernel<4>), dim3((unsigned)G.groups), dim3(kTruePeakLanes), 0, stream, d_planar, taps, n, G.tiles, G.per_lane, words);
    else if (F == 2)
        hipLaunchKernelGGL((dusp_true_peak_kernel<2>), dim3((unsigned)G.groups), dim3(kTruePeakLanes), 0, stream, d_planar, taps, n, G.tiles, G.per_lane, words);
    else
        hipLaunchKernelGGL((dusp_true_peak_kernel<1>), dim3((unsigned)G.groups), dim3(kTruePeakLanes), 0, stream, d_planar, taps, n, G.tiles, G.per_lane, words);
    return hipGetLastError();
}

}  // namespace dusp
