// limiter_engine.hip — the linked look-ahead true-peak limiter of a delivery (dusp_amd/mix.py limiter_envelope, limiter_gain and limit
// are the contract): ONE gain curve g[s] for signals [S][C][n] f32 on the device, made from the largest oversampled
// magnitude of ANY row around sample s and applied to every row in place.  -ffp-contract=off -fno-fast-math, as truepeak_engine.hip.
//
// TWO kernels, one launch each, over the same tiles: a workgroup of 256 lanes owns W = 256 x per_lane consecutive samples [s0, s0 + W)
// of the timeline (limiter_plan.hpp limiter_grid) and loops over the rows itself, so what is reduced over the rows stays in registers
// and no atomic is needed for it.
//
//   dusp_limit_envelope_kernel<F>   for every row the true-peak kernel's accumulators at u = s + D (D = (K - 1) / 2, the interpolator's
//       delay): acc = 0.0, acc = acc + h[p + F k] * f64(x[u - k]), k ascending, no FMA, x zero outside [0, n), from an LDS tile of
//       x[s0 + D - (K - 1) .. s0 + D + W) loaded with 4-byte coalesced loads.  A lane keeps, a position, the largest |acc| of all rows
//       and phases as unsigned bits; an |acc| that is not finite contributes nothing.  After the last row: r = T / e where e > T, else
//       1 — one f64 division — and q = floor(r x 2^30), one 32-bit word a sample.
//   dusp_limit_apply_kernel<LONG>   loads q[s0 - (L - 1) .. s0 + W + L - 1) into LDS, ONE = 2^30 outside [0, n); the sliding minimum
//       over L by doubling passes a'[i] = min(a[i], a[i + 2^k]) between two LDS arrays (no pass reads what it writes), then two
//       overlapping windows of 2^p = the largest power of two <= L; the sliding sum over L of the minima as the difference of two
//       entries of a prefix sum over the tile's minima, exact in integers (the minima split into 16-bit halves whose prefix sums fit
//       32 bits), four LDS reads a sample whatever L; g = f64(sum) / f64(L x ONE); then for every row
//       x = f32(f64(x) x g) in place, consecutive lanes consecutive samples.  The smallest sum of a workgroup goes to ONE word by a
//       64-bit unsigned atomicMin (integer minima commute: the word is exact and the same on every run); the envelope kernel's first
//       lane has set that word to L x ONE.
//
// Everything between the envelope's division and the gain's division is integer: no tiling can change a bit.
// LDS: the envelope (2048 + 24) floats, 8.3 KB; the gain kernel 2 x (W_max + 2 (L_max - 1)) words — 24.6 KB with L <= 512 and tiles up
// to 2048 samples, 73.7 KB with L <= 4096 and tiles up to 1024 — and 2 KB for the lanes' totals: two workgroups a CU of 160 KB.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "limiter_plan.hpp"

namespace dusp {

// x: [rows][n] floats; workgroup b: samples [b W, b W + W) of every row.  q: [n].  smallest: the apply kernel's word, set here
template <int F>
__global__ void __launch_bounds__(kTruePeakLanes) dusp_limit_envelope_kernel(const float *__restrict__ x, TruePeakTaps taps, uint64_t rows, uint64_t n, uint32_t per_lane, double T,
                                                                             uint32_t L, uint32_t *__restrict__ q, unsigned long long *__restrict__ smallest) {
    constexpr uint32_t K = F == 1 ? 1 : (kTruePeakTaps + F - 1) / F, D = (K - 1) / 2;
    __shared__ float tile[kTruePeakLanes * kTruePeakPerLaneMax + kTruePeakHaloMax];
    const uint32_t t = threadIdx.x, W = kTruePeakLanes * per_lane;
    const uint64_t s0 = (uint64_t)blockIdx.x * W;
    if (blockIdx.x == 0 && t == 0) *smallest = (unsigned long long)L * kLimiterOne;
    unsigned long long best[kTruePeakPerLaneMax];
#pragma unroll
    for (uint32_t i = 0; i < kTruePeakPerLaneMax; i++) best[i] = 0;
    for (uint64_t row = 0; row < rows; row++) {
        const float *r = x + row * n;
        __syncthreads();                                            // (the row before has been read)
        for (uint32_t j = t; j < W + K - 1; j += kTruePeakLanes) {  // tile[j] = x[s0 + D - (K - 1) + j], zero outside the ROW
            const uint64_t at = s0 + D + j;                         // (... + (K - 1): no negative number is formed)
            tile[j] = at >= K - 1 && at - (K - 1) < n ? r[at - (K - 1)] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kTruePeakPerLaneMax; i++) {
            const uint32_t o = t + kTruePeakLanes * i;
            if (i >= per_lane || s0 + o >= n) break;
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
                if (bits < 0x7ff0000000000000ull && bits > best[i]) best[i] = bits;  // (not finite: no part in the envelope)
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kTruePeakPerLaneMax; i++) {
        const uint64_t s = s0 + t + kTruePeakLanes * i;
        if (i >= per_lane || s >= n) break;
        const double e = __longlong_as_double((long long)best[i]);
        const double ratio = e > T ? T / e : 1.0;
        q[s] = (uint32_t)(ratio * (double)kLimiterOne);  // (0 <= ratio <= 1: the conversion is the floor)
    }
}

// x: [rows][n] floats, limited in place; q: [n]; smallest: one word, L x ONE before the launch; gain: [n] or NULL, the curve.  LONG: L up to 4096 and tiles up to
// 256 x kLimiterPerLaneLong samples; else L up to kLimiterWindowShort and tiles up to 2048
template <bool LONG>
__global__ void __launch_bounds__(kTruePeakLanes) dusp_limit_apply_kernel(float *__restrict__ x, const uint32_t *__restrict__ q, uint64_t rows, uint64_t n, uint32_t L, uint32_t per_lane,
                                                                          unsigned long long *__restrict__ smallest, double *__restrict__ gain) {
    constexpr uint32_t kPerLaneMax = LONG ? kLimiterPerLaneLong : kTruePeakPerLaneMax;
    constexpr uint32_t kWords = kTruePeakLanes * kPerLaneMax + 2 * ((LONG ? kLimiterWindowMax : kLimiterWindowShort) - 1);
    __shared__ uint32_t lds[2 * kWords];  // two arrays: a pass reads one and writes the other
    __shared__ unsigned long long wave_min[kTruePeakLanes / 64];
    __shared__ uint32_t lane_lo[kTruePeakLanes], lane_hi[kTruePeakLanes];
    const uint32_t t = threadIdx.x, W = kTruePeakLanes * per_lane, N = W + 2 * (L - 1), M = W + L - 1;
    const uint64_t s0 = (uint64_t)blockIdx.x * W;
    uint32_t src = 0, dst = kWords;
    for (uint32_t j = t; j < N; j += kTruePeakLanes) {  // a[j] = q[s0 - (L - 1) + j], ONE outside [0, n)
        const uint64_t at = s0 + j;
        lds[src + j] = at >= L - 1 && at - (L - 1) < n ? q[at - (L - 1)] : kLimiterOne;
    }
    __syncthreads();
    uint32_t step = 1;  // src[i] = min(a[i .. i + step - 1]) wherever that window lies inside a
    for (; 2 * step <= L; step *= 2) {
        for (uint32_t j = t; j < N; j += kTruePeakLanes) {
            const uint32_t v = lds[src + j], w = j + step < N ? lds[src + j + step] : v;
            lds[dst + j] = w < v ? w : v;
        }
        __syncthreads();
        const uint32_t was = src;
        src = dst, dst = was;
    }
    for (uint32_t j = t; j < M; j += kTruePeakLanes) {  // m[j] = min(a[j .. j + L - 1]): two windows of `step`, j + L - step + step - 1 <= N - 1
        const uint32_t v = lds[src + j], w = lds[src + j + (L - step)];
        lds[dst + j] = w < v ? w : v;
    }
    __syncthreads();
    // the sliding sum as differences of a prefix sum over m — exact: m = hi x 2^16 + lo, and the prefix sums of the halves fit 32 bits
    // (at most 6143 terms below 2^16 and 2^15).  Lane t sums m[t c .. t c + c), the lanes' totals are put in order through LDS, and
    // the lane walks its c words again: P_lo[i] goes where the last pass read from, P_hi[i] over m[i] itself, which no other lane reads
    const uint32_t c = (M + kTruePeakLanes - 1) / kTruePeakLanes, begin = t * c < M ? t * c : M, end = begin + c < M ? begin + c : M;
    uint32_t lo = 0, hi = 0;
    for (uint32_t j = begin; j < end; j++) {
        const uint32_t v = lds[dst + j];
        lo += v & 0xffffu, hi += v >> 16;
    }
    lane_lo[t] = lo, lane_hi[t] = hi;
    __syncthreads();
    lo = 0, hi = 0;
    for (uint32_t j = 0; j < t; j++) lo += lane_lo[j], hi += lane_hi[j];  // (every lane reads the same word: a broadcast)
    for (uint32_t j = begin; j < end; j++) {
        const uint32_t v = lds[dst + j];
        lds[src + j] = lo, lds[dst + j] = hi;
        lo += v & 0xffffu, hi += v >> 16;
    }
    if (end == M && begin < M) lds[src + M] = lo, lds[dst + M] = hi;  // (M + 1 <= kWords: the windows' caps are above 1)
    __syncthreads();
    unsigned long long sum[kPerLaneMax];
#pragma unroll
    for (uint32_t i = 0; i < kPerLaneMax; i++) {  // sum of m[o .. o + L - 1] = P[o + L] - P[o], o + L <= M
        sum[i] = 0;
        if (i >= per_lane) break;
        const uint32_t o = t + kTruePeakLanes * i;
        sum[i] = ((unsigned long long)(lds[dst + o + L] - lds[dst + o]) << 16) + (lds[src + o + L] - lds[src + o]);
    }
    unsigned long long least = (unsigned long long)L * kLimiterOne;
    double g[kPerLaneMax];
#pragma unroll
    for (uint32_t i = 0; i < kPerLaneMax; i++) {
        g[i] = 1.0;
        if (i >= per_lane || s0 + t + kTruePeakLanes * i >= n) break;
        least = sum[i] < least ? sum[i] : least;
        g[i] = (double)sum[i] / (double)((unsigned long long)L * kLimiterOne);
        if (gain) gain[s0 + t + kTruePeakLanes * i] = g[i];
    }
    for (uint64_t row = 0; row < rows; row++) {
        float *r = x + row * n;
#pragma unroll
        for (uint32_t i = 0; i < kPerLaneMax; i++) {
            const uint64_t s = s0 + t + kTruePeakLanes * i;
            if (i >= per_lane || s >= n) break;
            r[s] = (float)((double)r[s] * g[i]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(least, off);
        least = other < least ? other : least;
    }
    if ((t & 63) == 0) wave_min[t >> 6] = least;
    __syncthreads();
    if (t == 0) {
        for (uint32_t w = 1; w < kTruePeakLanes / 64; w++) least = wave_min[w] < least ? wave_min[w] : least;
        if (least < (unsigned long long)L * kLimiterOne) atomicMin(smallest, least);
    }
}

// The envelope's words of d_planar [rows][n] oversampled F times with `taps`, against the threshold T: d_q [n]; *d_smallest = L x ONE.
// n >= 1, 1 <= L <= 4096, F is 1, 2 or 4 (the callers have checked the shapes)
hipError_t launch_limit_envelope(const float *d_planar, uint64_t rows, uint64_t n, uint32_t F, const TruePeakTaps &taps, double T, uint32_t L, int n_cus, uint32_t *d_q,
                                 uint64_t *d_smallest, hipStream_t stream) {
    const LimiterGrid G = limiter_grid(n, L, n_cus);
    if (G.tiles > 0x7fffffffull || (F != 1 && F != 2 && F != 4) || L < 1 || L > kLimiterWindowMax) return (hipError_t)1;  // (hipErrorInvalidValue)
    unsigned long long *word = (unsigned long long *)d_smallest;
    if (F == 4)
        hipLaunchKernelGGL((dusp_limit_envelope_kernel<4>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, taps, rows, n, G.per_lane, T, L, d_q, word);
    else if (F == 2)
        hipLaunchKernelGGL((dusp_limit_envelope_kernel<2>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, taps, rows, n, G.per_lane, T, L, d_q, word);
    else
        hipLaunchKernelGGL((dusp_limit_envelope_kernel<1>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, taps, rows, n, G.per_lane, T, L, d_q, word);
    return hipGetLastError();
}

// d_planar [rows][n] limited in place by the curve d_q gives over a window of L; *d_smallest, L x ONE before, takes the smallest sum;
// d_gain: [n] doubles or NULL, the curve itself
hipError_t launch_limit_apply(float *d_planar, uint64_t rows, uint64_t n, uint32_t L, int n_cus, const uint32_t *d_q, uint64_t *d_smallest, double *d_gain, hipStream_t stream) {
    const LimiterGrid G = limiter_grid(n, L, n_cus);
    if (G.tiles > 0x7fffffffull || L < 1 || L > kLimiterWindowMax) return (hipError_t)1;
    unsigned long long *word = (unsigned long long *)d_smallest;
    if (L > kLimiterWindowShort)
        hipLaunchKernelGGL((dusp_limit_apply_kernel<true>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, d_q, rows, n, L, G.per_lane, word, d_gain);
    else
        hipLaunchKernelGGL((dusp_limit_apply_kernel<false>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, d_q, rows, n, L, G.per_lane, word, d_gain);
    return hipGetLastError();
}

}  // namespace dusp
