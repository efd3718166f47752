// limiter_release_engine.hip — the limiter's release of its own (dusp_amd/mix.py limiter_gain_release is the contract):
// between the sliding minimum m and the sliding mean of limiter_engine.hip's curve stands the HELD curve,
//     held[j] = min(m[j], held[j - 1] + d),  d = ceil(ONE / R),
// a recurrence over the whole timeline that is linear in the (min, +) semiring: held[j] = min over i <= j of m[i] + d (j - i).  It is
// cut in time exactly, in integers, by a scan over the tiles in which NO workgroup waits for another of its own launch: what a tile
// needs from before it, a launch that has ended has written.  -ffp-contract=off -fno-fast-math, as limiter_engine.hip.
//
// THREE kernels behind dusp_limit_envelope_kernel (limiter_engine.hip, used as it is), one launch each; a workgroup of 256 lanes owns
// W = 256 x per_lane consecutive positions (limiter_release_plan.hpp limiter_release_grid; the tiles are limiter_grid's).  j' = j + (L - 1)
// counts the positions of m and held from 0 to n + L - 2.
//
//   dusp_limit_hold_kernel<LONG>     tile b: positions [b W, b W + W).  Loads q[b W - (L - 1) .. b W + W + L - 1) into LDS, ONE = 2^30
//       outside [0, n), forms m by the apply kernel's doubling passes between two LDS arrays and writes it to the scratch; and ONE
//       summary word a tile, a_b = min(ONE, min over i of m[i] + d (W - 1 - i)): the tile's held at its last position had nothing
//       come before it.
//   dusp_limit_release_kernel        tile b takes its carry, the held just in front of it, from the summaries of the launch that has
//       ended: c = min(ONE, min over k >= 1 of a_{b-k} + d W (k - 1)), k up to look_back = ceil(ONE / (d W)) + 1 (a term further back is at
//       least ONE) and dealt over the lanes.  Then held[i] = min(P[i] - d (W - 1 - i), c + d (i + 1)) with P the prefix minimum of
//       v[i] = m[i] + d (W - 1 - i) — no negative number appears, everything is below 2^43 — a lane over its per_lane consecutive
//       positions, the lanes of a wavefront by shuffles, the four wavefronts through LDS.  held goes where m was, in place: a tile
//       reads and writes its own positions only.
//   dusp_limit_mean_apply_kernel<LONG>   the apply kernel's second half over held: loads held[s0 .. s0 + W + L - 1) into LDS, the
//       prefix sums in 16-bit halves, sum[s] = P[s + L] - P[s], g = f64(sum) / f64(L x ONE), x = f32(f64(x) x g) for every row in
//       place, one 64-bit atomicMin of the smallest sum (the envelope kernel has set that word to L x ONE).
//
// Everything between the envelope's division and the gain's division is integer: no tiling can change a bit.
// LDS: hold 2 x (W_max + L_max - 1) words, 20.5 KB short and 40.9 KB long; release W_max words + the waves' words, 8.3 KB; mean / apply
// 2 x (W_max + L_max) words + 2 KB, 22.5 KB short and 43 KB long.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "limiter_release_plan.hpp"

namespace dusp {

// the smallest `v` of a workgroup's 256 lanes, for every lane (two barriers; `waves` is the caller's LDS, one word a wavefront)
__device__ __forceinline__ unsigned long long limit_group_min(unsigned long long v, unsigned long long *waves) {
    const uint32_t t = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(v, off);
        v = other < v ? other : v;
    }
    __syncthreads();  // (what the last use of `waves` read)
    if ((t & 63) == 0) waves[t >> 6] = v;
    __syncthreads();
    v = waves[0];
    for (uint32_t w = 1; w < kTruePeakLanes / 64; w++) v = waves[w] < v ? waves[w] : v;
    return v;
}

// q: [n]; m: [n + L - 1], position j' holds min(q[j' - (L - 1) .. j']); summary: one word a tile.  LONG as dusp_limit_apply_kernel's
template <bool LONG>
__global__ void __launch_bounds__(kTruePeakLanes) dusp_limit_hold_kernel(const uint32_t *__restrict__ q, uint64_t n, uint32_t L, uint32_t per_lane, uint32_t d, uint32_t *__restrict__ m,
                                                                         uint32_t *__restrict__ summary) {
    constexpr uint32_t kPerLaneMax = LONG ? kLimiterPerLaneLong : kTruePeakPerLaneMax;
    constexpr uint32_t kWords = kTruePeakLanes * kPerLaneMax + (LONG ? kLimiterWindowMax : kLimiterWindowShort) - 1;
    __shared__ uint32_t lds[2 * kWords];  // two arrays: a pass reads one and writes the other
    __shared__ unsigned long long waves[kTruePeakLanes / 64];
    const uint32_t t = threadIdx.x, W = kTruePeakLanes * per_lane, N = W + L - 1;
    const uint64_t j0 = (uint64_t)blockIdx.x * W, positions = n + L - 1;
    uint32_t src = 0, dst = kWords;
    for (uint32_t j = t; j < N; j += kTruePeakLanes) {  // a[j] = q[j0 - (L - 1) + j], ONE outside [0, n)
        const uint64_t at = j0 + j;
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
    unsigned long long least = kLimiterOne;
    for (uint32_t j = t; j < W; j += kTruePeakLanes) {  // m[j] = min(a[j .. j + L - 1]): two windows of `step`, j + L - 1 <= N - 1
        const uint32_t v = lds[src + j], w = lds[src + j + (L - step)], least_of = w < v ? w : v;
        if (j0 + j < positions) m[j0 + j] = least_of;  // (behind the last position the word is ONE: no part in the summary)
        const unsigned long long reach = least_of + (unsigned long long)d * (W - 1 - j);
        least = reach < least ? reach : least;
    }
    least = limit_group_min(least, waves);
    if (t == 0) summary[blockIdx.x] = (uint32_t)least;  // (at most ONE)
}

// held: [positions], m before and the held curve after; summary: the hold launch's, one word a tile
__global__ void __launch_bounds__(kTruePeakLanes) dusp_limit_release_kernel(uint32_t *__restrict__ held, const uint32_t *__restrict__ summary, uint64_t positions, uint32_t per_lane, uint32_t d,
                                                                            uint32_t look_back) {
    __shared__ uint32_t tile[kTruePeakLanes * kTruePeakPerLaneMax];
    __shared__ unsigned long long waves[kTruePeakLanes / 64];
    const uint32_t t = threadIdx.x, W = kTruePeakLanes * per_lane, b = blockIdx.x;
    const uint64_t j0 = (uint64_t)b * W;
    for (uint32_t j = t; j < W; j += kTruePeakLanes) tile[j] = j0 + j < positions ? held[j0 + j] : kLimiterOne;
    // the carry: the held curve just in front of the tile, from the tiles that can still reach it
    const unsigned long long dW = (unsigned long long)d * W;
    unsigned long long c = kLimiterOne;
    const uint32_t back = b < look_back ? b : look_back;
    for (uint32_t k = 1 + t; k <= back; k += kTruePeakLanes) {
        const unsigned long long reach = summary[b - k] + dW * (k - 1);
        c = reach < c ? reach : c;
    }
    c = limit_group_min(c, waves);  // (its barriers stand behind the tile's load too)
    // P: the prefix minimum of v[i] = m[i] + d (W - 1 - i); lane t has the positions [t per_lane, t per_lane + per_lane)
    const uint32_t begin = t * per_lane;
    unsigned long long own = ~0ull;
    for (uint32_t k = 0; k < per_lane; k++) {
        const unsigned long long v = tile[begin + k] + (unsigned long long)d * (W - 1 - (begin + k));
        own = v < own ? v : own;
    }
    unsigned long long upto = own;  // the minimum over this lane and the lanes below it in its wavefront
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long other = __shfl_up(upto, off);
        if ((t & 63) >= (uint32_t)off && other < upto) upto = other;
    }
    unsigned long long before = __shfl_up(upto, 1);  // ... over the lanes below it alone
    if ((t & 63) == 0) before = ~0ull;
    __syncthreads();  // (limit_group_min's last read of `waves`)
    if ((t & 63) == 63) waves[t >> 6] = upto;
    __syncthreads();
    for (uint32_t w = 0; w < (t >> 6); w++) before = waves[w] < before ? waves[w] : before;
    for (uint32_t k = 0; k < per_lane; k++) {
        const uint32_t i = begin + k;
        const unsigned long long v = tile[i] + (unsigned long long)d * (W - 1 - i);
        before = v < before ? v : before;
        const unsigned long long own_reach = before - (unsigned long long)d * (W - 1 - i), carried = c + (unsigned long long)d * (i + 1);
        tile[i] = (uint32_t)(own_reach < carried ? own_reach : carried);  // (at most m[i]: no other lane reads this word)
    }
    __syncthreads();
    for (uint32_t j = t; j < W; j += kTruePeakLanes)
        if (j0 + j < positions) held[j0 + j] = tile[j];
}

// x: [rows][n] floats, limited in place; held: [n + L - 1]; smallest: one word, L x ONE before the launch; gain: [n] or NULL, the curve
template <bool LONG>
__global__ void __launch_bounds__(kTruePeakLanes) dusp_limit_mean_apply_kernel(float *__restrict__ x, const uint32_t *__restrict__ held, uint64_t rows, uint64_t n, uint32_t L, uint32_t per_lane,
                                                                               unsigned long long *__restrict__ smallest, double *__restrict__ gain) {
    constexpr uint32_t kPerLaneMax = LONG ? kLimiterPerLaneLong : kTruePeakPerLaneMax;
    constexpr uint32_t kWords = kTruePeakLanes * kPerLaneMax + (LONG ? kLimiterWindowMax : kLimiterWindowShort);
    __shared__ uint32_t lds[2 * kWords];
    __shared__ unsigned long long wave_min[kTruePeakLanes / 64];
    __shared__ uint32_t lane_lo[kTruePeakLanes], lane_hi[kTruePeakLanes];
    const uint32_t t = threadIdx.x, W = kTruePeakLanes * per_lane, M = W + L - 1;
    const uint64_t s0 = (uint64_t)blockIdx.x * W, positions = n + L - 1;
    const uint32_t src = 0, dst = kWords;
    for (uint32_t j = t; j < M; j += kTruePeakLanes) lds[dst + j] = s0 + j < positions ? held[s0 + j] : kLimiterOne;
    __syncthreads();
    // the sliding sum as differences of a prefix sum over held — exact: held = hi x 2^16 + lo, and the prefix sums of the halves fit
    // 32 bits (at most 5119 terms below 2^16 and 2^15).  Lane t sums held[t c .. t c + c), the lanes' totals are put in order through
    // LDS, and the lane walks its c words again: P_lo[i] goes to the other array, P_hi[i] over held[i] itself, which no other lane reads
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
    if (end == M && begin < M) lds[src + M] = lo, lds[dst + M] = hi;  // (M + 1 <= kWords)
    __syncthreads();
    unsigned long long sum[kPerLaneMax];
#pragma unroll
    for (uint32_t i = 0; i < kPerLaneMax; i++) {  // sum of held[o .. o + L - 1] = P[o + L] - P[o], o + L <= M
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

static bool limit_release_shape(const LimiterReleaseGrid &P, uint32_t L, uint32_t R) {
    return P.tiles <= 0x7fffffffull && P.hold_tiles <= 0x7fffffffull && L >= 1 && L <= kLimiterWindowMax && R >= 1 && R <= kLimiterReleaseMax;
}

// The minima of d_q [n] over a window of L -> d_held [n + L - 1], and a summary a hold tile -> d_summary, for a release of R samples
hipError_t launch_limit_hold(uint64_t n, uint32_t L, uint32_t R, int n_cus, const uint32_t *d_q, uint32_t *d_held, uint32_t *d_summary, hipStream_t stream) {
    const LimiterReleaseGrid P = limiter_release_grid(n, L, R, n_cus);
    if (!limit_release_shape(P, L, R)) return (hipError_t)1;  // (hipErrorInvalidValue)
    if (L > kLimiterWindowShort)
        hipLaunchKernelGGL((dusp_limit_hold_kernel<true>), dim3((unsigned)P.hold_tiles), dim3(kTruePeakLanes), 0, stream, d_q, n, L, P.per_lane, P.d, d_held, d_summary);
    else
        hipLaunchKernelGGL((dusp_limit_hold_kernel<false>), dim3((unsigned)P.hold_tiles), dim3(kTruePeakLanes), 0, stream, d_q, n, L, P.per_lane, P.d, d_held, d_summary);
    return hipGetLastError();
}

// d_held: the minima -> the held curve, in place, by the summaries of the hold launch that has ended
hipError_t launch_limit_release(uint64_t n, uint32_t L, uint32_t R, int n_cus, uint32_t *d_held, const uint32_t *d_summary, hipStream_t stream) {
    const LimiterReleaseGrid P = limiter_release_grid(n, L, R, n_cus);
    if (!limit_release_shape(P, L, R)) return (hipError_t)1;
    hipLaunchKernelGGL(dusp_limit_release_kernel, dim3((unsigned)P.hold_tiles), dim3(kTruePeakLanes), 0, stream, d_held, d_summary, P.positions, P.per_lane, P.d, P.look_back);
    return hipGetLastError();
}

// d_planar [rows][n] limited in place by the mean of d_held over L; *d_smallest, L x ONE before, takes the smallest sum; d_gain: [n] or NULL
hipError_t launch_limit_mean_apply(float *d_planar, uint64_t rows, uint64_t n, uint32_t L, int n_cus, const uint32_t *d_held, uint64_t *d_smallest, double *d_gain, hipStream_t stream) {
    const LimiterGrid G = limiter_grid(n, L, n_cus);
    if (G.tiles > 0x7fffffffull || L < 1 || L > kLimiterWindowMax) return (hipError_t)1;
    unsigned long long *word = (unsigned long long *)d_smallest;
    if (L > kLimiterWindowShort)
        hipLaunchKernelGGL((dusp_limit_mean_apply_kernel<true>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, d_held, rows, n, L, G.per_lane, word, d_gain);
    else
        hipLaunchKernelGGL((dusp_limit_mean_apply_kernel<false>), dim3((unsigned)G.tiles), dim3(kTruePeakLanes), 0, stream, d_planar, d_held, rows, n, L, G.per_lane, word, d_gain);
    return hipGetLastError();
}

}  // namespace dusp
