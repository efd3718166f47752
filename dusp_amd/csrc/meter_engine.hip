// meter_engine.hip — the meters of a delivery (dusp_amd/mix.py meters is the contract): for signals [S][C][n] f32 on the
// device, the sum of squares of every (signal, channel) in f64, and per (signal, hop of 100 ms) the sum over the channels of z^2, z the
// channel through the K-weighting of ITU-R BS.1770-4 — two biquad sections, direct form I, f64, -ffp-contract=off -fno-fast-math:
//
//     y = b0 x + b1 x1 + b2 x2 - a1 y1 - a2 y2        z = c0 y + c1 y1 + c2 y2 - d1 z1 - d2 z2        (left to right, no FMA)
//
// THE CUT IN TIME.  The K-weighting has constant coefficients: it is linear and time-invariant, so its state at the end of a stretch of
// L samples is  M_L s + zs,  s the state (x1, x2, y1, y2, z1, z2) at the stretch's start (six doubles: the second section's input
// history is the first's output history), M_L the 6 x 6 zero-input transition over L samples and zs what the stretch's own samples
// leave behind from rest.  Exact in exact arithmetic; in f64 the roundings differ from the one sequential loop's, by what
// tests/test_gpu_meters.py bounds.  A row (one channel of one signal) is cut into segments of L samples, the last one shorter; L divides
// the hop (or is the hop), so no segment straddles a hop boundary.
//
//   pass A   dusp_meter_pass_kernel<false>: a lane runs its segment from rest and stores zs.
//   combine  dusp_meter_combine_kernel: one lane a row walks the row's segments in order, s_{j+1} = M_L s_j + zs_j, and stores every
//            segment's true initial state s_j.  M_L is made on the host (launch_meter) and passed BY VALUE; its sixteen entries that
//            are zero whatever the coefficients (meter_advance) are not multiplied.  The last segment of a
//            row may be shorter; nothing follows it, so its end state is never formed and it needs no matrix of its own.
//   pass B   dusp_meter_pass_kernel<true>: a lane reruns its segment from s_j and stores the segment's sum of z^2 and of f64(x)^2.
//   reduce   dusp_meter_hop_kernel: one lane a (row, hop) adds the hop's segments in segment order; dusp_meter_sum_kernel: one lane a
//            (signal, hop) adds the rows' hop sums in channel order -> d_hops, and one lane a row adds its hops' sums of x^2 in hop
//            order -> d_sumsq.  A fixed order throughout and no floating-point atomic: two runs give the same bits.
//
// MEMORY.  Lanes a segment apart read addresses 4 L bytes apart.  A workgroup owns 256 consecutive segments and moves them through LDS
// 32 samples a row at a time: the tile is [256][33] floats (the pad keeps the lanes' row reads off one bank), filled by loads in which
// 32 consecutive lanes read 128 consecutive bytes of one row, and then every lane reads its own row; the next slice is loaded into
// registers while the lanes run through the one in the tile.  The loads are 4 bytes a lane, not
// 16: rows start wherever n and L put them, on no 16-byte boundary in general, and the pass is bound by the lanes' dependent f64
// chains, not by the loads' issue (profiles/score_meters.txt).  The rows' start and length are worked out once a lane (one 64-bit
// division) and shared through LDS.  37 KB of LDS a workgroup.  No cross-lane operation but the barriers around the tile.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "meter_plan.hpp"

namespace dusp {

// one sample through both sections, every operation rounded by itself
static __device__ __forceinline__ double meter_step(const MeterCoef &k, double x, double &x1, double &x2, double &y1, double &y2, double &z1, double &z2) {
    const double y = k.s[0][0] * x + k.s[0][1] * x1 + k.s[0][2] * x2 - k.s[0][3] * y1 - k.s[0][4] * y2;
    const double z = k.s[1][0] * y + k.s[1][1] * y1 + k.s[1][2] * y2 - k.s[1][3] * z1 - k.s[1][4] * z2;
    x2 = x1;
    x1 = x;
    y2 = y1;
    y1 = y;
    z2 = z1;
    z1 = z;
    return z;
}

// x: [rows][n] floats.  Segment g (of n_segs = rows * n_seg) is segment g % n_seg of row g / n_seg: its samples [j L, min(n, (j + 1) L)).
// PASS_B false: from rest, state[g][6] = the end state.  PASS_B true: from state[g][6], part[g] = sum z^2, part[n_segs + g] = sum x^2.
template <bool PASS_B>
__global__ void __launch_bounds__(kMeterLanes) dusp_meter_pass_kernel(const float *__restrict__ x, MeterCoef k, uint64_t n, uint32_t L, uint64_t n_seg, uint64_t n_segs,
                                                                       double *__restrict__ state, double *__restrict__ part) {
    __shared__ float tile[kMeterLanes][kMeterSlice + 1];
    __shared__ uint64_t row_at[kMeterLanes];   // where the row's first sample lies in x
    __shared__ uint32_t row_len[kMeterLanes];  // its samples: 0 behind the last segment
    const uint32_t t = threadIdx.x;
    const uint64_t g = (uint64_t)blockIdx.x * kMeterLanes + t;
    uint32_t len = 0;
    if (g < n_segs) {
        const uint64_t row = g / n_seg, first = (g - row * n_seg) * L;
        len = n - first < L ? (uint32_t)(n - first) : L;
        row_at[t] = row * n + first;
    } else {
        row_at[t] = 0;
    }
    row_len[t] = len;
    double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0, z1 = 0.0, z2 = 0.0, sum_z = 0.0, sum_x = 0.0;
    if (PASS_B && g < n_segs) {
        const double *s = state + g * 6;
        x1 = s[0], x2 = s[1], y1 = s[2], y2 = s[3], z1 = s[4], z2 = s[5];
    }
    __syncthreads();
    // (a lane moves column t % 32 of the rows t / 32, t / 32 + 8, ...: 32 lanes a row, 128 consecutive bytes.  The next slice is on its
    // way from memory, in registers, while the lanes run through this one.)
    constexpr uint32_t kRowStep = kMeterLanes / kMeterSlice, kPerLane = kMeterLanes / kRowStep;  // a lane moves every 8th row: 32 values a slice
    const uint32_t col = t % kMeterSlice, row0 = t / kMeterSlice;
    float stage[kPerLane];
#pragma unroll
    for (uint32_t i = 0; i < kPerLane; i++) {
        const uint32_t r = row0 + i * kRowStep;
        stage[i] = col < row_len[r] ? x[row_at[r] + col] : 0.0f;
    }
    for (uint32_t at = 0; at < L; at += kMeterSlice) {
#pragma unroll
        for (uint32_t i = 0; i < kPerLane; i++) tile[row0 + i * kRowStep][col] = stage[i];
        __syncthreads();
        if (at + kMeterSlice < L) {
            const uint32_t next = at + kMeterSlice + col;
#pragma unroll
            for (uint32_t i = 0; i < kPerLane; i++) {
                const uint32_t r = row0 + i * kRowStep;
                stage[i] = next < row_len[r] ? x[row_at[r] + next] : 0.0f;
            }
        }
        const uint32_t m = len > at ? (len - at < kMeterSlice ? len - at : kMeterSlice) : 0;
        for (uint32_t i = 0; i < m; i++) {
            const double v = (double)tile[t][i];
            const double z = meter_step(k, v, x1, x2, y1, y2, z1, z2);
            if (PASS_B) {
                sum_z = sum_z + z * z;
                sum_x = sum_x + v * v;
            }
        }
        __syncthreads();
    }
    if (g >= n_segs) return;
    if (PASS_B) {
        part[g] = sum_z;
        part[n_segs + g] = sum_x;
    } else {
        double *s = state + g * 6;
        s[0] = x1, s[1] = x2, s[2] = y1, s[3] = y2, s[4] = z1, s[5] = z2;
    }
}

// s = M s + zs, the products added left to right.  Over L >= 2 samples of silence the input history is silence, so rows 0 and 1 of M are
// exactly zero, and the first section never hears the second, so are columns 4 and 5 of rows 2 and 3: 20 products, not 36.
static __device__ __forceinline__ void meter_advance(const MeterMatrix &M, double (&s)[6], const double (&zs)[6]) {
    double next[6];
    next[0] = zs[0];
    next[1] = zs[1];
#pragma unroll
    for (int i = 2; i < 6; i++) {
        double acc = M.m[i][0] * s[0];
#pragma unroll
        for (int c = 1; c < (i < 4 ? 4 : 6); c++) acc = acc + M.m[i][c] * s[c];
        next[i] = acc + zs[i];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) s[i] = next[i];
}

// zs: [rows][n_seg][6] what every segment leaves from rest -> init: [rows][n_seg][6] every segment's true initial state.  One lane a row;
// the segments' records are read kMeterBatch ahead of the chain that needs them.  init is not zs.
__global__ void __launch_bounds__(64) dusp_meter_combine_kernel(const double *__restrict__ zs, double *__restrict__ init, MeterMatrix M, uint64_t n_seg, uint32_t rows) {
    const uint32_t row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const double *in = zs + (uint64_t)row * n_seg * 6;
    double *out = init + (uint64_t)row * n_seg * 6;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint64_t j = 0;
    double cur[kMeterBatch][6], ahead[kMeterBatch][6];
    if (kMeterBatch <= n_seg) {
#pragma unroll
        for (uint32_t b = 0; b < kMeterBatch; b++)
#pragma unroll
            for (int i = 0; i < 6; i++) cur[b][i] = in[b * 6 + i];
    }
    for (; j + kMeterBatch <= n_seg; j += kMeterBatch) {
        const bool more = j + 2 * kMeterBatch <= n_seg;  // (the next batch is on its way while the chain runs through this one)
        if (more) {
#pragma unroll
            for (uint32_t b = 0; b < kMeterBatch; b++)
#pragma unroll
                for (int i = 0; i < 6; i++) ahead[b][i] = in[(j + kMeterBatch + b) * 6 + i];
        }
#pragma unroll
        for (uint32_t b = 0; b < kMeterBatch; b++) {
#pragma unroll
            for (int i = 0; i < 6; i++) out[(j + b) * 6 + i] = s[i];
            meter_advance(M, s, cur[b]);
        }
        if (more) {
#pragma unroll
            for (uint32_t b = 0; b < kMeterBatch; b++)
#pragma unroll
                for (int i = 0; i < 6; i++) cur[b][i] = ahead[b][i];
        }
    }
    for (; j < n_seg; j++) {
        double left[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            out[j * 6 + i] = s[i];
            left[i] = in[j * 6 + i];
        }
        meter_advance(M, s, left);
    }
}

// part: [2][rows][n_seg] the segments' sums (z^2, then x^2) -> per_hop: [2][rows][n_hops], every hop's segments added in segment order.
// One lane a (kind, row, hop); per: the segments of a whole hop.
__global__ void __launch_bounds__(256) dusp_meter_hop_kernel(const double *__restrict__ part, double *__restrict__ per_hop, uint64_t n_seg, uint64_t n_hops, uint32_t per,
                                                             uint64_t items) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const uint64_t kr = i / n_hops, h = i - kr * n_hops;  // (kr: kind * rows + row)
    const uint64_t lo = h * per, hi = lo + per < n_seg ? lo + per : n_seg;
    const double *p = part + kr * n_seg;
    double acc = 0.0;
    for (uint64_t j = lo; j < hi; j++) acc = acc + p[j];
    per_hop[i] = acc;
}

// per_hop: [2][rows][n_hops], rows = n_signals * n_channels -> hops[s][h] = the channels' z^2 sums added in channel order (lanes below
// n_signals * n_hops), and sumsq[row] = the row's x^2 sums added in hop order (the rows lanes behind them)
__global__ void __launch_bounds__(256) dusp_meter_sum_kernel(const double *__restrict__ per_hop, double *__restrict__ hops, double *__restrict__ sumsq, uint32_t n_signals,
                                                             uint32_t n_channels, uint64_t n_hops) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, n_first = (uint64_t)n_signals * n_hops, rows = (uint64_t)n_signals * n_channels;
    if (i < n_first) {
        const uint64_t s = i / n_hops, h = i - s * n_hops;
        double acc = 0.0;
        for (uint32_t c = 0; c < n_channels; c++) acc = acc + per_hop[(s * n_channels + c) * n_hops + h];
        hops[i] = acc;
    } else if (i - n_first < rows) {
        const double *p = per_hop + (rows + (i - n_first)) * n_hops;
        double acc = 0.0;
        for (uint64_t h = 0; h < n_hops; h++) acc = acc + p[h];
        sumsq[i - n_first] = acc;
    }
}

// The meters of d_planar [n_signals][n_channels][n] at `hop` samples a hop: d_sumsq f64 [n_signals][n_channels], d_hops f64
// [n_signals][ceil(n / hop)]; d_scratch: meter_geometry(...).doubles doubles.  n >= 1; the segments must fit a grid (the callers have
// checked).  marks (optional): five events, recorded in front of pass A and behind pass A, the combine, pass B and the reduction, for
// a call that is timed pass by pass.
hipError_t launch_meter(const float *d_planar, uint32_t n_signals, uint32_t n_channels, uint64_t n, uint32_t hop, const MeterCoef &k, double *d_scratch, double *d_sumsq,
                        double *d_hops, hipStream_t stream, hipEvent_t *marks) {
    const uint64_t rows = (uint64_t)n_signals * n_channels;
    const MeterGeometry G = meter_geometry(rows, n, hop);
    const uint64_t groups = (G.n_segs + kMeterLanes - 1) / kMeterLanes;
    if (groups > 0x7fffffffull || rows > 0x7fffffffull) return (hipError_t)1;  // (hipErrorInvalidValue)
    MeterMatrix M;
    meter_matrix(k, G.L, M);
    double *d_zs = d_scratch, *d_init = d_scratch + G.at_init, *d_part = d_scratch + G.at_part, *d_per_hop = d_scratch + G.at_hop;
    if (marks) (void)hipEventRecord(marks[0], stream);
    hipLaunchKernelGGL((dusp_meter_pass_kernel<false>), dim3((unsigned)groups), dim3(kMeterLanes), 0, stream, d_planar, k, n, G.L, G.n_seg, G.n_segs, d_zs, (double *)nullptr);
    if (marks) (void)hipEventRecord(marks[1], stream);
    hipLaunchKernelGGL(dusp_meter_combine_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, stream, (const double *)d_zs, d_init, M, G.n_seg, (uint32_t)rows);
    if (marks) (void)hipEventRecord(marks[2], stream);
    hipLaunchKernelGGL((dusp_meter_pass_kernel<true>), dim3((unsigned)groups), dim3(kMeterLanes), 0, stream, d_planar, k, n, G.L, G.n_seg, G.n_segs, d_init, d_part);
    if (marks) (void)hipEventRecord(marks[3], stream);
    const uint64_t items = 2 * rows * G.n_hops, lanes = (uint64_t)n_signals * G.n_hops + rows;
    hipLaunchKernelGGL(dusp_meter_hop_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, (const double *)d_part, d_per_hop, G.n_seg, G.n_hops, G.per, items);
    hipLaunchKernelGGL(dusp_meter_sum_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, (const double *)d_per_hop, d_hops, d_sumsq, n_signals, n_channels, G.n_hops);
    if (marks) (void)hipEventRecord(marks[4], stream);
    return hipGetLastError();
}

}  // namespace dusp
