// score_send_engine.hip — the chain of score_rows_engine.hip and of score_pan_engine.hip with effect sends, and the return of the buses
// (dusp_amd/mix.py score_chain_sends and bus_return are the contracts).  A voice's row is read ONCE and its term goes to
// the dry timeline and, multiplied by the voice's level into that bus, to each of B send timelines:
//
//     acc = init ? init[c][t] : +0;   snd_b = send_init ? send_init[b][c][t] : +0
//     for k in index order: s = t - onset_k; if (0 <= s < len_k):
//         acc   = f32(acc + term_k)                       term_k: the rows kernel's (row or f32(row * g_k)), or the pan kernel's two
//         snd_b = f32(snd_b + f32(term_k * level_k[b]))   for every bus b: a plain f32 product and a plain f32 add
//
// -ffp-contract=off -fno-fast-math, no FMA: the send term is f32(f32(x * g) * s), two roundings, which is why it cannot be a second
// launch of the rows kernel with the gain g * s.  Every voice is in every bus's chain: a level of 0 is a multiplication by 0 (NaN * 0
// poisons the bus, -x * 0 is -0), there is no skipped add.  The dry expressions are the two kernels' own, character for character, and
// tests/native/score_send_kernel_check.cpp holds the dry output to theirs bit for bit.
//
//   * the PLAN is score_rows_plan's, unchanged, and what score_rows_engine.hip says about lanes, batches of DEPTH, the wide scalar loads
//     and the load of a lane that an entry does not cover (the entry's own row[0], readable by the planner's doing) holds word for word.
//     The levels are a parallel array of ScoreSend (16 bytes on a 16-byte boundary) read beside the records and gains: the first B words
//     of a voice's record as one scalar load (one, two or four dwords).
//   * B is a COMPILE-TIME parameter, 1 .. 4: a lane keeps 1 + B accumulators (rows) or 2 + 2B (pan), and with B known every one of
//     them is a register — a run-time B would index the accumulators and put them in scratch memory.  profiles/score_sends.txt has the
//     register counts of the sixteen instantiations; none has a private segment.
//   * DEPTH stays 8, the other kernels': a batch holds 8 records (64 scalar registers) and at most 8 x 4 levels, more than the scalar file
//     has beside the kernel's arguments: the compiler keeps what does not fit in vector registers, of which a lane has few in use
//     (at most 36), and no instantiation has scratch memory (profile).
//   * the send timelines are [B][C][n_total] beside the dry [C][n_total], always raw; send_init may be send_out, init may be out, none is
//     __restrict__.  Lanes are independent: no LDS, no barrier, no cross-lane operation.
//
// dusp_score_return_kernel: out = dry; for b: out = f32(out + wet_b); `|| 0` unless raw — Sum.many([dry, wet_0, ...]), left-deep.  All
// buffers are [C][n_total], taken as flat arrays of n floats: four floats a lane as one 16-byte load and store where every buffer is on
// a 16-byte boundary, and the n % 4 floats behind them (or, where one is not, all n) one a lane.  out may be dry.  Its STEMS instance
// also copies every wet_b it reads into the bus's slot and, where asked, dry || 0 into the direct slot.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScoreSendDepth = 8;  // entries a lane has in flight

// the first B levels of a voice's record as one load
template <int B>
struct ScoreLevels {
    float l[B];
};
template <int B>
static __device__ __forceinline__ ScoreLevels<B> score_load_levels(const ScoreSend *p) {
    ScoreLevels<B> r;
    if (B == 1) {
        r.l[0] = p->level[0];
    } else if (B == 2) {
        const ScoreWords2 w = *(const ScoreWords2 *)p;
        __builtin_memcpy(&r, &w, sizeof r);
    } else {
        const ScoreWords4 w = *(const ScoreWords4 *)p;
        __builtin_memcpy(&r, &w, sizeof r);
    }
    return r;
}

// rows of n_channels: the grid is groups x channels, as dusp_score_rows_kernel's.  send_init, send_out: [B][n_channels][n_total].
// block_first == nullptr: no voices at all (init -> out and send_init -> send_out alone).
template <int DEPTH, int B, bool GAINS>  // (DEPTH: a multiple of 8, the padding of entries[])
__global__ void __launch_bounds__(256) dusp_score_rows_send_kernel(const float *__restrict__ gains, const ScoreSend *__restrict__ sends, const ScoreRow *__restrict__ voices,
                                                                    const uint32_t *__restrict__ block_first, const uint32_t *__restrict__ entries, const float *init, float *out,
                                                                    const float *send_init, float *send_out, uint32_t n_total, uint32_t n_channels, uint32_t w_lo, uint32_t w_hi,
                                                                    uint32_t group0, uint32_t groups, uint32_t group_to_block, uint32_t first_block, int raw) {
    const uint32_t c = blockIdx.x / groups, group = group0 + (blockIdx.x - c * groups);
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;
    const uint64_t o = (uint64_t)c * n_total + t, bus_stride = (uint64_t)n_channels * n_total;  // (o < bus_stride <= 2^31)
    float acc = init ? init[o] : 0.0f;
    float snd[B];
#pragma unroll
    for (int b = 0; b < B; b++) snd[b] = send_init ? send_init[(uint64_t)b * bus_stride + o] : 0.0f;
    uint32_t e = 0, e_end = 0;
    if (block_first) {
        const uint32_t blk = (group >> group_to_block) - first_block;
        e = block_first[blk];
        e_end = block_first[blk + 1];
    }
    for (; e < e_end; e += DEPTH) {  // (a last batch that is not full: the entries past the list's end are nobody's, a wave-uniform test)
        float v[DEPTH], g[DEPTH];
        bool in[DEPTH];
        uint32_t idx[DEPTH];
        ScoreRow V[DEPTH];
        ScoreLevels<B> S[DEPTH];
        // the batch's scalar loads first, side by side — the indices, then the records, gains and levels — so that one wait covers each stage
#pragma unroll
        for (int k = 0; k < DEPTH; k += 8) {  // (past the list's end: another list's entry, or the padding's voice 0; nobody's either way)
            const ScoreEntryWords w = *(const ScoreEntryWords *)(entries + e + k);
#pragma unroll
            for (int j = 0; j < 8; j++) idx[k + j] = w[j];
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            V[k] = score_load32(voices + idx[k]);
            g[k] = GAINS ? gains[idx[k]] : 1.0f;
            S[k] = score_load_levels<B>(sends + idx[k]);
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            in[k] = e + k < e_end && t >= V[k].lo && t < V[k].hi;
            // a lane the entry does not cover reads the entry's own row[0] instead (readable for every record: ScoreRow) and drops it:
            // no branch around the load, and the batch's vector loads are issued back to back
            // (in: c * stride + s < channels * row_samples <= 2^31 floats)
            const uint64_t at = (uint64_t)c * V[k].stride + (uint64_t)((int64_t)t - V[k].onset);
            v[k] = ((ScoreRowFloats)V[k].row)[in[k] ? at : (uint64_t)0];
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++)
            if (in[k]) {
                const float term = GAINS ? v[k] * g[k] : v[k];  // (the rows kernel's term, rounded by itself)
                acc = acc + term;
#pragma unroll
                for (int b = 0; b < B; b++) snd[b] = snd[b] + term * S[k].l[b];
            }
    }
    out[o] = raw ? acc : score_or0(acc);
#pragma unroll
    for (int b = 0; b < B; b++) send_out[(uint64_t)b * bus_stride + o] = snd[b];
}

// mono rows panned into two channels: the grid is over the groups, a lane owns both channels, as dusp_score_pan_kernel's.
// init, out: [2][n_total]; send_init, send_out: [B][2][n_total].
template <int DEPTH, int B, bool GAINS>
__global__ void __launch_bounds__(256) dusp_score_pan_send_kernel(const float *__restrict__ gains, const ScoreSend *__restrict__ sends, const ScorePan *__restrict__ pans,
                                                                   const ScoreRow *__restrict__ voices, const uint32_t *__restrict__ block_first,
                                                                   const uint32_t *__restrict__ entries, const float *init, float *out, const float *send_init, float *send_out,
                                                                   uint32_t n_total, uint32_t w_lo, uint32_t w_hi, uint32_t group0, uint32_t group_to_block, uint32_t first_block,
                                                                   int raw) {
    const uint32_t group = group0 + blockIdx.x;
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;  // (here group <= 2^22 and t < 2^30 + 256)
    const uint64_t oL = t, oR = (uint64_t)n_total + t, bus_stride = (uint64_t)2 * n_total;
    float accL = init ? init[oL] : 0.0f, accR = init ? init[oR] : 0.0f;
    float sndL[B], sndR[B];
#pragma unroll
    for (int b = 0; b < B; b++) {
        sndL[b] = send_init ? send_init[(uint64_t)b * bus_stride + oL] : 0.0f;
        sndR[b] = send_init ? send_init[(uint64_t)b * bus_stride + oR] : 0.0f;
    }
    uint32_t e = 0, e_end = 0;
    if (block_first) {
        const uint32_t blk = (group >> group_to_block) - first_block;
        e = block_first[blk];
        e_end = block_first[blk + 1];
    }
    for (; e < e_end; e += DEPTH) {  // (a last batch that is not full: the entries past the list's end are nobody's, a wave-uniform test)
        float v[DEPTH], g[DEPTH];
        bool in[DEPTH];
        uint32_t idx[DEPTH];
        ScoreRow V[DEPTH];
        ScorePan P[DEPTH];
        ScoreLevels<B> S[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; k += 8) {  // (past the list's end: another list's entry, or the padding's voice 0; nobody's either way)
            const ScoreEntryWords w = *(const ScoreEntryWords *)(entries + e + k);
#pragma unroll
            for (int j = 0; j < 8; j++) idx[k + j] = w[j];
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            V[k] = score_load32(voices + idx[k]);
            P[k] = score_load32(pans + idx[k]);
            g[k] = GAINS ? gains[idx[k]] : 1.0f;
            S[k] = score_load_levels<B>(sends + idx[k]);
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            in[k] = e + k < e_end && t >= V[k].lo && t < V[k].hi;
            // a lane the entry does not cover reads the entry's own row[0] instead (readable for every record: ScoreRow) and drops it
            // (in: s < row_samples <= 2^31 floats)
            const uint64_t at = (uint64_t)((int64_t)t - V[k].onset);
            v[k] = ((ScoreRowFloats)V[k].row)[in[k] ? at : (uint64_t)0];
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++)
            if (in[k]) {
                const double x = (double)(GAINS ? v[k] * g[k] : v[k]);  // (the f32 product rounded by itself, as the rows kernel's term)
                const float left = (float)((x * P[k].lm) * P[k].ch), right = (float)((x * P[k].rp) * P[k].ch);
                accL = accL + left;
                accR = accR + right;
#pragma unroll
                for (int b = 0; b < B; b++) {
                    sndL[b] = sndL[b] + left * S[k].l[b];
                    sndR[b] = sndR[b] + right * S[k].l[b];
                }
            }
    }
    out[oL] = raw ? accL : score_or0(accL);
    out[oR] = raw ? accR : score_or0(accR);
#pragma unroll
    for (int b = 0; b < B; b++) {
        send_out[(uint64_t)b * bus_stride + oL] = sndL[b];
        send_out[(uint64_t)b * bus_stride + oR] = sndR[b];
    }
}

template <int B>
static void launch_score_send_b(const float *d_gains, const ScoreSend *d_sends, const ScorePan *d_pans, const ScoreRow *d_voices, const uint32_t *d_block_first,
                                const uint32_t *d_entries, const float *d_init, float *d_out, const float *d_send_init, float *d_send_out, uint32_t n_channels, uint64_t n_total,
                                uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw, bool pan, hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(pan ? G.count : G.count * n_channels), block(kScoreGroup);
    const bool gains = d_gains && d_block_first;
    const uint32_t to_block = block_shift - kScoreGroupShift;
    if (pan && gains)
        hipLaunchKernelGGL((dusp_score_pan_send_kernel<kScoreSendDepth, B, true>), grid, block, 0, stream, d_gains, d_sends, d_pans, d_voices, d_block_first, d_entries, d_init, d_out,
                           d_send_init, d_send_out, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, to_block, (uint32_t)first_block, raw);
    else if (pan)
        hipLaunchKernelGGL((dusp_score_pan_send_kernel<kScoreSendDepth, B, false>), grid, block, 0, stream, d_gains, d_sends, d_pans, d_voices, d_block_first, d_entries, d_init, d_out,
                           d_send_init, d_send_out, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, to_block, (uint32_t)first_block, raw);
    else if (gains)
        hipLaunchKernelGGL((dusp_score_rows_send_kernel<kScoreSendDepth, B, true>), grid, block, 0, stream, d_gains, d_sends, d_voices, d_block_first, d_entries, d_init, d_out,
                           d_send_init, d_send_out, (uint32_t)n_total, n_channels, (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, to_block, (uint32_t)first_block, raw);
    else
        hipLaunchKernelGGL((dusp_score_rows_send_kernel<kScoreSendDepth, B, false>), grid, block, 0, stream, d_gains, d_sends, d_voices, d_block_first, d_entries, d_init, d_out,
                           d_send_init, d_send_out, (uint32_t)n_total, n_channels, (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, to_block, (uint32_t)first_block, raw);
}

// One launch over the window [w_lo, w_hi) of every channel of the dry timeline [n_channels][n_total] and of the n_buses send timelines
// [n_buses][n_channels][n_total], 1 <= n_buses <= kScoreBusMax, under launch_score_rows' limits (d_pans: launch_score_pan's, mono rows
// and n_channels == 2).  d_voices / d_block_first / d_entries: the plan's image on the device, d_sends (and d_pans) the records of the
// same voices — or all nullptr for a launch without voices.
hipError_t launch_score_send(const float *d_gains, const ScoreSend *d_sends, const ScorePan *d_pans, const ScoreRow *d_voices, const uint32_t *d_block_first,
                             const uint32_t *d_entries, const float *d_init, float *d_out, const float *d_send_init, float *d_send_out, uint32_t n_buses, uint32_t n_channels,
                             uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw, bool pan, hipStream_t stream) {
    switch (n_buses) {
    case 1:
        launch_score_send_b<1>(d_gains, d_sends, d_pans, d_voices, d_block_first, d_entries, d_init, d_out, d_send_init, d_send_out, n_channels, n_total, w_lo, w_hi, block_shift, first_block, raw, pan, stream);
        break;
    case 2:
        launch_score_send_b<2>(d_gains, d_sends, d_pans, d_voices, d_block_first, d_entries, d_init, d_out, d_send_init, d_send_out, n_channels, n_total, w_lo, w_hi, block_shift, first_block, raw, pan, stream);
        break;
    case 3:
        launch_score_send_b<3>(d_gains, d_sends, d_pans, d_voices, d_block_first, d_entries, d_init, d_out, d_send_init, d_send_out, n_channels, n_total, w_lo, w_hi, block_shift, first_block, raw, pan, stream);
        break;
    case 4:
        launch_score_send_b<4>(d_gains, d_sends, d_pans, d_voices, d_block_first, d_entries, d_init, d_out, d_send_init, d_send_out, n_channels, n_total, w_lo, w_hi, block_shift, first_block, raw, pan, stream);
        break;
    default:
        return (hipError_t)1;  // (hipErrorInvalidValue: the callers have checked)
    }
    return hipGetLastError();
}

// ---- the return of the buses ----

template <bool STEMS>
struct ScoreWets {  // the buses' outputs, each [n] floats; the first n_buses are read
    const float *p[kScoreBusMax];
};
template <>
struct ScoreWets<true> {  // ... and the buses' slots, each [n] floats
    const float *p[kScoreBusMax];
    float *stem[kScoreBusMax];
};

// n_vec lanes take four floats each, the n - 4 * n_vec floats behind them one lane each.  StemDirect: with STEMS one float *, nullptr
// or where dry || 0 goes; without, nothing — the arguments of that instance hold no stem pointer at all
template <bool STEMS, class... StemDirect>
__global__ void __launch_bounds__(256) dusp_score_return_kernel(const float *dry, ScoreWets<STEMS> wets, uint32_t n_buses, float *out, StemDirect... stem_direct_, uint64_t n,
                                                                 uint64_t n_vec, int raw) {
    static_assert(sizeof...(StemDirect) == (STEMS ? 1 : 0), "stem_direct is an argument of the STEMS instance alone");
    float *stem_direct = score_stem_direct(stem_direct_...);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_vec) {
        float4 a = ((const float4 *)dry)[i];
        if (STEMS && stem_direct) ((float4 *)stem_direct)[i] = make_float4(score_or0(a.x), score_or0(a.y), score_or0(a.z), score_or0(a.w));
        for (uint32_t b = 0; b < n_buses; b++) {
            const float4 w = ((const float4 *)wets.p[b])[i];
            if constexpr (STEMS) ((float4 *)wets.stem[b])[i] = w;
            a.x = a.x + w.x;
            a.y = a.y + w.y;
            a.z = a.z + w.z;
            a.w = a.w + w.w;
        }
        if (!raw) a = make_float4(score_or0(a.x), score_or0(a.y), score_or0(a.z), score_or0(a.w));
        ((float4 *)out)[i] = a;
        return;
    }
    const uint64_t j = 4 * n_vec + (i - n_vec);
    if (j >= n) return;
    float a = dry[j];
    if (STEMS && stem_direct) stem_direct[j] = score_or0(a);
    for (uint32_t b = 0; b < n_buses; b++) {
        const float w = wets.p[b][j];
        if constexpr (STEMS) wets.stem[b][j] = w;
        a = a + w;
    }
    out[j] = raw ? a : score_or0(a);
}

template <bool STEMS>
static void launch_score_return_as(const float *d_dry, const float *const *d_wets, uint32_t n_buses, float *d_out, float *d_stem_direct, float *const *d_stem_buses, uint64_t n, int raw,
                                   hipStream_t stream) {
    ScoreWets<STEMS> wets{};
    uintptr_t low = (uintptr_t)d_dry | (uintptr_t)d_out | (uintptr_t)d_stem_direct;
    for (uint32_t b = 0; b < n_buses; b++) {
        wets.p[b] = d_wets[b];
        low |= (uintptr_t)d_wets[b];
        if constexpr (STEMS) {
            wets.stem[b] = d_stem_buses[b];
            low |= (uintptr_t)d_stem_buses[b];
        }
    }
    const uint64_t n_vec = (low & 15) ? 0 : n / 4, lanes = n_vec + (n - 4 * n_vec);
    const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
    if constexpr (STEMS)
        hipLaunchKernelGGL((dusp_score_return_kernel<true, float *>), grid, block, 0, stream, d_dry, wets, n_buses, d_out, d_stem_direct, n, n_vec, raw);
    else
        hipLaunchKernelGGL((dusp_score_return_kernel<false>), grid, block, 0, stream, d_dry, wets, n_buses, d_out, n, n_vec, raw);
}

// out[j] = dry[j] + wets[0][j] + ... (left-deep), `|| 0` unless raw, over n floats, 1 <= n <= 2^31; n_buses <= kScoreBusMax (0: dry -> out).
// d_stem_buses given (the stems of a piece): the launch also writes d_stem_buses[b][j] = d_wets[b][j], as it is (the
// bus's copy-out has made it `|| 0`), and, d_stem_direct given — the dry timeline has no slot yet: per-note sends without tracks —
// d_stem_direct[j] = d_dry[j] || 0.  The slots are n floats each and alias nothing.  d_stem_buses nullptr: d_stem_direct is not looked at.
hipError_t launch_score_return(const float *d_dry, const float *const *d_wets, uint32_t n_buses, float *d_out, float *d_stem_direct, float *const *d_stem_buses, uint64_t n, int raw,
                               hipStream_t stream) {
    if (n_buses > kScoreBusMax) return (hipError_t)1;  // (hipErrorInvalidValue: the callers have checked)
    d_stem_buses ? launch_score_return_as<true>(d_dry, d_wets, n_buses, d_out, d_stem_direct, d_stem_buses, n, raw, stream)
                 : launch_score_return_as<false>(d_dry, d_wets, n_buses, d_out, nullptr, nullptr, n, raw, stream);
    return hipGetLastError();
}

}  // namespace dusp
