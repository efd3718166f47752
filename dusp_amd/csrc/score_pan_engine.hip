// score_pan_engine.hip — score_rows_engine.hip's chain over MONO rows, every voice placed in the stereo field where it is added to the
// timeline (dusp_amd/mix.py score_chain_rows_panned is the contract; score_plan.hpp's score_rows_plan the plan, unchanged: lists are per
// block of the timeline and know nothing of channels).  A pan that is constant over a note is a property of the placement: the
// reference's Pan unit (Pan.js:21-22) behind voice k is, per timeline sample t,
//
//     accL, accR = init ? init[0][t], init[1][t] : +0, +0
//     for k in index order: s = t - onset_k; if (0 <= s < len_k):
//         x    = gains ? f32(row_k[s] * g_k) : row_k[s]
//         accL = f32(accL + f32(((f64(x) * (1 - f64(p_k))) / 2) * comp_k))
//         accR = f32(accR + f32(((f64(x) * (1 + f64(p_k))) / 2) * comp_k))
//
// The host hands over lm = 1 - f64(p), rp = 1 + f64(p) and ch = comp / 2 per voice (score_plan.hpp ScorePan, where it is shown that
// (y / 2) * comp and y * (comp / 2) round to the same f32), so a term is two f64 products, one rounding to f32 and one plain f32 add:
// -ffp-contract=off -fno-fast-math, no FMA.
//
//   * a lane owns ONE sample of the timeline and BOTH channels: the row's sample is loaded once and feeds two accumulators.  The grid is
//     over the groups of the window, not groups x channels.
//   * the list is walked as in dusp_score_rows_kernel: batches of DEPTH, the batch's indices (one scalar load), then the records, pan
//     coefficients (ScorePan: 32 bytes on a 32-byte boundary, one eight-dword scalar load each) and gains side by side, then DEPTH vector
//     loads back to back before the first add.
//   * the ADD is predicated on the lane's own `lo <= t < hi`; the LOAD of a lane that an entry does not cover goes to the entry's own
//     row[0] and is dropped.  That address is readable by the planner's doing (score_plan.hpp ScoreRow), as in the rows kernel;
//     tests/native/score_pan_kernel_check.cpp runs this text on the host with every row a heap allocation of exactly its size.
//   * init may be out; neither is __restrict__.  Lanes are independent: no LDS, no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScorePanDepth = 8;  // entries a lane has in flight

// group0: the first group of kScoreGroup samples the grid covers (w_lo >> kScoreGroupShift).  init, out: [2][n_total].
// block_first == nullptr: no voices at all (init -> out alone).
template <int DEPTH, bool GAINS>  // (DEPTH: a multiple of 8, the padding of entries[])
__global__ void __launch_bounds__(256) dusp_score_pan_kernel(const float *__restrict__ gains, const ScorePan *__restrict__ pans, const ScoreRow *__restrict__ voices,
                                                              const uint32_t *__restrict__ block_first, const uint32_t *__restrict__ entries, const float *init, float *out,
                                                              uint32_t n_total, uint32_t w_lo, uint32_t w_hi, uint32_t group0, uint32_t group_to_block, uint32_t first_block,
                                                              int raw) {
    const uint32_t group = group0 + blockIdx.x;
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;  // (here group <= 2^22 and t < 2^30 + 256)
    const uint64_t oL = t, oR = (uint64_t)n_total + t;
    float accL = init ? init[oL] : 0.0f, accR = init ? init[oR] : 0.0f;
    uint32_t e = 0, e_end = 0;
    if (block_first) {
        const uint32_t b = (group >> group_to_block) - first_block;
        e = block_first[b];
        e_end = block_first[b + 1];
    }
    for (; e < e_end; e += DEPTH) {  // (a last batch that is not full: the entries past the list's end are nobody's, a wave-uniform test)
        float v[DEPTH], g[DEPTH];
        bool in[DEPTH];
        uint32_t idx[DEPTH];
        ScoreRow V[DEPTH];
        ScorePan P[DEPTH];
        // the batch's scalar loads first, side by side — the indices, then the records, coefficients (and gains) — so that one wait covers each stage
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
            }
    }
    out[oL] = raw ? accL : score_or0(accL);
    out[oR] = raw ? accR : score_or0(accR);
}

// One launch over the window [w_lo, w_hi) of both channels of the timeline, 0 <= w_lo < w_hi <= n_total <= 2^30.  d_voices /
// d_block_first / d_entries: the plan's image on the device (score_plan_pack), made for this window over MONO rows, and d_pans the
// coefficients of the same voices — or all nullptr for a launch without voices.
hipError_t launch_score_pan(const float *d_gains, const ScorePan *d_pans, const ScoreRow *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries,
                            const float *d_init, float *d_out, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw,
                            hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(G.count), block(kScoreGroup);
    if (d_gains && d_block_first)
        hipLaunchKernelGGL((dusp_score_pan_kernel<kScorePanDepth, true>), grid, block, 0, stream, d_gains, d_pans, d_voices, d_block_first, d_entries, d_init, d_out,
                           (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, block_shift - kScoreGroupShift, (uint32_t)first_block, raw);
    else
        hipLaunchKernelGGL((dusp_score_pan_kernel<kScorePanDepth, false>), grid, block, 0, stream, d_gains, d_pans, d_voices, d_block_first, d_entries, d_init, d_out,
                           (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, block_shift - kScoreGroupShift, (uint32_t)first_block, raw);
    return hipGetLastError();
}

}  // namespace dusp
