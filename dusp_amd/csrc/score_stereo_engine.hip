// score_stereo_engine.hip — the chain of score_rows_engine.hip, score_pan_engine.hip and score_frac_engine.hip over voices of THREE
// kinds into a timeline of two channels, the kind a property of the voice (dusp_amd/mix.py score_chain_rows_stereo is the contract;
// score_plan.hpp's score_rows_plan with row_channels the plan).  With s = t - onset_k and x_c[s] = f32(row_k[c][s] * g_k) or
// row_k[c][s], voice k adds to the left and to the right accumulator of every timeline sample it covers
//
//     a mono row, panned:      f32((f64(x_0) * lm_k) * ch_k)  and  f32((f64(x_0) * rp_k) * ch_k)    (score_pan_engine.hip's term: Pan.js:21-22)
//     a mono row, not placed:  x_0  and  x_0                  (Sum.js:37-38: a mono input feeds every channel of a wider one)
//     a row of two channels:   x_0  and  x_1
//
// each by a plain f32 add in voice index order; a voice with a fraction in its onset is heard through score_frac_engine.hip's two taps,
// applied per channel to the values above.  -ffp-contract=off -fno-fast-math, no FMA.
//
// The kind of an entry is in its record's stride (score_plan.hpp: kScoreStrideMono, kScoreStridePanned, else the floats from channel 0
// to channel 1 of a two-channel row): a scalar, so every test on it is wave-uniform.
//
//   * a lane owns ONE sample of the timeline and BOTH channels; the grid is over the groups of the window.
//   * the list is walked as in dusp_score_frac_kernel: batches of DEPTH = 8 indices (one scalar load); then, in sub-batches of SUB
//     entries, the records and the gains side by side, the sub-batch's vector loads back to back, and behind them — while they are in
//     flight — the pan coefficients (the 24 bytes of a ScorePan that are used; an unplaced voice's are zeros that nobody multiplies by)
//     and, FRAC, the weights, before the first add.
//   * a panned or plain mono entry makes ONE load, row[s] (two with a fraction: row[s - 1]); only a two-channel entry loads
//     row[stride + s] (and row[stride + s - 1]) as well, and only a panned one does f64 work without a fraction.
//   * a load a lane must not make — s >= len, s < 1, or a lane the entry does not cover — goes to the entry's own row[0] and its value is
//     dropped.  row[len] and row[-1] are never touched, nor anything beyond channels * len floats of a row: a row may be an allocation
//     of exactly that.  row[0] is readable for every record a batch can meet, by the planner's doing (score_plan.hpp ScoreRow).
//     tests/native/score_stereo_kernel_check.cpp runs this text on the host with every row a heap allocation of exactly its size.
//   * FRAC false — no listed voice has a fraction, every record's pad is 0 — is a kernel without the two-tap form.
//   * init may be out; neither is __restrict__.  Lanes are independent: no LDS, no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScoreStereoDepth = 8;  // entries of a list whose indices are read at once
constexpr int kScoreStereoSub = 4;      // entries a lane has in flight without the two-tap form: up to two vector loads each
constexpr int kScoreStereoFracSub = 2;  // ... and with it: up to four vector loads each, and 19 scalar registers an entry (four at once spill: DESIGN.md 6.13)

// group0: the first group of kScoreGroup samples the grid covers (w_lo >> kScoreGroupShift).  init, out: [2][n_total].  block_first is
// never nullptr: a launch without voices is the pan kernel's.  fracs: nullptr unless FRAC.
template <int DEPTH, int SUB, bool GAINS, bool FRAC>  // (DEPTH: a multiple of 8, the padding of entries[]; SUB divides it)
__global__ void __launch_bounds__(256) dusp_score_stereo_kernel(const float *__restrict__ gains, const ScorePan *__restrict__ pans, const ScoreFrac *__restrict__ fracs,
                                                                 const ScoreRow *__restrict__ voices, const uint32_t *__restrict__ block_first,
                                                                 const uint32_t *__restrict__ entries, const float *init, float *out, uint32_t n_total, uint32_t w_lo,
                                                                 uint32_t w_hi, uint32_t group0, uint32_t group_to_block, uint32_t first_block, int raw) {
    const uint32_t group = group0 + blockIdx.x;
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;  // (here group <= 2^22 and t < 2^30 + 256)
    const uint64_t oL = t, oR = (uint64_t)n_total + t;
    float accL = init ? init[oL] : 0.0f, accR = init ? init[oR] : 0.0f;
    const uint32_t b = (group >> group_to_block) - first_block;
    uint32_t e = block_first[b];
    const uint32_t e_end = block_first[b + 1];
    for (; e < e_end; e += DEPTH) {  // (a last batch that is not full: the entries past the list's end are nobody's, a wave-uniform test)
        uint32_t idx[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; k += 8) {  // (past the list's end: another list's entry, or the padding's voice 0; nobody's either way)
            const ScoreEntryWords w = *(const ScoreEntryWords *)(entries + e + k);
#pragma unroll
            for (int j = 0; j < 8; j++) idx[k + j] = w[j];
        }
#pragma unroll
        for (int h = 0; h < DEPTH; h += SUB) {
            if (e + h >= e_end) break;  // (wave-uniform)
            float a0[SUB], a1[SUB], b0[SUB], b1[SUB], g[SUB];  // a: channel 0 at s and s - 1; b: channel 1 of a two-channel row
            bool in[SUB], has0[SUB], has1[SUB], two[SUB], panned[SUB];
            ScoreRow V[SUB];
            ScoreFrac W[SUB];
            ScorePanUsed P[SUB];
            // the scalar loads the addresses need first, side by side — the records (and gains) — so that one wait covers them
#pragma unroll
            for (int k = 0; k < SUB; k++) {
                V[k] = score_load32(voices + idx[h + k]);
                g[k] = GAINS ? gains[idx[h + k]] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < SUB; k++) {
                in[k] = e + h + k < e_end && t >= V[k].lo && t < V[k].hi;
                panned[k] = V[k].stride == kScoreStridePanned;                    // (wave-uniform, as two[k])
                two[k] = V[k].stride != kScoreStrideMono && !panned[k];
                // in: 0 <= s <= len for a voice with a fraction (pad = len, never 0), 0 <= s < len for a whole one (pad = 0)
                const int64_t s = (int64_t)t - V[k].onset;
                has0[k] = in[k] && (!FRAC || V[k].pad == 0 || s < (int64_t)V[k].pad);
                has1[k] = FRAC && in[k] && V[k].pad != 0 && s >= 1;
                // a load the lane must not make goes to the entry's own row[0] instead (readable for every record: ScoreRow) and is dropped
                // (has0, two: stride + s < 2 * row_samples <= 2^31 floats)
                const ScoreRowFloats row = (ScoreRowFloats)V[k].row;
                a0[k] = row[has0[k] ? (uint64_t)s : (uint64_t)0];
                a1[k] = b0[k] = b1[k] = 0.0f;
                if (FRAC && V[k].pad != 0) a1[k] = row[has1[k] ? (uint64_t)s - 1 : (uint64_t)0];
                if (two[k]) {
                    b0[k] = row[has0[k] ? (uint64_t)V[k].stride + (uint64_t)s : (uint64_t)0];
                    if (FRAC && V[k].pad != 0) b1[k] = row[has1[k] ? (uint64_t)V[k].stride + (uint64_t)s - 1 : (uint64_t)0];
                }
            }
            // what only the arithmetic needs is fetched behind the vector loads, while they are in flight
#pragma unroll
            for (int k = 0; k < SUB; k++) {
                P[k] = score_load_pan(pans + idx[h + k]);
                if (FRAC) W[k] = score_load16(fracs + idx[h + k]);
            }
#pragma unroll
            for (int k = 0; k < SUB; k++)
                if (in[k]) {
                    const float x0 = GAINS ? a0[k] * g[k] : a0[k], x1 = GAINS ? a1[k] * g[k] : a1[k];  // (the f32 product rounded by itself)
                    const bool whole = !FRAC || V[k].pad == 0;  // (wave-uniform: today's term)
                    if (panned[k]) {
                        const double d0 = (double)x0, d1 = (double)x1;
                        const float l0 = (float)((d0 * P[k].lm) * P[k].ch), r0 = (float)((d0 * P[k].rp) * P[k].ch);
                        if (whole) {
                            accL = accL + l0;
                            accR = accR + r0;
                        } else {
                            const float l1 = (float)((d1 * P[k].lm) * P[k].ch), r1 = (float)((d1 * P[k].rp) * P[k].ch);
                            accL = accL + score_two_tap_term(l0, l1, has0[k], has1[k], W[k].w0, W[k].w1);
                            accR = accR + score_two_tap_term(r0, r1, has0[k], has1[k], W[k].w0, W[k].w1);
                        }
                    } else if (two[k]) {
                        const float y0 = GAINS ? b0[k] * g[k] : b0[k], y1 = GAINS ? b1[k] * g[k] : b1[k];
                        if (whole) {
                            accL = accL + x0;
                            accR = accR + y0;
                        } else {
                            accL = accL + score_two_tap_term(x0, x1, has0[k], has1[k], W[k].w0, W[k].w1);
                            accR = accR + score_two_tap_term(y0, y1, has0[k], has1[k], W[k].w0, W[k].w1);
                        }
                    } else {  // (a mono row that is not placed: one term, both channels)
                        const float term = whole ? x0 : score_two_tap_term(x0, x1, has0[k], has1[k], W[k].w0, W[k].w1);
                        accL = accL + term;
                        accR = accR + term;
                    }
                }
        }
    }
    out[oL] = raw ? accL : score_or0(accL);
    out[oR] = raw ? accR : score_or0(accR);
}

// One launch over the window [w_lo, w_hi) of both channels of the timeline, 0 <= w_lo < w_hi <= n_total <= 2^30.  d_voices /
// d_block_first / d_entries: the plan's image on the device (score_plan_pack), made for this window by score_rows_plan with
// row_channels, and d_pans the coefficients of the same voices (zeros for a voice that is not placed); none is nullptr.  d_fracs: the
// weights of the same voices where a listed one has a fraction, else nullptr: the kernel without the two-tap form.
hipError_t launch_score_stereo(const float *d_gains, const ScorePan *d_pans, const ScoreFrac *d_fracs, const ScoreRow *d_voices, const uint32_t *d_block_first,
                               const uint32_t *d_entries, const float *d_init, float *d_out, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift,
                               uint64_t first_block, int raw, hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(G.count), block(kScoreGroup);
#define DUSP_SCORE_STEREO_LAUNCH(GAINS, FRAC)                                                                                                                           \
    hipLaunchKernelGGL((dusp_score_stereo_kernel<kScoreStereoDepth, FRAC ? kScoreStereoFracSub : kScoreStereoSub, GAINS, FRAC>), grid, block, 0, stream, d_gains, d_pans, d_fracs, d_voices, d_block_first, \
                       d_entries, d_init, d_out, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, block_shift - kScoreGroupShift, (uint32_t)first_block, raw)
    if (d_fracs) {
        if (d_gains) DUSP_SCORE_STEREO_LAUNCH(true, true);
        else DUSP_SCORE_STEREO_LAUNCH(false, true);
    } else {
        if (d_gains) DUSP_SCORE_STEREO_LAUNCH(true, false);
        else DUSP_SCORE_STEREO_LAUNCH(false, false);
    }
#undef DUSP_SCORE_STEREO_LAUNCH
    return hipGetLastError();
}

}  // namespace dusp
