// score_frac_engine.hip — score_rows_engine.hip's and score_pan_engine.hip's chains with onsets BETWEEN samples: voice k starts at
// onset_k + frac_k samples, 0 <= frac_k < 1 (dusp_amd/mix.py score_chain_rows / score_chain_rows_panned with fracs, and two_tap_terms,
// are the contract; score_plan.hpp's score_rows_plan with fracs the plan).  The reference's Delay (Delay.js:36-38) writes every input
// sample to two neighbouring ring slots with the weights 1 - frac and frac; a voice with a fraction therefore covers the len + 1
// timeline samples onset .. onset + len, and with s = t - onset, w1 = frac, w0 = 1.0 - frac (made on the host: ScoreFrac)
//
//     c(s)      = f32(f64(x[s-1]) * w1)                  1 <= s <= len    (the ceil tap of sample s - 1, alone in its slot)
//     term(0)   = f32(f64(x[0]) * w0)
//     term(s)   = f32(f64(c(s)) + f64(x[s]) * w0)        1 <= s <  len    (product rounded to f64, sum rounded to f64, then to f32)
//     term(len) = c(len)
//     acc       = f32(acc + term(s))                                      (a plain f32 add, in voice index order)
//
// x[s] is the voice's sample after the gain, f32(row[s] * g) or row[s]; in the PAN form it is the Pan unit's output per channel,
// f32((f64(x) * lm) * ch) and f32((f64(x) * rp) * ch) (score_plan.hpp ScorePan), and the two taps are applied to each channel:
// Delay(Pan(Multiply(v, g), p), onset + frac).  -ffp-contract=off -fno-fast-math, no FMA.  A voice whose fraction is 0 is today's
// voice, term x[s] over onset .. onset + len - 1: its record's pad is 0, a wave-uniform test.
//
// What the anchor in the reference does not cover, and this kernel does not reproduce:
//   1. the reference's ring drops a ceil tap that lands on ring index maxDelay, once a trip round the ring: a quirk of the ring;
//   2. a delay in (0, 1) puts the floor tap into the slot the unit has just read, so it is heard a whole ring later;
//   3. an inlet constant is rounded to f32, the fraction here stays a double: where onset + frac is no f32 the contract is more exact.
//
//   * a lane owns ONE sample of the timeline: of one channel of n_channels (PAN false; the grid is groups x channels), or of BOTH
//     channels of a mono row (PAN true; the grid is over the groups).
//   * the list is walked as in dusp_score_rows_kernel: batches of DEPTH = 8 indices (one scalar load); then, in sub-batches of SUB = 4
//     entries, the records and the gains side by side, the sub-batch's 2 * SUB vector loads back to back, and behind them — while they
//     are in flight, and a record's address, onset and bounds are used up — the weights (ScoreFrac: 16 bytes on a 16-byte boundary, one
//     four-dword scalar load each) and the pan coefficients (the 24 bytes of a ScorePan that are used), before the first add: as many
//     vector loads in flight as the rows kernel has, and scalar registers for all of it without a spill.
//   * per entry a lane makes TWO loads, row[s] and row[s - 1]; the second lies in the cache lines the neighbouring lanes fetch.  Each is
//     pointed at the entry's own row[0] where the lane must not read it — s >= len, s < 1, or a lane the entry does not cover — and its
//     value dropped.  row[len] is never touched: a row may be an allocation of exactly len floats.  row[0] is readable for every
//     record a batch can meet, by the planner's doing (score_plan.hpp ScoreRow).  tests/native/score_frac_kernel_check.cpp runs this
//     text on the host with every row a heap allocation of exactly its size.
//   * init may be out; neither is __restrict__.  Lanes are independent: no LDS, no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScoreFracDepth = 8;  // entries of a list whose indices are read at once
constexpr int kScoreFracSub = 4;    // entries a lane has in flight: two vector loads each

// group0: the first group of kScoreGroup samples the grid covers (w_lo >> kScoreGroupShift); groups: how many (per channel).
// PAN false: init, out [n_channels][n_total], the grid groups x n_channels, pans unused.  PAN true: rows are mono, init, out [2][n_total],
// the grid groups.  block_first is never nullptr: a launch without voices is the existing kernels'.
template <int DEPTH, int SUB, bool GAINS, bool PAN>  // (DEPTH: a multiple of 8, the padding of entries[]; SUB divides it)
__global__ void __launch_bounds__(256) dusp_score_frac_kernel(const float *__restrict__ gains, const ScorePan *__restrict__ pans, const ScoreFrac *__restrict__ fracs,
                                                               const ScoreRow *__restrict__ voices, const uint32_t *__restrict__ block_first,
                                                               const uint32_t *__restrict__ entries, const float *init, float *out, uint32_t n_total, uint32_t w_lo,
                                                               uint32_t w_hi, uint32_t group0, uint32_t groups, uint32_t group_to_block, uint32_t first_block, int raw) {
    const uint32_t c = PAN ? 0u : blockIdx.x / groups, group = group0 + (blockIdx.x - c * groups);
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;
    const uint64_t o0 = (uint64_t)c * n_total + t, o1 = (uint64_t)n_total + t;  // (PAN: left and right)
    float acc0 = init ? init[o0] : 0.0f, acc1 = (PAN && init) ? init[o1] : 0.0f;
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
        // the batch in sub-batches of SUB entries: a record, its weights and its pan coefficients are up to 20 scalar registers an entry,
        // and SUB * 2 vector loads are in flight — DEPTH at once would not fit the scalar registers
#pragma unroll
        for (int h = 0; h < DEPTH; h += SUB) {
            if (e + h >= e_end) break;  // (wave-uniform)
            float v0[SUB], v1[SUB], g[SUB];
            bool in[SUB], has0[SUB], has1[SUB];
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
                // in: 0 <= s <= len for a voice with a fraction (pad = len, never 0), 0 <= s < len for a whole one (pad = 0)
                const int64_t s = (int64_t)t - V[k].onset;
                has0[k] = in[k] && (V[k].pad == 0 || s < (int64_t)V[k].pad);
                has1[k] = in[k] && V[k].pad != 0 && s >= 1;
                // a load the lane must not make goes to the entry's own row[0] instead (readable for every record: ScoreRow) and is
                // dropped: no branch around the loads, and the sub-batch's are issued back to back
                // (has0: c * stride + s < channels * row_samples <= 2^31 floats)
                const uint64_t at = (uint64_t)c * V[k].stride + (uint64_t)s;
                v0[k] = ((ScoreRowFloats)V[k].row)[has0[k] ? at : (uint64_t)0];
                v1[k] = ((ScoreRowFloats)V[k].row)[has1[k] ? at - 1 : (uint64_t)0];
            }
            // what only the arithmetic needs is fetched behind the vector loads, while they are in flight: by now a record's address,
            // onset and bounds are used up, and their scalar registers are free
#pragma unroll
            for (int k = 0; k < SUB; k++) {
                W[k] = score_load16(fracs + idx[h + k]);
                if (PAN) P[k] = score_load_pan(pans + idx[h + k]);
            }
#pragma unroll
            for (int k = 0; k < SUB; k++)
                if (in[k]) {
                    const float x0 = GAINS ? v0[k] * g[k] : v0[k], x1 = GAINS ? v1[k] * g[k] : v1[k];  // (the f32 product rounded by itself)
                    if (PAN) {
                        const double d0 = (double)x0, d1 = (double)x1;
                        const float l0 = (float)((d0 * P[k].lm) * P[k].ch), r0 = (float)((d0 * P[k].rp) * P[k].ch);
                        if (V[k].pad == 0) {  // (wave-uniform: today's term)
                            acc0 = acc0 + l0;
                            acc1 = acc1 + r0;
                        } else {
                            const float l1 = (float)((d1 * P[k].lm) * P[k].ch), r1 = (float)((d1 * P[k].rp) * P[k].ch);
                            acc0 = acc0 + score_two_tap_term(l0, l1, has0[k], has1[k], W[k].w0, W[k].w1);
                            acc1 = acc1 + score_two_tap_term(r0, r1, has0[k], has1[k], W[k].w0, W[k].w1);
                        }
                    } else if (V[k].pad == 0) {
                        acc0 = acc0 + x0;
                    } else {
                        acc0 = acc0 + score_two_tap_term(x0, x1, has0[k], has1[k], W[k].w0, W[k].w1);
                    }
                }
        }
    }
    out[o0] = raw ? acc0 : score_or0(acc0);
    if (PAN) out[o1] = raw ? acc1 : score_or0(acc1);
}

// One launch over the window [w_lo, w_hi) of the timeline, 0 <= w_lo < w_hi <= n_total, for a plan at least one of whose voices has a
// fraction.  d_pans nullptr: rows of n_channels into a timeline of n_channels, n_channels * n_total <= 2^31.  With d_pans: mono rows
// (n_channels == 1) into a timeline of two, n_total <= 2^30.  d_voices / d_block_first / d_entries: the plan's image on the device
// (score_plan_pack), made for this window, d_fracs (and d_pans) the weights (and coefficients) of the same voices; none is nullptr.
hipError_t launch_score_frac(const float *d_gains, const ScorePan *d_pans, const ScoreFrac *d_fracs, const ScoreRow *d_voices, const uint32_t *d_block_first,
                             const uint32_t *d_entries, const float *d_init, float *d_out, uint32_t n_channels, uint64_t n_total, uint64_t w_lo, uint64_t w_hi,
                             uint32_t block_shift, uint64_t first_block, int raw, hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(d_pans ? G.count : G.count * n_channels), block(kScoreGroup);
#define DUSP_SCORE_FRAC_LAUNCH(GAINS, PAN)                                                                                                                              \
    hipLaunchKernelGGL((dusp_score_frac_kernel<kScoreFracDepth, kScoreFracSub, GAINS, PAN>), grid, block, 0, stream, d_gains, d_pans, d_fracs, d_voices, d_block_first, d_entries, d_init, \
                       d_out, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, block_shift - kScoreGroupShift, (uint32_t)first_block, raw)
    if (d_pans) {
        if (d_gains) DUSP_SCORE_FRAC_LAUNCH(true, true);
        else DUSP_SCORE_FRAC_LAUNCH(false, true);
    } else {
        if (d_gains) DUSP_SCORE_FRAC_LAUNCH(true, false);
        else DUSP_SCORE_FRAC_LAUNCH(false, false);
    }
#undef DUSP_SCORE_FRAC_LAUNCH
    return hipGetLastError();
}

}  // namespace dusp
