// score_space_engine.hip — score_rows_engine.hip's chain over MONO voices placed in a space: voice k reaches each of C speakers, the
// timeline's channels, through a gain G_kc and a delay of D_kc samples of its own (dusp_amd/mix.py score_chain_rows_placed is the
// contract; score_plan.hpp's score_rows_plan with taps the plan, ScoreSpaceTap the tap).  It is what the reference's SpaceChannel puts
// behind a sound — a Gain (Gain.js:22) and a MonoDelay (MonoDelay.js:24-26), which writes every input sample to the two ring slots
// around its delayed position with the weights 1 - frac and frac — done where the voice is added to the timeline.  With
// shift = floor(D), w1 = D - shift, w0 = 1.0 - w1 (made on the host), x[s] the voice's sample after the per-voice gain (f32(row[s] * g)
// or row[s]), len its length and s = t - onset - shift
//
//     y[s]      = f32(G * f64(x[s]))                     (one f64 product, one rounding)
//     w1 == 0:    term(s) = y[s]                          0 <= s <  len
//     w1 != 0:    c(s)      = f32(f64(y[s-1]) * w1)       1 <= s <= len    (the ceil tap of sample s - 1, alone in its slot)
//                 term(0)   = f32(f64(y[0]) * w0)
//                 term(s)   = f32(f64(c(s)) + f64(y[s]) * w0)   1 <= s < len   (product rounded to f64, sum rounded to f64, then to f32)
//                 term(len) = c(len)
//     acc       = f32(acc + term(s))                      (a plain f32 add, in voice index order; no add where the voice does not cover t)
//
// -ffp-contract=off -fno-fast-math, no FMA.  DESIGN.md 6.12 says where the anchor in the reference ends.
//
//   * a lane owns ONE sample of ONE channel of the timeline; the grid is groups x C.  The tap of (voice, channel) is uniform over the
//     workgroup, so the choice between the one-load and the two-load term is a wave-uniform branch.
//   * the list is walked as in dusp_score_frac_kernel: batches of DEPTH = 8 indices (one scalar load); then, in sub-batches of SUB
//     entries, the records, the gains and the HALF of a tap the addresses need (w1 and the shift: one four-dword scalar load) side by
//     side, the sub-batch's 2 * SUB vector loads back to back, and behind them — while they are in flight — the other half (w0 and G).
//   * per entry a lane makes TWO loads, row[s] and row[s - 1].  Each is pointed at the entry's own row[0] where the lane must not read
//     it — s >= len, s < 1, a one-tap entry, a lane the entry does not cover, or this channel's span being empty in the window while
//     another's is not — and its value dropped.  row[len] and row[-1] are never touched: a row may be an allocation of exactly len
//     floats.  row[0] is readable for every record a batch can meet, by the planner's doing (score_plan.hpp ScoreRow).
//     tests/native/score_space_kernel_check.cpp runs this text on the host with every row a heap allocation of exactly its size.
//   * init may be out; neither is __restrict__.  Lanes are independent: no LDS, no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScoreSpaceDepth = 8;  // entries of a list whose indices are read at once
constexpr int kScoreSpaceSub = 4;    // entries a lane has in flight: two vector loads each

// a tap's halves as one four-dword scalar load each
struct ScoreSpaceWhere {
    double w1;
    int64_t shift;
};
struct ScoreSpaceHow {
    double w0, gain;
};
static __device__ __forceinline__ ScoreSpaceWhere score_space_where(const ScoreSpaceTap *p) {
    const ScoreWords4 w = *(const ScoreWords4 *)&p->w1;
    ScoreSpaceWhere r;
    __builtin_memcpy(&r, &w, sizeof r);
    return r;
}
static __device__ __forceinline__ ScoreSpaceHow score_space_how(const ScoreSpaceTap *p) {
    const ScoreWords4 w = *(const ScoreWords4 *)p;
    ScoreSpaceHow r;
    __builtin_memcpy(&r, &w, sizeof r);
    return r;
}

// group0: the first group of kScoreGroup samples the grid covers (w_lo >> kScoreGroupShift); groups: how many (per channel).
// rows are mono; init, out [n_channels][n_total]; taps [n voices][n_channels]; the grid groups x n_channels.  block_first is never
// nullptr: a launch without voices is the rows kernel's.
template <int DEPTH, int SUB, bool GAINS>  // (DEPTH: a multiple of 8, the padding of entries[]; SUB divides it)
__global__ void __launch_bounds__(256) dusp_score_space_kernel(const float *__restrict__ gains, const ScoreSpaceTap *__restrict__ taps, const ScoreRow *__restrict__ voices,
                                                                const uint32_t *__restrict__ block_first, const uint32_t *__restrict__ entries, const float *init, float *out,
                                                                uint32_t n_channels, uint32_t n_total, uint32_t w_lo, uint32_t w_hi, uint32_t group0, uint32_t groups,
                                                                uint32_t group_to_block, uint32_t first_block, int raw) {
    const uint32_t c = blockIdx.x / groups, group = group0 + (blockIdx.x - c * groups);
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;
    const uint64_t o = (uint64_t)c * n_total + t;
    float acc = init ? init[o] : 0.0f;
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
            float v0[SUB], v1[SUB], g[SUB];
            bool in[SUB], has0[SUB], has1[SUB];
            ScoreRow V[SUB];
            ScoreSpaceWhere W[SUB];
            ScoreSpaceHow H[SUB];
            // the scalar loads the addresses need first, side by side, so that one wait covers them
#pragma unroll
            for (int k = 0; k < SUB; k++) {
                V[k] = score_load32(voices + idx[h + k]);
                W[k] = score_space_where(taps + (uint64_t)idx[h + k] * n_channels + c);
                g[k] = GAINS ? gains[idx[h + k]] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < SUB; k++) {
                // in: 0 <= s <= len on a channel with two taps, 0 <= s < len on one with one (pad = len; 0 for a record that is in no
                // list).  The record's [lo, hi) is the union of the channels' spans: this channel's may be any part of it, or none
                // (|onset| < 2^34 for a listed voice and 0 <= shift <= 2^24: s cannot overflow)
                const int64_t s = (int64_t)t - V[k].onset - W[k].shift, len = (int64_t)V[k].pad;
                const bool two = W[k].w1 != 0.0;
                in[k] = e + h + k < e_end && t >= V[k].lo && t < V[k].hi && s >= 0 && (two ? s <= len : s < len);
                has0[k] = in[k] && s < len;
                has1[k] = in[k] && two && s >= 1;
                // a load the lane must not make goes to the entry's own row[0] instead (readable for every record: ScoreRow) and is
                // dropped: no branch around the loads, and the sub-batch's are issued back to back
                v0[k] = ((ScoreRowFloats)V[k].row)[has0[k] ? (uint64_t)s : (uint64_t)0];
                v1[k] = ((ScoreRowFloats)V[k].row)[has1[k] ? (uint64_t)s - 1 : (uint64_t)0];
            }
            // what only the arithmetic needs is fetched behind the vector loads, while they are in flight
#pragma unroll
            for (int k = 0; k < SUB; k++) H[k] = score_space_how(taps + (uint64_t)idx[h + k] * n_channels + c);
#pragma unroll
            for (int k = 0; k < SUB; k++)
                if (in[k]) {
                    const float x0 = GAINS ? v0[k] * g[k] : v0[k];  // (the f32 product rounded by itself)
                    const float y0 = (float)(H[k].gain * (double)x0);
                    if (W[k].w1 == 0.0) {  // (wave-uniform: one tap)
                        acc = acc + y0;
                    } else {
                        const float x1 = GAINS ? v1[k] * g[k] : v1[k];
                        const float y1 = (float)(H[k].gain * (double)x1);
                        acc = acc + score_two_tap_term(y0, y1, has0[k], has1[k], H[k].w0, W[k].w1);
                    }
                }
        }
    }
    out[o] = raw ? acc : score_or0(acc);
}

// One launch over the window [w_lo, w_hi) of the timeline, 0 <= w_lo < w_hi <= n_total, n_channels * n_total <= 2^31, for a plan made
// with taps: d_voices / d_block_first / d_entries are the plan's image on the device (score_plan_pack), made for this window, d_taps
// the taps of the same voices, [voice][channel]; none is nullptr.
hipError_t launch_score_space(const float *d_gains, const ScoreSpaceTap *d_taps, const ScoreRow *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries,
                              const float *d_init, float *d_out, uint32_t n_channels, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block,
                              int raw, hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(G.count * n_channels), block(kScoreGroup);
#define DUSP_SCORE_SPACE_LAUNCH(GAINS)                                                                                                                                 \
    hipLaunchKernelGGL((dusp_score_space_kernel<kScoreSpaceDepth, kScoreSpaceSub, GAINS>), grid, block, 0, stream, d_gains, d_taps, d_voices, d_block_first, d_entries, d_init, \
                       d_out, n_channels, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, block_shift - kScoreGroupShift, (uint32_t)first_block, raw)
    if (d_gains) DUSP_SCORE_SPACE_LAUNCH(true);
    else DUSP_SCORE_SPACE_LAUNCH(false);
#undef DUSP_SCORE_SPACE_LAUNCH
    return hipGetLastError();
}

}  // namespace dusp
