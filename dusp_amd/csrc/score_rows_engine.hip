// score_rows_engine.hip — score_engine.hip's chain over voices that each lie in a buffer of their own: rows of any length, rendered by
// any program, mixed at per-voice onsets into one timeline in Sum.many's chain order (dusp_amd/mix.py score_chain_rows is the contract;
// score_plan.hpp's score_rows_plan the plan the host makes for a launch).  A piece of several instruments is one such chain over the
// caller's voice list, whichever instrument a voice belongs to:
//
//     acc = init ? init[c][t] : +0;   for k in index order: s = t - onset_k; if (0 <= s < len_k) acc = f32(acc + term_k)
//
// with term_k = gains ? f32(row_k[c][s] * g_k) : row_k[c][s], a plain f32 product and a plain f32 add (-ffp-contract=off -fno-fast-math).
// The kernel has score_engine.hip's shape, and what is said there about skipped adds, raw and `|| 0` holds word for word:
//
//   * a lane owns one sample of one channel of the launch's window; a workgroup is kScoreGroup consecutive samples.  One float a lane:
//     the rows have unrelated alignments against the timeline AND against one another.
//   * the lane walks its block's list in batches of DEPTH: the batch's indices are contiguous (one scalar load), then the DEPTH records
//     (ScoreRow: 32 bytes on a 32-byte boundary, one eight-dword scalar load each) and gains side by side behind one wait, then DEPTH
//     vector loads back to back before the first add.  A voice's sample is ((const float *)V.row)[c * V.stride + (t - V.onset)].
//   * the ADD is predicated on the lane's own `lo <= t < hi`.  The LOAD of a lane that an entry does not cover is not branched around: it
//     goes to the entry's own row[0] and its value is dropped.  That address is readable for every record a batch can meet, by the
//     planner's doing (score_plan.hpp ScoreRow): a listed voice has lo < hi, hence at least one sample; a record that is in no list —
//     the one the padding's zeros name, if voice 0 is such — carries the first listed voice's row.  A launch with no listed voice has
//     no plan (block_first == nullptr) and loads nothing.  tests/native/score_rows_kernel_check.cpp enforces this: every row there is a
//     heap allocation of exactly its size under AddressSanitizer.
//   * init may be out; neither is __restrict__.  Lanes are independent: no LDS, no barrier, no cross-lane operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScoreRowsDepth = 8;  // entries a lane has in flight

// group0: the first group of kScoreGroup samples the grid covers (w_lo >> kScoreGroupShift); groups: how many per channel.
// block_first == nullptr: no voices at all (init -> out alone).
template <int DEPTH, bool GAINS>  // (DEPTH: a multiple of 8, the padding of entries[])
__global__ void __launch_bounds__(256) dusp_score_rows_kernel(const float *__restrict__ gains, const ScoreRow *__restrict__ voices, const uint32_t *__restrict__ block_first,
                                                               const uint32_t *__restrict__ entries, const float *init, float *out, uint32_t n_total, uint32_t w_lo,
                                                               uint32_t w_hi, uint32_t group0, uint32_t groups, uint32_t group_to_block, uint32_t first_block, int raw) {
    const uint32_t c = blockIdx.x / groups, group = group0 + (blockIdx.x - c * groups);
    uint32_t t;
    if (!score_lane_sample(group, w_lo, w_hi, t)) return;
    const uint64_t o = (uint64_t)c * n_total + t;
    float acc = init ? init[o] : 0.0f;
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
        // the batch's scalar loads first, side by side — the indices, then the records (and gains) — so that one wait covers each stage
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
            if (in[k]) acc = acc + (GAINS ? v[k] * g[k] : v[k]);
    }
    out[o] = raw ? acc : score_or0(acc);
}

// One launch over the window [w_lo, w_hi) of every channel of the timeline, 0 <= w_lo < w_hi <= n_total <= 2^31 and
// n_channels * n_total <= 2^31.  d_voices / d_block_first / d_entries: the plan's image on the device (score_plan_pack), made for
// this window — or all nullptr for a launch without voices.
hipError_t launch_score_rows(const float *d_gains, const ScoreRow *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries, const float *d_init, float *d_out,
                             uint32_t n_channels, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw,
                             hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(G.count * n_channels), block(kScoreGroup);
    if (d_gains && d_block_first)
        hipLaunchKernelGGL((dusp_score_rows_kernel<kScoreRowsDepth, true>), grid, block, 0, stream, d_gains, d_voices, d_block_first, d_entries, d_init, d_out, (uint32_t)n_total,
                           (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, block_shift - kScoreGroupShift, (uint32_t)first_block, raw);
    else
        hipLaunchKernelGGL((dusp_score_rows_kernel<kScoreRowsDepth, false>), grid, block, 0, stream, d_gains, d_voices, d_block_first, d_entries, d_init, d_out, (uint32_t)n_total,
                           (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, block_shift - kScoreGroupShift, (uint32_t)first_block, raw);
    return hipGetLastError();
}

}  // namespace dusp
