// score_engine.hip — a batch of rendered voices mixed at per-voice onsets into a timeline longer than a voice, on the device, in
// Sum.many's chain order (dusp_amd/mix.py score_chain is the contract; score_plan.hpp the plan the host makes for a launch).
//
// The reference writes such a piece as `Sum.many(voices.map((v, k) => new Delay(v, onset_k, maxDelay)))`: a Delay by a whole number of
// samples is its input behind zeros (Delay.js:27-38), and the Sum chain adds the voices in index order with one f32 rounding per add
// (Sum.js:18-29).  Here every voice is a short render of its own, and the chain is
//
//     acc = init ? init[c][t] : +0;   for k in index order: s = t - onset_k; if (0 <= s < len_k) acc = f32(acc + term_k)
//
// with term_k = gains ? f32(x * g_k) : x, a plain f32 product and a plain f32 add (-ffp-contract=off -fno-fast-math keep them apart).
// A voice takes no part in a sample outside its span: a lane it does not cover SKIPS the add, it does not add a zero (a raw partial sum
// of -0 stays -0, so a chain continued through init is the same chain wherever it is cut).  Unlike dusp_mix_kernel's, the chain starts
// from +0 and not from the first voice itself.  raw stores the sum as it stands; otherwise NaN and -0 leave as +0 (`x || 0`).
//
//   * a lane owns one sample of one channel of the timeline: a workgroup of 256 is kScoreGroup consecutive samples, the grid is
//     channels x groups of the launch's window [w_lo, w_hi).  A voice's floats land at t = s + onset_k, at phase onset_k mod 4 against
//     a 16-byte unit of the output, and its span's edges fall inside units: one float a lane is correct for every shape, and a
//     wavefront's accesses are still whole contiguous 256-byte runs (DESIGN.md 6.8 has the decision against a four-float form).
//   * the workgroup's block of the timeline has a list of the voices that intersect it (score_plan.hpp); the lane walks it in order.
//     The list, and a voice's onset, span and gain, depend on blockIdx only: wave-uniform (scalar) loads, a batch's 8 indices
//     contiguous (entries[] is padded by 8 so that a batch may read past its list's end) and a voice's record one 16-byte load.  Only the adds depend on one
//     another: the loads of kScoreDepth entries are issued before the first add.  The ADD is predicated on the lane's own `lo <= t < hi`;
//     the load of a lane the entry does not cover is pointed at voice 0's first sample and its value dropped, which keeps the loads free
//     of branches.
//   * init may be out (a tile of a score continues the timeline in place): a lane reads its sample before it writes it, and no other
//     lane touches it.  Neither is __restrict__.
//   * lanes are independent — no LDS, no barrier, no cross-lane operation — so tests/native/score_kernel_check.cpp runs this text on the
//     CPU, lane after lane, under AddressSanitizer.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_device.hpp"

namespace dusp {

constexpr int kScoreDepth = 8;  // entries a lane has in flight

// voice_row: floats from one voice's PCM to the next (n_channels * n_voice).  group0: the first group of kScoreGroup samples the grid
// covers (w_lo >> kScoreGroupShift); groups: how many per channel.  block_first == nullptr: no voices at all (init -> out alone).
template <int DEPTH, bool GAINS>
__global__ void __launch_bounds__(256) dusp_score_kernel(const float *__restrict__ planar, const float *__restrict__ gains, const ScoreVoice *__restrict__ voices,
                                                          const uint32_t *__restrict__ block_first, const uint32_t *__restrict__ entries, const float *init,
                                                          float *out, uint64_t voice_row, uint32_t n_voice, uint32_t n_total, uint32_t w_lo, uint32_t w_hi,
                                                          uint32_t group0, uint32_t groups, uint32_t group_to_block, uint32_t first_block, int raw) {
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
    const float *src = planar + (uint64_t)c * n_voice;
    for (; e < e_end; e += DEPTH) {  // (a last batch that is not full: the entries past the list's end are nobody's, a wave-uniform test)
        float v[DEPTH], g[DEPTH];
        bool in[DEPTH];
        uint32_t idx[DEPTH];
        ScoreVoice V[DEPTH];
        // the batch's scalar loads first, side by side — 8 indices, then 8 records (and gains) — so that one wait covers each stage
#pragma unroll
        for (int k = 0; k < DEPTH; k++) idx[k] = entries[e + k];  // (past the list's end: another list's entry, or the padding's voice 0; nobody's either way)
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            V[k] = voices[idx[k]];
            g[k] = GAINS ? gains[idx[k]] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++) {
            in[k] = e + k < e_end && t >= V[k].lo && t < V[k].hi;
            // a lane the entry does not cover reads voice 0's first sample instead (in bounds, one address for all such lanes) and drops it:
            // no branch around the load, and the batch's 8 vector loads are issued back to back
            const uint64_t at = (uint64_t)idx[k] * voice_row + (uint64_t)((int64_t)t - V[k].onset);
            v[k] = src[in[k] ? at : (uint64_t)0];
        }
#pragma unroll
        for (int k = 0; k < DEPTH; k++)
            if (in[k]) acc = acc + (GAINS ? v[k] * g[k] : v[k]);
    }
    out[o] = raw ? acc : score_or0(acc);
}

// One launch over the window [w_lo, w_hi) of every channel of the timeline, 0 <= w_lo < w_hi <= n_total <= 2^31 and
// n_channels * n_total <= 2^31 (the grid stays far below 2^31 workgroups).  d_voices / d_block_first / d_entries: the plan's image on the
// device (score_plan_pack), made for this window — or all nullptr for a launch without voices.
hipError_t launch_score(const float *d_planar, const float *d_gains, const ScoreVoice *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries,
                        const float *d_init, float *d_out, uint32_t n_channels, uint64_t n_voice, uint64_t n_total, uint64_t w_lo, uint64_t w_hi,
                        uint32_t block_shift, uint64_t first_block, int raw, hipStream_t stream) {
    const ScoreGroups G = score_groups(w_lo, w_hi);
    const dim3 grid(G.count * n_channels), block(kScoreGroup);
    const uint64_t voice_row = (uint64_t)n_channels * n_voice;
    if (d_gains && d_block_first)
        hipLaunchKernelGGL((dusp_score_kernel<kScoreDepth, true>), grid, block, 0, stream, d_planar, d_gains, d_voices, d_block_first, d_entries, d_init, d_out, voice_row,
                           (uint32_t)n_voice, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, block_shift - kScoreGroupShift, (uint32_t)first_block, raw);
    else
        hipLaunchKernelGGL((dusp_score_kernel<kScoreDepth, false>), grid, block, 0, stream, d_planar, d_gains, d_voices, d_block_first, d_entries, d_init, d_out, voice_row,
                           (uint32_t)n_voice, (uint32_t)n_total, (uint32_t)w_lo, (uint32_t)w_hi, G.first, G.count, block_shift - kScoreGroupShift, (uint32_t)first_block, raw);
    return hipGetLastError();
}

}  // namespace dusp
