// score_device.hpp — what the six score kernels share (score_engine.hip, score_rows_engine.hip, score_pan_engine.hip,
// score_frac_engine.hip, score_space_engine.hip, score_stereo_engine.hip): `x || 0`, a plan record as one wide load, the pan coefficients
// that are used as two loads, the two-tap term, the typedefs of a batch's indices and of a row's floats, the head of every kernel (lane
// to sample, window test) and the groups a launch covers.  The lookup of the block's list behind that head stays in
// each kernel: as a shared function it changed the order of two scalar moves in three of the four device listings
// (profiles/score_refactor.txt).  Like the engines, this compiles for the host under tests/native/hip_host_stub, where the kernels' text
// runs lane after lane.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "score_plan.hpp"

namespace dusp {

// NaN and -0 leave as +0 (`x || 0`)
static __device__ __forceinline__ float score_or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }

// the one argument the STEMS instance of a kernel takes beyond the plain one's, as a parameter pack of one float * or of nothing
// (score_tracks_engine.hip, score_send_engine.hip's return): the pointer, or nullptr where the pack is empty
static __device__ __forceinline__ float *score_stem_direct() { return nullptr; }
static __device__ __forceinline__ float *score_stem_direct(float *stem_direct) { return stem_direct; }

// a record of 32 bytes (ScoreRow, ScorePan) or of 16 (ScoreFrac) as ONE load: its words as a vector (field by field the compiler splits
// a ScoreRow into four, two and one dwords)
typedef uint32_t ScoreWords8 __attribute__((vector_size(32), may_alias));
typedef uint32_t ScoreWords4 __attribute__((vector_size(16), may_alias));
template <class T>
static __device__ __forceinline__ T score_load32(const T *p) {
    static_assert(sizeof(T) == 32, "eight dwords");
    const ScoreWords8 w = *(const ScoreWords8 *)p;
    T r;
    __builtin_memcpy(&r, &w, sizeof r);
    return r;
}
static __device__ __forceinline__ ScoreFrac score_load16(const ScoreFrac *p) {
    const ScoreWords4 w = *(const ScoreWords4 *)p;
    ScoreFrac r;
    __builtin_memcpy(&r, &w, sizeof r);
    return r;
}

// a voice's pan coefficients without the record's unused last quarter: four dwords and two, six scalar registers an entry, not eight
// (score_frac_engine.hip, score_stereo_engine.hip)
struct ScorePanUsed {
    double lm, rp, ch;
};
typedef uint32_t ScoreWords2 __attribute__((vector_size(8), may_alias));
static __device__ __forceinline__ ScorePanUsed score_load_pan(const ScorePan *p) {
    const ScoreWords4 a = *(const ScoreWords4 *)p;
    const ScoreWords2 b = *(const ScoreWords2 *)&p->ch;
    ScorePanUsed r;
    __builtin_memcpy(&r.lm, &a, sizeof a);
    __builtin_memcpy(&r.ch, &b, sizeof b);
    return r;
}

// the two taps of one timeline sample (score_frac_engine.hip says where they come from; score_stereo_engine.hip and, with a tap's own
// weights, score_space_engine.hip): x0 = x[s] (used where s < len), x1 = x[s - 1] (used where s >= 1), w0 = 1.0 - frac, w1 = frac
static __device__ __forceinline__ float score_two_tap_term(float x0, float x1, bool has0, bool has1, double w0, double w1) {
    const float c = (float)((double)x1 * w1);
    const double floor_tap = (double)x0 * w0;
    const float both = (float)((double)c + floor_tap);
    return has1 ? (has0 ? both : c) : (float)floor_tap;
}

// a batch's eight indices as one load too: contiguous in entries[], on a 4-byte boundary only
typedef uint32_t ScoreEntryWords __attribute__((vector_size(32), aligned(4), may_alias));

// a row's address is a number in the record: on the device it names GLOBAL memory (a global load, not a flat one)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) float *ScoreRowFloats;
#else
typedef const float *ScoreRowFloats;
#endif

// The head of every kernel: a lane owns sample t of the timeline, lane threadIdx.x of its workgroup's `group` of kScoreGroup samples
// (group <= 2^23, t < 2^31 + 256); false: the launch's window [w_lo, w_hi) does not hold it and the lane is done.
static __device__ __forceinline__ bool score_lane_sample(uint32_t group, uint32_t w_lo, uint32_t w_hi, uint32_t &t) {
    t = (group << kScoreGroupShift) + threadIdx.x;
    return t >= w_lo && t < w_hi;
}

// The groups of kScoreGroup samples a launch over the window [w_lo, w_hi) covers, 0 <= w_lo < w_hi <= 2^31: the first (the kernels'
// group0) and how many (per channel).  The grid is that many workgroups of kScoreGroup lanes, times the channels a lane does not own.
struct ScoreGroups {
    uint32_t first, count;
};
inline ScoreGroups score_groups(uint64_t w_lo, uint64_t w_hi) {
    const uint32_t first = (uint32_t)(w_lo >> kScoreGroupShift);
    return ScoreGroups{first, (uint32_t)((w_hi - 1) >> kScoreGroupShift) - first + 1};
}

}  // namespace dusp
