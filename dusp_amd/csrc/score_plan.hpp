// score_plan.hpp — the plan of a score launch (score_engine.hip and its kin): which voices of a tile a block of the timeline has to look at.  Plain data
// in, plain data out: host code only (no HIP), checked against brute force on the CPU (tests/native/score_plan_check.cpp).
//
// A score places voice k — a row of n_voice samples per channel, of which the first len_k count — at sample onset_k of a timeline of
// n_total samples (dusp_amd/mix.py score_chain is the contract).  A lane of the kernel owns one sample of the timeline and adds, in index
// order, the voices that cover it.  Testing every voice of the tile against every sample would be n tests for a handful of hits, so the
// timeline is cut into blocks of B samples — a power of two, at least the kScoreGroup samples one workgroup covers — and every block gets
// the ascending list of the voices whose span, clipped to the timeline, intersects it: CSR, block_first[n_blocks + 1] into entries[].
// A lane walks its block's list and tests only those.  The list costs 4 bytes per (voice, block) pair; B is doubled until the whole
// plan fits the byte budget (kScorePlanBytes by default), or one block covers the window.
//
// All arithmetic is in int64 and nothing overflows for any int64 onset: a voice is clipped before anything is added to its onset.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dusp {

constexpr uint32_t kScoreGroupShift = 8;                    // one workgroup: 256 lanes, one sample each
constexpr uint32_t kScoreGroup = 1u << kScoreGroupShift;
constexpr size_t kScorePlanBytes = (size_t)16 << 20;        // what a plan may take on the device: voices + block_first + entries
constexpr uint64_t kScoreRowMax = (uint64_t)1 << 31;        // floats in one voice's PCM, and in the timeline's (the kernel's 32-bit sample positions)

// A voice as the kernel reads it: timeline samples [lo, hi) take planar[k][c][t - onset].  (lo < hi <= n_total <= 2^31, and
// -2^31 < onset < 2^31 for every voice that is in a list; the others are never read.)
// (16 bytes on a 16-byte boundary: one four-dword scalar load a voice)
struct alignas(16) ScoreVoice {
    int64_t onset;
    uint32_t lo, hi;
};

// A voice as the rows kernel reads it: timeline samples [lo, hi) take ((const float *)row)[c * stride + (t - onset)].
// (32 bytes on a 32-byte boundary: one eight-dword scalar load a voice)
// A record that is in no list (lo == hi == 0) still carries a READABLE row: the first listed voice's.  The kernel points the load of a
// lane that an entry does not cover at the entry's own row[0], and the entries it may meet are (a) its list's, (b) another list's — both
// name voices with lo < hi, whose rows hold at least one float — and (c) the padding's zeros, which name voice 0 whether or not voice 0
// is anywhere on the timeline (its own row may be NULL or empty).
struct alignas(32) ScoreRow {
    int64_t onset;
    uint32_t lo, hi;
    uint64_t row;     // device address of the voice's channel 0, sample 0
    uint32_t stride;  // floats from one channel of this voice to the next (a stereo plan's mono rows: kScoreStrideMono, kScoreStridePanned)
    uint32_t pad;     // 0; a voice with a fraction of a sample in its onset (score_rows_plan's fracs): its unclipped length, never 0
};
static_assert(sizeof(ScoreRow) == 32, "one eight-dword scalar load");

// entries[] ends in this many zeros behind the last list: the kernel reads a batch of 8 indices with one wide scalar load, also where
// fewer than 8 of them are left in the list, and masks the rest
constexpr size_t kScoreEntryPad = 8;

// The plan of one launch over records of either kind
template <class Record>
struct ScorePlanT {
    int64_t t_lo = 0, t_hi = 0;   // the union of the voices' clipped spans (t_lo == t_hi: no voice reaches the timeline)
    int64_t w_lo = 0, w_hi = 0;   // the window of the timeline the plan covers: the union, or the whole timeline
    uint32_t block_shift = kScoreGroupShift;  // B = 1 << block_shift
    uint64_t first_block = 0;     // block_first[0] is block first_block of the timeline (w_lo >> block_shift)
    std::vector<Record> voices;          // [n]; lo == hi == 0 for a voice that appears nowhere
    std::vector<uint32_t> block_first;   // [n_blocks + 1]
    std::vector<uint32_t> entries;       // voice indices, ascending within a block; then kScoreEntryPad zeros (block_first.back() is where they begin)
    size_t n_entries() const { return block_first.empty() ? 0 : block_first.back(); }
    size_t n_blocks() const { return block_first.empty() ? 0 : block_first.size() - 1; }
    size_t bytes() const { return voices.size() * sizeof(Record) + (block_first.size() + entries.size()) * sizeof(uint32_t); }
};
using ScorePlan = ScorePlanT<ScoreVoice>;    // score_engine.hip: the voices of one contiguous batch
using ScoreRowsPlan = ScorePlanT<ScoreRow>;  // score_rows_engine.hip and what stands on it: every voice a buffer of its own

// The lists of a plan whose records (ScoreVoice, ScoreRow: anything with lo and hi) are made: the block, doubled from kScoreGroup until
// records + block_first + entries (+ kScoreEntryPad) fit budget_bytes or one block covers the window [w_lo, w_hi), w_lo < w_hi; then the
// CSR lists, every one ascending, and the padding's zeros behind the last.
template <class Record>
inline void score_plan_lists(const std::vector<Record> &voices, int64_t w_lo, int64_t w_hi, size_t budget_bytes, uint32_t &block_shift, uint64_t &first_block,
                             std::vector<uint32_t> &block_first, std::vector<uint32_t> &entries) {
    const size_t n = voices.size();
    auto blocks_of = [&](uint32_t shift, uint64_t &first, uint64_t &count, uint64_t &n_entries) {
        first = (uint64_t)w_lo >> shift;
        count = (((uint64_t)w_hi - 1) >> shift) - first + 1;
        n_entries = 0;
        for (const Record &v : voices)
            if (v.hi > v.lo) n_entries += ((uint64_t)(v.hi - 1) >> shift) - ((uint64_t)v.lo >> shift) + 1;
    };
    uint32_t shift = kScoreGroupShift;
    uint64_t first, count, n_entries;
    for (;; shift++) {
        blocks_of(shift, first, count, n_entries);
        const uint64_t bytes = (uint64_t)n * sizeof(Record) + (count + 1 + n_entries + kScoreEntryPad) * sizeof(uint32_t);
        if ((bytes <= budget_bytes && n_entries <= 0xffffffffull) || count == 1) break;
    }
    block_shift = shift;
    first_block = first;
    block_first.assign((size_t)count + 1, 0u);
    for (const Record &v : voices)  // counts, one place up ...
        if (v.hi > v.lo)
            for (uint64_t b = ((uint64_t)v.lo >> shift) - first, b1 = ((uint64_t)(v.hi - 1) >> shift) - first; b <= b1; b++) block_first[(size_t)b + 1]++;
    for (size_t b = 0; b < (size_t)count; b++) block_first[b + 1] += block_first[b];  // ... become the lists' starts
    entries.assign((size_t)n_entries + kScoreEntryPad, 0u);
    std::vector<uint32_t> at(block_first.begin(), block_first.end() - 1);
    for (size_t k = 0; k < n; k++) {  // voices in index order: every list comes out ascending
        const Record &v = voices[k];
        if (v.hi > v.lo)
            for (uint64_t b = ((uint64_t)v.lo >> shift) - first, b1 = ((uint64_t)(v.hi - 1) >> shift) - first; b <= b1; b++) entries[at[(size_t)b]++] = (uint32_t)k;
    }
}

// What a planner ends with, its records clipped and [t_lo, t_hi) the union of their spans (t_hi <= t_lo: no voice reaches the timeline of
// `total` samples): the window — the whole timeline or the union — and, unless it is empty (nothing to launch), the lists.
template <class Record>
inline void score_plan_finish(ScorePlanT<Record> &P, int64_t t_lo, int64_t t_hi, int64_t total, bool whole_timeline, size_t budget_bytes) {
    if (t_hi <= t_lo) t_lo = t_hi = 0;
    P.t_lo = t_lo;
    P.t_hi = t_hi;
    P.w_lo = whole_timeline ? 0 : t_lo;
    P.w_hi = whole_timeline ? total : t_hi;
    if (P.w_hi > P.w_lo) score_plan_lists(P.voices, P.w_lo, P.w_hi, budget_bytes, P.block_shift, P.first_block, P.block_first, P.entries);
}

// The plan as the device reads it, appended to `image` on a boundary of the record's own alignment — 16 bytes for ScoreVoice, 32 for
// ScoreRow (the image itself starts on one on the device): voices, block_first, entries.  Returns the byte offset of the voices;
// block_first follows at + n * sizeof(Record), the entries (and their padding) behind it.
template <class Record>
inline size_t score_plan_pack(const ScorePlanT<Record> &P, std::vector<unsigned char> &image) {
    const size_t at = (image.size() + alignof(Record) - 1) & ~(alignof(Record) - 1);
    image.resize(at + P.bytes());
    unsigned char *p = image.data() + at;
    auto put = [&](const void *src, size_t n_bytes) {
        if (n_bytes) std::copy((const unsigned char *)src, (const unsigned char *)src + n_bytes, p);
        p += n_bytes;
    };
    put(P.voices.data(), P.voices.size() * sizeof(Record));
    put(P.block_first.data(), P.block_first.size() * sizeof(uint32_t));
    put(P.entries.data(), P.entries.size() * sizeof(uint32_t));
    return at;
}

// lengths: nullptr for n_voice everywhere.  whole_timeline: the plan covers [0, n_total) (a launch that writes every sample), else the
// union window only (a raw launch in place: samples no voice of the tile reaches stay as they are).
// Returns -1 when the plan is made, else the index of the first voice whose length is not in [0, n_voice].
// Needs n <= 2^32 - 1, n_voice and n_total <= kScoreRowMax.
inline int64_t score_plan(const int64_t *onsets, const int64_t *lengths, size_t n, uint64_t n_voice, uint64_t n_total, bool whole_timeline,
                          size_t budget_bytes, ScorePlan &P) {
    P = ScorePlan();
    P.voices.assign(n, ScoreVoice{0, 0u, 0u});
    const int64_t total = (int64_t)n_total;
    int64_t t_lo = total, t_hi = 0;
    for (size_t k = 0; k < n; k++) {
        const int64_t len = lengths ? lengths[k] : (int64_t)n_voice, onset = onsets[k];
        if (len < 0 || len > (int64_t)n_voice) return (int64_t)k;
        if (len == 0 || onset >= total || onset <= -len) continue;  // empty, behind the end, wholly in front of sample 0
        // here -2^31 <= -len < onset < n_total <= 2^31: onset + len cannot overflow
        const int64_t lo = std::max<int64_t>(onset, 0), hi = std::min(onset + len, total);
        P.voices[k] = ScoreVoice{onset, (uint32_t)lo, (uint32_t)hi};
        t_lo = std::min(t_lo, lo);
        t_hi = std::max(t_hi, hi);
    }
    score_plan_finish(P, t_lo, t_hi, total, whole_timeline, budget_bytes);
    return -1;
}

// ---- space: a whole shift, two weights and a gain per voice and channel (score_space_engine.hip; dusp_amd/mix.py score_chain_rows_placed) ----

// What the space kernel needs of voice k at channel c, made on the host from a delay D (finite, 0 <= D <= 2^24 samples) and a gain G:
// shift = floor(D), w1 = D - shift (exact in f64), w0 = 1.0 - w1 (the IEEE subtraction itself), as the reference's MonoDelay writes a
// sample to the ring slots floor and ceil of its delayed position with the weights 1 - frac and frac (MonoDelay.js:24-26), behind a
// Gain whose factor is G (Gain.js:22).  w1 == 0: one tap, the voice shifted by whole samples.  The half the addresses need (w1's test,
// the shift) is the second 16 bytes, the half only the arithmetic needs the first: two four-dword scalar loads.
// (32 bytes on a 32-byte boundary)
constexpr int64_t kScoreSpaceShiftMax = (int64_t)1 << 24;
constexpr size_t kScoreSpaceChannelsMax = 8;
struct alignas(32) ScoreSpaceTap {
    double w0, gain;
    double w1;
    int64_t shift;
};
static_assert(sizeof(ScoreSpaceTap) == 32, "two four-dword scalar loads");

inline ScoreSpaceTap score_space_tap(double delay, double gain) {
    const double whole = std::floor(delay), frac = delay - whole;
    return ScoreSpaceTap{1.0 - frac, gain, frac, (int64_t)whole};
}

// ---- rows: every voice a buffer of its own (score_rows_engine.hip; dusp_amd/mix.py score_chain_rows is the contract) ----

// score_plan over voices of their own row lengths: row_samples[k] samples a channel (which is also the voice's channel stride) at device
// address rows[k] (nullptr: all 0, for a plan that is only looked at).  lengths: nullptr for row_samples[k] everywhere.
// fracs (nullptr: none): voice k starts at onset_k + fracs[k] samples, 0 <= fracs[k] < 1 (the caller has checked that).  A voice whose
// fraction is not 0 is heard through two taps (score_frac_engine.hip; dusp_amd/mix.py two_tap_terms) and covers ONE MORE sample, the
// ceil tap of its last: its span is [onset, onset + len + 1) before clipping, it is dropped only when onset + len + 1 <= 0 (a voice
// that ends exactly at sample 0 still has its tail tap ON sample 0), and its record carries pad = len — the unclipped length, which the
// kernel needs to tell s < len where hi is clipped by the timeline, and, being non-zero, the wave-uniform mark of a voice with a
// fraction.  A voice without one has pad = 0 and is today's voice.  t_hi and the union window grow by that one sample.
// The weights of such voices go up as a parallel array of ScoreFrac (below), 16 bytes a voice ON TOP of the plan's byte budget, which
// counts records and lists as before.
// taps (nullptr: none; then fracs is nullptr): voice k reaches channel c of taps_channels >= 1 behind a whole shift of taps[k *
// taps_channels + c].shift samples, 0 <= shift <= kScoreSpaceShiftMax, through two taps where that entry's w1 is not 0 (ScoreSpaceTap
// above; score_space_engine.hip; dusp_amd/mix.py score_chain_rows_placed).  The voice's span is the UNION over its channels,
// [onset + min shift, onset + max(shift + len + (w1 != 0))) before clipping, and its record carries pad = len whether or not any of its
// taps has a fraction: the kernel tells channel by channel which samples the voice covers.  A voice whose onset lies at or behind the
// timeline's end takes no part whatever its shifts are (they are not negative), so nothing is ever added to an onset near the top of
// int64; one far in front of sample 0 is dropped before its end is clipped.  The taps go up as a parallel array, 32 bytes a voice and
// channel ON TOP of the plan's byte budget.
// row_channels (nullptr: every row has the call's one channel count and its record's stride is row_samples[k], as ever): voice k is a
// row of row_channels[k] channels, 1 or 2, into a timeline of two (score_stereo_engine.hip; dusp_amd/mix.py score_chain_rows_stereo), and
// its record's stride says which kind of voice it is: row_samples[k], the floats from channel 0 to channel 1, for a row of two channels
// (1 .. 2^30), kScoreStridePanned for a mono row with a finite pans[k], kScoreStrideMono for a mono row that is not placed (pans
// nullptr, or pans[k] NaN).  Spans, lists and everything else are the same arithmetic.
// Returns -1 when the plan is made, else the index of the first voice whose length is not in [0, row_samples[k]].
// Needs n <= 2^32 - 1, row_samples and n_total <= kScoreRowMax.
constexpr uint32_t kScoreStrideMono = 0u, kScoreStridePanned = 0xffffffffu;
struct ScorePlacing {  // what places the voices of a rows plan, each as described above; all null: plain rows
    const double *fracs = nullptr;
    const ScoreSpaceTap *taps = nullptr;
    size_t taps_channels = 0;
    const uint32_t *row_channels = nullptr;
    const float *pans = nullptr;
};
inline int64_t score_rows_plan(const int64_t *onsets, const int64_t *lengths, const uint32_t *row_samples, const uint64_t *rows, size_t n, uint64_t n_total,
                               bool whole_timeline, size_t budget_bytes, ScoreRowsPlan &P, const ScorePlacing &by) {
    P = ScoreRowsPlan();
    P.voices.assign(n, ScoreRow{0, 0u, 0u, 0u, 0u, 0u});
    const int64_t total = (int64_t)n_total;
    int64_t t_lo = total, t_hi = 0;
    size_t first_listed = n;
    for (size_t k = 0; k < n; k++) {
        const int64_t len = lengths ? lengths[k] : (int64_t)row_samples[k], onset = onsets[k];
        if (len < 0 || len > (int64_t)row_samples[k]) return (int64_t)k;
        if (by.taps) {
            // the union of the channels' spans, relative to the onset: [first, last), 0 <= first < last <= 2^24 + 2^31 + 1
            int64_t first = INT64_MAX, last = 0;
            for (size_t c = 0; c < by.taps_channels; c++) {
                const ScoreSpaceTap &T = by.taps[k * by.taps_channels + c];
                first = std::min(first, T.shift);
                last = std::max(last, T.shift + len + (T.w1 != 0.0 ? 1 : 0));
            }
            if (len == 0 || onset >= total || onset <= -last) continue;  // (onset + first >= total: below, where the sum cannot overflow)
            // here -2^33 < -last < onset < n_total <= 2^31: onset + first and onset + last cannot overflow
            if (onset + first >= total) continue;
            const int64_t lo = std::max<int64_t>(onset + first, 0), hi = std::min(onset + last, total);
            P.voices[k] = ScoreRow{onset, (uint32_t)lo, (uint32_t)hi, rows ? rows[k] : 0, row_samples[k], (uint32_t)len};
            if (first_listed == n) first_listed = k;
            t_lo = std::min(t_lo, lo);
            t_hi = std::max(t_hi, hi);
            continue;
        }
        const bool two_taps = by.fracs && by.fracs[k] != 0.0;
        // empty, behind the end, wholly in front of sample 0 (two taps: the tail tap too, onset + len + 1 <= 0)
        if (len == 0 || onset >= total || (two_taps ? onset < -len : onset <= -len)) continue;
        // here -2^31 <= -len <= onset < n_total <= 2^31: onset + len + 1 cannot overflow
        const int64_t lo = std::max<int64_t>(onset, 0), hi = std::min(onset + len + (two_taps ? 1 : 0), total);
        const uint32_t stride = !by.row_channels || by.row_channels[k] == 2 ? row_samples[k] : by.pans && std::isfinite(by.pans[k]) ? kScoreStridePanned : kScoreStrideMono;
        P.voices[k] = ScoreRow{onset, (uint32_t)lo, (uint32_t)hi, rows ? rows[k] : 0, stride, two_taps ? (uint32_t)len : 0u};
        if (first_listed == n) first_listed = k;
        t_lo = std::min(t_lo, lo);
        t_hi = std::max(t_hi, hi);
    }
    if (first_listed < n)  // (the records nobody adds from: readable all the same, see ScoreRow)
        for (ScoreRow &v : P.voices)
            if (v.hi == v.lo) v.row = P.voices[first_listed].row;
    score_plan_finish(P, t_lo, t_hi, total, whole_timeline, budget_bytes);
    return -1;
}

// ---- pans: a place in the stereo field per voice of a rows plan (score_pan_engine.hip; dusp_amd/mix.py score_chain_rows_panned) ----

// What the panned kernel multiplies a voice's sample by, made on the host: the reference's Pan unit (Pan.js:21-22) gives a sample x of a
// voice panned to p
//     left = f32(((f64(x) * (1 - f64(p))) / 2) * comp),   right = f32(((f64(x) * (1 + f64(p))) / 2) * comp),   comp = 10^((1 - |p|) * 1.5 / 20)
// every f64 operation rounded by itself.  lm and rp are the IEEE operations 1 -+ f64(p) themselves.  The kernel computes
// f32((f64(x) * lm) * ch) with ch = comp / 2 — one division a voice on the host instead of two a sample on the device — which is the same
// f32: with y = f64(x) * lm, y / 2 is exact (y is 0, infinite, NaN, or no smaller than 2^-149 * 2^-24: halving a double so far above
// the subnormals only lowers its exponent) and, as long as comp is a normal double (|p| < 4100), so is comp / 2; then (y / 2) * comp and
// y * (comp / 2) are roundings of one and the same real number.  A comp that has underflowed to a subnormal or to 0 may lose its last
// bit in the halving, and there both products are below 1e-260 in magnitude whatever x and p are: the same +-0 in f32, or the same NaN
// from an infinite x.  tests/native/score_pan_kernel_check.cpp holds both statements.
// (32 bytes on a 32-byte boundary: one eight-dword scalar load a voice, as ScoreRow)
struct alignas(32) ScorePan {
    double lm, rp;  // 1 - f64(p), 1 + f64(p)
    double ch;      // comp / 2
    double pad;
};
static_assert(sizeof(ScorePan) == 32, "one eight-dword scalar load");

inline ScorePan score_pan_coefficients(float pan, double comp) { return ScorePan{1.0 - (double)pan, 1.0 + (double)pan, comp / 2.0, 0.0}; }

// ---- fractions: onsets between samples (score_frac_engine.hip; dusp_amd/mix.py two_tap_terms) ----

// The weights of a voice's two taps, made on the host: the reference's Delay (Delay.js:36-38) writes a sample to the ring slot at
// floor(delay) with the weight 1 - frac and to the next with frac.  w0 = 1.0 - frac is the IEEE subtraction itself.  One record a voice
// of the plan, whole voices included (theirs is never read): a parallel array behind the plan in the context's image, as ScorePan.
// (16 bytes on a 16-byte boundary: one four-dword scalar load a voice)
struct alignas(16) ScoreFrac {
    double w0, w1;  // 1.0 - frac, frac
};
static_assert(sizeof(ScoreFrac) == 16, "one four-dword scalar load");

inline ScoreFrac score_frac_weights(double frac) { return ScoreFrac{1.0 - frac, frac}; }

// ---- sends: a level per voice and bus (score_send_engine.hip; dusp_amd/mix.py score_chain_sends) ----

// What a voice gives to each of up to kScoreBusMax buses: the f32 factor of its dry term.  One record a voice of the plan, a parallel
// array behind the plan in the context's image and on top of its byte budget, as ScorePan and ScoreFrac; the levels of buses the call
// does not have are 0 and are not read.
// (16 bytes on a 16-byte boundary: one four-dword scalar load a voice)
constexpr size_t kScoreBusMax = 4;
struct alignas(16) ScoreSend {
    float level[kScoreBusMax];
};
static_assert(sizeof(ScoreSend) == 16, "one four-dword scalar load");

// ---- tracks: sub-mixes of a piece through circuits of their own (score_tracks_engine.hip; dusp_amd/mix.py track_mix) ----
constexpr size_t kScoreTrackMax = 8;

}  // namespace dusp
