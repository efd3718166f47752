// abi_internal.hpp — what the translation units of the C ABI (include/dusp_hip.h) share: the context and program objects, device workspaces
// and their registry, the error macros and the exception firewall, the engines' launch functions, and the internal functions that cross files.
//   abi_context.hip     contexts, knobs, wave tables, pinned host memory
//   abi_program.hip     build / continue / destroy, program info, state download
//   abi_render.hip      device renders: one step per engine
//   abi_render_jit.hip  ... the render on a compiled circuit kernel
//   abi_deliver.hip     interleave / peak / encode, host renders and their delivery
//   abi_mix.hip         mix of a batch on the device, the tiles of a large batch, the host render of a mix
//   abi_score.hip       scores: plans' image, the one launch path, device entries with a plan, the host render of a score (abi_score.hpp: what
//                       the files that launch score kernels share)
//   abi_piece.hip       pieces: the host renders of several instruments, with a master, buses, tracks, stems and meters
//   abi_score_sweep.hip device entries without a plan: the buses' return, the tracks' mix, the common peak
//   abi_meter.hip       meters: RMS and BS.1770 loudness of signals on the device, and the gates on the host
//   abi_loudness.hip    the true peak of signals on the device
//   abi_limiter.hip     the linked look-ahead true-peak limiter of signals on the device
#pragma once
#include <limits>
#include <cmath>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dusp_hip.h"
#include "device_types.hpp"
#include "fused_plan.hpp"
#include "jit_codegen.hpp"
#include "limiter_plan.hpp"
#include "limiter_release_plan.hpp"
#include "meter_plan.hpp"
#include "program.hpp"
#include "score_plan.hpp"
#include "truepeak_plan.hpp"

namespace dusp {
hipError_t launch_chunk_engine(const ChunkArgs &a, hipStream_t stream);
hipError_t launch_state_init(double *state, const double *init, uint32_t n_slots, uint32_t n_pad, hipStream_t stream);
hipError_t launch_fill(float *out, size_t n_floats, float value, hipStream_t stream);
hipError_t launch_wave_to_chunk(const float *wave_rings, float *chunk_rings, uint64_t ring_samples, const float *saved_bufs, float *chunk_scratch,
                                uint32_t n_bufs, uint32_t n_inst, uint32_t n_pad, hipStream_t stream);
hipError_t launch_chunk_to_wave(const float *chunk_rings, float *wave_rings, uint64_t ring_samples, const float *chunk_scratch, float *saved_bufs, uint32_t n_bufs,
                                uint32_t n_inst, uint32_t n_pad, const double *state, double *init_state, uint32_t n_slots, hipStream_t stream);
hipError_t launch_interleave(const float *d_planar, float *d_out, uint32_t n_instances, uint32_t n_channels, uint64_t n_samples, hipStream_t stream);
hipError_t launch_pcm_peak(const float *d_planar, float *d_peaks, uint32_t n_instances, uint32_t n_channels, uint64_t n_samples, int n_cus, hipStream_t stream);
hipError_t launch_pcm_encode(const float *d_planar, const float *d_peaks, int format, int normalise, void *d_out, uint32_t n_instances, uint32_t n_channels,
                             uint64_t n_samples, int n_cus, hipStream_t stream);
uint64_t pcm_encode_tiles(uint64_t n_instances, uint32_t n_channels, uint64_t n_samples, int format);
hipError_t launch_mix(const float *d_planar, const float *d_gains, const float *d_init, float *d_out, uint64_t row_len, uint32_t n_inst, int raw, int n_cus,
                      int width_knob, int depth_knob, hipStream_t stream);
hipError_t launch_score(const float *d_planar, const float *d_gains, const ScoreVoice *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries,
                        const float *d_init, float *d_out, uint32_t n_channels, uint64_t n_voice, uint64_t n_total, uint64_t w_lo, uint64_t w_hi,
                        uint32_t block_shift, uint64_t first_block, int raw, hipStream_t stream);
hipError_t launch_score_rows(const float *d_gains, const ScoreRow *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries, const float *d_init, float *d_out,
                             uint32_t n_channels, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw,
                             hipStream_t stream);
hipError_t launch_score_pan(const float *d_gains, const ScorePan *d_pans, const ScoreRow *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries,
                            const float *d_init, float *d_out, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw,
                            hipStream_t stream);
hipError_t launch_score_frac(const float *d_gains, const ScorePan *d_pans, const ScoreFrac *d_fracs, const ScoreRow *d_voices, const uint32_t *d_block_first,
                             const uint32_t *d_entries, const float *d_init, float *d_out, uint32_t n_channels, uint64_t n_total, uint64_t w_lo, uint64_t w_hi,
                             uint32_t block_shift, uint64_t first_block, int raw, hipStream_t stream);
hipError_t launch_score_space(const float *d_gains, const ScoreSpaceTap *d_taps, const ScoreRow *d_voices, const uint32_t *d_block_first, const uint32_t *d_entries,
                              const float *d_init, float *d_out, uint32_t n_channels, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block,
                              int raw, hipStream_t stream);
hipError_t launch_score_stereo(const float *d_gains, const ScorePan *d_pans, const ScoreFrac *d_fracs, const ScoreRow *d_voices, const uint32_t *d_block_first,
                               const uint32_t *d_entries, const float *d_init, float *d_out, uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift,
                               uint64_t first_block, int raw, hipStream_t stream);
hipError_t launch_score_send(const float *d_gains, const ScoreSend *d_sends, const ScorePan *d_pans, const ScoreRow *d_voices, const uint32_t *d_block_first,
                             const uint32_t *d_entries, const float *d_init, float *d_out, const float *d_send_init, float *d_send_out, uint32_t n_buses, uint32_t n_channels,
                             uint64_t n_total, uint64_t w_lo, uint64_t w_hi, uint32_t block_shift, uint64_t first_block, int raw, bool pan, hipStream_t stream);
hipError_t launch_score_return(const float *d_dry, const float *const *d_wets, uint32_t n_buses, float *d_out, float *d_stem_direct, float *const *d_stem_buses, uint64_t n, int raw,
                               hipStream_t stream);
hipError_t launch_score_tracks(const float *d_direct, const float *const *d_tracks, const float *h_faders, const float *h_levels, uint32_t n_tracks, uint32_t n_buses,
                               float *d_out, const float *d_feed_init, float *d_feed_out, float *d_stem_direct, float *const *d_stem_tracks, uint64_t n, int raw,
                               hipStream_t stream);
hipError_t launch_pcm_peak_common(const float *d_peaks, float *d_common, uint32_t n, hipStream_t stream);
hipError_t launch_meter(const float *d_planar, uint32_t n_signals, uint32_t n_channels, uint64_t n, uint32_t hop, const MeterCoef &k, double *d_scratch, double *d_sumsq,
                        double *d_hops, hipStream_t stream, hipEvent_t *marks);
hipError_t launch_true_peak(const float *d_planar, uint64_t rows, uint64_t n, uint32_t F, const TruePeakTaps &taps, int n_cus, uint64_t *d_words, hipStream_t stream);
hipError_t launch_limit_envelope(const float *d_planar, uint64_t rows, uint64_t n, uint32_t F, const TruePeakTaps &taps, double T, uint32_t L, int n_cus, uint32_t *d_q,
                                 uint64_t *d_smallest, hipStream_t stream);
hipError_t launch_limit_apply(float *d_planar, uint64_t rows, uint64_t n, uint32_t L, int n_cus, const uint32_t *d_q, uint64_t *d_smallest, double *d_gain, hipStream_t stream);
hipError_t launch_limit_hold(uint64_t n, uint32_t L, uint32_t R, int n_cus, const uint32_t *d_q, uint32_t *d_held, uint32_t *d_summary, hipStream_t stream);
hipError_t launch_limit_release(uint64_t n, uint32_t L, uint32_t R, int n_cus, uint32_t *d_held, const uint32_t *d_summary, hipStream_t stream);
hipError_t launch_limit_mean_apply(float *d_planar, uint64_t rows, uint64_t n, uint32_t L, int n_cus, const uint32_t *d_held, uint64_t *d_smallest, double *d_gain, hipStream_t stream);
hipError_t launch_fused(const FusedPlan &plan, const FusedLaunch &L, hipStream_t stream);
hipError_t launch_wave_engine(WaveArgs A, bool lds_table_ok, int max_waves_cap, hipStream_t stream);
hipError_t launch_sumchain(const FusedPlan &plan, const FusedLaunch &L, const SumVoice *d_voices, int gb, hipStream_t stream);
}  // namespace dusp

extern thread_local std::string g_error;  // dusp_last_error(NULL): failures of calls that have no context (abi_context.hip)

struct dusp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    float *d_tables = nullptr;  // [kNumTables][table_stride]
    uint32_t table_len = 0;     // entries per uploaded table (= sample_rate + 1), 0 until the first upload
    uint32_t table_stride = 0;
    bool table_set[dusp::kNumTables] = {false, false, false, false, false};
    bool table_antisym[dusp::kNumTables] = {false, false, false, false, false};
    bool table_finite[dusp::kNumTables] = {false, false, false, false, false};
    bool table_fx32_ok[dusp::kNumTables] = {false, false, false, false, false};  // min nonzero |T| >= 2^-20
    int table_bound[dusp::kNumTables] = {1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000};  // every |entry| <= 2^bound (1000: not finite / not set)
    int table_delta[dusp::kNumTables] = {0, 0, 0, 0, 0};  // the lerp's delta form (device_util.hpp lerp_delta): 2 every T[t+1] - T[t] is an f32, 1 exact in f64, 0 neither (or not finite)
    // TABLE_FORM_*: the uploaded table equals a closed form of the index (saw, square, triangle) or of the sine table's entry
    // (8bit) on EVERY entry, bit for bit — checked at upload — so kernels may evaluate it instead of gathering (device_util.hpp)
    int table_form[dusp::kNumTables] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<float> h_tables[2];  // host copies of table 0 (sine) and table 4 (8bit) for that check
    int n_cus = 256;
    dusp::Knobs knobs;  // A/B switches, read from the environment once (dusp_ctx_create)
    // pinned host buffers handed out by dusp_host_alloc (in_use) or waiting for reuse
    struct HostBuf { void *p; size_t bytes; bool in_use; };
    std::vector<HostBuf> host_pool;
    std::mutex host_pool_mutex;  // dusp_host_free may come from a finalizer thread (a garbage collector) while the owner allocates
    // bumped by every dusp_table_upload: compiled kernels are generated against what the context knows about its tables
    // (closed forms, antisymmetry, the LDS image's table), so a program's generated text is dropped when this has moved on
    uint64_t table_generation = 0;
    bool tables_guarded = false;
    // the plans of score launches (score_plan.hpp), as the device reads them: one image per call, built in h_score_plan and uploaded into
    // d_score_plan on the call's stream.  score_uploaded: the last upload has read h_score_plan (waited for before the next call rewrites
    // it); score_done: the last launch has read d_score_plan (the next call's stream waits for it before the upload overwrites it)
    std::vector<unsigned char> h_score_plan;
    unsigned char *d_score_plan = nullptr;
    size_t score_plan_cap = 0;
    hipEvent_t score_uploaded = nullptr, score_done = nullptr;
    // the last dusp_score_device call, for dusp_score_last_ms: events around its plan upload (score_up0 .. score_uploaded) and around its
    // launch (score_t0 .. score_t1), and what its plan took on the host
    hipEvent_t score_up0 = nullptr, score_t0 = nullptr, score_t1 = nullptr;
    double score_plan_ms = 0;
    bool score_timed = false, score_upload_timed = false;
    // the meters' scratch (abi_meter.hip; meter_plan.hpp MeterGeometry says what lies where), grown on demand, with the call's sums
    // behind it where the caller gave no device memory for them; and the events around the passes of the last dusp_meter_device call
    double *d_meter = nullptr;
    size_t meter_cap = 0;  // doubles
    hipEvent_t meter_marks[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool meter_timed = false;
    // the true peaks' words (abi_loudness.hip; truepeak_engine.hip), one a (signal, channel), grown on demand
    uint64_t *d_true_peak = nullptr;
    size_t true_peak_cap = 0;  // words
    // the limiter's scratch (abi_limiter.hip; limiter_engine.hip): the word that takes the smallest window sum, then one 32-bit word a
    // sample of the timeline, grown on demand
    uint64_t *d_limit = nullptr;
    size_t limit_cap = 0;  // samples
    hipEvent_t limit_marks[3] = {nullptr, nullptr, nullptr};  // around the two kernels of the last dusp_limit_device call
    bool limit_timed = false;
    // the release's scratch (abi_limiter.hip; limiter_release_engine.hip): one 32-bit word a position of the held curve, n + L - 1 of
    // them, then one summary word a tile, grown on demand
    uint32_t *d_limit_release = nullptr;
    size_t limit_release_cap = 0;  // words
    hipEvent_t limit_release_marks[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // around the four kernels of the last dusp_limit_release_device call
    bool limit_release_timed = false;
};

// DUSP_GUARD=1 (tests): every device allocation of the library carries guard bytes behind its end, filled with a pattern and
// checked after each render — a kernel that writes past the end of a workspace (state, rings, parked chunks, staging PCM, the
// tables) fails THAT render with a message instead of corrupting whatever the allocator placed next to it.
// (ONE object for the whole library: set by dusp_ctx_create, read wherever a DevBuf grows or is checked)
inline size_t g_guard_bytes = 0;
constexpr unsigned char kGuardPattern = 0xA5;

inline bool guard_intact(const void *end_of_payload) {
    unsigned char tail[4096];
    const size_t n = std::min(g_guard_bytes, sizeof tail);
    if (hipMemcpy(tail, end_of_payload, n, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t i = 0; i < n; i++)
        if (tail[i] != kGuardPattern) return false;
    return true;
}

template <class T>
struct DevBuf {  // grow-only device allocation
    T *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T) + g_guard_bytes);
        if (e == hipSuccess && g_guard_bytes) e = hipMemset((char *)p + n * sizeof(T), kGuardPattern, g_guard_bytes);
        if (e == hipSuccess) cap = n;
        return e;
    }
    bool intact() const { return !p || !g_guard_bytes || guard_intact((const char *)p + cap * sizeof(T)); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    void swap(DevBuf &other) {
        std::swap(p, other.p);
        std::swap(cap, other.cap);
    }
};

// Every device workspace a program owns, and nothing else.  for_each_workspace is the ONE list of them (with the name check_guards
// reports): the destructor and the guard check both walk it, so a new buffer is declared here and named there.
struct dusp_workspaces {
    // program constants on the device
    DevBuf<dusp::DevOp> d_ops;
    DevBuf<int32_t> d_out_bufs;
    DevBuf<double> d_init;
    // per-render workspaces (grown on demand)
    DevBuf<float> d_scratch, d_rings;
    DevBuf<double> d_state;
    DevBuf<unsigned long long> d_seg;  // WAVE, time-split: segment phase totals + start phases
    DevBuf<double> d_fused_state;  // FUSED: [n_state_words][n_inst] end-of-render state
    DevBuf<dusp::OscRec> d_recs;   // FUSED: per-voice oscillator records
    DevBuf<dusp::SumVoice> d_sum_voices;  // FUSED sum chain: per-oscillator records, and behind them every oscillator's (256 x block step) mod S
    DevBuf<float> d_host_out, d_host_par, d_host_frames, d_host_in;  // dusp_render_host staging, grown on demand
    DevBuf<unsigned char> d_host_pcm;                                // dusp_render_host_pcm: the encoded frames ...
    DevBuf<float> d_host_peaks;                                      // ... and the instances' peaks
    DevBuf<float> d_host_peak_common;                                // ... a call with stems: the one peak of all its signals, once a signal (pcm_peak_common.hpp)
    DevBuf<float> d_mix, d_mix_gains;                                // dusp_render_host_mix: the running sums [n_out_channels][n_samples]; one tile's gains
    DevBuf<float> d_mix_sends;                                       // a piece with buses: the send timelines [n_buses][n_out_channels][n_total] (abi_piece.hip)
    DevBuf<float> d_mix_tracks;                                      // a piece with tracks: the track timelines [n_tracks][n_out_channels][n_total], in the order of the track programs (abi_piece.hip)
    DevBuf<float> d_stems;                                           // a piece with stems: the signals [1 + n_tracks + n_buses + 1][n_out_channels][n_total], the mix last (abi_piece.hip)
    DevBuf<float> d_saved_bufs, d_rings_wave;  // wave engine, resumable: outlets' last chunk; rings parked during a migration
    // WAVE programs the circuit compiler takes (jit_codegen.hpp): the generated text's constants
    DevBuf<float> d_jit_fk;
    DevBuf<double> d_jit_dk;
    DevBuf<int> d_jit_scan;  // [2][n_scans]: state slot, FM level of every scanned oscillator
    DevBuf<double> d_handoff_init;   // the unit state the chunk engine left (instance 0), as the compiled kernel's start state
    DevBuf<double> d_warm_records;   // segments that warm up (JitArgs::warm): [Filter stage][segment][8] what the stage held where the segment's own chunks began / ended
    DevBuf<double> d_warm_init;      // ... and the start state of the launch that finishes a render whose check failed
    DevBuf<float> d_handoff_out;     // the two parts' PCM before they are put side by side
    DevBuf<int64_t> d_jit_regime;  // per-instance delays: [slot, ring length, mono] per unit, then the verdicts (render_jit)

    static constexpr size_t kCount = 32;

    template <class F>
    void for_each_workspace(F &&f) {  // f(name, buffer); buffers that share a name are reported together
        f("chunk buffers", d_scratch);
        f("rings", d_rings);
        f("unit state", d_state);
        f("segment phases", d_seg);
        f("fused end state", d_fused_state);
        f("voice records", d_recs);
        f("sum-chain records", d_sum_voices);
        f("parked chunks", d_saved_bufs);
        f("parked rings", d_rings_wave);
        f("staging PCM", d_host_out);
        f("staging frames", d_host_frames);
        f("staging PCM frames / peaks", d_host_pcm);
        f("staging PCM frames / peaks", d_host_peaks);
        f("staging PCM frames / peaks", d_host_peak_common);
        f("mix sums / gains", d_mix);
        f("mix sums / gains", d_mix_gains);
        f("send timelines", d_mix_sends);
        f("track timelines", d_mix_tracks);
        f("stems", d_stems);
        f("staging parameters", d_host_par);
        f("staging inputs", d_host_in);
        f("hand-off buffers", d_handoff_init);
        f("hand-off buffers", d_handoff_out);
        f("program constants", d_ops);
        f("program constants", d_out_bufs);
        f("program constants", d_init);
        f("compiled kernel's constants", d_jit_fk);
        f("compiled kernel's constants", d_jit_dk);
        f("compiled kernel's constants", d_jit_scan);
        f("warm-up records", d_warm_records);
        f("warm-up start state", d_warm_init);
        f("column verdicts", d_jit_regime);
    }
    // the name of the first workspace whose guard bytes a kernel has overwritten (nullptr: all intact)
    const char *first_overwritten() {
        const char *hit = nullptr;
        for_each_workspace([&](const char *name, auto &buf) {
            if (!hit && !buf.intact()) hit = name;
        });
        return hit;
    }
};
// (a DevBuf member that kCount does not know about fails here; one that for_each_workspace does not visit fails
// tests/native/workspace_registry_check.cpp, which counts the visits)
static_assert(sizeof(dusp_workspaces) == dusp_workspaces::kCount * sizeof(DevBuf<char>), "dusp_workspaces holds DevBufs only: update kCount and for_each_workspace");

struct dusp_program : dusp_workspaces {
    dusp_ctx *ctx = nullptr;
    dusp::Program P;
    int engine = DUSP_ENGINE_CHUNK;
    dusp::FusedPlan fused;
    dusp::WavePlan wave;
    std::vector<dusp::SumVoice> h_sum_voices;
    std::vector<double> h_sum_end;
    uint32_t last_n_inst = 0, last_n_pad = 0;
    bool rendered = false;
    // host-side conveniences for segment-by-segment rendering (many short renders + state downloads per second)
    std::vector<double> h_state;   // copy of d_state / d_fused_state, fetched once per render on the first state download
    bool h_state_valid = false;
    bool mixed = false;  // the last thing rendered was a mix: unit state describes its last tile only (dusp_state_download refuses)
    // ... while its tiles render: the range of every parameter column over the WHOLE batch, [n_params][3] as dusp_column_range_kernel
    // states it (empty otherwise).  What a render decides from a column's values and that changes bits (Filters as scans:
    // jit_classify_columns) is decided from these, so every tile renders as the one render of the whole batch would
    std::vector<unsigned> mix_range;
    // ... and the instance count of the whole batch (0 otherwise).  A tile waits for its compiled kernel whatever DUSP_WAVE_JIT says
    // (render_jit), and plans warming segments — which keep the Filter stage where an unsplit render may scan — as the whole batch would
    // (jit_plan.hpp JitBatch::whole_n_inst): all tiles of a mix run the same arithmetic, the one render of all instances' own
    uint32_t mix_n_inst = 0;
    int requested_engine = DUSP_ENGINE_AUTO;
    bool resumable = false;      // built with DUSP_ENGINE_RESUMABLE
    bool persistent = false;     // rings / feedback edges: device memory carries over between segments (CHUNK engine only)
    bool keep_memory = false;    // the next render continues: do not clear chunk buffers and rings
    bool delay_changed = false;     // a continuation changed a Delay's constant: the wave engine's write-once ring protocol no longer applies
    bool migrate_to_chunk = false;  // ... and first moves the wave engine's rings / saved buffers into the chunk layout
    int64_t next_clock = 0;      // circuit clock the last render stopped at
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last_stream = nullptr;  // stream of the most recent render (workspaces and state are ordered on it)
    // WAVE programs the circuit compiler takes (jit_codegen.hpp): generated text per workgroup geometry, constants on the device
    bool jit_ok = false;
    std::string jit_why;
    std::map<std::pair<int, int>, dusp::JitSource> jit_src;  // jit_plan.hpp jit_source_key -> kernel text (+ constants, scan list)
    bool jit_consts_uploaded = false;
    int voice_loop = -1;  // the circuit's voices run in a loop on its compiled kernel (jit_codegen.hpp VoicePlan): -1 not looked at yet
    uint64_t jit_table_generation = 0;  // ctx->table_generation the texts in jit_src were generated against
    int jit_waves = 0, jit_per_wave = 0;  // geometry of the last compiled launch (shown in dusp_program_info.shape)
    unsigned jit_segments = 1;            // ... the time segments it was cut into
    unsigned wave_segments = 1;           // the interpreter kernel's last render: the time segments it was cut into
    std::vector<double> param_bound;      // during a render whose parameter table is in host memory: largest magnitude of every column (else empty: not known)
    bool jit_voices = false;              // ... its voices ran in a loop (jit_codegen.hpp VoicePlan)
    bool jit_scan = false;                // ... its Filters ran as scans over the chunk (jit_filter_scan_ok)
    // channel counts that grow during the first chunks (Program::warm_ops): those chunks on the chunk engine, the rest on a compiled kernel
    bool handoff_ok = false;
    std::string handoff_why;  // when not: what keeps the settled circuit on the chunk engine
    unsigned warm_redo_from = 0;     // the last render's check failed at this segment: finished sequentially from there (0: it held)
    // dusp_render_host* into pageable memory: pinned staging tiles, two per copy worker (download_staged)
    unsigned char *pin[1] = {nullptr};
    size_t pin_bytes = 0;

    dusp_program() = default;
    dusp_program(const dusp_program &) = delete;
    dusp_program &operator=(const dusp_program &) = delete;
    ~dusp_program() {  // every exit path — a failed build included — gives the device memory back
        if (ctx) (void)hipSetDevice(ctx->device);
        for_each_workspace([](const char *, auto &buf) { buf.release(); });
        if (pin[0]) (void)hipHostFree(pin[0]);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

#define CTX_FAIL(ctx, code, msg)  \
    do {                          \
        (ctx)->err = (msg);       \
        return (code);            \
    } while (0)

#define HIP_TRY(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (ctx)->err = std::string("HIP error: ") + hipGetErrorString(e_) + " in " + #expr;     \
            return DUSP_ERR_HIP;                                                                  \
        }                                                                                         \
    } while (0)

// Exception firewall: nothing thrown inside the library (std::bad_alloc / std::length_error from a container sized by a
// descriptor, ...) may cross the C boundary — it would be std::terminate for the caller.  Every entry point that can
// allocate runs its body through guarded(): the exception becomes a status + message like any other failure.
template <class F>
int guarded(std::string &err, const char *who, F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        try { err = std::string(who) + ": out of host memory"; } catch (...) {}
        return DUSP_ERR_NOMEM;
    } catch (const std::length_error &e) {
        try { err = std::string(who) + ": size out of range (" + e.what() + ")"; } catch (...) {}
        return DUSP_ERR_ARG;
    } catch (const std::exception &e) {
        try { err = std::string(who) + ": " + e.what(); } catch (...) {}
        return DUSP_ERR_ARG;
    } catch (...) {
        try { err = std::string(who) + ": unknown internal error"; } catch (...) {}
        return DUSP_ERR_ARG;
    }
}

// ---- one set of argument checks; `who` is the entry point's name as its messages begin ("render", "dusp_peak_device", ...) ----
inline bool instances_in_range(size_t n_instances) { return n_instances >= 1 && n_instances <= (1u << 24); }
inline bool samples_in_range(size_t n_samples) { return n_samples >= 1 && n_samples <= (1ull << 31); }
inline bool batch_in_range(size_t n_instances, size_t n_samples) { return instances_in_range(n_instances) && samples_in_range(n_samples); }
inline bool channels_in_range(size_t n_channels) { return n_channels >= 1 && n_channels <= 64; }

// n_instances in [1, 2^24], n_samples in [1, 2^31]
inline int check_batch(dusp_ctx *ctx, const char *who, size_t n_instances, size_t n_samples) {
    if (!batch_in_range(n_instances, n_samples)) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": n_instances must be in [1, 2^24] and n_samples in [1, 2^31]");
    return DUSP_OK;
}
// a program's outlet as PCM frames: 1..64 channels
inline int check_channels(dusp_ctx *ctx, const char *who, size_t n_channels) {
    if (!channels_in_range(n_channels)) CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, std::string(who) + ": the outlet must have 1..64 channels");
    return DUSP_OK;
}
// DUSP_PCM_S16 / S24 / F32, and — allow_planar — 0 for planar f32
inline int check_pcm_format(dusp_ctx *ctx, const char *who, int format, bool allow_planar) {
    if ((format != 0 || !allow_planar) && format != DUSP_PCM_S16 && format != DUSP_PCM_S24 && format != DUSP_PCM_F32)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": format must be " + (allow_planar ? "0 (planar f32), " : "") + "DUSP_PCM_S16 (1), DUSP_PCM_S24 (2) or DUSP_PCM_F32 (3)");
    return DUSP_OK;
}
inline int check_normalise(dusp_ctx *ctx, const char *who, int normalise) {
    if (normalise != DUSP_NORMALISE_NONE && normalise != DUSP_NORMALISE_CLIP && normalise != DUSP_NORMALISE_FULL)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)");
    return DUSP_OK;
}

inline hipStream_t stream_of(dusp_ctx *ctx, void *stream_) { return stream_ ? (hipStream_t)stream_ : ctx->stream; }

// ---- internal functions that cross files ----
constexpr int kJitLater = 1;  // render_jit: the kernel is being compiled in the background; render this one on the interpreter

// abi_render.hip
// The window of the timeline a sum-chain launch renders (dusp_render_chain_window; a plain render is the window from sample 0)
struct ChainWindow {
    uint64_t first = 0;           // the window's first sample
    const float *init = nullptr;  // the sums another rank's voices left, laid out like the output
    bool raw = false;             // no `x || 0` at the copy-out (a partial sum)
};
int render_device_unguarded(dusp_program *prog, size_t n_instances, size_t n_samples, const float *d_params, const float *d_inputs, float *d_out, void *stream_,
                            const ChainWindow *window = nullptr);
int check_guards(dusp_program *prog, hipStream_t stream);
hipError_t zero_rings(dusp_program *prog, uint32_t n_pad, uint32_t n_chunks, bool instance_major, hipStream_t stream);
void finish_render(dusp_program *prog, uint32_t n_inst, uint32_t n_pad, uint64_t n_chunks_total);

// abi_render_jit.hip
int render_jit(dusp_program *prog, uint32_t n_inst, size_t n_samples, uint32_t n_chunks, const float *d_params, const float *d_inputs, float *d_out,
               hipStream_t stream, uint32_t handoff_chunks = 0, bool probe = false);

#pragma GCC visibility push(hidden)  // (what follows crosses files of the library and is no symbol of it)
// 1..64 channels of [1, 2^24] instances x [1, 2^31] samples: what the kernels over planar PCM take (dusp_peak_device, dusp_mix_device)
inline int check_planar_pcm(dusp_ctx *ctx, const char *who, size_t n_instances, size_t n_channels, size_t n_samples) {
    if (!channels_in_range(n_channels) || !batch_in_range(n_instances, n_samples))
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": need 1..64 channels, 1..2^24 instances and 1..2^31 samples");
    return DUSP_OK;
}

// abi_deliver.hip
// What a host render ends with: d_planar f32 [n_instances][n_ch][n_samples] (or, already transposed, d_frames) reaches h_out — as it is,
// or (pcm_format != 0) through the peak and encode kernels; waits for the stream.  common_peak (a call with stems): the instances are
// the signals of one call — their peaks are taken whatever the format (h_peaks: all of them), and what normalises is the largest.
int deliver_host(dusp_program *prog, const float *d_planar, const float *d_frames, size_t n_instances, size_t n_ch, size_t n_samples, int pcm_format,
                 int normalise, float *h_peaks, void *h_out, bool common_peak = false);
// ... and its two halves, for a delivery that decides between them (abi_piece.hip, a delivery at a loudness target).  deliver_peaks: the
// instances' sample peaks into the program's d_host_peaks and, asynchronously, into h_peaks (NULL: not asked for).  deliver_at_level:
// every instance's frames encoded under pcm_gain(bits(level), FULL) — `level` goes into the word array the encoder reads, once an
// instance — and downloaded; waits for the stream
int deliver_peaks(dusp_program *prog, const float *d_planar, size_t n_instances, size_t n_ch, size_t n_samples, float *h_peaks);
int deliver_at_level(dusp_program *prog, const float *d_planar, size_t n_instances, size_t n_ch, size_t n_samples, int pcm_format, float level, void *h_out);

// abi_meter.hip
// What a call may be metered at: refuses a sample rate below 8000 and shapes the kernels do not take, in `who`'s name
int meter_check(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate);
// The meters of d_planar [n_signals][n_channels][n_samples] on `stream`: the sums stay on the device, in the context's scratch, until
// meter_finish — which waits for the stream — turns them into h_rms [n_signals][n_channels], h_lufs [n_signals] and (optional)
// h_momentary [n_signals][n_blocks].  The caller has run meter_check.
int meter_launch(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, hipStream_t stream);
int meter_finish(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, hipStream_t stream, double *h_rms, double *h_lufs,
                 double *h_momentary);
// the scratch of a call, grown on demand: `extra` doubles behind what the kernels take
int meter_scratch(dusp_ctx *ctx, size_t rows, size_t n_samples, uint32_t hop, size_t extra, dusp::MeterGeometry &G);

// abi_loudness.hip
// The true peaks of d_planar [n_signals][n_channels][n_samples] on `stream`, into the context's words; true_peak_download copies them
// down behind what the stream holds (asynchronously: the caller waits for the stream, then calls true_peak_values)
int true_peak_launch(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, hipStream_t stream);
int true_peak_download(dusp_ctx *ctx, size_t rows, std::vector<uint64_t> &h_words, hipStream_t stream);
// the words of a call, once the stream has been waited for -> h_true_peak [rows]; the largest of them, a NaN winning; the guard checked
int true_peak_values(dusp_ctx *ctx, const char *who, const std::vector<uint64_t> &h_words, double *h_true_peak, double *largest);

// abi_limiter.hip
// The limiter over d_planar [n_signals][n_channels][n_samples], in place, on `stream`: the envelope kernel against `threshold`, then the
// gain / apply kernel over a window of L samples; the smallest window sum stays in the context's scratch.  limit_download copies it
// down behind what the stream holds (asynchronously: the caller waits for the stream, then calls limit_reduction, which also checks
// the scratch's guard).  The caller has checked the shapes, threshold and L (limit_check)
int limit_check(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, size_t window_samples);
// (R: the release in samples; 0: none — the envelope kernel and the gain / apply kernel, as before there was a release.  Else the
// envelope kernel, then the hold, release and mean / apply kernels of limiter_release_engine.hip; limit_reduction then checks the
// release's scratch too)
int limit_launch(dusp_ctx *ctx, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, uint32_t L, hipStream_t stream,
                 uint32_t R = 0);
int limit_download(dusp_ctx *ctx, uint64_t *h_smallest, hipStream_t stream);
int limit_reduction(dusp_ctx *ctx, const char *who, uint64_t smallest, uint32_t L, double *reduction);

// abi_mix.hip
constexpr size_t kMixRowMax = (size_t)1 << 31;  // floats in one voice's PCM that the mix kernel's grid covers (mix_engine.hip launch_mix)

// What a parameter table in host memory ([n_params][n_instances]) bounds its columns by — for the planner's time-split gate
// (fused_plan.hpp wave_split_exact).  Every host path that renders from such a table sets it before it renders and clears it behind.
inline void host_param_bounds(dusp_program *prog, const float *h_params, size_t n_instances) {
    const size_t n_params = (size_t)prog->P.g.n_params;
    prog->param_bound.clear();
    if (!h_params || !n_params || !n_instances) return;
    prog->param_bound.assign(n_params, 0.0);
    for (size_t p = 0; p < n_params; p++)
        for (size_t i = 0; i < n_instances; i++) {
            const double a = std::fabs((double)h_params[p * n_instances + i]);
            double &b = prog->param_bound[p];
            b = a <= b ? b : a == a ? a : std::numeric_limits<double>::infinity();
        }
}

// The tiles of one batch (dusp_render_host_mix, dusp_render_host_score, a part of dusp_render_host_score_parts).  Tiling must not change a
// bit.  What a render decides from the batch and that changes bits is, while the tiles render, decided from the WHOLE batch: a Filter with
// a per-instance cutoff runs as a scan or as a recurrence — not the same bits — by the range of its column (mix_range), and so does every
// scan-eligible Filter by whether the render is cut into warming segments, which the instance count decides (mix_n_inst, which also makes
// every tile wait for its compiled kernel).  Per-instance Delays are classified per tile: their regimes differ in speed only.
struct TiledBatch {
    dusp_program *prog;
    hipStream_t stream;
    size_t n_instances, n_params, tile;
    const float *h_gains;
    bool staged = false;      // host vectors of this call may still be on their way to the device
    std::vector<float> cols;  // (a member: it outlives the destructor's wait for the stream)


    TiledBatch(dusp_program *prog, size_t n_instances, const float *h_params, const float *h_gains, size_t tile);  // tiles of `tile` instances
    TiledBatch(dusp_program *prog, size_t n_instances, const float *h_params, const std::vector<size_t> &starts);  // tiles [starts[i], starts[i + 1])
    ~TiledBatch();
    // instances [lo, lo + n): their columns and gains to the device, their PCM into d_host_out.  d_inputs: the input streams of a
    // program that has some, [n_inputs][n][n_samples] in device memory (the master of a piece reads the timeline: abi_piece.hip)
    int render_tile(size_t lo, size_t n, size_t n_samples, const float *d_inputs = nullptr);

private:
    void gather(const float *h_params, size_t lo, size_t n);
    void whole_batch_decisions(const float *h_params);
};
// what dusp_render_host_mix and the host renders of scores refuse alike, and the tile a program renders in
int tiled_batch_prepare(dusp_program *prog, const char *who, size_t n_instances, size_t n_samples, const float *h_params, const float *h_gains, size_t tile_instances,
                        int format, int normalise, const void *h_out, size_t *tile_out);
#pragma GCC visibility pop
