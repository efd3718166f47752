// abi_score.hpp — what the files of the C ABI that launch score kernels share (abi_score.hip, abi_piece.hip, abi_score_sweep.hip,
// abi_meter.hip): the placement record of a rows call and its checks, the description of one launch, the plans' image on the device
// (abi_score.hip has the functions), the one launch path, the frame of a device entry with and without a plan, and the one check of the
// guard bytes behind the buffers a host render used.  Nothing here is a symbol of the library.
#pragma once
#include <chrono>
#include <cmath>
#include <initializer_list>

#include "abi_internal.hpp"

#pragma GCC visibility push(hidden)

// ---- the plans of a call: an image on the host, uploaded once, and one description per launch ----

// which kernel a launch is: voices of one contiguous batch (score_engine.hip; dusp_amd/mix.py score_chain is the contract), rows of their
// own (score_rows_engine.hip; score_chain_rows), mono rows placed in the stereo field (score_pan_engine.hip; score_chain_rows_panned), or
// mono rows placed in a space, a delay and a gain per speaker (score_space_engine.hip; score_chain_rows_placed), or rows of one and of two
// channels, the mono ones panned or not, into a timeline of two (score_stereo_engine.hip; score_chain_rows_stereo)
enum class ScoreKind { contiguous, rows, pan, space, stereo };

// What places the voices of a rows call: its kind and the host arrays that go with it, one entry a voice, which the caller owns.  An
// entry fills one in (nothing but the kind set: plain rows) and everything between it and the launch takes it by reference.
struct ScoreGathered {  // what a gathered placement points into
    std::vector<double> fracs, comp, delays, tap_gains;
    std::vector<float> pans;
    std::vector<uint32_t> row_channels;
};

struct ScorePlacement {
    ScoreKind kind;                    // what the call is, whether or not it has voices: the entry says it, once
    const double *h_fracs = nullptr;   // rows, pan, stereo: the voices' fractions of a sample (NULL: none)
    const float *h_pans = nullptr;     // pan: a finite pan a voice.  stereo: NaN says "not placed", and a voice of two channels is not
    const double *h_comp = nullptr;    // ... and the compensation (NULL: the reference's, by the host's pow, Pan.js:20)
    size_t n_speakers = 0;             // space: the taps, f64 [voice][speaker] each
    const double *h_delays = nullptr, *h_tap_gains = nullptr;
    const uint32_t *h_row_channels = nullptr;  // stereo: voice k is a row of h_row_channels[k] channels, one or two
    // rows, pan, with buses (score_send_engine.hip): what voice k gives to bus b is h_sends[b * sends_stride + k], finite
    size_t n_buses = 0, sends_stride = 0;
    const float *h_sends = nullptr;
    explicit ScorePlacement(ScoreKind kind_) : kind(kind_) {}
    ScorePlacement(ScoreKind kind_, const double *fracs, const float *pans, const double *comp) : kind(kind_), h_fracs(fracs), h_pans(pans), h_comp(comp) {}
    ScorePlacement(size_t speakers, const double *delays, const double *tap_gains) : kind(ScoreKind::space), n_speakers(speakers), h_delays(delays), h_tap_gains(tap_gains) {}

    size_t timeline_channels(size_t voice_channels) const { return kind == ScoreKind::space ? n_speakers : kind == ScoreKind::rows ? voice_channels : 2; }
    ScorePlacement tile(size_t lo) const {  // the same placement for the voices from `lo` on
        ScorePlacement t = *this;
        if (h_fracs) t.h_fracs += lo;
        if (h_pans) t.h_pans += lo;
        if (h_comp) t.h_comp += lo;
        if (h_delays) t.h_delays += lo * n_speakers;
        if (h_tap_gains) t.h_tap_gains += lo * n_speakers;
        if (h_row_channels) t.h_row_channels += lo;
        if (h_sends) t.h_sends += lo;
        return t;
    }
    // the same placement for the n voices which[0], which[1], ... alone (a track's of a tile), its arrays copied into `into`; a call
    // with tracks has no per-voice levels (h_sends)
    ScorePlacement gather(const size_t *which, size_t n, ScoreGathered &into) const {
        ScorePlacement t = *this;
        auto take = [&](auto &v, const auto *&h, size_t width) {
            if (!h) return;
            v.resize(n * width);
            for (size_t k = 0; k < n; k++)
                for (size_t c = 0; c < width; c++) v[k * width + c] = h[which[k] * width + c];
            h = v.data();
        };
        take(into.fracs, t.h_fracs, 1);
        take(into.pans, t.h_pans, 1);
        take(into.comp, t.h_comp, 1);
        take(into.delays, t.h_delays, n_speakers);
        take(into.tap_gains, t.h_tap_gains, n_speakers);
        take(into.row_channels, t.h_row_channels, 1);
        return t;
    }

    // buses: how many, the levels, and what sends do not go with (fractions, a space, a stereo piece: later changes); n voices
    int check_sends(dusp_ctx *ctx, const char *who, size_t n) const {
        const std::string w(who);
        if (n_buses < 1 || n_buses > dusp::kScoreBusMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 4 buses, not " + std::to_string(n_buses));
        if (!h_sends) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buses' h_sends is NULL: every bus needs a send level a voice");
        if (h_fracs || kind == ScoreKind::space || kind == ScoreKind::stereo)
            CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": sends go with plain rows and with pans at whole-sample onsets: together with fracs, places or stereo they are refused");
        for (size_t b = 0; b < n_buses; b++)
            for (size_t k = 0; k < n; k++)
                if (!std::isfinite(h_sends[b * sends_stride + k]))
                    CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the send level of voice " + std::to_string(k) + " into bus " + std::to_string(b) + " is not finite");
        return DUSP_OK;
    }

    // The checks of n voices, before anything renders; each holds where the kind has nothing of its sort.  The two entry families run
    // them between checks of their own, each in its own order (which refusal a call with several faults gets is behaviour): the device
    // entries taps, kinds, values; the host renders taps, values and — once the parts say how many channels a voice has — kinds.
    // space: the taps at n_speakers speakers over a timeline of n_total samples
    int check_taps(dusp_ctx *ctx, const char *who, size_t n, size_t n_total) const {
        if (kind != ScoreKind::space) return DUSP_OK;
        const std::string w(who);
        if (n_speakers < 1 || n_speakers > dusp::kScoreSpaceChannelsMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a Space has 1 .. 8 speakers, not " + std::to_string(n_speakers));
        if (n && (!h_delays || !h_tap_gains)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the taps' delays or gains are NULL");
        if (n_speakers * n_total > dusp::kScoreRowMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": speakers x timeline samples must not exceed 2^31: score such a piece speaker by speaker or in windows of the timeline");
        for (size_t k = 0; k < n; k++)
            for (size_t c = 0; c < n_speakers; c++) {
                const double D = h_delays[k * n_speakers + c], G = h_tap_gains[k * n_speakers + c];
                const std::string at = " of voice " + std::to_string(k) + " at speaker " + std::to_string(c);
                if (!std::isfinite(D)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the delay" + at + " is not finite");
                if (D < 0.0 || D > (double)dusp::kScoreSpaceShiftMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the delay" + at + " is outside [0, 2^24] samples");
                if (!std::isfinite(G)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the gain" + at + " is not finite");
            }
        return DUSP_OK;
    }

    // stereo: the kinds of the voices — a row of one or of two channels; a pan that is NaN says "not placed", and a voice of two
    // channels is not placed
    int check_kinds(dusp_ctx *ctx, const char *who, size_t n) const {
        if (kind != ScoreKind::stereo) return DUSP_OK;
        for (size_t k = 0; k < n; k++) {
            const uint32_t channels = h_row_channels[k];
            if (channels != 1 && channels != 2)
                CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": voice " + std::to_string(k) + " has " + std::to_string(channels) + " channels: a voice of a stereo piece has one or two");
            if (std::isinf(h_pans[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the pan of voice " + std::to_string(k) + " is not finite");
            if (channels == 2 && !std::isnan(h_pans[k]))
                CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": voice " + std::to_string(k) + " has two channels and a pan: a two-channel voice is not panned (its pan must be NaN)");
            if (h_comp && !std::isnan(h_pans[k]) && std::isnan(h_comp[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the compensation of voice " + std::to_string(k) + " is NaN");
        }
        return DUSP_OK;
    }

    // pan: the pans and their compensation; then, whatever the kind, the fractions
    int check_values(dusp_ctx *ctx, const char *who, size_t n) const {
        for (size_t k = 0; kind == ScoreKind::pan && k < n; k++) {
            if (!std::isfinite(h_pans[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the pan of voice " + std::to_string(k) + " is not finite");
            if (h_comp && std::isnan(h_comp[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the compensation of voice " + std::to_string(k) + " is NaN");
        }
        for (size_t k = 0; h_fracs && k < n; k++) {
            if (!std::isfinite(h_fracs[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the fraction of voice " + std::to_string(k) + " is not finite");
            if (h_fracs[k] < 0.0 || h_fracs[k] >= 1.0) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the fraction of voice " + std::to_string(k) + " is outside [0, 1)");
        }
        return DUSP_OK;
    }
};

// one launch's plan inside the context's image
struct ScoreLaunch {
    ScoreKind kind;      // a launch without voices (`|| 0`, or a copy, of d_init alone) keeps the kind of its call
    size_t at = 0, n_voices = 0, n_block_first = 0;  // byte offset of the voices; block_first and the entries follow
    uint64_t w_lo = 0, w_hi = 0, first_block = 0;
    uint32_t block_shift = dusp::kScoreGroupShift;
    bool any = false;  // some voice reaches the timeline (else: no plan in the image)
    size_t pan_at = 0;  // a panned launch: byte offset of its voices' coefficients (dusp::ScorePan), behind the plan
    bool frac = false;   // some listed voice starts between samples: the launch is score_frac_engine.hip's, plain rows or panned ...
    size_t frac_at = 0;  // ... and this the byte offset of its voices' weights (dusp::ScoreFrac), behind the plan
    size_t space_at = 0;  // a space launch: byte offset of its voices' taps (dusp::ScoreSpaceTap, [voice][speaker]), behind the plan
    size_t n_buses = 0, send_at = 0;  // a launch with sends (score_send_engine.hip): how many buses, and the byte offset of its voices' levels (dusp::ScoreSend), behind the plan
    explicit ScoreLaunch(ScoreKind kind_, uint64_t n_total = 0) : kind(kind_), w_hi(n_total) {}  // (n_total: over the whole timeline)
};

// the image (abi_score.hip).  score_image_begin: before a call rewrites the context's host image — the last upload has read it.
// score_image_upload: the image to the device, ordered on `stream` behind the last launch that read the buffer
int score_image_begin(dusp_ctx *ctx);
int score_image_upload(dusp_ctx *ctx, hipStream_t stream);
// what the plans of ONE call may take together, on the host and on the device
inline size_t score_plan_budget(dusp_ctx *ctx) { return ctx->knobs.score_plan_kb > 0 ? (size_t)ctx->knobs.score_plan_kb << 10 : dusp::kScorePlanBytes; }
inline bool score_plan_intact(dusp_ctx *ctx) { return !ctx->d_score_plan || !g_guard_bytes || guard_intact(ctx->d_score_plan + ctx->score_plan_cap); }
// a plan of the voices [0, n) of a contiguous batch, or of n rows placed as `place` says, made within budget_bytes, added to the image
// and its launch described in L (abi_score.hip says what each takes)
int score_voices_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, size_t n, size_t first_voice, uint64_t n_voice, uint64_t n_total,
                     bool whole_timeline, size_t budget_bytes, ScoreLaunch &L);
int score_rows_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, const uint32_t *row_samples, const uint64_t *rows, size_t n, size_t first_voice,
                   uint64_t n_total, bool whole_timeline, size_t budget_bytes, const ScorePlacement &place, ScoreLaunch &L, std::vector<unsigned char> *listed,
                   const size_t *voice_ids = nullptr);
// the one launch path (abi_score.hip)
int score_launch(dusp_ctx *ctx, const ScoreLaunch &L, size_t n_channels, size_t n_total, const float *d_gains, const float *d_init, int raw, float *d_out, hipStream_t stream,
                 const float *d_planar, size_t n_voice, const float *d_send_init = nullptr, float *d_send_out = nullptr);

// What a device entry does once its arguments hold (dusp_score_device, score_rows_device): a fresh image, the call's plan — plan() adds
// it and describes the launch in L; it is not called without voices, and what it takes on the host is score_plan_ms — its upload, and
// launch() between the events score_t0 and score_t1 (dusp_score_last_ms)
template <class Plan, class Launch>
int score_device_call(dusp_ctx *ctx, hipStream_t stream, bool voices, const ScoreLaunch &L, Plan &&plan, Launch &&launch) {
    if (voices) {
        if (int rc = score_image_begin(ctx)) return rc;
        const auto t_plan = std::chrono::steady_clock::now();
        if (int rc = plan()) return rc;
        ctx->score_plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan).count();
        if (int rc = score_image_upload(ctx, stream)) return rc;
    } else {
        if (!ctx->score_t0) {  // (no plan, but the launch is timed like any other)
            if (int rc = score_image_begin(ctx)) return rc;
        }
        ctx->score_plan_ms = 0;
    }
    ctx->score_timed = false;
    ctx->score_upload_timed = L.any;
    HIP_TRY(ctx, hipEventRecord(ctx->score_t0, stream));
    if (int rc = launch()) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->score_t1, stream));
    ctx->score_timed = true;
    return DUSP_OK;
}

// A device entry that launches a kernel without a plan (the flat sweeps of abi_score_sweep.hip, dusp_meter_device), timed like any other:
// launch(stream) between the events score_t0 and score_t1
template <class Launch>
int score_unplanned_call(dusp_ctx *ctx, void *stream_, Launch &&launch) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    const ScoreLaunch none(ScoreKind::rows);
    return score_device_call(ctx, stream, false, none, []() { return DUSP_OK; }, [&]() { return launch(stream); });
}

// What a host render ends with behind its delivery: the guard bytes of the buffers of the piece (or score) that the call used — the
// timeline's sums and gains and, where used, the send and track timelines, the stems and their common peak — and of the plans' image
inline int score_guards(dusp_ctx *ctx, const char *who, std::initializer_list<const DevBuf<float> *> used) {
    if (!g_guard_bytes) return DUSP_OK;
    bool intact = score_plan_intact(ctx);
    for (const DevBuf<float> *buf : used) intact = intact && (!buf || buf->intact());
    if (!intact) CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    return DUSP_OK;
}

#pragma GCC visibility pop
