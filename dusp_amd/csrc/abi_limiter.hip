// abi_limiter.hip — the C ABI (include/dusp_hip.h): the linked look-ahead true-peak limiter of signals on the device (limiter_engine.hip:
// an envelope kernel and a gain / apply kernel; limiter_plan.hpp: the tiles, the threshold) — dusp_limit_tile, dusp_limiter_threshold,
// dusp_limit_device, dusp_limit_last_ms, dusp_limit_host, and what dusp_render_host_score_piece_limiter (abi_piece.hip) limits its delivery with.
// DESIGN.md 6.20; dusp_amd/mix.py limiter_envelope, limiter_gain and limit are the contract.  With a release of its own (DESIGN.md 6.21;
// limiter_release_engine.hip: hold, release and mean / apply kernels behind the envelope kernel; mix.limiter_gain_release) the
// dusp_limit_release_* entries, and what dusp_render_host_score_piece_limiter_release limits with.
#include <cmath>
#include <string>
#include <vector>

#include "abi_score.hpp"

// What the limiter takes: the true-peak kernel's shapes and sample rates, a threshold above 0, a window of 1 .. 4096 samples
int limit_check(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, size_t window_samples) {
    const std::string w(who);
    if (sample_rate == 0) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the limiter needs a sample rate, not 0: it decides the oversampling");
    if (!channels_in_range(n_channels) || !batch_in_range(n_signals, n_samples) || n_signals * n_channels * n_samples > ((size_t)1 << 33))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the limiter needs 1..64 channels, 1..2^24 signals, 1..2^31 samples and at most 2^33 samples in all");
    if (!(threshold > 0.0) || !std::isfinite(threshold)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + dusp::kLimiterThresholdBad);
    if (window_samples < 1 || window_samples > dusp::kLimiterWindowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + dusp::kLimiterWindowRange + std::to_string(window_samples));
    return DUSP_OK;
}

// the context's scratch: one 8-byte word, then n_samples 4-byte words
static int limit_scratch(dusp_ctx *ctx, size_t n_samples) {
    if (n_samples <= ctx->limit_cap) return DUSP_OK;
    if (ctx->d_limit) HIP_TRY(ctx, hipFree(ctx->d_limit));  // (waits for the device: no launch is using it any more)
    ctx->d_limit = nullptr;
    ctx->limit_cap = 0;
    const size_t bytes = sizeof(uint64_t) + n_samples * sizeof(uint32_t);
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_limit, bytes + g_guard_bytes));
    if (g_guard_bytes) HIP_TRY(ctx, hipMemset((char *)ctx->d_limit + bytes, kGuardPattern, g_guard_bytes));
    ctx->limit_cap = n_samples;
    return DUSP_OK;
}

static uint32_t *limit_words(dusp_ctx *ctx) { return (uint32_t *)(ctx->d_limit + 1); }

// the release's scratch: n + L - 1 words of the held curve, then one summary a tile
static int limit_release_scratch(dusp_ctx *ctx, size_t n_samples, uint32_t L) {
    const size_t words = (size_t)dusp::limiter_release_words(n_samples, L);
    if (words <= ctx->limit_release_cap) return DUSP_OK;
    if (ctx->d_limit_release) HIP_TRY(ctx, hipFree(ctx->d_limit_release));  // (waits for the device: no launch is using it any more)
    ctx->d_limit_release = nullptr;
    ctx->limit_release_cap = 0;
    const size_t bytes = words * sizeof(uint32_t);
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_limit_release, bytes + g_guard_bytes));
    if (g_guard_bytes) HIP_TRY(ctx, hipMemset((char *)ctx->d_limit_release + bytes, kGuardPattern, g_guard_bytes));
    ctx->limit_release_cap = words;
    return DUSP_OK;
}

static int limit_release_refused(dusp_ctx *ctx, const char *who, size_t release_samples) {
    if (release_samples < 1 || release_samples > dusp::kLimiterReleaseMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": " + dusp::kLimiterReleaseRange + std::to_string(release_samples));
    return DUSP_OK;
}

// (marks: events recorded in front of, between and behind the kernels, or NULL — three without a release, five with one.  R = 0: the
// two kernels of limiter_engine.hip, as before there was a release)
static int limit_run(dusp_ctx *ctx, float *d_planar, size_t rows, size_t n_samples, uint32_t sample_rate, double threshold, uint32_t L, uint32_t R, double *d_gain, hipStream_t stream,
                     hipEvent_t *marks = nullptr) {
    const uint32_t F = dusp::true_peak_factor(sample_rate);
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[0], stream));
    HIP_TRY(ctx, dusp::launch_limit_envelope(d_planar, rows, n_samples, F, dusp::true_peak_taps(F), threshold, L, ctx->n_cus, limit_words(ctx), ctx->d_limit, stream));
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[1], stream));
    if (!R) {
        HIP_TRY(ctx, dusp::launch_limit_apply(d_planar, rows, n_samples, L, ctx->n_cus, limit_words(ctx), ctx->d_limit, d_gain, stream));
        if (marks) HIP_TRY(ctx, hipEventRecord(marks[2], stream));
        return DUSP_OK;
    }
    uint32_t *d_held = ctx->d_limit_release, *d_summary = d_held + (n_samples + L - 1);
    HIP_TRY(ctx, dusp::launch_limit_hold(n_samples, L, R, ctx->n_cus, limit_words(ctx), d_held, d_summary, stream));
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[2], stream));
    HIP_TRY(ctx, dusp::launch_limit_release(n_samples, L, R, ctx->n_cus, d_held, d_summary, stream));
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[3], stream));
    HIP_TRY(ctx, dusp::launch_limit_mean_apply(d_planar, rows, n_samples, L, ctx->n_cus, d_held, ctx->d_limit, d_gain, stream));
    if (marks) HIP_TRY(ctx, hipEventRecord(marks[4], stream));
    return DUSP_OK;
}

int limit_launch(dusp_ctx *ctx, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, uint32_t L, hipStream_t stream,
                 uint32_t R) {
    if (int rc = limit_scratch(ctx, n_samples)) return rc;
    if (R)
        if (int rc = limit_release_scratch(ctx, n_samples, L)) return rc;
    return limit_run(ctx, d_planar, n_signals * n_channels, n_samples, sample_rate, threshold, L, R, nullptr, stream);
}

int limit_download(dusp_ctx *ctx, uint64_t *h_smallest, hipStream_t stream) {
    HIP_TRY(ctx, hipMemcpyAsync(h_smallest, ctx->d_limit, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    return DUSP_OK;
}

int limit_reduction(dusp_ctx *ctx, const char *who, uint64_t smallest, uint32_t L, double *reduction) {
    if (ctx->d_limit && g_guard_bytes && !guard_intact((char *)ctx->d_limit + sizeof(uint64_t) + ctx->limit_cap * sizeof(uint32_t)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": a limiter kernel wrote past the end of its scratch: guard bytes overwritten");
    if (ctx->d_limit_release && g_guard_bytes && !guard_intact((char *)ctx->d_limit_release + ctx->limit_release_cap * sizeof(uint32_t)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": a kernel of the limiter's release wrote past the end of its scratch: guard bytes overwritten");
    if (reduction) *reduction = dusp::limiter_reduction(smallest, L);
    return DUSP_OK;
}

extern "C" {

double dusp_limiter_threshold(double lufs, double target_lufs, double ceiling_dbtp) { return dusp::limiter_threshold(lufs, target_lufs, ceiling_dbtp); }

size_t dusp_limit_tile(dusp_ctx *ctx, size_t n_samples, size_t window_samples) {
    if (!ctx || !n_samples || window_samples < 1 || window_samples > dusp::kLimiterWindowMax) return 0;
    return dusp::limiter_grid(n_samples, (uint32_t)window_samples, ctx->n_cus).W;
}

int dusp_limit_last_ms(dusp_ctx *ctx, float ms[2]) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!ms) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_limit_last_ms: NULL buffer");
    if (!ctx->limit_timed) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_limit_last_ms: no dusp_limit_device call has been launched on this context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->limit_marks[2]));
    for (int i = 0; i < 2; i++) HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->limit_marks[i], ctx->limit_marks[i + 1]));
    // (the kernels of that call have ended: dusp_limit_device itself does not wait, so this is where its scratch's guard is looked at)
    return limit_reduction(ctx, "dusp_limit_last_ms", 0, 1, nullptr);
}

// The limiter's kernels alone, in place over signals on the device: dusp_limit_device (release NULL: limiter_engine.hip's two) and
// dusp_limit_release_device (the envelope kernel and limiter_release_engine.hip's three), each under its own name
static int limit_device(dusp_ctx *ctx, const char *who, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold,
                        size_t window_samples, const size_t *release, uint32_t *d_q, uint32_t *d_held, double *d_gain, uint64_t *d_smallest, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (!d_planar) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (int rc = limit_check(ctx, who, n_signals, n_channels, n_samples, sample_rate, threshold, window_samples)) return rc;
    if (release)
        if (int rc = limit_release_refused(ctx, who, *release)) return rc;
    if (((uintptr_t)d_planar & 3) || ((uintptr_t)d_q & 3) || ((uintptr_t)d_held & 3) || (((uintptr_t)d_gain | (uintptr_t)d_smallest) & 7))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + (release ? ": d_planar, d_q and d_held must be 4-byte aligned, d_gain and d_smallest 8-byte aligned"
                                                 : ": d_planar and d_q must be 4-byte aligned, d_gain and d_smallest 8-byte aligned"));
    const uint32_t L = (uint32_t)window_samples, R = release ? (uint32_t)*release : 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = limit_scratch(ctx, n_samples)) return rc;
    if (R)
        if (int rc = limit_release_scratch(ctx, n_samples, L)) return rc;
    hipEvent_t *marks = R ? ctx->limit_release_marks : ctx->limit_marks;
    for (int i = 0; i < (R ? 5 : 3); i++)
        if (!marks[i]) HIP_TRY(ctx, hipEventCreate(&marks[i]));
    bool &timed = R ? ctx->limit_release_timed : ctx->limit_timed;
    timed = false;
    const int rc = score_unplanned_call(ctx, stream_, [&](hipStream_t stream) -> int {  // (timed like a score launch: dusp_score_last_ms)
        return limit_run(ctx, d_planar, n_signals * n_channels, n_samples, sample_rate, threshold, L, R, d_gain, stream, marks);
    });
    if (rc) return rc;
    timed = true;
    hipStream_t stream = stream_of(ctx, stream_);  // (the copies of what was asked for: behind the kernels, outside the timed span)
    if (d_q) HIP_TRY(ctx, hipMemcpyAsync(d_q, limit_words(ctx), n_samples * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    if (R && d_held) HIP_TRY(ctx, hipMemcpyAsync(d_held, ctx->d_limit_release, (n_samples + L - 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    if (d_smallest) HIP_TRY(ctx, hipMemcpyAsync(d_smallest, ctx->d_limit, sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    return DUSP_OK;
    });
}

int dusp_limit_device(dusp_ctx *ctx, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, size_t window_samples,
                      uint32_t *d_q, double *d_gain, uint64_t *d_smallest, void *stream_) {
    return limit_device(ctx, "dusp_limit_device", d_planar, n_signals, n_channels, n_samples, sample_rate, threshold, window_samples, nullptr, d_q, nullptr, d_gain, d_smallest, stream_);
}

int dusp_limit_release_device(dusp_ctx *ctx, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, size_t window_samples,
                              size_t release_samples, uint32_t *d_q, uint32_t *d_held, double *d_gain, uint64_t *d_smallest, void *stream_) {
    return limit_device(ctx, "dusp_limit_release_device", d_planar, n_signals, n_channels, n_samples, sample_rate, threshold, window_samples, &release_samples, d_q, d_held, d_gain,
                        d_smallest, stream_);
}

size_t dusp_limit_release_tile(dusp_ctx *ctx, size_t n_samples, size_t window_samples, size_t release_samples) {
    if (release_samples < 1 || release_samples > dusp::kLimiterReleaseMax) return 0;
    return dusp_limit_tile(ctx, n_samples, window_samples);
}

int dusp_limit_release_last_ms(dusp_ctx *ctx, float ms[4]) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!ms) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_limit_release_last_ms: NULL buffer");
    if (!ctx->limit_release_timed) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_limit_release_last_ms: no dusp_limit_release_device call has been launched on this context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->limit_release_marks[4]));
    for (int i = 0; i < 4; i++) HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->limit_release_marks[i], ctx->limit_release_marks[i + 1]));
    return limit_reduction(ctx, "dusp_limit_release_last_ms", 0, 1, nullptr);  // (the kernels have ended: the scratch's guards)
}

// dusp_limit_host (release NULL) and dusp_limit_release_host, each under its own name
static int limit_host(dusp_ctx *ctx, const char *who, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold,
                      size_t window_samples, const size_t *release, float *h_limited, double *h_gain, double *h_reduction) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, who, [&]() -> int {
    if (!h_planar || !h_limited) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": NULL buffer");
    if (int rc = limit_check(ctx, who, n_signals, n_channels, n_samples, sample_rate, threshold, window_samples)) return rc;
    if (release)
        if (int rc = limit_release_refused(ctx, who, *release)) return rc;
    const uint32_t R = release ? (uint32_t)*release : 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = limit_scratch(ctx, n_samples)) return rc;
    if (R)
        if (int rc = limit_release_scratch(ctx, n_samples, (uint32_t)window_samples)) return rc;
    const size_t n_floats = n_signals * n_channels * n_samples;
    float *d_planar = nullptr;
    double *d_gain = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&d_planar, n_floats * sizeof(float)));
    uint64_t smallest = 0;
    int rc = DUSP_OK;
    auto tried = [&](hipError_t e, const char *what) {
        if (e == hipSuccess || rc) return;
        ctx->err = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what + who;
        rc = DUSP_ERR_HIP;
    };
    if (h_gain) tried(hipMalloc((void **)&d_gain, n_samples * sizeof(double)), "the gain curve's buffer of ");
    tried(hipMemcpyAsync(d_planar, h_planar, n_floats * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "the upload of ");
    if (!rc) rc = limit_run(ctx, d_planar, n_signals * n_channels, n_samples, sample_rate, threshold, (uint32_t)window_samples, R, d_gain, ctx->stream);
    if (!rc) tried(hipMemcpyAsync(h_limited, d_planar, n_floats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream), "the download of ");
    if (!rc && h_gain) tried(hipMemcpyAsync(h_gain, d_gain, n_samples * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "the download of ");
    if (!rc) rc = limit_download(ctx, &smallest, ctx->stream);
    tried(hipStreamSynchronize(ctx->stream), "");
    (void)hipFree(d_planar);
    if (d_gain) (void)hipFree(d_gain);
    if (!rc) rc = limit_reduction(ctx, who, smallest, (uint32_t)window_samples, h_reduction);
    return rc;
    });
}

int dusp_limit_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, size_t window_samples,
                    float *h_limited, double *h_gain, double *h_reduction) {
    return limit_host(ctx, "dusp_limit_host", h_planar, n_signals, n_channels, n_samples, sample_rate, threshold, window_samples, nullptr, h_limited, h_gain, h_reduction);
}

int dusp_limit_release_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold, size_t window_samples,
                            size_t release_samples, float *h_limited, double *h_gain, double *h_reduction) {
    return limit_host(ctx, "dusp_limit_release_host", h_planar, n_signals, n_channels, n_samples, sample_rate, threshold, window_samples, &release_samples, h_limited, h_gain, h_reduction);
}

}  // extern "C"
