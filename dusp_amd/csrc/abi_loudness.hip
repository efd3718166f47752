// abi_loudness.hip — the C ABI (include/dusp_hip.h): the true peak of signals on the device (truepeak_engine.hip: a polyphase windowed
// sinc in f64, one word a row) and what the library makes of the words that come down (truepeak_plan.hpp) — dusp_true_peak_taps,
// dusp_true_peak_tile, dusp_true_peak_device, dusp_true_peak_host, and what dusp_render_host_score_piece_loudness (abi_piece.hip) takes
// the true peaks of its delivery with.  DESIGN.md 6.19; dusp_amd/mix.py true_peak and loudness_gain are the contract.
#include <cmath>
#include <string>
#include <vector>

#include "abi_score.hpp"

// What the true-peak kernel takes: meter_check's shapes, and any sample rate but 0
static int true_peak_check(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate) {
    const std::string w(who);
    if (sample_rate == 0) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the true peak needs a sample rate, not 0: it decides the oversampling");
    if (!channels_in_range(n_channels) || !batch_in_range(n_signals, n_samples) || n_signals * n_channels * n_samples > ((size_t)1 << 33))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the true peak needs 1..64 channels, 1..2^24 signals, 1..2^31 samples and at most 2^33 samples in all");
    return DUSP_OK;
}

static int true_peak_scratch(dusp_ctx *ctx, size_t rows) {
    if (rows <= ctx->true_peak_cap) return DUSP_OK;
    if (ctx->d_true_peak) HIP_TRY(ctx, hipFree(ctx->d_true_peak));  // (waits for the device: no launch is writing it any more)
    ctx->d_true_peak = nullptr;
    ctx->true_peak_cap = 0;
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_true_peak, rows * sizeof(uint64_t) + g_guard_bytes));
    if (g_guard_bytes) HIP_TRY(ctx, hipMemset((char *)(ctx->d_true_peak + rows), kGuardPattern, g_guard_bytes));
    ctx->true_peak_cap = rows;
    return DUSP_OK;
}

static int true_peak_run(dusp_ctx *ctx, const float *d_planar, size_t rows, size_t n_samples, uint32_t sample_rate, uint64_t *d_words, hipStream_t stream) {
    const uint32_t F = dusp::true_peak_factor(sample_rate);
    HIP_TRY(ctx, dusp::launch_true_peak(d_planar, rows, n_samples, F, dusp::true_peak_taps(F), ctx->n_cus, d_words, stream));
    return DUSP_OK;
}

int true_peak_launch(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, hipStream_t stream) {
    if (int rc = true_peak_scratch(ctx, n_signals * n_channels)) return rc;
    return true_peak_run(ctx, d_planar, n_signals * n_channels, n_samples, sample_rate, ctx->d_true_peak, stream);
}

int true_peak_download(dusp_ctx *ctx, size_t rows, std::vector<uint64_t> &h_words, hipStream_t stream) {
    h_words.resize(rows);
    HIP_TRY(ctx, hipMemcpyAsync(h_words.data(), ctx->d_true_peak, rows * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    return DUSP_OK;
}

int true_peak_values(dusp_ctx *ctx, const char *who, const std::vector<uint64_t> &h_words, double *h_true_peak, double *largest) {
    if (ctx->d_true_peak && g_guard_bytes && !guard_intact(ctx->d_true_peak + ctx->true_peak_cap))
        CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": the true-peak kernel wrote past the end of its words: guard bytes overwritten");
    uint64_t most = 0;
    for (size_t r = 0; r < h_words.size(); r++) {
        h_true_peak[r] = dusp::true_peak_of_word(h_words[r]);
        most = h_words[r] > most ? h_words[r] : most;  // (as unsigned words: a NaN wins)
    }
    if (largest) *largest = dusp::true_peak_of_word(most);
    return DUSP_OK;
}

extern "C" {

int dusp_true_peak_taps(uint32_t sample_rate, int *factor, double *h49) {
    if (!factor || !h49 || sample_rate == 0) return DUSP_ERR_ARG;
    const uint32_t F = dusp::true_peak_factor(sample_rate);
    const dusp::TruePeakTaps taps = dusp::true_peak_taps(F);
    *factor = (int)F;
    for (uint32_t j = 0; j < dusp::kTruePeakTaps; j++) h49[j] = taps.h[j];
    return DUSP_OK;
}

size_t dusp_true_peak_tile(dusp_ctx *ctx, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate) {
    if (!ctx || !sample_rate || !n_samples || !n_signals || !n_channels) return 0;
    return dusp::true_peak_grid(n_signals * n_channels, n_samples, dusp::true_peak_phase_taps(dusp::true_peak_factor(sample_rate)), ctx->n_cus).W;
}

// The true-peak kernel alone (truepeak_engine.hip): one word a (signal, channel) of signals on the device
int dusp_true_peak_device(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, uint64_t *d_words, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_true_peak_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (!d_planar || !d_words) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (int rc = true_peak_check(ctx, who, n_signals, n_channels, n_samples, sample_rate)) return rc;
    if (((uintptr_t)d_planar & 3) || ((uintptr_t)d_words & 7)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": d_planar must be 4-byte aligned, d_words 8-byte aligned");
    return score_unplanned_call(ctx, stream_, [&](hipStream_t stream) {  // (timed like a score launch: dusp_score_last_ms)
        return true_peak_run(ctx, d_planar, n_signals * n_channels, n_samples, sample_rate, d_words, stream);
    });
    });
}

int dusp_true_peak_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double *h_true_peak) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_true_peak_host";
    return guarded(ctx->err, who, [&]() -> int {
    if (!h_planar || !h_true_peak) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": NULL buffer");
    if (int rc = true_peak_check(ctx, who, n_signals, n_channels, n_samples, sample_rate)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n_floats = n_signals * n_channels * n_samples;
    float *d_planar = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&d_planar, n_floats * sizeof(float)));
    std::vector<uint64_t> words;
    int rc = DUSP_OK;
    if (hipError_t e = hipMemcpyAsync(d_planar, h_planar, n_floats * sizeof(float), hipMemcpyHostToDevice, ctx->stream)) {
        ctx->err = std::string("HIP error: ") + hipGetErrorString(e) + " in the upload of " + who;
        rc = DUSP_ERR_HIP;
    }
    if (!rc) rc = true_peak_launch(ctx, d_planar, n_signals, n_channels, n_samples, sample_rate, ctx->stream);
    if (!rc) rc = true_peak_download(ctx, n_signals * n_channels, words, ctx->stream);
    if (hipError_t e = hipStreamSynchronize(ctx->stream)) {
        if (!rc) ctx->err = std::string("HIP error: ") + hipGetErrorString(e) + " in " + who;
        if (!rc) rc = DUSP_ERR_HIP;
    }
    (void)hipFree(d_planar);
    if (!rc) rc = true_peak_values(ctx, who, words, h_true_peak, nullptr);
    return rc;
    });
}

}  // extern "C"
