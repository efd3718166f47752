// abi_meter.hip — the C ABI (include/dusp_hip.h): the meters of signals on the device (meter_engine.hip: sums of squares and K-weighted hop
// sums, the K-weighting cut in time) and what the library makes of the few thousand doubles that come down, on the host in f64
// (meter_plan.hpp: blocks from hops, the two gates, log10) — dusp_meter_blocks, dusp_meter_device, dusp_meter_host, dusp_meter_last_ms,
// and what dusp_render_host_score_piece_meters (abi_piece.hip) meters its delivery with.  DESIGN.md 6.18; dusp_amd/mix.py meters is the
// contract.
#include <cmath>
#include <string>
#include <vector>

#include "abi_score.hpp"

int meter_check(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate) {
    const std::string w(who);
    if (sample_rate < dusp::kMeterRateMin)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": meters need a sample rate of at least 8000 Hz, not " + std::to_string(sample_rate) + ": the K-weighting's shelf lies at 1682 Hz");
    if (!channels_in_range(n_channels) || !batch_in_range(n_signals, n_samples) || n_signals * n_channels * n_samples > ((size_t)1 << 33))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": meters need 1..64 channels, 1..2^24 signals, 1..2^31 samples and at most 2^33 samples in all");
    return DUSP_OK;
}

int meter_scratch(dusp_ctx *ctx, size_t rows, size_t n_samples, uint32_t hop, size_t extra, dusp::MeterGeometry &G) {
    G = dusp::meter_geometry(rows, n_samples, hop);
    const size_t need = (size_t)G.doubles + extra;
    if (need <= ctx->meter_cap) return DUSP_OK;
    if (ctx->d_meter) HIP_TRY(ctx, hipFree(ctx->d_meter));  // (waits for the device: no launch is reading it any more)
    ctx->d_meter = nullptr;
    ctx->meter_cap = 0;
    HIP_TRY(ctx, hipMalloc((void **)&ctx->d_meter, need * sizeof(double) + g_guard_bytes));
    if (g_guard_bytes) HIP_TRY(ctx, hipMemset((char *)(ctx->d_meter + need), kGuardPattern, g_guard_bytes));
    ctx->meter_cap = need;
    return DUSP_OK;
}

static bool meter_scratch_intact(dusp_ctx *ctx) { return !ctx->d_meter || !g_guard_bytes || guard_intact(ctx->d_meter + ctx->meter_cap); }

// (the sums of a call that gave no device memory for them: d_sumsq [rows] and d_hops [n_signals][n_hops] behind the kernels' scratch)
int meter_launch(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, hipStream_t stream) {
    const uint32_t hop = dusp::meter_hop(sample_rate);
    const size_t rows = n_signals * n_channels, n_hops = (n_samples + hop - 1) / hop;
    dusp::MeterGeometry G;
    if (int rc = meter_scratch(ctx, rows, n_samples, hop, rows + n_signals * n_hops, G)) return rc;
    double *d_sumsq = ctx->d_meter + G.doubles, *d_hops = d_sumsq + rows;
    HIP_TRY(ctx, dusp::launch_meter(d_planar, (uint32_t)n_signals, (uint32_t)n_channels, n_samples, hop, dusp::meter_k_weighting(sample_rate), ctx->d_meter, d_sumsq, d_hops, stream,
                                    nullptr));
    return DUSP_OK;
}

int meter_finish(dusp_ctx *ctx, const char *who, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, hipStream_t stream, double *h_rms, double *h_lufs,
                 double *h_momentary) {
    const uint32_t hop = dusp::meter_hop(sample_rate);
    const size_t rows = n_signals * n_channels, n_hops = (n_samples + hop - 1) / hop, n_blocks = dusp::meter_blocks(n_samples, sample_rate);
    const dusp::MeterGeometry G = dusp::meter_geometry(rows, n_samples, hop);
    std::vector<double> sums(rows + n_signals * n_hops);
    HIP_TRY(ctx, hipMemcpyAsync(sums.data(), ctx->d_meter + G.doubles, sums.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (!meter_scratch_intact(ctx)) CTX_FAIL(ctx, DUSP_ERR_HIP, std::string(who) + ": a meter kernel wrote past the end of its scratch: guard bytes overwritten");
    for (size_t r = 0; r < rows; r++) h_rms[r] = std::sqrt(sums[r] / (double)n_samples);
    for (size_t s = 0; s < n_signals; s++)
        h_lufs[s] = dusp::meter_loudness(sums.data() + rows + s * n_hops, n_blocks, (size_t)4 * hop, h_momentary ? h_momentary + s * n_blocks : nullptr);
    return DUSP_OK;
}

extern "C" {

size_t dusp_meter_blocks(size_t n_samples, uint32_t sample_rate) { return sample_rate < dusp::kMeterRateMin ? 0 : dusp::meter_blocks(n_samples, sample_rate); }

int dusp_meter_last_ms(dusp_ctx *ctx, float ms[4]) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!ms) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_meter_last_ms: NULL buffer");
    if (!ctx->meter_timed) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_meter_last_ms: no dusp_meter_device call has been launched on this context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->meter_marks[4]));
    for (int i = 0; i < 4; i++) HIP_TRY(ctx, hipEventElapsedTime(&ms[i], ctx->meter_marks[i], ctx->meter_marks[i + 1]));
    return DUSP_OK;
}

// The meter kernels alone (meter_engine.hip): the sums of squares and the K-weighted hop sums of signals on the device
int dusp_meter_device(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double *d_sumsq, double *d_hops,
                      void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_meter_device";
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    if (!d_planar || !d_sumsq || !d_hops) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (int rc = meter_check(ctx, who, n_signals, n_channels, n_samples, sample_rate)) return rc;
    if (((uintptr_t)d_planar & 3) || (((uintptr_t)d_sumsq | (uintptr_t)d_hops) & 7)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": d_planar must be 4-byte aligned, d_sumsq and d_hops 8-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    dusp::MeterGeometry G;
    if (int rc = meter_scratch(ctx, n_signals * n_channels, n_samples, dusp::meter_hop(sample_rate), 0, G)) return rc;
    for (hipEvent_t &ev : ctx->meter_marks)
        if (!ev) HIP_TRY(ctx, hipEventCreate(&ev));
    ctx->meter_timed = false;
    const int rc = score_unplanned_call(ctx, stream_, [&](hipStream_t stream) {  // (timed like a score launch too: dusp_score_last_ms)
        HIP_TRY(ctx, dusp::launch_meter(d_planar, (uint32_t)n_signals, (uint32_t)n_channels, n_samples, dusp::meter_hop(sample_rate), dusp::meter_k_weighting(sample_rate),
                                        ctx->d_meter, d_sumsq, d_hops, stream, ctx->meter_marks));
        return DUSP_OK;
    });
    ctx->meter_timed = rc == DUSP_OK;
    return rc;
    });
}

int dusp_meter_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double *h_rms, double *h_lufs,
                    double *h_momentary) {
    if (!ctx) return DUSP_ERR_ARG;
    const char *who = "dusp_meter_host";
    return guarded(ctx->err, who, [&]() -> int {
    if (!h_planar || !h_rms || !h_lufs) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": NULL buffer");
    if (int rc = meter_check(ctx, who, n_signals, n_channels, n_samples, sample_rate)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n_floats = n_signals * n_channels * n_samples;
    float *d_planar = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&d_planar, n_floats * sizeof(float)));
    int rc = DUSP_OK;
    if (hipError_t e = hipMemcpyAsync(d_planar, h_planar, n_floats * sizeof(float), hipMemcpyHostToDevice, ctx->stream)) {
        ctx->err = std::string("HIP error: ") + hipGetErrorString(e) + " in the upload of " + who;
        rc = DUSP_ERR_HIP;
    }
    if (!rc) rc = meter_launch(ctx, d_planar, n_signals, n_channels, n_samples, sample_rate, ctx->stream);
    if (!rc) rc = meter_finish(ctx, who, n_signals, n_channels, n_samples, sample_rate, ctx->stream, h_rms, h_lufs, h_momentary);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_planar);
    return rc;
    });
}

}  // extern "C"
