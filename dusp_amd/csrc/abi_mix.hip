// abi_mix.hip — the C ABI (include/dusp_hip.h): a batch of rendered voices mixed on the device in Sum.many's chain order (dusp_mix_device;
// mix_engine.hip), the tiles a batch too large for the device renders in (TiledBatch, also under the scores of abi_score.hip), and the
// host round trip that delivers a mix (dusp_render_host_mix).
#include <cstring>

#include "abi_internal.hpp"
#include "render_plan.hpp"

extern "C" {

int dusp_mix_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples, const float *d_gains, const float *d_init,
                    int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, "dusp_mix_device", [&]() -> int {
    if (!d_planar || !d_out) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_mix_device: NULL buffer");
    if (int rc = check_planar_pcm(ctx, "dusp_mix_device", n_instances, n_channels, n_samples)) return rc;
    if (n_channels * n_samples > kMixRowMax)  // (one lane per float of the row at the most: the grid's 2^32 threads)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_mix_device: channels x samples must not exceed 2^31: mix such a batch channel by channel or in windows of the timeline");
    if ((((uintptr_t)d_planar | (uintptr_t)d_gains | (uintptr_t)d_init | (uintptr_t)d_out) & 3) != 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_mix_device: the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, dusp::launch_mix(d_planar, d_gains, d_init, d_out, (uint64_t)n_channels * n_samples, (uint32_t)n_instances, raw != 0, ctx->n_cus,
                                  ctx->knobs.mix_width, ctx->knobs.mix_depth, stream_of(ctx, stream_)));
    return DUSP_OK;
    });
}

}  // extern "C"

// The tiles of one batch (abi_internal.hpp TiledBatch).  Every tile's columns of the slot-major table [n_params][n_instances], tile after
// tile, are gathered once: nothing on the host is reused from one tile to the next, so the tiles queue up on the stream without the host
// waiting for any of them
TiledBatch::TiledBatch(dusp_program *prog_, size_t n_instances_, const float *h_params, const float *h_gains_, size_t tile_)
    : prog(prog_), stream(prog_->ctx->stream), n_instances(n_instances_), n_params(prog_->P.g.n_params), tile(tile_), h_gains(h_gains_) {
    whole_batch_decisions(h_params);
    cols.resize(n_params * n_instances);
    for (size_t lo = 0; lo < n_instances && n_params; lo += tile) gather(h_params, lo, std::min(tile, n_instances - lo));
}
// ... or the tiles are the instance ranges [starts[i], starts[i + 1]) (dusp_render_host_score_parts: a part's share of every tile of
// the piece), gathered the same way
TiledBatch::TiledBatch(dusp_program *prog_, size_t n_instances_, const float *h_params, const std::vector<size_t> &starts)
    : prog(prog_), stream(prog_->ctx->stream), n_instances(n_instances_), n_params(prog_->P.g.n_params), tile(0), h_gains(nullptr) {
    whole_batch_decisions(h_params);
    cols.resize(n_params * n_instances);
    for (size_t i = 0; i + 1 < starts.size() && n_params; i++) gather(h_params, starts[i], starts[i + 1] - starts[i]);
}
void TiledBatch::gather(const float *h_params, size_t lo, size_t n) {
    for (size_t p = 0; p < n_params; p++) std::memcpy(&cols[n_params * lo + p * n], h_params + p * n_instances + lo, n * sizeof(float));
}
void TiledBatch::whole_batch_decisions(const float *h_params) {
    prog->mix_n_inst = (uint32_t)n_instances;
    host_param_bounds(prog, n_params ? h_params : nullptr, n_instances);  // (the whole batch's: every tile decides alike)
    prog->mix_range.assign(3 * n_params, 0u);
    for (size_t p = 0; p < n_params; p++)
        for (size_t i = 0; i < n_instances; i++) {
            const float v = h_params[p * n_instances + i];
            if (!(v > 0.f && v <= 3.0e38f)) prog->mix_range[3 * p + 2] = 1u;
            else {
                unsigned b;
                std::memcpy(&b, &v, 4);  // (positive floats order like their bits)
                prog->mix_range[3 * p] = std::max(prog->mix_range[3 * p], 0x7fffffffu - b);
                prog->mix_range[3 * p + 1] = std::max(prog->mix_range[3 * p + 1], b);
            }
        }
}
TiledBatch::~TiledBatch() {
    if (staged) (void)hipStreamSynchronize(stream);  // (a return in the middle of the tiles)
    prog->mix_range.clear();
    prog->mix_n_inst = 0;
    prog->param_bound.clear();
    prog->mixed = true;  // (whichever tile was the last to render, the whole batch it was not)
}
int TiledBatch::render_tile(size_t lo, size_t n, size_t n_samples, const float *d_inputs) {
    dusp_ctx *ctx = prog->ctx;
    if (n_params) {
        HIP_TRY(ctx, hipMemcpyAsync(prog->d_host_par.p, &cols[n_params * lo], n_params * n * sizeof(float), hipMemcpyHostToDevice, stream));
        staged = true;
    }
    if (h_gains) HIP_TRY(ctx, hipMemcpyAsync(prog->d_mix_gains.p, h_gains + lo, n * sizeof(float), hipMemcpyHostToDevice, stream));
    if (int rc = render_device_unguarded(prog, n, n_samples, n_params ? prog->d_host_par.p : nullptr, d_inputs, prog->d_host_out.p, stream)) return rc;
    return check_guards(prog, stream);
}

// what dusp_render_host_mix and dusp_render_host_score refuse alike, and the tile both render in: the tile's PCM, its parameter columns
// and gains are all that lives on the device beside the sums, whatever n_instances is
int tiled_batch_prepare(dusp_program *prog, const char *who, size_t n_instances, size_t n_samples, const float *h_params, const float *h_gains,
                               size_t tile_instances, int format, int normalise, const void *h_out, size_t *tile_out) {
    dusp_ctx *ctx = prog->ctx;
    const std::string w(who);
    if (!h_out) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_out is NULL");
    if (int rc = check_batch(ctx, who, n_instances, n_samples)) return rc;
    if (int rc = check_pcm_format(ctx, who, format, /*allow_planar=*/true)) return rc;
    if (int rc = check_normalise(ctx, who, normalise)) return rc;
    if (prog->P.g.n_inputs > 0)
        CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": the program reads host-generated input streams; render it with dusp_render_host_inputs and mix on the host");
    if (prog->resumable) CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": a resumable program (DUSP_ENGINE_RESUMABLE) is not mixed: its tiles would continue one another");
    const size_t n_ch = prog->P.out_bufs.size(), n_params = prog->P.g.n_params;
    if (int rc = check_channels(ctx, who, n_ch)) return rc;
    const size_t row = n_ch * n_samples;
    if (row > kMixRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": channels x samples must not exceed 2^31: mix such a render in windows of the timeline");
    if (n_params && !h_params) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": program has parameters but h_params is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t free_bytes = 0, total_bytes = 0;
    if (tile_instances == 0 && ctx->knobs.mix_tile_mb <= 0) HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));  // (the default tile: by the device's free memory)
    const size_t tile = dusp::mix_tile_instances(tile_instances, ctx->knobs.mix_tile_mb, free_bytes, prog->d_host_out.cap * sizeof(float), ctx->n_cus, row, n_instances);
    HIP_TRY(ctx, prog->d_host_out.ensure(tile * row));
    if (n_params) HIP_TRY(ctx, prog->d_host_par.ensure(n_params * tile));
    if (h_gains) HIP_TRY(ctx, prog->d_mix_gains.ensure(tile));
    *tile_out = tile;
    return DUSP_OK;
}

extern "C" {

int dusp_render_host_mix(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_gains, size_t tile_instances,
                         int format, int normalise, void *h_out, float *h_peak) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    return guarded(ctx->err, "dusp_render_host_mix", [&]() -> int {
    size_t tile = 0;
    if (int rc = tiled_batch_prepare(prog, "dusp_render_host_mix", n_instances, n_samples, h_params, h_gains, tile_instances, format, normalise, h_out, &tile)) return rc;
    const size_t n_ch = prog->P.out_bufs.size();
    HIP_TRY(ctx, prog->d_mix.ensure(n_ch * n_samples));  // the running sums
    TiledBatch whole(prog, n_instances, h_params, h_gains, tile);
    for (size_t lo = 0; lo < n_instances; lo += tile) {
        const size_t n = std::min(tile, n_instances - lo);
        const bool last = lo + n == n_instances;
        if (int rc = whole.render_tile(lo, n, n_samples)) return rc;
        if (int rc = dusp_mix_device(ctx, prog->d_host_out.p, n, n_ch, n_samples, h_gains ? prog->d_mix_gains.p : nullptr, lo > 0 ? prog->d_mix.p : nullptr, !last,
                                     prog->d_mix.p, ctx->stream))
            return rc;
    }
    if (int rc = deliver_host(prog, prog->d_mix.p, nullptr, 1, n_ch, n_samples, format, normalise, h_peak, h_out)) return rc;
    whole.staged = false;  // (the delivery has waited for the stream)
    if (g_guard_bytes && (!prog->d_mix.intact() || !prog->d_mix_gains.intact()))
        CTX_FAIL(ctx, DUSP_ERR_HIP, "dusp_render_host_mix: the mix kernel wrote past the end of a device buffer: guard bytes overwritten");
    return DUSP_OK;
    });
}

}  // extern "C"
