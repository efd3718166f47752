// abi_deliver.hip — the C ABI (include/dusp_hip.h): what happens to rendered PCM on the device before it leaves (interleave, peak, encode) and how
// it reaches the host (dusp_render_host* and the delivery paths every host render ends with: deliver_host).
#include <limits>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "abi_internal.hpp"
#include "pcm_quant.hpp"

extern "C" {

// (pcm_format 0: f32 as rendered, planar or interleaved; DUSP_PCM_*: encoded frames, dusp_render_host_pcm)
static int render_host(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_inputs, void *h_out,
                       bool interleaved, int pcm_format = 0, int normalise = 0, float *h_peaks = nullptr);

int dusp_render_host(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, float *h_out) {
    return render_host(prog, n_instances, n_samples, h_params, nullptr, h_out, false);
}

int dusp_render_host_interleaved(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, float *h_out) {
    return render_host(prog, n_instances, n_samples, h_params, nullptr, h_out, true);
}

int dusp_render_host_inputs(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_inputs,
                            float *h_out, int interleaved) {
    if (!prog) return DUSP_ERR_ARG;
    if (prog->P.g.n_inputs > 0 && !h_inputs) CTX_FAIL(prog->ctx, DUSP_ERR_ARG, "render: the program has input streams but h_inputs is NULL");
    return render_host(prog, n_instances, n_samples, h_params, h_inputs, h_out, interleaved != 0);
}

int dusp_interleave_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples, float *d_interleaved,
                           void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!d_planar || !d_interleaved) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_interleave_device: NULL buffer");
    if (!channels_in_range(n_channels) || n_instances < 1 || !samples_in_range(n_samples) || (n_samples + 127) / 128 * n_instances > 0x7fffffffull)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_interleave_device: need 1..64 channels and at most 2^31 tiles of 128 frames");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, dusp::launch_interleave(d_planar, d_interleaved, (uint32_t)n_instances, (uint32_t)n_channels, n_samples,
                                         stream_of(ctx, stream_)));
    return DUSP_OK;
}

int dusp_peak_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples, float *d_peaks, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!d_planar || !d_peaks) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_peak_device: NULL buffer");
    if (int rc = check_planar_pcm(ctx, "dusp_peak_device", n_instances, n_channels, n_samples)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, dusp::launch_pcm_peak(d_planar, d_peaks, (uint32_t)n_instances, (uint32_t)n_channels, n_samples, ctx->n_cus,
                                       stream_of(ctx, stream_)));
    return DUSP_OK;
}

int dusp_encode_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples, int format, int normalise,
                       const float *d_peaks, void *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!d_planar || !d_out) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_encode_device: NULL buffer");
    if (int rc = check_pcm_format(ctx, "dusp_encode_device", format, /*allow_planar=*/false)) return rc;
    if (int rc = check_normalise(ctx, "dusp_encode_device", normalise)) return rc;
    if (normalise != DUSP_NORMALISE_NONE && !d_peaks) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_encode_device: normalising needs d_peaks (dusp_peak_device)");
    if (!channels_in_range(n_channels) || !batch_in_range(n_instances, n_samples) ||
        dusp::pcm_encode_tiles(n_instances, (uint32_t)n_channels, n_samples, format) > 0x7fffffffull)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_encode_device: need 1..64 channels, 1..2^24 instances, 1..2^31 samples and at most 2^31 tiles");
    if (format == DUSP_PCM_F32 && ((uintptr_t)d_out & 3)) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_encode_device: f32 frames need a 4-byte aligned d_out");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, dusp::launch_pcm_encode(d_planar, d_peaks, format, normalise, d_out, (uint32_t)n_instances, (uint32_t)n_channels, n_samples, ctx->n_cus,
                                         stream_of(ctx, stream_)));
    return DUSP_OK;
}

int dusp_render_host_pcm(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_inputs, int format, int normalise,
                         void *h_out, float *h_peaks) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    if (int rc = check_pcm_format(ctx, "dusp_render_host_pcm", format, /*allow_planar=*/false)) return rc;
    if (int rc = check_normalise(ctx, "dusp_render_host_pcm", normalise)) return rc;
    if (int rc = check_channels(ctx, "dusp_render_host_pcm", prog->P.out_bufs.size())) return rc;
    if (prog->P.g.n_inputs > 0 && !h_inputs) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: the program has input streams but h_inputs is NULL");
    return render_host(prog, n_instances, n_samples, h_params, prog->P.g.n_inputs > 0 ? h_inputs : nullptr, h_out, false, format, normalise, h_peaks);
}

// Device -> host delivery of the rendered PCM (what renderChannelData's caller finally holds).
//   * h_out is pinned memory (dusp_host_alloc, or registered by the caller): one asynchronous DMA straight into it.
//   * h_out is pageable and large: kCopyWorkers worker threads, each with its own stream and a pair of pinned staging
//     tiles, walk disjoint ranges of the output — DMA of tile i+1 into one tile while the CPU copies tile i out of the
//     other.  (A plain hipMemcpy to pageable memory stages through ONE pinned buffer with ONE copying thread: 10-13 GB/s.)
//   * small outputs (event-segmented rendering: hundreds of short renders a second): plain asynchronous copy.
constexpr size_t kCopyTileBytes = (size_t)8 << 20;   // 8 MiB staging tiles
constexpr int kCopyWorkers = 4;
constexpr size_t kStagedMinBytes = (size_t)32 << 20;  // 32 MiB: below this the staging pipeline is not worth its threads

static bool is_pinned_host(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // an unregistered pointer is reported as an error: not one of ours
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

static hipError_t download_staged(dusp_program *prog, void *h_out_, const void *d_src_, size_t n_bytes) {
    dusp_ctx *ctx = prog->ctx;
    unsigned char *h_out = (unsigned char *)h_out_;
    const unsigned char *d_src = (const unsigned char *)d_src_;
    const size_t need = (size_t)kCopyWorkers * 2 * kCopyTileBytes;
    if (prog->pin_bytes < need) {
        if (prog->pin[0]) (void)hipHostFree(prog->pin[0]);
        prog->pin[0] = nullptr;
        prog->pin_bytes = 0;
        hipError_t e = hipHostMalloc((void **)&prog->pin[0], need, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        prog->pin_bytes = need;
    }
    hipError_t e = hipStreamSynchronize(ctx->stream);  // the render (and the interleave) have finished: the workers only copy
    if (e != hipSuccess) return e;
    hipError_t results[kCopyWorkers];
    std::thread workers[kCopyWorkers];
    const size_t n_tiles = (n_bytes + kCopyTileBytes - 1) / kCopyTileBytes;
    for (int w = 0; w < kCopyWorkers; w++) {
        results[w] = hipSuccess;
        workers[w] = std::thread([&, w]() {
            hipError_t &r = results[w];
            hipStream_t st = nullptr;
            if ((r = hipSetDevice(ctx->device)) != hipSuccess || (r = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) return;
            unsigned char *tile[2] = {prog->pin[0] + (size_t)(2 * w) * kCopyTileBytes, prog->pin[0] + (size_t)(2 * w + 1) * kCopyTileBytes};
            // this worker's tiles: a contiguous range (neighbouring pages of h_out are faulted in by one thread)
            const size_t t0 = n_tiles * (size_t)w / kCopyWorkers, t1 = n_tiles * (size_t)(w + 1) / kCopyWorkers;
            auto span = [&](size_t t, size_t &at, size_t &n) {
                at = t * kCopyTileBytes;
                n = std::min(kCopyTileBytes, n_bytes - at);
            };
            hipEvent_t done[2] = {nullptr, nullptr};
            if ((r = hipEventCreateWithFlags(&done[0], hipEventDisableTiming)) == hipSuccess) r = hipEventCreateWithFlags(&done[1], hipEventDisableTiming);
            size_t at, n;
            for (size_t t = t0; r == hipSuccess && t < std::min(t0 + 2, t1); t++) {  // prime both tiles
                span(t, at, n);
                if ((r = hipMemcpyAsync(tile[(t - t0) & 1], d_src + at, n, hipMemcpyDeviceToHost, st)) == hipSuccess)
                    r = hipEventRecord(done[(t - t0) & 1], st);
            }
            for (size_t t = t0; r == hipSuccess && t < t1; t++) {
                const int k = (int)((t - t0) & 1);
                if ((r = hipEventSynchronize(done[k])) != hipSuccess) break;
                span(t, at, n);
                std::memcpy(h_out + at, tile[k], n);
                if (t + 2 < t1) {
                    span(t + 2, at, n);
                    if ((r = hipMemcpyAsync(tile[k], d_src + at, n, hipMemcpyDeviceToHost, st)) == hipSuccess)
                        r = hipEventRecord(done[k], st);
                }
            }
            (void)hipStreamSynchronize(st);
            if (done[0]) (void)hipEventDestroy(done[0]);
            if (done[1]) (void)hipEventDestroy(done[1]);
            (void)hipStreamDestroy(st);
        });
    }
    for (auto &t : workers) t.join();
    for (hipError_t r : results)
        if (r != hipSuccess) return r;
    return hipSuccess;
}

}  // extern "C"

// d_src, n_bytes of device memory, reaches h_out by the delivery paths above; waits for the stream
static int deliver_download(dusp_program *prog, const void *d_src, size_t n_bytes, void *h_out) {
    dusp_ctx *ctx = prog->ctx;
    if (n_bytes >= kStagedMinBytes && !is_pinned_host(h_out)) {
        HIP_TRY(ctx, download_staged(prog, h_out, d_src, n_bytes));
    } else {  // pinned destination: one DMA at link speed; small output: not worth more
        HIP_TRY(ctx, hipMemcpyAsync(h_out, d_src, n_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return DUSP_OK;
}

// gain, quantisation and interleave on the device, into the program's d_host_pcm: 2 or 3 bytes a sample cross the link.  -> its bytes
static int deliver_encode(dusp_program *prog, const float *d_planar, size_t n_instances, size_t n_ch, size_t n_samples, int pcm_format, int normalise, const float *d_peaks,
                          size_t &n_bytes) {
    dusp_ctx *ctx = prog->ctx;
    n_bytes = n_instances * n_ch * n_samples * (size_t)dusp::pcm_bytes_per_sample(pcm_format);
    HIP_TRY(ctx, prog->d_host_pcm.ensure(n_bytes));
    if (int rc = dusp_encode_device(ctx, d_planar, n_instances, n_ch, n_samples, pcm_format, normalise, d_peaks, prog->d_host_pcm.p, ctx->stream)) return rc;
    if (g_guard_bytes) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (!prog->d_host_pcm.intact() || !prog->d_host_peaks.intact() || !prog->d_host_peak_common.intact())
            CTX_FAIL(ctx, DUSP_ERR_HIP, "render: the PCM encoder wrote past the end of a device buffer: guard bytes overwritten");
    }
    return DUSP_OK;
}

int deliver_peaks(dusp_program *prog, const float *d_planar, size_t n_instances, size_t n_ch, size_t n_samples, float *h_peaks) {
    dusp_ctx *ctx = prog->ctx;
    HIP_TRY(ctx, prog->d_host_peaks.ensure(n_instances));
    if (int rc = dusp_peak_device(ctx, d_planar, n_instances, n_ch, n_samples, prog->d_host_peaks.p, ctx->stream)) return rc;
    if (h_peaks) HIP_TRY(ctx, hipMemcpyAsync(h_peaks, prog->d_host_peaks.p, n_instances * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return DUSP_OK;
}

int deliver_at_level(dusp_program *prog, const float *d_planar, size_t n_instances, size_t n_ch, size_t n_samples, int pcm_format, float level, void *h_out) {
    dusp_ctx *ctx = prog->ctx;
    const std::vector<float> levels(n_instances, level);  // (the upload has read it once the delivery has waited for the stream)
    HIP_TRY(ctx, prog->d_host_peak_common.ensure(n_instances));
    HIP_TRY(ctx, hipMemcpyAsync(prog->d_host_peak_common.p, levels.data(), n_instances * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    size_t n_bytes = 0;
    int rc = deliver_encode(prog, d_planar, n_instances, n_ch, n_samples, pcm_format, DUSP_NORMALISE_FULL, prog->d_host_peak_common.p, n_bytes);
    if (!rc) rc = deliver_download(prog, prog->d_host_pcm.p, n_bytes, h_out);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// What a host render ends with: d_planar f32 [n_instances][n_ch][n_samples] (or, already transposed, d_frames) reaches h_out — as it is,
// or (pcm_format != 0) through the peak and encode kernels — by the delivery paths above; waits for the stream.
int deliver_host(dusp_program *prog, const float *d_planar, const float *d_frames, size_t n_instances, size_t n_ch, size_t n_samples, int pcm_format,
                 int normalise, float *h_peaks, void *h_out, bool common_peak) {
    dusp_ctx *ctx = prog->ctx;
    const void *d_src = d_frames ? d_frames : d_planar;
    size_t n_bytes = n_instances * n_ch * n_samples * sizeof(float);
    const float *d_peaks = nullptr;
    if ((pcm_format && (normalise || h_peaks)) || (common_peak && h_peaks)) {  // (the signals of a call with stems are metered whatever the format)
        if (int rc = deliver_peaks(prog, d_planar, n_instances, n_ch, n_samples, h_peaks)) return rc;
        d_peaks = prog->d_host_peaks.p;
    }
    if (pcm_format) {
        if (common_peak && normalise) {  // (one gain for all: the encoder reads peaks[inst], every one of them the largest)
            HIP_TRY(ctx, prog->d_host_peak_common.ensure(n_instances));
            HIP_TRY(ctx, dusp::launch_pcm_peak_common(d_peaks, prog->d_host_peak_common.p, (uint32_t)n_instances, ctx->stream));
            d_peaks = prog->d_host_peak_common.p;
        }
        if (int rc = deliver_encode(prog, d_planar, n_instances, n_ch, n_samples, pcm_format, normalise, d_peaks, n_bytes)) return rc;
        d_src = prog->d_host_pcm.p;
    }
    return deliver_download(prog, d_src, n_bytes, h_out);
}

extern "C" {

static int render_host(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_inputs, void *h_out,
                       bool interleaved, int pcm_format, int normalise, float *h_peaks) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    return guarded(ctx->err, "render", [&]() -> int {
    if (!h_out) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: h_out is NULL");
    if (int rc = check_batch(ctx, "render", n_instances, n_samples)) return rc;
    const size_t n_par = (size_t)prog->P.g.n_params * n_instances;
    if (n_par && !h_params) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: program has parameters but h_params is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(); };
    const size_t n_out = n_instances * prog->P.out_bufs.size() * n_samples;
    // staging buffers live with the program (grown on demand): a segmented render calls this hundreds of times a second
    HIP_TRY(ctx, prog->d_host_out.ensure(std::max<size_t>(1, n_out)));
    const double us_alloc = since();
    float *d_out = prog->d_host_out.p, *d_par = nullptr, *d_frames = nullptr;
    if (n_par) {
        HIP_TRY(ctx, prog->d_host_par.ensure(n_par));
        d_par = prog->d_host_par.p;
        HIP_TRY(ctx, hipMemcpyAsync(d_par, h_params, n_par * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    const size_t n_in = (size_t)prog->P.g.n_inputs * n_instances * n_samples;
    float *d_in = nullptr;
    if (n_in && !h_inputs) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: the program reads host-generated input streams; use dusp_render_host_inputs");
    if (n_in) {
        HIP_TRY(ctx, prog->d_host_in.ensure(n_in));
        d_in = prog->d_host_in.p;
        HIP_TRY(ctx, hipMemcpyAsync(d_in, h_inputs, n_in * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    host_param_bounds(prog, n_par ? h_params : nullptr, n_instances);  // (for the planner's time-split gate)
    const int rc_render = render_device_unguarded(prog, n_instances, n_samples, d_par, d_in, d_out, ctx->stream);
    prog->param_bound.clear();  // (a render from device memory brings no table the host can read)
    if (rc_render) return rc_render;
    const double us_enqueued = since();
    if (int rc = check_guards(prog, ctx->stream)) return rc;
    const size_t n_ch = prog->P.out_bufs.size();
    if (interleaved && n_ch > 1) {  // frames: transpose on the device, then download those
        HIP_TRY(ctx, prog->d_host_frames.ensure(n_out));
        d_frames = prog->d_host_frames.p;
        if (int rc = dusp_interleave_device(ctx, d_out, n_instances, n_ch, n_samples, d_frames, ctx->stream)) return rc;
    }
    if (int rc = deliver_host(prog, d_out, d_frames, n_instances, n_ch, n_samples, pcm_format, normalise, h_peaks, h_out)) return rc;
    if (ctx->knobs.jit_log >= 2)  // (DUSP_JIT_LOG=2: where a host render's time goes)
        fprintf(stderr, "[dusp host render] output buffer %.0f us, render enqueued (workspaces, constants, launches) %.0f us, download + wait %.0f us\n", us_alloc, us_enqueued - us_alloc,
                since() - us_enqueued);
    return DUSP_OK;
    });
}

}  // extern "C"
