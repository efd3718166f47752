// abi_deliver.hip — the C ABI (include/dusp_hip.h): what happens to rendered PCM on the device (interleave, peak, encode, mix, score, score over rows) and how
// it reaches the host (dusp_render_host* and their delivery paths, dusp_render_host_mix, dusp_render_host_score, dusp_render_host_score_parts).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

#include "abi_internal.hpp"
#include "pcm_quant.hpp"
#include "render_plan.hpp"

extern "C" {

// (pcm_format 0: f32 as rendered, planar or interleaved; DUSP_PCM_*: encoded frames, dusp_render_host_pcm)
static int render_host(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_inputs, void *h_out,
                       bool interleaved, int pcm_format = 0, int normalise = 0, float *h_peaks = nullptr);

// 1..64 channels of [1, 2^24] instances x [1, 2^31] samples: what the kernels over planar PCM take
static int check_planar_pcm(dusp_ctx *ctx, const char *who, size_t n_instances, size_t n_channels, size_t n_samples) {
    if (!channels_in_range(n_channels) || !batch_in_range(n_instances, n_samples))
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": need 1..64 channels, 1..2^24 instances and 1..2^31 samples");
    return DUSP_OK;
}

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

// What a host render ends with: d_planar f32 [n_instances][n_ch][n_samples] (or, already transposed, d_frames) reaches h_out — as it is,
// or (pcm_format != 0) through the peak and encode kernels — by the delivery paths above; waits for the stream.
static int deliver_host(dusp_program *prog, const float *d_planar, const float *d_frames, size_t n_instances, size_t n_ch, size_t n_samples, int pcm_format,
                        int normalise, float *h_peaks, void *h_out) {
    dusp_ctx *ctx = prog->ctx;
    const size_t n_out = n_instances * n_ch * n_samples;
    const void *d_src = d_frames ? d_frames : d_planar;
    size_t n_bytes = n_out * sizeof(float);
    if (pcm_format) {  // peak, gain, quantisation and interleave on the device: 2 or 3 bytes a sample cross the link
        const float *d_peaks = nullptr;
        if (normalise || h_peaks) {
            HIP_TRY(ctx, prog->d_host_peaks.ensure(n_instances));
            d_peaks = prog->d_host_peaks.p;
            if (int rc = dusp_peak_device(ctx, d_planar, n_instances, n_ch, n_samples, prog->d_host_peaks.p, ctx->stream)) return rc;
            if (h_peaks) HIP_TRY(ctx, hipMemcpyAsync(h_peaks, d_peaks, n_instances * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        }
        n_bytes = n_out * (size_t)dusp::pcm_bytes_per_sample(pcm_format);
        HIP_TRY(ctx, prog->d_host_pcm.ensure(n_bytes));
        if (int rc = dusp_encode_device(ctx, d_planar, n_instances, n_ch, n_samples, pcm_format, normalise, d_peaks, prog->d_host_pcm.p, ctx->stream)) return rc;
        if (g_guard_bytes) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (!prog->d_host_pcm.intact() || !prog->d_host_peaks.intact())
                CTX_FAIL(ctx, DUSP_ERR_HIP, "render: the PCM encoder wrote past the end of a device buffer: guard bytes overwritten");
        }
        d_src = prog->d_host_pcm.p;
    }
    if (n_bytes >= kStagedMinBytes && !is_pinned_host(h_out)) {
        HIP_TRY(ctx, download_staged(prog, h_out, d_src, n_bytes));
    } else {  // pinned destination: one DMA at link speed; small output: not worth more
        HIP_TRY(ctx, hipMemcpyAsync(h_out, d_src, n_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return DUSP_OK;
}

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
    if (int rc = render_device_unguarded(prog, n_instances, n_samples, d_par, d_in, d_out, ctx->stream)) return rc;
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

constexpr size_t kMixRowMax = (size_t)1 << 31;  // floats in one voice's PCM that the mix kernel's grid covers (mix_engine.hip launch_mix)

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

// The tiles of one batch (dusp_render_host_mix, dusp_render_host_score).  Tiling must not change a bit.  What a render decides from the
// batch and that changes bits is, while the tiles render, decided from the WHOLE batch: a Filter with a per-instance cutoff runs as a scan
// or as a recurrence — not the same bits — by the range of its column (mix_range), and so does every scan-eligible Filter by whether the
// render is cut into warming segments, which the instance count decides (mix_n_inst, which also makes every tile wait for its compiled
// kernel).  Per-instance Delays are classified per tile: their regimes differ in speed only.
struct TiledBatch {
    dusp_program *prog;
    hipStream_t stream;
    size_t n_instances, n_params, tile;
    const float *h_gains;
    bool staged = false;      // host vectors of this call may still be on their way to the device
    std::vector<float> cols;  // (a member: it outlives the destructor's wait for the stream)

    // every tile's columns of the slot-major table [n_params][n_instances], tile after tile, gathered once: nothing on the host is
    // reused from one tile to the next, so the tiles queue up on the stream without the host waiting for any of them
    TiledBatch(dusp_program *prog_, size_t n_instances_, const float *h_params, const float *h_gains_, size_t tile_)
        : prog(prog_), stream(prog_->ctx->stream), n_instances(n_instances_), n_params(prog_->P.g.n_params), tile(tile_), h_gains(h_gains_) {
        whole_batch_decisions(h_params);
        cols.resize(n_params * n_instances);
        for (size_t lo = 0; lo < n_instances && n_params; lo += tile) gather(h_params, lo, std::min(tile, n_instances - lo));
    }
    // ... or the tiles are the instance ranges [starts[i], starts[i + 1]) (dusp_render_host_score_parts: a part's share of every tile of
    // the piece), gathered the same way
    TiledBatch(dusp_program *prog_, size_t n_instances_, const float *h_params, const std::vector<size_t> &starts)
        : prog(prog_), stream(prog_->ctx->stream), n_instances(n_instances_), n_params(prog_->P.g.n_params), tile(0), h_gains(nullptr) {
        whole_batch_decisions(h_params);
        cols.resize(n_params * n_instances);
        for (size_t i = 0; i + 1 < starts.size() && n_params; i++) gather(h_params, starts[i], starts[i + 1] - starts[i]);
    }
    void gather(const float *h_params, size_t lo, size_t n) {
        for (size_t p = 0; p < n_params; p++) std::memcpy(&cols[n_params * lo + p * n], h_params + p * n_instances + lo, n * sizeof(float));
    }
    void whole_batch_decisions(const float *h_params) {
        prog->mix_n_inst = (uint32_t)n_instances;
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
    ~TiledBatch() {
        if (staged) (void)hipStreamSynchronize(stream);  // (a return in the middle of the tiles)
        prog->mix_range.clear();
        prog->mix_n_inst = 0;
        prog->mixed = true;  // (whichever tile was the last to render, the whole batch it was not)
    }
    // instances [lo, lo + n): their columns and gains to the device, their PCM into d_host_out
    int render_tile(size_t lo, size_t n, size_t n_samples) {
        dusp_ctx *ctx = prog->ctx;
        if (n_params) {
            HIP_TRY(ctx, hipMemcpyAsync(prog->d_host_par.p, &cols[n_params * lo], n_params * n * sizeof(float), hipMemcpyHostToDevice, stream));
            staged = true;
        }
        if (h_gains) HIP_TRY(ctx, hipMemcpyAsync(prog->d_mix_gains.p, h_gains + lo, n * sizeof(float), hipMemcpyHostToDevice, stream));
        if (int rc = render_device_unguarded(prog, n, n_samples, n_params ? prog->d_host_par.p : nullptr, nullptr, prog->d_host_out.p, stream)) return rc;
        return check_guards(prog, stream);
    }
};

// what dusp_render_host_mix and dusp_render_host_score refuse alike, and the tile both render in: the tile's PCM, its parameter columns
// and gains are all that lives on the device beside the sums, whatever n_instances is
static int tiled_batch_prepare(dusp_program *prog, const char *who, size_t n_instances, size_t n_samples, const float *h_params, const float *h_gains,
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

// ---- scores: voices mixed at per-voice onsets (score_engine.hip; dusp_amd/mix.py score_chain is the contract) ----

// one launch's plan inside the context's image
struct ScoreLaunch {
    size_t at = 0, n_voices = 0, n_block_first = 0;  // byte offset of the voices; block_first and the entries follow
    uint64_t w_lo = 0, w_hi = 0, first_block = 0;
    uint32_t block_shift = dusp::kScoreGroupShift;
    bool any = false;  // some voice reaches the timeline (else: no plan in the image)
    size_t pan_at = 0;  // a panned launch: byte offset of its voices' coefficients (dusp::ScorePan), behind the plan
    bool frac = false;   // some listed voice starts between samples: the launch is score_frac_engine.hip's ...
    size_t frac_at = 0;  // ... and this the byte offset of its voices' weights (dusp::ScoreFrac), behind the plan
};

// before a call rewrites the context's host image: the last upload has read it
static int score_image_begin(dusp_ctx *ctx) {
    if (!ctx->score_uploaded) {
        HIP_TRY(ctx, hipEventCreate(&ctx->score_uploaded));  // (with timing: dusp_score_last_ms)
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->score_done, hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreate(&ctx->score_up0));
        HIP_TRY(ctx, hipEventCreate(&ctx->score_t0));
        HIP_TRY(ctx, hipEventCreate(&ctx->score_t1));
    } else {
        HIP_TRY(ctx, hipEventSynchronize(ctx->score_uploaded));
    }
    ctx->h_score_plan.clear();
    ctx->score_upload_timed = false;  // (score_up0 .. score_uploaded are about to be another call's)
    return DUSP_OK;
}

// what the plans of ONE call may take together, on the host and on the device
static size_t score_plan_budget(dusp_ctx *ctx) { return ctx->knobs.score_plan_kb > 0 ? (size_t)ctx->knobs.score_plan_kb << 10 : dusp::kScorePlanBytes; }

// plans the voices [0, n) within budget_bytes and appends the plan to the context's host image
static int score_image_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, size_t n, size_t first_voice, uint64_t n_voice,
                           uint64_t n_total, bool whole_timeline, size_t budget_bytes, ScoreLaunch &L) {
    dusp::ScorePlan P;
    const int64_t bad = dusp::score_plan(h_onsets, h_lengths, n, n_voice, n_total, whole_timeline, budget_bytes, P);
    if (bad >= 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the length of voice " + std::to_string(first_voice + (size_t)bad) + " is " + std::to_string(h_lengths[bad]) +
                                        ": lengths must lie in 0 .. n_voice_samples");
    L = ScoreLaunch();
    L.w_lo = (uint64_t)P.w_lo;
    L.w_hi = (uint64_t)P.w_hi;
    L.block_shift = P.block_shift;
    L.first_block = P.first_block;
    L.any = P.n_entries() > 0;
    if (L.any) {
        L.n_voices = n;
        L.n_block_first = P.block_first.size();
        L.at = dusp::score_plan_pack(P, ctx->h_score_plan);
    }
    return DUSP_OK;
}

// the image to the device, ordered on `stream` behind the last launch that read the buffer (whatever stream that one ran on)
static int score_image_upload(dusp_ctx *ctx, hipStream_t stream) {
    const size_t n_bytes = ctx->h_score_plan.size();
    if (!n_bytes) return DUSP_OK;
    if (n_bytes > ctx->score_plan_cap) {
        if (ctx->d_score_plan) HIP_TRY(ctx, hipFree(ctx->d_score_plan));  // (waits for the device: no launch is reading it any more)
        ctx->d_score_plan = nullptr;
        ctx->score_plan_cap = 0;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_score_plan, n_bytes + g_guard_bytes));
        if (g_guard_bytes) HIP_TRY(ctx, hipMemset(ctx->d_score_plan + n_bytes, kGuardPattern, g_guard_bytes));
        ctx->score_plan_cap = n_bytes;
    }
    HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->score_done, 0));
    HIP_TRY(ctx, hipEventRecord(ctx->score_up0, stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_score_plan, ctx->h_score_plan.data(), n_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->score_uploaded, stream));
    return DUSP_OK;
}

static int score_launch(dusp_ctx *ctx, const ScoreLaunch &L, const float *d_planar, size_t n_channels, size_t n_voice, size_t n_total, const float *d_gains,
                        const float *d_init, int raw, float *d_out, hipStream_t stream) {
    if (L.w_hi <= L.w_lo) return DUSP_OK;
    const dusp::ScoreVoice *d_voices = L.any ? (const dusp::ScoreVoice *)(ctx->d_score_plan + L.at) : nullptr;
    const uint32_t *d_block_first = L.any ? (const uint32_t *)(d_voices + L.n_voices) : nullptr;
    HIP_TRY(ctx, dusp::launch_score(d_planar, d_gains, d_voices, d_block_first, L.any ? d_block_first + L.n_block_first : nullptr, d_init, d_out, (uint32_t)n_channels, n_voice,
                                    n_total, L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    if (L.any) HIP_TRY(ctx, hipEventRecord(ctx->score_done, stream));
    return DUSP_OK;
}

static bool score_plan_intact(dusp_ctx *ctx) { return !ctx->d_score_plan || !g_guard_bytes || guard_intact(ctx->d_score_plan + ctx->score_plan_cap); }

int dusp_score_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_voice_samples, const int64_t *h_onsets,
                      const int64_t *h_lengths, const float *d_gains, size_t n_total_samples, const float *d_init, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, "dusp_score_device", [&]() -> int {
    if (!d_out || (n_instances && (!d_planar || !h_onsets))) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: NULL buffer");
    if (!channels_in_range(n_channels) || n_instances > (1u << 24) || !samples_in_range(n_voice_samples) || !samples_in_range(n_total_samples))
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: need 1..64 channels, 0..2^24 instances, 1..2^31 samples a voice and 1..2^31 samples of timeline");
    if (n_channels * n_total_samples > dusp::kScoreRowMax)  // (one lane per float of the timeline: the grid, and the kernel's 32-bit sample positions)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: channels x timeline samples must not exceed 2^31: score such a piece channel by channel or in windows of the timeline");
    if (n_channels * n_voice_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: channels x voice samples must not exceed 2^31");
    if ((((uintptr_t)d_planar | (uintptr_t)d_gains | (uintptr_t)d_init | (uintptr_t)d_out) & 3) != 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_device: the buffers must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    ScoreLaunch L;
    L.w_hi = n_total_samples;  // (no voices: `|| 0`, or a copy, of d_init alone)
    if (n_instances) {
        if (int rc = score_image_begin(ctx)) return rc;
        const auto t_plan = std::chrono::steady_clock::now();
        if (int rc = score_image_add(ctx, "dusp_score_device", h_onsets, h_lengths, n_instances, 0, n_voice_samples, n_total_samples, /*whole_timeline=*/true,
                                     score_plan_budget(ctx), L))
            return rc;
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
    if (int rc = score_launch(ctx, L, d_planar, n_channels, n_voice_samples, n_total_samples, d_gains, d_init, raw != 0, d_out, stream)) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->score_t1, stream));
    ctx->score_timed = true;
    return DUSP_OK;
    });
}

int dusp_score_last_ms(dusp_ctx *ctx, float *kernel_ms, float *plan_ms, float *upload_ms) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!ctx->score_timed) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_score_last_ms: no dusp_score_device call has been launched on this context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->score_t1));
    float k = 0, u = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&k, ctx->score_t0, ctx->score_t1));
    if (ctx->score_upload_timed) HIP_TRY(ctx, hipEventElapsedTime(&u, ctx->score_up0, ctx->score_uploaded));
    if (kernel_ms) *kernel_ms = k;
    if (plan_ms) *plan_ms = (float)ctx->score_plan_ms;
    if (upload_ms) *upload_ms = u;
    return DUSP_OK;
}

int dusp_render_host_score(dusp_program *prog, size_t n_instances, size_t n_voice_samples, size_t n_total_samples, const float *h_params, const float *h_gains,
                           const int64_t *h_onsets, const int64_t *h_lengths, size_t tile_instances, int format, int normalise, void *h_out, float *h_peak) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    return guarded(ctx->err, "dusp_render_host_score", [&]() -> int {
    const size_t n_ch = prog->P.out_bufs.size();
    if (!h_onsets) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_render_host_score: h_onsets is NULL");
    if (!samples_in_range(n_total_samples) || n_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_render_host_score: the timeline must have 1..2^31 samples and channels x timeline samples must not exceed 2^31: render such a piece in windows of the timeline");
    size_t tile = 0;  // (sized over the VOICE's row: the tile holds voices, the timeline is one row beside it)
    if (int rc = tiled_batch_prepare(prog, "dusp_render_host_score", n_instances, n_voice_samples, h_params, h_gains, tile_instances, format, normalise, h_out, &tile))
        return rc;
    // every tile's plan, over the tile's union window, made and uploaded once: the tiles queue up on the stream without the host waiting
    // (the byte budget is the CALL's, shared out over the tiles: a tile whose lists do not fit its share doubles its block.  What no block
    // size takes away is 28 bytes a voice — its record, one list entry, one block_first word — and 40 a tile)
    std::vector<ScoreLaunch> launches((n_instances + tile - 1) / tile);
    const size_t tile_budget = score_plan_budget(ctx) / launches.size();
    if (int rc = score_image_begin(ctx)) return rc;
    const auto t_plan = std::chrono::steady_clock::now();
    for (size_t lo = 0, i = 0; lo < n_instances; lo += tile, i++)
        if (int rc = score_image_add(ctx, "dusp_render_host_score", h_onsets + lo, h_lengths ? h_lengths + lo : nullptr, std::min(tile, n_instances - lo), lo, n_voice_samples,
                                     n_total_samples, /*whole_timeline=*/false, tile_budget, launches[i]))
            return rc;
    if (ctx->knobs.jit_log >= 2)  // (DUSP_JIT_LOG=2: what the plans cost the host)
        fprintf(stderr, "[dusp host score] %zu plans (tiles of %zu voices) in %.0f us on the host: %zu bytes, blocks of %u samples in the first tile\n", launches.size(), tile,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count(), ctx->h_score_plan.size(), 1u << launches[0].block_shift);
    HIP_TRY(ctx, prog->d_mix.ensure(n_ch * n_total_samples));  // the timeline's running sums
    if (int rc = score_image_upload(ctx, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(prog->d_mix.p, 0, n_ch * n_total_samples * sizeof(float), ctx->stream));
    TiledBatch whole(prog, n_instances, h_params, h_gains, tile);
    for (size_t lo = 0, i = 0; lo < n_instances; lo += tile, i++) {
        if (launches[i].w_hi <= launches[i].w_lo) continue;  // (no voice of the tile reaches the timeline: nothing to render)
        if (int rc = whole.render_tile(lo, std::min(tile, n_instances - lo), n_voice_samples)) return rc;
        if (int rc = score_launch(ctx, launches[i], prog->d_host_out.p, n_ch, n_voice_samples, n_total_samples, h_gains ? prog->d_mix_gains.p : nullptr, prog->d_mix.p,
                                  /*raw=*/1, prog->d_mix.p, ctx->stream))
            return rc;
    }
    ScoreLaunch all;  // `|| 0` over the whole timeline
    all.w_hi = n_total_samples;
    if (int rc = score_launch(ctx, all, nullptr, n_ch, n_voice_samples, n_total_samples, nullptr, prog->d_mix.p, /*raw=*/0, prog->d_mix.p, ctx->stream)) return rc;
    if (int rc = deliver_host(prog, prog->d_mix.p, nullptr, 1, n_ch, n_total_samples, format, normalise, h_peak, h_out)) return rc;
    whole.staged = false;  // (the delivery has waited for the stream)
    if (g_guard_bytes && (!prog->d_mix.intact() || !prog->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, "dusp_render_host_score: the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    return DUSP_OK;
    });
}

// ---- rows: scores over voices that each lie in a buffer of their own (score_rows_engine.hip; dusp_amd/mix.py score_chain_rows) ----

// score_image_add for rows: plans the voices [0, n) — voice k row_samples[k] samples a channel at device address rows[k] — within
// budget_bytes and appends the plan to the context's host image.  listed (optional): which voices reach the timeline.
// h_fracs (optional): the voices' fractions of a sample, checked; where a listed voice has one, its weights (dusp::ScoreFrac, 16 bytes a
// voice on top of the budget) follow the plan and the launch is the two-tap kernel's — else the image and the launch are as without.
static int score_rows_image_add(dusp_ctx *ctx, const char *who, const int64_t *h_onsets, const int64_t *h_lengths, const uint32_t *row_samples, const uint64_t *rows, size_t n,
                                size_t first_voice, uint64_t n_total, bool whole_timeline, size_t budget_bytes, ScoreLaunch &L, std::vector<unsigned char> *listed = nullptr,
                                const double *h_fracs = nullptr) {
    dusp::ScoreRowsPlan P;
    const int64_t bad = dusp::score_rows_plan(h_onsets, h_lengths, row_samples, rows, n, n_total, whole_timeline, budget_bytes, P, h_fracs);
    if (bad >= 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the length of voice " + std::to_string(first_voice + (size_t)bad) + " is " + std::to_string(h_lengths[bad]) +
                                        ": lengths must lie in 0 .. the voice's own row samples (" + std::to_string(row_samples[bad]) + ")");
    L = ScoreLaunch();
    L.w_lo = (uint64_t)P.w_lo;
    L.w_hi = (uint64_t)P.w_hi;
    L.block_shift = P.block_shift;
    L.first_block = P.first_block;
    L.any = P.n_entries() > 0;
    if (L.any) {
        L.n_voices = n;
        L.n_block_first = P.block_first.size();
        L.at = dusp::score_rows_plan_pack(P, ctx->h_score_plan);
        for (size_t k = 0; k < n && !L.frac; k++) L.frac = P.voices[k].hi > P.voices[k].lo && P.voices[k].pad != 0;
        if (L.frac) {
            std::vector<unsigned char> &image = ctx->h_score_plan;
            L.frac_at = (image.size() + 15) & ~(size_t)15;
            image.resize(L.frac_at + n * sizeof(dusp::ScoreFrac));
            for (size_t k = 0; k < n; k++) {
                const dusp::ScoreFrac w = dusp::score_frac_weights(h_fracs[k]);
                std::memcpy(image.data() + L.frac_at + k * sizeof w, &w, sizeof w);
            }
        }
    }
    if (listed) {
        listed->resize(n);
        for (size_t k = 0; k < n; k++) (*listed)[k] = P.voices[k].hi > P.voices[k].lo;
    }
    return DUSP_OK;
}

// a launch some voice of which starts between samples (score_frac_engine.hip): plain rows of n_channels, or (L.pan_at: panned) mono rows
static int score_frac_launch(dusp_ctx *ctx, const ScoreLaunch &L, bool panned, size_t n_channels, size_t n_total, const float *d_gains, const float *d_init, int raw,
                             float *d_out, hipStream_t stream) {
    const dusp::ScoreRow *d_voices = (const dusp::ScoreRow *)(ctx->d_score_plan + L.at);
    const dusp::ScorePan *d_pans = panned ? (const dusp::ScorePan *)(ctx->d_score_plan + L.pan_at) : nullptr;
    const dusp::ScoreFrac *d_fracs = (const dusp::ScoreFrac *)(ctx->d_score_plan + L.frac_at);
    const uint32_t *d_block_first = (const uint32_t *)(d_voices + L.n_voices);
    HIP_TRY(ctx, dusp::launch_score_frac(d_gains, d_pans, d_fracs, d_voices, d_block_first, d_block_first + L.n_block_first, d_init, d_out, (uint32_t)n_channels, n_total,
                                         L.w_lo, L.w_hi, L.block_shift, L.first_block, raw, stream));
    HIP_TRY(ctx, hipEventRecord(ctx->score_done, stream));
    return DUSP_OK;
}

static int score_rows_launch(dusp_ctx *ctx, const ScoreLaunch &L, size_t n_channels, size_t n_total, const float *d_gains, const float *d_init, int raw, float *d_out,
                             hipStream_t stream) {
    if (L.w_hi <= L.w_lo) return DUSP_OK;
    if (L.any && L.frac) return score_frac_launch(ctx, L, false, n_channels, n_total, d_gains, d_init, raw, d_out, stream);
    const dusp::ScoreRow *d_voices = L.any ? (const dusp::ScoreRow *)(ctx->d_score_plan + L.at) : nullptr;  // (the buffer and L.at: both on 32-byte boundaries)
    const uint32_t *d_block_first = L.any ? (const uint32_t *)(d_voices + L.n_voices) : nullptr;
    HIP_TRY(ctx, dusp::launch_score_rows(d_gains, d_voices, d_block_first, L.any ? d_block_first + L.n_block_first : nullptr, d_init, d_out, (uint32_t)n_channels, n_total, L.w_lo,
                                         L.w_hi, L.block_shift, L.first_block, raw, stream));
    if (L.any) HIP_TRY(ctx, hipEventRecord(ctx->score_done, stream));
    return DUSP_OK;
}

// ---- pans: mono rows placed in the stereo field where they are added (score_pan_engine.hip; dusp_amd/mix.py score_chain_rows_panned) ----

static int check_pans(dusp_ctx *ctx, const char *who, const float *h_pans, const double *h_comp, size_t n) {
    for (size_t k = 0; k < n; k++) {
        if (!std::isfinite(h_pans[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the pan of voice " + std::to_string(k) + " is not finite");
        if (h_comp && std::isnan(h_comp[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the compensation of voice " + std::to_string(k) + " is NaN");
    }
    return DUSP_OK;
}

static int check_fracs(dusp_ctx *ctx, const char *who, const double *h_fracs, size_t n) {
    for (size_t k = 0; h_fracs && k < n; k++) {
        if (!std::isfinite(h_fracs[k])) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the fraction of voice " + std::to_string(k) + " is not finite");
        if (h_fracs[k] < 0.0 || h_fracs[k] >= 1.0) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the fraction of voice " + std::to_string(k) + " is outside [0, 1)");
    }
    return DUSP_OK;
}

// the coefficients of the voices [0, n) of the plan just added (L), appended to the context's host image on a 32-byte boundary: they go
// up with the plan.  h_comp NULL: the reference's compensation by the host's pow (Pan.js:20)
static void score_pan_image_add(dusp_ctx *ctx, const float *h_pans, const double *h_comp, size_t n, ScoreLaunch &L) {
    if (!L.any) return;
    std::vector<unsigned char> &image = ctx->h_score_plan;
    L.pan_at = (image.size() + 31) & ~(size_t)31;
    image.resize(L.pan_at + n * sizeof(dusp::ScorePan));
    for (size_t k = 0; k < n; k++) {
        const double comp = h_comp ? h_comp[k] : std::pow(10.0, ((1.0 - std::fabs((double)h_pans[k])) * 1.5) / 20.0);
        const dusp::ScorePan c = dusp::score_pan_coefficients(h_pans[k], comp);
        std::memcpy(image.data() + L.pan_at + k * sizeof c, &c, sizeof c);
    }
}

// score_rows_launch over mono rows into a timeline of two channels
static int score_pan_launch(dusp_ctx *ctx, const ScoreLaunch &L, size_t n_total, const float *d_gains, const float *d_init, int raw, float *d_out, hipStream_t stream) {
    if (L.w_hi <= L.w_lo) return DUSP_OK;
    if (L.any && L.frac) return score_frac_launch(ctx, L, true, 1, n_total, d_gains, d_init, raw, d_out, stream);
    const dusp::ScoreRow *d_voices = L.any ? (const dusp::ScoreRow *)(ctx->d_score_plan + L.at) : nullptr;
    const dusp::ScorePan *d_pans = L.any ? (const dusp::ScorePan *)(ctx->d_score_plan + L.pan_at) : nullptr;
    const uint32_t *d_block_first = L.any ? (const uint32_t *)(d_voices + L.n_voices) : nullptr;
    HIP_TRY(ctx, dusp::launch_score_pan(d_gains, d_pans, d_voices, d_block_first, L.any ? d_block_first + L.n_block_first : nullptr, d_init, d_out, n_total, L.w_lo, L.w_hi,
                                        L.block_shift, L.first_block, raw, stream));
    if (L.any) HIP_TRY(ctx, hipEventRecord(ctx->score_done, stream));
    return DUSP_OK;
}

// dusp_score_rows_device, (h_pans: rows of one channel into a timeline of two) dusp_score_rows_pan_device, and (h_fracs: onsets between
// samples) dusp_score_rows_frac_device
static int score_rows_device(dusp_ctx *ctx, const char *who, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                             const int64_t *h_lengths, const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, const float *d_init, int raw,
                             float *d_out, void *stream_, const double *h_fracs = nullptr) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    const size_t n_out_channels = h_pans ? 2 : n_channels;  // (the timeline's)
    if (!d_out || (n_voices && (!h_rows || !h_row_samples || !h_onsets))) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": NULL buffer");
    if (!channels_in_range(n_channels) || n_voices > (1u << 24) || !samples_in_range(n_total_samples))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..64 channels, 0..2^24 voices and 1..2^31 samples of timeline");
    if (n_out_channels * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": channels x timeline samples must not exceed 2^31: score such a piece channel by channel or in windows of the timeline");
    if ((((uintptr_t)d_gains | (uintptr_t)d_init | (uintptr_t)d_out) & 3) != 0) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buffers must be 4-byte aligned");
    for (size_t k = 0; k < n_voices; k++) {
        if ((uint64_t)h_row_samples[k] * n_channels > dusp::kScoreRowMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + ": channels x row samples must not exceed 2^31");
        if (h_row_samples[k] && !h_rows[k]) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the row of voice " + std::to_string(k) + " is NULL");
        if (h_row_samples[k] && ((uintptr_t)h_rows[k] & 3)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the row of voice " + std::to_string(k) + " must be 4-byte aligned");
    }
    if (h_pans)
        if (int rc = check_pans(ctx, who, h_pans, h_comp, n_voices)) return rc;
    if (int rc = check_fracs(ctx, who, h_fracs, n_voices)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t stream = stream_of(ctx, stream_);
    ScoreLaunch L;
    L.w_hi = n_total_samples;  // (no voices: `|| 0`, or a copy, of d_init alone)
    if (n_voices) {
        if (int rc = score_image_begin(ctx)) return rc;
        const auto t_plan = std::chrono::steady_clock::now();
        static_assert(sizeof(const float *) == sizeof(uint64_t), "rows are handed to the planner as 64-bit addresses");
        if (int rc = score_rows_image_add(ctx, who, h_onsets, h_lengths, h_row_samples, (const uint64_t *)h_rows, n_voices, 0, n_total_samples,
                                          /*whole_timeline=*/true, score_plan_budget(ctx), L, nullptr, h_fracs))
            return rc;
        if (h_pans) score_pan_image_add(ctx, h_pans, h_comp, n_voices, L);
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
    if (h_pans) {
        if (int rc = score_pan_launch(ctx, L, n_total_samples, d_gains, d_init, raw != 0, d_out, stream)) return rc;
    } else if (int rc = score_rows_launch(ctx, L, n_channels, n_total_samples, d_gains, d_init, raw != 0, d_out, stream))
        return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->score_t1, stream));
    ctx->score_timed = true;
    return DUSP_OK;
    });
}

int dusp_score_rows_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                           const int64_t *h_lengths, const float *d_gains, size_t n_total_samples, const float *d_init, int raw, float *d_out, void *stream_) {
    return score_rows_device(ctx, "dusp_score_rows_device", h_rows, h_row_samples, n_voices, n_channels, h_onsets, h_lengths, d_gains, nullptr, nullptr, n_total_samples, d_init,
                             raw, d_out, stream_);
}

int dusp_score_rows_pan_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, const int64_t *h_onsets, const int64_t *h_lengths,
                               const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, const float *d_init, int raw, float *d_out,
                               void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (n_voices && !h_pans) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_pan_device: h_pans is NULL");
    static const float no_pans[1] = {0.0f};  // (no voices: `|| 0`, or a copy, of both channels of d_init)
    return score_rows_device(ctx, "dusp_score_rows_pan_device", h_rows, h_row_samples, n_voices, 1, h_onsets, h_lengths, d_gains, h_pans ? h_pans : no_pans, h_comp,
                             n_total_samples, d_init, raw, d_out, stream_);
}

// dusp_render_host_score_parts, (h_pans: mono parts into a timeline of two channels) dusp_render_host_score_parts_pan, and (h_fracs:
// onsets between samples, with or without pans) dusp_render_host_score_parts_frac
static int render_host_score_parts(const char *who, const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                   const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                   int format, int normalise, void *h_out, float *h_peak, const double *h_fracs = nullptr) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    dusp_program *prog0 = parts[0].prog;  // (its buffers hold what belongs to the piece: the timeline, the gains, the encoded frames)
    dusp_ctx *ctx = prog0->ctx;
    return guarded(ctx->err, who, [&]() -> int {
    const std::string w(who);
    const size_t n_ch = prog0->P.out_bufs.size(), n_out_ch = h_pans ? 2 : n_ch;  // (a voice's, the timeline's)
    if (!h_part_of || !h_onsets) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_part_of or h_onsets is NULL");
    if (n_voices < 1 || n_voices > (1u << 24)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^24 voices");
    size_t n_listed = 0;
    for (size_t p = 0; p < n_parts; p++) {
        if (!parts[p].prog) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the program of part " + std::to_string(p) + " is NULL");
        if (parts[p].prog->ctx != ctx) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " was built on another context: all parts of a piece share one");
        if (h_pans && parts[p].prog->P.out_bufs.size() != 1)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(parts[p].prog->P.out_bufs.size()) +
                                            " output channels: a panned voice is mono");
        if (parts[p].prog->P.out_bufs.size() != n_ch)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(parts[p].prog->P.out_bufs.size()) + " output channels, part 0 has " +
                                            std::to_string(n_ch) + ": all parts of a piece have the same number");
        for (size_t q = 0; q < p; q++)
            if (parts[q].prog == parts[p].prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": parts " + std::to_string(q) + " and " + std::to_string(p) + " are the same program: its tile buffer would be used twice; make them one part or build it twice");
        n_listed += parts[p].n_instances;
    }
    if (!samples_in_range(n_total_samples) || n_out_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the timeline must have 1..2^31 samples and channels x timeline samples must not exceed 2^31: render such a piece in windows of the timeline");
    if (h_pans)
        if (int rc = check_pans(ctx, who, h_pans, h_comp, n_voices)) return rc;
    if (int rc = check_fracs(ctx, who, h_fracs, n_voices)) return rc;
    // voice k of the chain: the next unused instance of part h_part_of[k]
    std::vector<size_t> instance_of(n_voices), used(n_parts, 0);
    for (size_t k = 0; k < n_voices; k++) {
        if (h_part_of[k] >= n_parts) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + " names part " + std::to_string(h_part_of[k]) + " of " + std::to_string(n_parts));
        instance_of[k] = used[h_part_of[k]]++;
    }
    for (size_t p = 0; p < n_parts; p++)
        if (used[p] != parts[p].n_instances || n_listed != n_voices)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_part_of names part " + std::to_string(p) + " " + std::to_string(used[p]) + " times, the part has " +
                                            std::to_string(parts[p].n_instances) + " instances: every instance is one voice of the chain");
    for (size_t p = 0; p < n_parts; p++) {  // (the sizes the tiles are made from; tiled_batch_prepare below refuses the rest, in front of any render)
        if (int rc = check_batch(ctx, who, parts[p].n_instances, parts[p].n_voice_samples)) return rc;
        if (n_ch * parts[p].n_voice_samples > kMixRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": channels x voice samples must not exceed 2^31");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the tiles: runs of the chain's voices whose rows together fit tile_bytes
    std::vector<uint64_t> row_bytes(n_voices);
    std::vector<uint32_t> row_samples(n_voices);
    size_t staged = 0, free_bytes = 0, total_bytes = 0;
    for (size_t k = 0; k < n_voices; k++) {
        row_samples[k] = (uint32_t)parts[h_part_of[k]].n_voice_samples;  // (at most 2^31 / channels: tiled_batch_prepare)
        row_bytes[k] = (uint64_t)n_ch * row_samples[k] * sizeof(float);
    }
    for (size_t p = 0; p < n_parts; p++) staged += parts[p].prog->d_host_out.cap * sizeof(float);
    if (tile_bytes == 0 && ctx->knobs.mix_tile_mb <= 0) HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    const std::vector<size_t> starts = dusp::piece_tile_starts(row_bytes.data(), n_voices, tile_bytes, ctx->knobs.mix_tile_mb, free_bytes, staged, ctx->n_cus);
    const size_t n_tiles = starts.size() - 1;
    // a part's share of tile i: its instances [share[p][i], share[p][i + 1]), one contiguous range since its instances enter the chain in
    // their own order; its tile buffer holds the largest share
    std::vector<std::vector<size_t>> share(n_parts, std::vector<size_t>(n_tiles + 1, 0));
    {
        std::vector<size_t> seen(n_parts, 0);
        for (size_t i = 0; i < n_tiles; i++) {
            for (size_t k = starts[i]; k < starts[i + 1]; k++) seen[h_part_of[k]]++;
            for (size_t p = 0; p < n_parts; p++) share[p][i + 1] = seen[p];
        }
    }
    for (size_t p = 0; p < n_parts; p++) {
        size_t most = 1, unused = 0;
        for (size_t i = 0; i < n_tiles; i++) most = std::max(most, share[p][i + 1] - share[p][i]);
        if (int rc = tiled_batch_prepare(parts[p].prog, who, parts[p].n_instances, parts[p].n_voice_samples, parts[p].h_params, nullptr, most, format, normalise, h_out, &unused)) return rc;
    }
    // every tile's plan, over the tile's union window, made up front under the call's one budget and uploaded once: the rows' addresses
    // are known, since the tile buffers stand
    std::vector<ScoreLaunch> launches(n_tiles);
    std::vector<std::vector<unsigned char>> renders(n_tiles, std::vector<unsigned char>(n_parts, 0));  // does part p render in tile i?
    const size_t tile_budget = score_plan_budget(ctx) / n_tiles;
    if (int rc = score_image_begin(ctx)) return rc;
    const auto t_plan = std::chrono::steady_clock::now();
    {
        std::vector<uint64_t> rows;
        std::vector<unsigned char> listed;
        for (size_t i = 0; i < n_tiles; i++) {
            const size_t lo = starts[i], n = starts[i + 1] - lo;
            rows.resize(n);
            for (size_t k = 0; k < n; k++) {
                const size_t p = h_part_of[lo + k];
                rows[k] = (uint64_t)(uintptr_t)(parts[p].prog->d_host_out.p + (instance_of[lo + k] - share[p][i]) * n_ch * parts[p].n_voice_samples);
            }
            if (int rc = score_rows_image_add(ctx, who, h_onsets + lo, h_lengths ? h_lengths + lo : nullptr, row_samples.data() + lo, rows.data(), n, lo, n_total_samples,
                                              /*whole_timeline=*/false, tile_budget, launches[i], &listed, h_fracs ? h_fracs + lo : nullptr))
                return rc;
            if (h_pans) score_pan_image_add(ctx, h_pans + lo, h_comp ? h_comp + lo : nullptr, n, launches[i]);
            for (size_t k = 0; k < n; k++)
                if (listed[k]) renders[i][h_part_of[lo + k]] = 1;
        }
    }
    if (ctx->knobs.jit_log >= 2)  // (DUSP_JIT_LOG=2: what the plans cost the host)
        fprintf(stderr, "[dusp host piece] %zu plans over %zu voices of %zu parts in %.0f us on the host: %zu bytes\n", n_tiles, n_voices, n_parts,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count(), ctx->h_score_plan.size());
    HIP_TRY(ctx, prog0->d_mix.ensure(n_out_ch * n_total_samples));  // the timeline's running sums
    if (h_gains) {  // (4 bytes a voice, where the plans take 32 and more: the whole piece's at once)
        HIP_TRY(ctx, prog0->d_mix_gains.ensure(n_voices));
        HIP_TRY(ctx, hipMemcpyAsync(prog0->d_mix_gains.p, h_gains, n_voices * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = score_image_upload(ctx, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(prog0->d_mix.p, 0, n_out_ch * n_total_samples * sizeof(float), ctx->stream));
    std::vector<std::unique_ptr<TiledBatch>> whole;  // what changes bits is decided from the WHOLE part
    for (size_t p = 0; p < n_parts; p++) whole.emplace_back(new TiledBatch(parts[p].prog, parts[p].n_instances, parts[p].h_params, share[p]));
    auto waited = [&]() {
        for (auto &b : whole) b->staged = false;
    };
    for (size_t i = 0; i < n_tiles; i++) {
        if (launches[i].w_hi <= launches[i].w_lo) continue;  // (no voice of the tile reaches the timeline: nothing to render)
        for (size_t p = 0; p < n_parts; p++)
            if (renders[i][p])
                if (int rc = whole[p]->render_tile(share[p][i], share[p][i + 1] - share[p][i], parts[p].n_voice_samples)) return rc;
        const float *d_gains = h_gains ? prog0->d_mix_gains.p + starts[i] : nullptr;
        if (h_pans) {
            if (int rc = score_pan_launch(ctx, launches[i], n_total_samples, d_gains, prog0->d_mix.p, /*raw=*/1, prog0->d_mix.p, ctx->stream)) return rc;
        } else if (int rc = score_rows_launch(ctx, launches[i], n_ch, n_total_samples, d_gains, prog0->d_mix.p, /*raw=*/1, prog0->d_mix.p, ctx->stream))
            return rc;
    }
    ScoreLaunch all;  // `|| 0` over the whole timeline
    all.w_hi = n_total_samples;
    if (int rc = score_rows_launch(ctx, all, n_out_ch, n_total_samples, nullptr, prog0->d_mix.p, /*raw=*/0, prog0->d_mix.p, ctx->stream)) return rc;
    if (int rc = deliver_host(prog0, prog0->d_mix.p, nullptr, 1, n_out_ch, n_total_samples, format, normalise, h_peak, h_out)) return rc;
    waited();  // (the delivery has waited for the stream)
    if (g_guard_bytes && (!prog0->d_mix.intact() || !prog0->d_mix_gains.intact() || !score_plan_intact(ctx)))
        CTX_FAIL(ctx, DUSP_ERR_HIP, w + ": the score kernel wrote past the end of a device buffer: guard bytes overwritten");
    return DUSP_OK;
    });
}

int dusp_render_host_score_parts(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                 const int64_t *h_lengths, const float *h_gains, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out,
                                 float *h_peak) {
    return render_host_score_parts("dusp_render_host_score_parts", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, nullptr, nullptr, n_total_samples,
                                   tile_bytes, format, normalise, h_out, h_peak);
}

int dusp_render_host_score_parts_pan(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                     const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                     int format, int normalise, void *h_out, float *h_peak) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    if (!h_pans) CTX_FAIL(parts[0].prog->ctx, DUSP_ERR_ARG, "dusp_render_host_score_parts_pan: h_pans is NULL");
    return render_host_score_parts("dusp_render_host_score_parts_pan", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, h_pans, h_comp, n_total_samples,
                                   tile_bytes, format, normalise, h_out, h_peak);
}

int dusp_score_rows_frac_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels, const int64_t *h_onsets,
                                const double *h_fracs, const int64_t *h_lengths, const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples,
                                const float *d_init, int raw, float *d_out, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (h_pans && n_channels != 1) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_score_rows_frac_device: a panned voice is mono: n_channels must be 1 with h_pans");
    return score_rows_device(ctx, "dusp_score_rows_frac_device", h_rows, h_row_samples, n_voices, n_channels, h_onsets, h_lengths, d_gains, h_pans, h_comp, n_total_samples, d_init,
                             raw, d_out, stream_, h_fracs);
}

int dusp_render_host_score_parts_frac(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const double *h_fracs,
                                      const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                      int format, int normalise, void *h_out, float *h_peak) {
    return render_host_score_parts("dusp_render_host_score_parts_frac", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, h_pans, h_comp, n_total_samples,
                                   tile_bytes, format, normalise, h_out, h_peak, h_fracs);
}

}  // extern "C"
