/* dusp_napi.c — thin N-API addon binding the C ABI of include/dusp_hip.h for Node.js.
 *
 * Raw C against <node_api.h> (N-API v4+, present in Node 12): no node-gyp, no node-addon-api.
 *   deviceCount() -> number of HIP devices this process sees
 *   ctxCreate(device) -> ctx            tableUpload(ctx, id, Float32Array)
 *   programBuild(ctx, Float64Array words, engine) -> prog
 *   programInfo(prog) -> { sampleRate, nUnits, nOutChannels, nParams, nInputs, engine, shape, nDeviceOps }
 *   render(prog, nInstances, nSamples, Float32Array params | null[, interleaved[, Float32Array inputs]]) -> Promise<Float32Array>
 *         (runs dusp_render_host on the libuv pool so the event loop stays live)
 *   stateDownload(prog, instance, unit) -> Float64Array
 *   renderPiece(progs[], ...) -> Promise: a piece of several instruments (dusp_render_host_score_parts; see fn_render_piece)
 *   renderPieceMaster(progs[], ..., master, masterParams) -> Promise: the same through a master (dusp_render_host_score_piece)
 *   renderPieceBuses(progs[], ..., master | null, masterParams, buses[], busParams[], sends) -> Promise: the same with effect sends
 *         (dusp_render_host_score_piece_buses)
 *   renderPieceTracks(the same — buses[] may be null —, nTracks, trackOf, trackProgs[], trackLists[], trackParams[], faders | null, trackSends | null)
 *         -> Promise: the same with tracks, sub-mixes through circuits of their own (dusp_render_host_score_piece_tracks)
 *   renderPieceStems(the same thirty-one — nTracks may be 0 and what follows it null: no tracks)
 *         -> Promise<{ data, peaks }>: the same, delivering the stems beside the mix (dusp_render_host_score_piece_stems)
 *   renderPieceMeters(the same thirty-one, stems, nBlocks)
 *         -> Promise<{ data, peaks, rms, lufs, momentary }>: the same, with stems or without, metering what it delivers
 *            (dusp_render_host_score_piece_meters)
 *   renderPieceLoudness(the same thirty-three, deliver, targetLufs, ceilingDbtp)
 *         -> Promise<{ data, peaks, rms, lufs, momentary, truePeak, gain, level }>: the same, with the true peak of every signal and channel
 *            and — deliver true — the frames encoded at the loudness target (dusp_render_host_score_piece_loudness)
 *   meter(ctx, Float32Array planar, nSignals, nChannels, nSamples, sampleRate) -> { rms, lufs, momentary }: the meters of signals in host
 *         memory (dusp_meter_host)
 *   renderPieceLimiter(the same thirty-six, windowSamples)
 *         -> Promise<{ ..., limiter: { engaged, threshold, window, reduction, lufsIn, truePeakIn } }>: the same with deliver true, the delivered
 *            signals limited to the ceiling in front of the one gain where the largest true peak lies above it
 *            (dusp_render_host_score_piece_limiter); what the call hands back then describes the limited signals
 *   renderPieceLimiterRelease(the same thirty-seven, releaseSamples)
 *         -> the same, the limiter with a release of its own (dusp_render_host_score_piece_limiter_release; 0: renderPieceLimiter); limiter has release
 *   limit(ctx, Float32Array planar, nSignals, nChannels, nSamples, sampleRate, threshold, windowSamples)
 *         -> { data: Float32Array, gain: Float64Array [nSamples], reduction }: signals in host memory limited under ONE look-ahead gain curve
 *            (dusp_limit_host)
 *   truePeak(ctx, Float32Array planar, nSignals, nChannels, nSamples, sampleRate) -> Float64Array [nSignals * nChannels]: the true peaks
 *         of signals in host memory, linear (dusp_true_peak_host)
 *   descriptorChannels(Float64Array words) -> the circuit's output channels (host code only: no context)
 *   programDestroy(prog), ctxDestroy(ctx), version(), abiVersion()
 * Failures surface the way the reference's do: synchronous calls THROW A STRING, render() REJECTS
 * WITH A STRING (reference src/renderChannelData.js:12-17 throws strings inside an async function).
 */
#include <node_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/dusp_hip.h"

#define PINNED_MIN_BYTES ((size_t)1 << 20) /* results of at least 1 MiB live in pinned memory (dusp_host_alloc) */

/* A dusp_ctx is not thread-safe and async renders run on pool threads: calls on ONE context are serialised by that context's
 * lock (ctx_box.lock).  Different contexts are independent (include/dusp_hip.h "Threading"), so renders on different contexts —
 * one per GPU when renderMany shards its instances over the node's devices — run side by side on the pool.  g_create_lock only
 * orders context creation and destruction (device enumeration, the process-wide settings the first context reads). */
static pthread_mutex_t g_create_lock = PTHREAD_MUTEX_INITIALIZER;

#define NAPI_OK(call)                                                          \
    do {                                                                       \
        if ((call) != napi_ok) {                                               \
            throw_string(env, "dusp-hip: N-API call failed: " #call);         \
            return NULL;                                                       \
        }                                                                      \
    } while (0)

static void throw_string(napi_env env, const char *msg) {
    napi_value s;
    if (napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &s) == napi_ok) napi_throw(env, s);
}

/* Lifetimes.  A program and a pinned PCM buffer both point into their context, and an async render points into its
 * program, so the boxes count what still depends on them (all counting happens on the JS thread):
 *   ctx_box.refs        the context external + every program box + every PCM ArrayBuffer backed by the context's pinned pool;
 *                       the box itself is freed when the last of them is finalized
 *   ctx_box.n_programs / n_buffers   live programs / pinned PCM buffers: ctxDestroy throws while either is non-zero
 *   prog_box.in_flight  renders queued or running: programDestroy during one is deferred to its completion */
typedef struct {
    dusp_ctx *ctx;
    pthread_mutex_t lock; /* every library call on this context or on one of its programs */
    int refs, n_programs, n_buffers;
} ctx_box;
typedef struct {
    dusp_program *prog;
    ctx_box *cb;
    int in_flight, destroy_deferred;
} prog_box;

static void ctx_unref(ctx_box *b) {
    if (--b->refs > 0) return;
    if (b->ctx) { /* never destroyed explicitly: the last dependant is gone, release the device side too */
        pthread_mutex_lock(&g_create_lock);
        dusp_ctx_destroy(b->ctx);
        pthread_mutex_unlock(&g_create_lock);
    }
    pthread_mutex_destroy(&b->lock);
    free(b);
}
static void ctx_finalize(napi_env env, void *data, void *hint) {
    (void)env; (void)hint;
    ctx_unref((ctx_box *)data);
}
static void prog_destroy_now(prog_box *b) {
    if (!b->prog) return;
    pthread_mutex_lock(&b->cb->lock);
    dusp_program_destroy(b->prog);
    pthread_mutex_unlock(&b->cb->lock);
    b->prog = NULL;
    b->cb->n_programs--;
}
static void prog_finalize(napi_env env, void *data, void *hint) {
    (void)env; (void)hint;
    prog_box *b = (prog_box *)data; /* (no render can be in flight: a job holds a reference on this external) */
    prog_destroy_now(b);
    ctx_unref(b->cb);
    free(b);
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
        throw_string(env, "dusp-hip: wrong number of arguments");
        return 0;
    }
    return 1;
}
static ctx_box *as_ctx(napi_env env, napi_value v) {
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((ctx_box *)p)->ctx) {
        throw_string(env, "dusp-hip: not a live context");
        return NULL;
    }
    return (ctx_box *)p;
}
static prog_box *as_prog(napi_env env, napi_value v) {
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((prog_box *)p)->prog || ((prog_box *)p)->destroy_deferred) {
        throw_string(env, "dusp-hip: not a live program");
        return NULL;
    }
    return (prog_box *)p;
}
static int typed_array(napi_env env, napi_value v, napi_typedarray_type want, void **data, size_t *len) {
    bool is = false;
    napi_typedarray_type type;
    napi_value ab;
    size_t off;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return 0;
    if (napi_get_typedarray_info(env, v, &type, len, data, &ab, &off) != napi_ok || type != want) return 0;
    return 1;
}

static napi_value fn_version(napi_env env, napi_callback_info info) {
    (void)info;
    napi_value s;
    NAPI_OK(napi_create_string_utf8(env, dusp_version(), NAPI_AUTO_LENGTH, &s));
    return s;
}
static napi_value fn_abi_version(napi_env env, napi_callback_info info) {
    (void)info;
    napi_value v;
    NAPI_OK(napi_create_int32(env, dusp_abi_version(), &v));
    return v;
}

/* deviceCount() -> HIP devices this process sees (dusp_device_count); throws the library's message when there is no usable device */
static napi_value fn_device_count(napi_env env, napi_callback_info info) {
    (void)info;
    pthread_mutex_lock(&g_create_lock);
    int n = dusp_device_count();
    char msg[512];
    if (n < 0) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(NULL));
    pthread_mutex_unlock(&g_create_lock);
    if (n < 0) {
        throw_string(env, msg);
        return NULL;
    }
    napi_value v;
    NAPI_OK(napi_create_int32(env, n, &v));
    return v;
}

static napi_value fn_ctx_create(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    int32_t device = -1;
    napi_get_value_int32(env, argv[0], &device);
    dusp_ctx *ctx = NULL;
    pthread_mutex_lock(&g_create_lock);
    int rc = dusp_ctx_create(device, &ctx);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(NULL));
    pthread_mutex_unlock(&g_create_lock);
    if (rc != DUSP_OK) {
        throw_string(env, msg);
        return NULL;
    }
    ctx_box *b = (ctx_box *)calloc(1, sizeof *b);
    if (!b) {
        dusp_ctx_destroy(ctx);
        throw_string(env, "dusp-hip: out of host memory");
        return NULL;
    }
    b->ctx = ctx;
    b->refs = 1;
    pthread_mutex_init(&b->lock, NULL);
    napi_value ext;
    if (napi_create_external(env, b, ctx_finalize, NULL, &ext) != napi_ok) {
        dusp_ctx_destroy(ctx);
        pthread_mutex_destroy(&b->lock);
        free(b);
        throw_string(env, "dusp-hip: could not wrap the context");
        return NULL;
    }
    return ext;
}

static napi_value fn_ctx_destroy(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    ctx_box *b = as_ctx(env, argv[0]);
    if (!b) return NULL;
    if (b->n_programs > 0 || b->n_buffers > 0) { /* they point into the context (device, pinned pool) */
        char msg[160];
        snprintf(msg, sizeof msg, "dusp-hip: ctxDestroy: %d program(s) and %d rendered PCM buffer(s) of this context are still alive",
                 b->n_programs, b->n_buffers);
        throw_string(env, msg);
        return NULL;
    }
    pthread_mutex_lock(&g_create_lock);
    dusp_ctx_destroy(b->ctx);
    pthread_mutex_unlock(&g_create_lock);
    b->ctx = NULL;
    return NULL;
}

static napi_value fn_table_upload(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    ctx_box *b = as_ctx(env, argv[0]);
    if (!b) return NULL;
    int32_t id = -1;
    napi_get_value_int32(env, argv[1], &id);
    void *data;
    size_t len;
    if (!typed_array(env, argv[2], napi_float32_array, &data, &len)) {
        throw_string(env, "dusp-hip: tableUpload expects a Float32Array");
        return NULL;
    }
    pthread_mutex_lock(&b->lock);
    int rc = dusp_table_upload(b->ctx, id, (const float *)data, len);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(b->ctx));
    pthread_mutex_unlock(&b->lock);
    if (rc != DUSP_OK) throw_string(env, msg);
    return NULL;
}

static napi_value fn_program_build(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    ctx_box *b = as_ctx(env, argv[0]);
    if (!b) return NULL;
    void *data;
    size_t len;
    if (!typed_array(env, argv[1], napi_float64_array, &data, &len)) {
        throw_string(env, "dusp-hip: programBuild expects a Float64Array of descriptor words");
        return NULL;
    }
    int32_t engine = 0;
    napi_get_value_int32(env, argv[2], &engine);
    dusp_program *prog = NULL;
    pthread_mutex_lock(&b->lock);
    int rc = dusp_program_build(b->ctx, (const double *)data, len, engine, &prog);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(b->ctx));
    pthread_mutex_unlock(&b->lock);
    if (rc != DUSP_OK) {
        throw_string(env, msg);
        return NULL;
    }
    prog_box *pb = (prog_box *)calloc(1, sizeof *pb);
    napi_value ext;
    if (!pb || napi_create_external(env, pb, prog_finalize, NULL, &ext) != napi_ok) {
        pthread_mutex_lock(&b->lock);
        dusp_program_destroy(prog);
        pthread_mutex_unlock(&b->lock);
        free(pb);
        throw_string(env, "dusp-hip: could not wrap the program");
        return NULL;
    }
    pb->prog = prog;
    pb->cb = b;
    b->refs++;
    b->n_programs++;
    return ext;
}

/* programContinue(prog, words): dusp_program_continue — re-arm a rendered program from a later extraction of
 * the same circuit (event-segmented rendering). */
static napi_value fn_program_continue(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    prog_box *pb = as_prog(env, argv[0]);
    if (!pb) return NULL;
    void *data;
    size_t len;
    if (!typed_array(env, argv[1], napi_float64_array, &data, &len)) {
        throw_string(env, "dusp-hip: programContinue expects a Float64Array of descriptor words");
        return NULL;
    }
    pthread_mutex_lock(&pb->cb->lock);
    int rc = dusp_program_continue(pb->prog, (const double *)data, len);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(pb->cb->ctx));
    pthread_mutex_unlock(&pb->cb->lock);
    if (rc != DUSP_OK) {
        throw_string(env, msg);
        return NULL;
    }
    napi_value undef;
    NAPI_OK(napi_get_undefined(env, &undef));
    return undef;
}

static napi_value fn_program_destroy(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    prog_box *pb = as_prog(env, argv[0]);
    if (!pb) return NULL;
    if (pb->in_flight > 0) pb->destroy_deferred = 1; /* a render is using it on a pool thread: destroyed when that completes */
    else prog_destroy_now(pb);
    return NULL;
}

static napi_value fn_program_info(napi_env env, napi_callback_info info) {
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    prog_box *pb = as_prog(env, argv[0]);
    if (!pb) return NULL;
    dusp_program_info pi;
    dusp_program_info_get(pb->prog, &pi);
    napi_value obj, v;
    NAPI_OK(napi_create_object(env, &obj));
#define SET_U32(name, val)                                   \
    NAPI_OK(napi_create_uint32(env, (val), &v));             \
    NAPI_OK(napi_set_named_property(env, obj, name, v))
    SET_U32("sampleRate", pi.sample_rate);
    SET_U32("chunkSize", pi.chunk_size);
    SET_U32("nUnits", pi.n_units);
    SET_U32("nOutChannels", pi.n_out_channels);
    SET_U32("nParams", pi.n_params);
    SET_U32("nInputs", pi.n_inputs);
    SET_U32("nDeviceOps", pi.n_device_ops);
#undef SET_U32
    NAPI_OK(napi_create_string_utf8(env, pi.engine == DUSP_ENGINE_FUSED ? "fused" : "chunk", NAPI_AUTO_LENGTH, &v));
    NAPI_OK(napi_set_named_property(env, obj, "engine", v));
    NAPI_OK(napi_create_string_utf8(env, pi.shape, NAPI_AUTO_LENGTH, &v));
    NAPI_OK(napi_set_named_property(env, obj, "shape", v));
    return obj;
}

static napi_value fn_state_download(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    prog_box *pb = as_prog(env, argv[0]);
    if (!pb) return NULL;
    uint32_t instance = 0, unit = 0;
    napi_get_value_uint32(env, argv[1], &instance);
    napi_get_value_uint32(env, argv[2], &unit);
    double words[512];
    pthread_mutex_lock(&pb->cb->lock);
    int n = dusp_state_download(pb->prog, instance, unit, words, 512);
    char msg[512];
    if (n < 0) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(pb->cb->ctx));
    pthread_mutex_unlock(&pb->cb->lock);
    if (n < 0) {
        throw_string(env, msg);
        return NULL;
    }
    if (n > 512) n = 512;
    napi_value ab, arr;
    void *mem;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n * sizeof(double), &mem, &ab));
    memcpy(mem, words, (size_t)n * sizeof(double));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, (size_t)n, ab, 0, &arr));
    return arr;
}

/* ---- async render ---- */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref prog_ref; /* keeps the program external alive while the render is in flight */
    prog_box *pb;
    int out_pinned; /* out comes from dusp_host_alloc (the context's pinned pool) rather than malloc */
    size_t n_instances, n_samples, n_floats;
    float *params;
    float *inputs; /* host-generated streams [nInputs][nInstances][nSamples] (copied: the caller may reuse its array) */
    float *out;
    int interleaved; /* frames [instance][sample][channel] instead of planar [instance][channel][sample] */
    int pcm_format, normalise; /* renderPcm: DUSP_PCM_* (0: a plain render) and DUSP_NORMALISE_* */
    size_t n_bytes;            /* size of out: n_floats f32, or the encoded frames */
    float *peaks;              /* renderPcm: every instance's peak; renderMix: the mix's */
    size_t n_peaks;
    int mix;                   /* renderMix: dusp_render_host_mix — pcm_format 0 delivers the mix as planar f32 */
    float *gains;              /* renderMix: a factor per instance, or NULL */
    size_t tile_instances;     /* renderMix: instances per tile (0: the library's default) */
    int score;                 /* renderScore: dusp_render_host_score — a mix at per-voice onsets (n_samples is a voice's length) */
    size_t n_total;            /* renderScore: samples of the timeline */
    int64_t *onsets, *lengths; /* renderScore: per instance, in samples; lengths may be NULL */
    int rc;
    char err[512];
} render_job;

static void render_execute(napi_env env, void *data) {
    (void)env;
    render_job *j = (render_job *)data;
    pthread_mutex_lock(&j->pb->cb->lock); /* (this context's: renders on other contexts — other GPUs — run beside this one) */
    dusp_program *prog = j->pb->prog; /* (in_flight > 0 keeps it alive: programDestroy defers) */
    if (!prog) {
        j->rc = DUSP_ERR_STATE;
        snprintf(j->err, sizeof j->err, "dusp-hip: render: the program has been destroyed");
    } else {
        if (j->score)
            j->rc = dusp_render_host_score(prog, j->n_instances, j->n_samples, j->n_total, j->params, j->gains, j->onsets, j->lengths, j->tile_instances, j->pcm_format,
                                           j->normalise, j->out, j->peaks);
        else if (j->mix)
            j->rc = dusp_render_host_mix(prog, j->n_instances, j->n_samples, j->params, j->gains, j->tile_instances, j->pcm_format, j->normalise, j->out, j->peaks);
        else if (j->pcm_format)
            j->rc = dusp_render_host_pcm(prog, j->n_instances, j->n_samples, j->params, j->inputs, j->pcm_format, j->normalise, j->out, j->peaks);
        else if (j->inputs) j->rc = dusp_render_host_inputs(prog, j->n_instances, j->n_samples, j->params, j->inputs, j->out, j->interleaved);
        else
            j->rc = j->interleaved ? dusp_render_host_interleaved(prog, j->n_instances, j->n_samples, j->params, j->out)
                                   : dusp_render_host(prog, j->n_instances, j->n_samples, j->params, j->out);
        if (j->rc != DUSP_OK) snprintf(j->err, sizeof j->err, "dusp-hip: %s", dusp_last_error(j->pb->cb->ctx));
    }
    pthread_mutex_unlock(&j->pb->cb->lock);
}
static void job_free(render_job *j) { /* the job and the host copies it owns (not `out`: release_out) */
    free(j->params);
    free(j->inputs);
    free(j->gains);
    free(j->onsets);
    free(j->lengths);
    free(j->peaks);
    free(j);
}
static void free_pcm(napi_env env, void *data, void *hint) {
    (void)env; (void)hint;
    free(data);
}
/* a PCM buffer from the context's pinned pool goes back to it when its ArrayBuffer is collected */
static void free_pinned_pcm(napi_env env, void *data, void *hint) {
    (void)env;
    ctx_box *cb = (ctx_box *)hint;
    if (cb->ctx) {
        pthread_mutex_lock(&cb->lock);
        dusp_host_free(cb->ctx, data);
        pthread_mutex_unlock(&cb->lock);
    }
    cb->n_buffers--;
    ctx_unref(cb);
}
static void release_out(render_job *j) { /* an output buffer that never reached JavaScript */
    if (!j->out) return;
    if (j->out_pinned) {
        ctx_box *cb = j->pb->cb;
        if (cb->ctx) {
            pthread_mutex_lock(&cb->lock);
            dusp_host_free(cb->ctx, j->out);
            pthread_mutex_unlock(&cb->lock);
        }
        cb->n_buffers--;
        ctx_unref(cb);
    } else
        free(j->out);
    j->out = NULL;
}
static void render_complete(napi_env env, napi_status status, void *data) {
    render_job *j = (render_job *)data;
    napi_value result;
    if (status != napi_ok && j->rc == DUSP_OK) {
        j->rc = DUSP_ERR_STATE;
        snprintf(j->err, sizeof j->err, "dusp-hip: render was cancelled");
    }
    if (j->rc == DUSP_OK && j->pcm_format) { /* { data: Buffer over the encoded frames, peaks: Float32Array } */
        napi_value data, peaks_ab, peaks;
        void *peaks_mem;
        if (napi_create_arraybuffer(env, j->n_peaks * sizeof(float), &peaks_mem, &peaks_ab) == napi_ok &&
            napi_create_typedarray(env, napi_float32_array, j->n_peaks, peaks_ab, 0, &peaks) == napi_ok && napi_create_object(env, &result) == napi_ok &&
            napi_create_external_buffer(env, j->n_bytes, j->out, j->out_pinned ? free_pinned_pcm : free_pcm, j->out_pinned ? (void *)j->pb->cb : NULL, &data) == napi_ok) {
            j->out = NULL; /* owned by the Buffer now */
            memcpy(peaks_mem, j->peaks, j->n_peaks * sizeof(float));
            napi_set_named_property(env, result, "data", data);
            napi_set_named_property(env, result, "peaks", peaks);
            napi_resolve_deferred(env, j->deferred, result);
        } else {
            napi_create_string_utf8(env, "dusp-hip: could not wrap the PCM buffer", NAPI_AUTO_LENGTH, &result);
            napi_reject_deferred(env, j->deferred, result);
        }
    } else if (j->rc == DUSP_OK) {
        napi_value ab;
        if (napi_create_external_arraybuffer(env, j->out, j->n_floats * sizeof(float), j->out_pinned ? free_pinned_pcm : free_pcm,
                                             j->out_pinned ? (void *)j->pb->cb : NULL, &ab) == napi_ok &&
            napi_create_typedarray(env, napi_float32_array, j->n_floats, ab, 0, &result) == napi_ok) {
            j->out = NULL; /* owned by the ArrayBuffer now */
            napi_resolve_deferred(env, j->deferred, result);
        } else {
            napi_create_string_utf8(env, "dusp-hip: could not wrap the PCM buffer", NAPI_AUTO_LENGTH, &result);
            napi_reject_deferred(env, j->deferred, result);
        }
    } else {
        napi_create_string_utf8(env, j->err, NAPI_AUTO_LENGTH, &result);
        napi_reject_deferred(env, j->deferred, result); /* a string, like the reference's rejections */
    }
    release_out(j);
    if (--j->pb->in_flight == 0 && j->pb->destroy_deferred) prog_destroy_now(j->pb); /* programDestroy came while this render ran */
    napi_delete_reference(env, j->prog_ref);
    napi_delete_async_work(env, j->work);
    job_free(j);
}

enum { CALL_RENDER = 0, CALL_PCM = 1, CALL_MIX = 2, CALL_SCORE = 3 };

/* onsets / lengths of a score: a BigInt64Array, or a Float64Array of whole numbers, of n values -> a malloc'ed int64 [n].
 * Anything else: NULL, and *why says what (a static string). */
static int64_t *whole_samples(napi_env env, napi_value v, size_t n, const char **why) {
    bool is = false;
    napi_typedarray_type type;
    napi_value ab;
    size_t off, len = 0;
    void *data = NULL;
    *why = "must be a BigInt64Array, or a Float64Array of whole numbers, of nInstances values (in samples)";
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return NULL;
    if (napi_get_typedarray_info(env, v, &type, &len, &data, &ab, &off) != napi_ok || (type != napi_bigint64_array && type != napi_float64_array) || len != n) return NULL;
    int64_t *out = (int64_t *)malloc(n * sizeof(int64_t) + 1);
    if (!out) {
        *why = "out of host memory";
        return NULL;
    }
    if (type == napi_bigint64_array) {
        memcpy(out, data, n * sizeof(int64_t));
        return out;
    }
    for (size_t i = 0; i < n; i++) {
        const double x = ((const double *)data)[i];
        if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0) || x != (double)(int64_t)x) { /* (NaN fails the range) */
            free(out);
            *why = "are in samples, whole numbers: a fraction (or what is no number) is refused";
            return NULL;
        }
        out[i] = (int64_t)x;
    }
    return out;
}

/* render(prog, nInstances, nSamples, params | null [, interleaved [, inputs]]) -> Promise<Float32Array>
 * renderPcm(prog, nInstances, nSamples, params | null, format, normalise [, inputs]) -> Promise<{ data: Buffer, peaks: Float32Array }>
 *   (dusp_render_host_pcm: peak, gain, quantisation and interleave on the device; format DUSP_PCM_*, normalise DUSP_NORMALISE_*)
 * renderMix(prog, nInstances, nSamples, params | null, gains | null, tileInstances, format, normalise)
 *   -> Promise<Float32Array [channel][nSamples]> (format 0) or Promise<{ data: Buffer, peaks: Float32Array(1) }> (format DUSP_PCM_*)
 *   (dusp_render_host_mix: the instances rendered tile by tile and summed on the device in Sum.many's chain order)
 * renderScore(prog, nInstances, nVoiceSamples, params | null, gains | null, tileInstances, format, normalise, nTotalSamples, onsets, lengths | null)
 *   -> as renderMix, over nTotalSamples (dusp_render_host_score: instance k mixed in at sample onsets[k] of the timeline; onsets and
 *   lengths are BigInt64Arrays, or Float64Arrays of whole numbers) */
static napi_value render_call(napi_env env, napi_callback_info info, int kind) {
    napi_value argv[11];
    size_t argc = 11;
    const int call = kind;
    const char *who = kind == CALL_SCORE ? "renderScore" : kind == CALL_MIX ? "renderMix" : kind == CALL_PCM ? "renderPcm" : "render";
    char msg[256];
    if (kind == CALL_SCORE) kind = CALL_MIX; /* a score is a mix with three more arguments (`who` keeps its name for the messages) */
    const int pcm = kind != CALL_RENDER; /* format and normalise are arguments */
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < (call == CALL_SCORE ? 10u : kind == CALL_MIX ? 8u : kind == CALL_PCM ? 6u : 4u)) {
        throw_string(env, "dusp-hip: wrong number of arguments");
        return NULL;
    }
    const size_t inputs_at = kind == CALL_MIX ? 8 : kind == CALL_PCM ? 6 : 5; /* (a mix takes no input streams) */
    const size_t format_at = kind == CALL_MIX ? 6 : 4;
    bool interleaved = false;
    double format = 0, normalise = 0, tile = 0;
    if (kind == CALL_RENDER && argc >= 5) napi_get_value_bool(env, argv[4], &interleaved);
    if (pcm) {
        if (napi_get_value_double(env, argv[format_at], &format) != napi_ok ||
            !(format == DUSP_PCM_S16 || format == DUSP_PCM_S24 || format == DUSP_PCM_F32 || (kind == CALL_MIX && format == 0))) {
            snprintf(msg, sizeof msg, "dusp-hip: %s: format must be %s1 (s16), 2 (s24) or 3 (f32)", who, kind == CALL_MIX ? "0 (planar f32), " : "");
            throw_string(env, msg);
            return NULL;
        }
        if (napi_get_value_double(env, argv[format_at + 1], &normalise) != napi_ok || !(normalise == 0 || normalise == 1 || normalise == 2)) {
            snprintf(msg, sizeof msg, "dusp-hip: %s: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)", who);
            throw_string(env, msg);
            return NULL;
        }
    }
    if (kind == CALL_MIX && (napi_get_value_double(env, argv[5], &tile) != napi_ok || !(tile >= 0 && tile <= 16777216.0 && tile == (double)(size_t)tile))) {
        snprintf(msg, sizeof msg, "dusp-hip: %s: tileInstances must be 0 (the default tile) or a whole number of instances", who);
        throw_string(env, msg);
        return NULL;
    }
    prog_box *pb = as_prog(env, argv[0]);
    if (!pb) return NULL;
    double n_inst = 0, n_samples = 0;
    napi_get_value_double(env, argv[1], &n_inst);
    napi_get_value_double(env, argv[2], &n_samples);
    if (!(n_inst >= 1 && n_inst <= 16777216.0 && n_samples >= 1 && n_samples <= 2147483648.0)) {
        throw_string(env, "dusp-hip: render: nInstances / nSamples out of range");
        return NULL;
    }
    double n_total = 0;
    if (call == CALL_SCORE && (napi_get_value_double(env, argv[8], &n_total) != napi_ok || !(n_total >= 1 && n_total <= 2147483648.0 && n_total == (double)(size_t)n_total))) {
        throw_string(env, "dusp-hip: renderScore: nTotalSamples out of range");
        return NULL;
    }
    dusp_program_info pi;
    dusp_program_info_get(pb->prog, &pi);
    render_job *j = (render_job *)calloc(1, sizeof *j);
    if (!j) {
        throw_string(env, "dusp-hip: render: out of host memory");
        return NULL;
    }
    j->pb = pb;
    j->n_instances = (size_t)n_inst;
    j->n_samples = (size_t)n_samples;
    j->mix = kind == CALL_MIX;
    j->tile_instances = (size_t)tile;
    j->score = call == CALL_SCORE;
    j->n_total = (size_t)n_total;
    /* (a mix is one instance's worth of samples, a score one timeline's) */
    j->n_floats = (j->mix ? 1 : j->n_instances) * pi.n_out_channels * (j->score ? j->n_total : j->n_samples);
    j->interleaved = interleaved ? 1 : 0;
    j->pcm_format = (int)format;
    j->normalise = (int)normalise;
    j->n_bytes = j->n_floats * (size_t)(!j->pcm_format || j->pcm_format == DUSP_PCM_F32 ? 4 : j->pcm_format == DUSP_PCM_S16 ? 2 : 3);
    j->n_peaks = j->mix ? 1 : j->n_instances;
    if (j->pcm_format && !(j->peaks = (float *)malloc(j->n_peaks * sizeof(float)))) {
        job_free(j);
        throw_string(env, "dusp-hip: render: out of host memory");
        return NULL;
    }
    napi_valuetype vt;
    napi_typeof(env, argv[3], &vt);
    if (vt != napi_null && vt != napi_undefined) {
        void *data;
        size_t len;
        if (!typed_array(env, argv[3], napi_float32_array, &data, &len) || len != (size_t)pi.n_params * j->n_instances) {
            job_free(j);
            throw_string(env, "dusp-hip: render: params must be a Float32Array of nParams * nInstances values");
            return NULL;
        }
        j->params = (float *)malloc(len * sizeof(float) + 1);
        if (!j->params) {
            job_free(j);
            throw_string(env, "dusp-hip: render: out of host memory for the parameter table");
            return NULL;
        }
        memcpy(j->params, data, len * sizeof(float));
    } else if (pi.n_params) {
        job_free(j);
        throw_string(env, "dusp-hip: render: this program needs a parameter table");
        return NULL;
    }
    if (kind == CALL_MIX) napi_typeof(env, argv[4], &vt);
    if (kind == CALL_MIX && vt != napi_null && vt != napi_undefined) { /* gains: Float32Array of nInstances values */
        void *data;
        size_t len;
        if (!typed_array(env, argv[4], napi_float32_array, &data, &len) || len != j->n_instances) {
            job_free(j);
            snprintf(msg, sizeof msg, "dusp-hip: %s: gains must be a Float32Array of nInstances values", who);
            throw_string(env, msg);
            return NULL;
        }
        j->gains = (float *)malloc(len * sizeof(float));
        if (!j->gains) {
            job_free(j);
            throw_string(env, "dusp-hip: render: out of host memory for the gains");
            return NULL;
        }
        memcpy(j->gains, data, len * sizeof(float));
    }
    if (j->score) {
        const char *why = NULL;
        if (!(j->onsets = whole_samples(env, argv[9], j->n_instances, &why))) {
            snprintf(msg, sizeof msg, "dusp-hip: renderScore: onsets %s", why);
            job_free(j);
            throw_string(env, msg);
            return NULL;
        }
        vt = napi_undefined;
        if (argc > 10) napi_typeof(env, argv[10], &vt);
        if (vt != napi_null && vt != napi_undefined && !(j->lengths = whole_samples(env, argv[10], j->n_instances, &why))) {
            snprintf(msg, sizeof msg, "dusp-hip: renderScore: lengths %s", why);
            job_free(j);
            throw_string(env, msg);
            return NULL;
        }
    }
    const int has_inputs_arg = !j->score && argc > inputs_at; /* (a score's further arguments are not input streams) */
    if (has_inputs_arg) napi_typeof(env, argv[inputs_at], &vt);
    if (has_inputs_arg && vt != napi_null && vt != napi_undefined) { /* inputs: Float32Array of nInputs * nInstances * nSamples values */
        void *data;
        size_t len;
        if (!typed_array(env, argv[inputs_at], napi_float32_array, &data, &len) || len != (size_t)pi.n_inputs * j->n_instances * j->n_samples || !len) {
            job_free(j);
            throw_string(env, "dusp-hip: render: inputs must be a Float32Array of nInputs * nInstances * nSamples values");
            return NULL;
        }
        j->inputs = (float *)malloc(len * sizeof(float) + 1);
        if (!j->inputs) {
            job_free(j);
            throw_string(env, "dusp-hip: render: out of host memory for the input streams");
            return NULL;
        }
        memcpy(j->inputs, data, len * sizeof(float));
    } else if (pi.n_inputs) {
        job_free(j);
        throw_string(env, "dusp-hip: render: this program reads host-generated input streams");
        return NULL;
    }
    /* The result buffer IS the ArrayBuffer JavaScript gets (renderChannelData.js:39 allocates per call; no copy here).  Large
     * results come from the context's pinned pool so that the download is one DMA at link speed; small ones (event-segmented
     * rendering makes hundreds a second) from malloc. */
    if (j->n_bytes >= PINNED_MIN_BYTES) {
        void *p = NULL;
        pthread_mutex_lock(&pb->cb->lock);
        int rc = dusp_host_alloc(pb->cb->ctx, j->n_bytes, &p);
        pthread_mutex_unlock(&pb->cb->lock);
        if (rc == DUSP_OK) {
            j->out = (float *)p;
            j->out_pinned = 1;
            pb->cb->n_buffers++;
            pb->cb->refs++;
        }
    }
    if (!j->out) j->out = (float *)malloc(j->n_bytes + 1);
    if (!j->out) {
        job_free(j);
        throw_string(env, "dusp-hip: render: out of host memory for the PCM buffer");
        return NULL;
    }
    napi_value promise, name;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok || napi_create_reference(env, argv[0], 1, &j->prog_ref) != napi_ok ||
        napi_create_string_utf8(env, "dusp-hip render", NAPI_AUTO_LENGTH, &name) != napi_ok ||
        napi_create_async_work(env, NULL, name, render_execute, render_complete, j, &j->work) != napi_ok) {
        release_out(j);
        job_free(j);
        throw_string(env, "dusp-hip: render: could not queue the render");
        return NULL;
    }
    pb->in_flight++;
    if (napi_queue_async_work(env, j->work) != napi_ok) {
        pb->in_flight--;
        release_out(j);
        job_free(j);
        throw_string(env, "dusp-hip: render: could not queue the render");
        return NULL;
    }
    return promise;
}
static napi_value fn_render(napi_env env, napi_callback_info info) { return render_call(env, info, CALL_RENDER); }
static napi_value fn_render_pcm(napi_env env, napi_callback_info info) { return render_call(env, info, CALL_PCM); }
static napi_value fn_render_mix(napi_env env, napi_callback_info info) { return render_call(env, info, CALL_MIX); }
static napi_value fn_render_score(napi_env env, napi_callback_info info) { return render_call(env, info, CALL_SCORE); }

/* ---- a piece of several instruments: dusp_render_host_score_parts ---- */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    size_t n_parts, n_voices, n_total, tile_bytes, n_floats, n_bytes;
    napi_ref *refs;   /* keep the program externals alive while the render is in flight */
    prog_box **pbs;
    dusp_score_part *parts;
    float **params;   /* host copies (the caller may reuse its arrays) */
    uint32_t *part_of;
    int64_t *onsets, *lengths;
    float *gains, *out;
    float *pans;      /* renderPiecePan: a pan per voice and its compensation (Math.pow's), else NULL */
    double *comp;
    double *fracs;    /* renderPieceFrac: a fraction of a sample per voice, else NULL */
    double *delays, *tap_gains; /* renderPieceSpace: a delay and a gain per voice and speaker, else NULL */
    size_t n_speakers;
    float peak;
    int stereo;       /* renderPieceStereo: parts of one or two channels, pans with NaN for "not placed", fracs or NULL */
    prog_box *master_pb; /* renderPieceMaster: the program the mix goes through (dusp_render_host_score_piece), else NULL ... */
    napi_ref master_ref;
    float *master_params; /* ... and a host copy of its table [nParams][timeline channels], or NULL */
    size_t n_buses;       /* renderPieceBuses: the bus programs (dusp_render_host_score_piece_buses), each kept as the master is ... */
    prog_box *bus_pb[4];
    napi_ref bus_ref[4];
    float *bus_params[4];
    float *sends;         /* ... and a host copy of the voices' levels [nBuses][nVoices] */
    int with_tracks;      /* renderPieceTracks (dusp_render_host_score_piece_tracks): where every voice goes, the track programs, each kept as the master is ... */
    size_t n_tracks, n_tprogs;
    int32_t *track_of;
    prog_box *tprog_pb[8];
    napi_ref tprog_ref[8];
    float *tprog_params[8];
    uint32_t *tprog_tracks[8]; /* ... with the tracks each serves, */
    size_t tprog_n[8];
    float *faders, *track_sends; /* ... the faders [nTracks] or NULL, and the tracks' levels [nBuses][nTracks] or NULL */
    int with_stems;       /* renderPieceStems (dusp_render_host_score_piece_stems): out holds n_signals signals, the mix last, and every one has a peak */
    size_t n_signals;
    float peaks[16];      /* (1 + 8 tracks + 4 buses + 1 at the most) */
    int with_meters, stems_asked; /* renderPieceMeters (dusp_render_host_score_piece_meters): the result is boxed as with stems, of one signal where stems_asked is 0; */
    size_t n_blocks, n_channels;  /* ... what the caller says the timeline's blocks are (the library checks), the timeline's channels, */
    double *m_rms, *m_lufs, *m_momentary; /* ... and the meters: [n_signals][n_channels], [n_signals], [n_signals][n_blocks] */
    int with_loud, deliver;       /* renderPieceLoudness (dusp_render_host_score_piece_loudness): renderPieceMeters with the true peaks, and with deliver at the target */
    double target, ceiling, *m_tp, l_gain; /* ... the target in LUFS and the ceiling in dBTP, the true peaks [n_signals][n_channels], the gain */
    float l_level;                /* ... and the level it came from */
    int with_limiter, lim_engaged; /* renderPieceLimiter (dusp_render_host_score_piece_limiter): renderPieceLoudness with a limiter in front of the gain: */
    size_t lim_window;            /* ... its window in samples, */
    size_t lim_release;           /* ... renderPieceLimiterRelease (dusp_render_host_score_piece_limiter_release): its release in samples, 0 without one, */
    double lim_threshold, lim_reduction, lim_lufs_in, lim_tp_in; /* ... and what it did */
    int format, normalise, rc;
    char err[512];
} piece_job;

static void piece_free(napi_env env, piece_job *j) {
    for (size_t p = 0; p < j->n_parts; p++) {
        if (j->params) free(j->params[p]);
        if (j->refs && j->refs[p]) napi_delete_reference(env, j->refs[p]);
    }
    if (j->master_ref) napi_delete_reference(env, j->master_ref);
    free(j->master_params);
    for (size_t b = 0; b < 4; b++) {
        if (j->bus_ref[b]) napi_delete_reference(env, j->bus_ref[b]);
        free(j->bus_params[b]);
    }
    free(j->sends);
    for (size_t t = 0; t < 8; t++) {
        if (j->tprog_ref[t]) napi_delete_reference(env, j->tprog_ref[t]);
        free(j->tprog_params[t]);
        free(j->tprog_tracks[t]);
    }
    free(j->track_of);
    free(j->faders);
    free(j->track_sends);
    free(j->params);
    free(j->refs);
    free(j->pbs);
    free(j->parts);
    free(j->part_of);
    free(j->onsets);
    free(j->lengths);
    free(j->gains);
    free(j->pans);
    free(j->comp);
    free(j->fracs);
    free(j->delays);
    free(j->tap_gains);
    free(j->out);
    free(j->m_rms);
    free(j->m_tp);
    free(j->m_lufs);
    free(j->m_momentary);
    free(j);
}
static void piece_execute(napi_env env, void *data) {
    (void)env;
    piece_job *j = (piece_job *)data;
    ctx_box *cb = j->pbs[0]->cb;
    pthread_mutex_lock(&cb->lock);
    j->rc = DUSP_OK;
    for (size_t p = 0; p < j->n_parts; p++) {
        if (!j->pbs[p]->prog) {
            j->rc = DUSP_ERR_STATE;
            snprintf(j->err, sizeof j->err, "dusp-hip: renderPiece: a program has been destroyed");
        }
        j->parts[p].prog = j->pbs[p]->prog;
    }
    if (j->master_pb && !j->master_pb->prog) {
        j->rc = DUSP_ERR_STATE;
        snprintf(j->err, sizeof j->err, "dusp-hip: renderPiece: a program has been destroyed");
    }
    for (size_t b = 0; b < j->n_buses; b++)
        if (!j->bus_pb[b]->prog) {
            j->rc = DUSP_ERR_STATE;
            snprintf(j->err, sizeof j->err, "dusp-hip: renderPiece: a program has been destroyed");
        }
    for (size_t t = 0; t < j->n_tprogs; t++)
        if (!j->tprog_pb[t]->prog) {
            j->rc = DUSP_ERR_STATE;
            snprintf(j->err, sizeof j->err, "dusp-hip: renderPiece: a program has been destroyed");
        }
    if (j->rc == DUSP_OK) {
        if (j->with_tracks || j->with_stems) { /* one entry for every placement, with or without buses and a master */
            dusp_score_placement place = {j->stereo ? DUSP_PLACE_STEREO : j->delays ? DUSP_PLACE_SPACE : j->pans ? DUSP_PLACE_PAN : DUSP_PLACE_ROWS,
                                          j->fracs, j->pans, j->comp, j->n_speakers, j->delays, j->tap_gains};
            dusp_score_master master = {j->master_pb ? j->master_pb->prog : NULL, j->master_params}, circuits[4];
            dusp_score_track_program served[8];
            for (size_t b = 0; b < j->n_buses; b++) {
                circuits[b].prog = j->bus_pb[b]->prog;
                circuits[b].h_params = j->bus_params[b];
            }
            for (size_t t = 0; t < j->n_tprogs; t++) {
                served[t].prog = j->tprog_pb[t]->prog;
                served[t].n_tracks = j->tprog_n[t];
                served[t].h_tracks = j->tprog_tracks[t];
                served[t].h_params = j->tprog_params[t];
            }
            dusp_score_buses buses = {j->n_buses, circuits, j->sends};
            dusp_score_tracks tracks = {j->n_tracks, j->track_of, j->n_tprogs, served, j->faders, j->track_sends};
            dusp_score_stems stems = {j->n_signals};
            dusp_score_meters meters = {j->n_signals, j->n_blocks, j->m_rms, j->m_lufs, j->m_momentary};
            dusp_score_loudness loud = {j->deliver, j->target, j->ceiling, j->m_tp, &j->l_gain, &j->l_level};
            dusp_score_limiter limiter = {j->lim_window, &j->lim_engaged, &j->lim_threshold, &j->lim_reduction, &j->lim_lufs_in, &j->lim_tp_in};
            dusp_score_limiter_release released = {limiter, j->lim_release};
            if (j->with_limiter && j->lim_release)
                j->rc = dusp_render_host_score_piece_limiter_release(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, j->with_tracks ? &tracks : NULL,
                                                                     j->n_buses ? &buses : NULL, j->master_pb ? &master : NULL, j->stems_asked ? &stems : NULL, &meters, &loud, &released,
                                                                     j->n_total, j->tile_bytes, j->format, j->normalise, j->out, j->peaks);
            else if (j->with_limiter)
                j->rc = dusp_render_host_score_piece_limiter(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, j->with_tracks ? &tracks : NULL,
                                                             j->n_buses ? &buses : NULL, j->master_pb ? &master : NULL, j->stems_asked ? &stems : NULL, &meters, &loud, &limiter,
                                                             j->n_total, j->tile_bytes, j->format, j->normalise, j->out, j->peaks);
            else if (j->with_loud)
                j->rc = dusp_render_host_score_piece_loudness(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, j->with_tracks ? &tracks : NULL,
                                                              j->n_buses ? &buses : NULL, j->master_pb ? &master : NULL, j->stems_asked ? &stems : NULL, &meters, &loud, j->n_total,
                                                              j->tile_bytes, j->format, j->normalise, j->out, j->peaks);
            else if (j->with_meters)
                j->rc = dusp_render_host_score_piece_meters(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, j->with_tracks ? &tracks : NULL,
                                                            j->n_buses ? &buses : NULL, j->master_pb ? &master : NULL, j->stems_asked ? &stems : NULL, &meters, j->n_total, j->tile_bytes,
                                                            j->format, j->normalise, j->out, j->peaks);
            else if (j->with_stems)
                j->rc = dusp_render_host_score_piece_stems(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, j->with_tracks ? &tracks : NULL,
                                                           j->n_buses ? &buses : NULL, j->master_pb ? &master : NULL, &stems, j->n_total, j->tile_bytes, j->format, j->normalise,
                                                           j->out, j->peaks);
            else
                j->rc = dusp_render_host_score_piece_tracks(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, &tracks, j->n_buses ? &buses : NULL,
                                                            j->master_pb ? &master : NULL, j->n_total, j->tile_bytes, j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        } else if (j->n_buses) { /* one entry for every placement, which refuses what sends do not go with */
            dusp_score_placement place = {j->stereo ? DUSP_PLACE_STEREO : j->delays ? DUSP_PLACE_SPACE : j->pans ? DUSP_PLACE_PAN : DUSP_PLACE_ROWS,
                                          j->fracs, j->pans, j->comp, j->n_speakers, j->delays, j->tap_gains};
            dusp_score_master master = {j->master_pb ? j->master_pb->prog : NULL, j->master_params}, circuits[4];
            for (size_t b = 0; b < j->n_buses; b++) {
                circuits[b].prog = j->bus_pb[b]->prog;
                circuits[b].h_params = j->bus_params[b];
            }
            dusp_score_buses buses = {j->n_buses, circuits, j->sends};
            j->rc = dusp_render_host_score_piece_buses(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, &buses, j->master_pb ? &master : NULL,
                                                       j->n_total, j->tile_bytes, j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        } else if (j->master_pb) { /* one entry for every placement */
            dusp_score_placement place = {j->stereo ? DUSP_PLACE_STEREO : j->delays ? DUSP_PLACE_SPACE : j->pans ? DUSP_PLACE_PAN : DUSP_PLACE_ROWS,
                                          j->fracs, j->pans, j->comp, j->n_speakers, j->delays, j->tap_gains};
            dusp_score_master master = {j->master_pb->prog, j->master_params};
            j->rc = dusp_render_host_score_piece(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, &place, &master, j->n_total, j->tile_bytes,
                                                 j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        } else if (j->stereo)
            j->rc = dusp_render_host_score_parts_stereo(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->fracs, j->lengths, j->gains, j->pans, j->comp, j->n_total,
                                                        j->tile_bytes, j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        else if (j->delays)
            j->rc = dusp_render_host_score_parts_space(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, j->n_speakers, j->delays, j->tap_gains,
                                                       j->n_total, j->tile_bytes, j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        else if (j->fracs)
            j->rc = dusp_render_host_score_parts_frac(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->fracs, j->lengths, j->gains, j->pans, j->comp, j->n_total,
                                                      j->tile_bytes, j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        else if (j->pans)
            j->rc = dusp_render_host_score_parts_pan(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, j->pans, j->comp, j->n_total, j->tile_bytes,
                                                     j->format, j->normalise, j->out, j->format ? &j->peak : NULL);
        else
            j->rc = dusp_render_host_score_parts(j->parts, j->n_parts, j->n_voices, j->part_of, j->onsets, j->lengths, j->gains, j->n_total, j->tile_bytes, j->format,
                                                 j->normalise, j->out, j->format ? &j->peak : NULL);
        if (j->rc != DUSP_OK) snprintf(j->err, sizeof j->err, "dusp-hip: %s", dusp_last_error(cb->ctx));
    }
    pthread_mutex_unlock(&cb->lock);
}
static void piece_complete(napi_env env, napi_status status, void *data) {
    piece_job *j = (piece_job *)data;
    napi_value result;
    if (status != napi_ok && j->rc == DUSP_OK) {
        j->rc = DUSP_ERR_STATE;
        snprintf(j->err, sizeof j->err, "dusp-hip: render was cancelled");
    }
    int ok = 0;
    if (j->rc == DUSP_OK && j->with_stems) { /* { data: Buffer over the encoded frames or Float32Array of planar f32, all signals; peaks: Float32Array(nSignals) } */
        napi_value data, ab, peaks_ab, peaks;
        void *peaks_mem;
        int wrapped = j->format ? napi_create_external_buffer(env, j->n_bytes, j->out, free_pcm, NULL, &data) == napi_ok
                                : napi_create_external_arraybuffer(env, j->out, j->n_floats * sizeof(float), free_pcm, NULL, &ab) == napi_ok &&
                                      napi_create_typedarray(env, napi_float32_array, j->n_floats, ab, 0, &data) == napi_ok;
        if (wrapped) j->out = NULL; /* owned by the Buffer or ArrayBuffer now */
        if (wrapped && napi_create_arraybuffer(env, j->n_signals * sizeof(float), &peaks_mem, &peaks_ab) == napi_ok &&
            napi_create_typedarray(env, napi_float32_array, j->n_signals, peaks_ab, 0, &peaks) == napi_ok && napi_create_object(env, &result) == napi_ok) {
            memcpy(peaks_mem, j->peaks, j->n_signals * sizeof(float));
            napi_set_named_property(env, result, "data", data);
            napi_set_named_property(env, result, "peaks", peaks);
            ok = 1;
            if (j->with_meters) { /* ... and rms, lufs, momentary: Float64Arrays */
                const char *names[3] = {"rms", "lufs", "momentary"};
                const double *from[3] = {j->m_rms, j->m_lufs, j->m_momentary};
                const size_t counts[3] = {j->n_signals * j->n_channels, j->n_signals, j->n_signals * j->n_blocks};
                for (int m = 0; m < 3 && ok; m++) {
                    napi_value mab, arr;
                    void *mem;
                    ok = napi_create_arraybuffer(env, counts[m] * sizeof(double), &mem, &mab) == napi_ok &&
                         napi_create_typedarray(env, napi_float64_array, counts[m], mab, 0, &arr) == napi_ok && napi_set_named_property(env, result, names[m], arr) == napi_ok;
                    if (ok && counts[m]) memcpy(mem, from[m], counts[m] * sizeof(double));
                }
            }
            if (j->with_loud && ok) { /* ... and truePeak: Float64Array; gain, level: numbers */
                napi_value mab, arr, gain, level;
                void *mem;
                const size_t count = j->n_signals * j->n_channels;
                ok = napi_create_arraybuffer(env, count * sizeof(double), &mem, &mab) == napi_ok && napi_create_typedarray(env, napi_float64_array, count, mab, 0, &arr) == napi_ok &&
                     napi_set_named_property(env, result, "truePeak", arr) == napi_ok && napi_create_double(env, j->l_gain, &gain) == napi_ok &&
                     napi_create_double(env, (double)j->l_level, &level) == napi_ok && napi_set_named_property(env, result, "gain", gain) == napi_ok &&
                     napi_set_named_property(env, result, "level", level) == napi_ok;
                if (ok && count) memcpy(mem, j->m_tp, count * sizeof(double));
            }
            if (j->with_limiter && ok) { /* ... and limiter: what the limiter did */
                napi_value box, v;
                const char *names[6] = {"threshold", "window", "reduction", "lufsIn", "truePeakIn", "release"};
                const double values[6] = {j->lim_threshold, (double)j->lim_window, j->lim_reduction, j->lim_lufs_in, j->lim_tp_in, (double)j->lim_release};
                ok = napi_create_object(env, &box) == napi_ok && napi_get_boolean(env, j->lim_engaged != 0, &v) == napi_ok && napi_set_named_property(env, box, "engaged", v) == napi_ok;
                for (int m = 0; m < 6 && ok; m++) ok = napi_create_double(env, values[m], &v) == napi_ok && napi_set_named_property(env, box, names[m], v) == napi_ok;
                ok = ok && napi_set_named_property(env, result, "limiter", box) == napi_ok;
            }
        }
    } else if (j->rc == DUSP_OK && j->format) { /* { data: Buffer over the encoded frames, peaks: Float32Array(1) } */
        napi_value buf, peaks_ab, peaks;
        void *peaks_mem;
        if (napi_create_arraybuffer(env, sizeof(float), &peaks_mem, &peaks_ab) == napi_ok && napi_create_typedarray(env, napi_float32_array, 1, peaks_ab, 0, &peaks) == napi_ok &&
            napi_create_object(env, &result) == napi_ok && napi_create_external_buffer(env, j->n_bytes, j->out, free_pcm, NULL, &buf) == napi_ok) {
            j->out = NULL; /* owned by the Buffer now */
            memcpy(peaks_mem, &j->peak, sizeof(float));
            napi_set_named_property(env, result, "data", buf);
            napi_set_named_property(env, result, "peaks", peaks);
            ok = 1;
        }
    } else if (j->rc == DUSP_OK) {
        napi_value ab;
        if (napi_create_external_arraybuffer(env, j->out, j->n_floats * sizeof(float), free_pcm, NULL, &ab) == napi_ok &&
            napi_create_typedarray(env, napi_float32_array, j->n_floats, ab, 0, &result) == napi_ok) {
            j->out = NULL; /* owned by the ArrayBuffer now */
            ok = 1;
        }
    }
    if (ok) napi_resolve_deferred(env, j->deferred, result);
    else {
        napi_create_string_utf8(env, j->rc == DUSP_OK ? "dusp-hip: could not wrap the PCM buffer" : j->err, NAPI_AUTO_LENGTH, &result);
        napi_reject_deferred(env, j->deferred, result); /* a string, like the reference's rejections */
    }
    for (size_t p = 0; p < j->n_parts; p++)
        if (--j->pbs[p]->in_flight == 0 && j->pbs[p]->destroy_deferred) prog_destroy_now(j->pbs[p]);
    if (j->master_pb && --j->master_pb->in_flight == 0 && j->master_pb->destroy_deferred) prog_destroy_now(j->master_pb);
    for (size_t b = 0; b < j->n_buses; b++)
        if (--j->bus_pb[b]->in_flight == 0 && j->bus_pb[b]->destroy_deferred) prog_destroy_now(j->bus_pb[b]);
    for (size_t t = 0; t < j->n_tprogs; t++)
        if (--j->tprog_pb[t]->in_flight == 0 && j->tprog_pb[t]->destroy_deferred) prog_destroy_now(j->tprog_pb[t]);
    napi_delete_async_work(env, j->work);
    piece_free(env, j);
}

/* renderPiece(progs[], nInstances Float64Array, nVoiceSamples Float64Array, params[] (Float32Array | null each), partOf Uint32Array, onsets, lengths | null,
 *             gains | null, nTotalSamples, tileBytes, format, normalise)
 *   -> as renderScore (dusp_render_host_score_parts: voice k of the chain is the next unused instance of part partOf[k])
 * renderPiecePan(the same twelve, pans Float32Array, comp Float64Array)
 *   -> the same over MONO parts, two channels out (dusp_render_host_score_parts_pan: voice k panned to pans[k] where it is added; comp[k] is
 *      the reference's compensation, computed by the caller with Math.pow)
 * renderPieceFrac(the same twelve, fracs Float64Array, pans Float32Array | null, comp Float64Array | null)
 *   -> either of the two with voice k starting at onsets[k] + fracs[k] samples, 0 <= fracs[k] < 1 (dusp_render_host_score_parts_frac)
 * renderPieceSpace(the same twelve, nSpeakers, delays Float64Array, tapGains Float64Array)
 *   -> the first over MONO parts, nSpeakers channels out (dusp_render_host_score_parts_space: voice k heard by speaker c through the gain
 *      tapGains[k * nSpeakers + c] and a delay of delays[k * nSpeakers + c] samples; the gains computed by the caller with Math.pow)
 * renderPieceStereo(the same twelve, fracs Float64Array | null, pans Float32Array, comp Float64Array)
 *   -> the first over parts of ONE OR TWO output channels, two channels out (dusp_render_host_score_parts_stereo: a mono voice panned to
 *      pans[k], or heard alike on both channels where pans[k] is NaN; a voice of two channels, whose pan is NaN, keeps its channels)
 * renderPieceMaster(the same twelve, kind, fracs | null, pans | null, comp | null, nSpeakers, delays | null, tapGains | null, master, masterParams | null)
 *   -> any of the five — kind 0 plain rows, 1 panned, 2 in a space, 3 stereo, each with the arrays of its kind as above — with the mix
 *      put through the program `master` before it is delivered (dusp_render_host_score_piece: a program with one input stream and one
 *      output channel, channel c of the timeline instance c of it; masterParams its table, nParams * timeline channels values)
 * renderPieceBuses(the same twenty-one — master and masterParams may be null —, buses[] (programs), busParams[] (Float32Array | null each), sends Float32Array)
 *   -> the same with effect sends (dusp_render_host_score_piece_buses): 1 .. 4 bus programs, each what a master is, with its table, and
 *      sends[b * nVoices + k] what voice k gives to bus b; the library refuses the kinds and arrays sends do not go with
 * renderPieceTracks(the same twenty-four — buses[] and busParams[] may be null (no buses), sends is null —, nTracks, trackOf Int32Array, trackProgs[] (programs),
 *                   trackLists[] (Uint32Array each), trackParams[] (Float32Array | null each), faders Float32Array | null, trackSends Float32Array | null)
 *   -> the same with tracks (dusp_render_host_score_piece_tracks): voice k goes to track trackOf[k], or with -1 straight to the mix; track program t
 *      serves the tracks trackLists[t], its table one column a (track, channel); faders[g] scales track g, trackSends[b * nTracks + g] is what
 *      track g gives to bus b; the library refuses the rest
 * renderPieceStems(the same thirty-one — nTracks may be 0 with trackOf, trackProgs, trackLists, trackParams, faders and trackSends null (no tracks); with buses and no tracks
 *                  sends holds the voices' levels —)
 *   -> the same, delivering the stems beside the mix (dusp_render_host_score_piece_stems): resolves to { data, peaks } whatever the format, data the
 *      1 + nTracks + nBuses + 1 signals one behind the other (a Float32Array of planar f32, or a Buffer of frames under ONE gain), the mix last, peaks a
 *      Float32Array of every signal's own peak */
static napi_value render_piece_call(napi_env env, napi_callback_info info, int form) { /* form: 0 plain, 1 panned, 2 with fractions, 3 in a space, 4 stereo, 5 any of them, with a master, 6 ... and buses */
    napi_value argv[38];
    char msg[256];
    const int with_release = form == 12; /* (renderPieceLimiterRelease: renderPieceLimiter's arguments, then the release in samples) */
    const int with_limiter = form == 11 || with_release; /* (renderPieceLimiter: renderPieceLoudness' arguments, then the window in samples) */
    const int with_loud = form == 10 || with_limiter; /* (renderPieceLoudness: renderPieceMeters' arguments, then deliver, the target and the ceiling) */
    const int with_meters = form == 9 || with_loud; /* (renderPieceMeters: renderPieceStems' arguments, then whether the stems are asked for and the blocks of the timeline) */
    const int with_stems = form == 8 || with_meters; /* (renderPieceStems: renderPieceTracks' arguments, the tracks among them or not) */
    int with_tracks = form == 7;
    if (with_tracks || with_stems) form = 6;
    if (!get_args(env, info, with_release ? 38 : with_limiter ? 37 : with_loud ? 36 : with_meters ? 33 : with_tracks || with_stems ? 31 : form == 6 ? 24 : form == 5 ? 21 : form >= 2 ? 15 : form == 1 ? 14 : 12, argv)) return NULL;
    if (with_stems) { /* (nTracks 0: a call without tracks) */
        double n_tracks = 0;
        with_tracks = napi_get_value_double(env, argv[24], &n_tracks) != napi_ok || n_tracks != 0;
    }
    int with_buses = form == 6;
    int with_master = form == 5 || form == 6; /* (the placement as a record; with buses the master itself may be null) */
    int fracs_at = 12, space_at = 12, pans_at = form == 2 || form == 4 ? 13 : 12;
    if (with_master) { /* the placement's kind says which of the four other forms this is */
        double kind = -1;
        if (napi_get_value_double(env, argv[12], &kind) != napi_ok || !(kind == 0 || kind == 1 || kind == 2 || kind == 3)) {
            throw_string(env, "dusp-hip: renderPiece: kind must be 0 (rows), 1 (pan), 2 (space) or 3 (stereo)");
            return NULL;
        }
        form = kind == 1 ? 1 : kind == 2 ? 3 : kind == 3 ? 4 : 2; /* (plain rows: the form with fractions, whose pans may be null) */
        fracs_at = 13, pans_at = 14, space_at = 16;
    }
    int panned = form == 1 || form == 4;
    int with_fracs = form == 2;
    if (form == 4 || (with_master && form == 1)) {
        napi_valuetype ft = napi_undefined;
        napi_typeof(env, argv[fracs_at], &ft);
        with_fracs = ft != napi_null && ft != napi_undefined;
    }
    if (form == 2) {
        napi_valuetype pt = napi_undefined, ft = napi_undefined;
        napi_typeof(env, argv[pans_at], &pt);
        panned = pt != napi_null && pt != napi_undefined;
        napi_typeof(env, argv[fracs_at], &ft);
        if (with_master) with_fracs = ft != napi_null && ft != napi_undefined;
    }
    uint32_t n_parts = 0;
    bool is_array = false;
    if (napi_is_array(env, argv[0], &is_array) != napi_ok || !is_array || napi_get_array_length(env, argv[0], &n_parts) != napi_ok || n_parts < 1) {
        throw_string(env, "dusp-hip: renderPiece: parts must be an array of at least one program");
        return NULL;
    }
    void *inst = NULL, *vs = NULL, *po = NULL;
    size_t n_inst = 0, n_vs = 0, n_voices = 0;
    if (!typed_array(env, argv[1], napi_float64_array, &inst, &n_inst) || !typed_array(env, argv[2], napi_float64_array, &vs, &n_vs) || n_inst != n_parts || n_vs != n_parts) {
        throw_string(env, "dusp-hip: renderPiece: nInstances and nVoiceSamples must be Float64Arrays of one value per part");
        return NULL;
    }
    if (!typed_array(env, argv[4], napi_uint32_array, &po, &n_voices) || n_voices < 1 || n_voices > 16777216u) {
        throw_string(env, "dusp-hip: renderPiece: partOf must be a Uint32Array of 1 .. 2^24 voices");
        return NULL;
    }
    double n_total = 0, tile = 0, format = 0, normalise = 0;
    if (napi_get_value_double(env, argv[8], &n_total) != napi_ok || !(n_total >= 1 && n_total <= 2147483648.0 && n_total == (double)(size_t)n_total)) {
        throw_string(env, "dusp-hip: renderPiece: nTotalSamples out of range");
        return NULL;
    }
    if (napi_get_value_double(env, argv[9], &tile) != napi_ok || !(tile >= 0 && tile <= 1e15 && tile == (double)(size_t)tile)) {
        throw_string(env, "dusp-hip: renderPiece: tileBytes must be 0 (the default tile) or a whole number of bytes");
        return NULL;
    }
    if (napi_get_value_double(env, argv[10], &format) != napi_ok || !(format == 0 || format == DUSP_PCM_S16 || format == DUSP_PCM_S24 || format == DUSP_PCM_F32)) {
        throw_string(env, "dusp-hip: renderPiece: format must be 0 (planar f32), 1 (s16), 2 (s24) or 3 (f32)");
        return NULL;
    }
    if (napi_get_value_double(env, argv[11], &normalise) != napi_ok || !(normalise == 0 || normalise == 1 || normalise == 2)) {
        throw_string(env, "dusp-hip: renderPiece: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)");
        return NULL;
    }
    piece_job *j = (piece_job *)calloc(1, sizeof *j);
    if (j) {
        j->n_parts = n_parts;
        j->refs = (napi_ref *)calloc(n_parts, sizeof *j->refs);
        j->pbs = (prog_box **)calloc(n_parts, sizeof *j->pbs);
        j->parts = (dusp_score_part *)calloc(n_parts, sizeof *j->parts);
        j->params = (float **)calloc(n_parts, sizeof *j->params);
        j->part_of = (uint32_t *)malloc(n_voices * sizeof(uint32_t));
    }
    if (!j || !j->refs || !j->pbs || !j->parts || !j->params || !j->part_of) {
        if (j) piece_free(env, j);
        throw_string(env, "dusp-hip: renderPiece: out of host memory");
        return NULL;
    }
    memcpy(j->part_of, po, n_voices * sizeof(uint32_t));
    j->n_voices = n_voices;
    j->n_total = (size_t)n_total;
    j->tile_bytes = (size_t)tile;
    j->format = (int)format;
    j->normalise = (int)normalise;
    uint32_t n_channels = 0;
    const char *bad = NULL;
    for (uint32_t p = 0; p < n_parts && !bad; p++) {
        napi_value prog_v, par_v;
        napi_valuetype vt = napi_undefined;
        if (napi_get_element(env, argv[0], p, &prog_v) != napi_ok || !(j->pbs[p] = as_prog(env, prog_v))) { /* (as_prog has thrown) */
            piece_free(env, j);
            return NULL;
        }
        dusp_program_info pi;
        dusp_program_info_get(j->pbs[p]->prog, &pi);
        const double ni = ((const double *)inst)[p], nv = ((const double *)vs)[p];
        if (j->pbs[p]->cb != j->pbs[0]->cb) bad = "all parts of a piece are built on one context";
        else if (!(ni >= 1 && ni <= 16777216.0 && ni == (double)(size_t)ni && nv >= 1 && nv <= 2147483648.0 && nv == (double)(size_t)nv)) bad = "nInstances / nVoiceSamples out of range";
        else if (form == 4 && pi.n_out_channels != 1 && pi.n_out_channels != 2) bad = "a voice of a stereo piece has one or two channels";
        else if (form != 4 && p && pi.n_out_channels != n_channels) bad = "all parts of a piece have one number of output channels";
        else if (form != 4 && panned && pi.n_out_channels != 1) bad = "a panned voice is mono: every part has one output channel";
        else if (form == 3 && pi.n_out_channels != 1) bad = "a placed voice is mono: every part has one output channel";
        if (bad) break;
        n_channels = pi.n_out_channels;
        j->parts[p].n_instances = (size_t)ni;
        j->parts[p].n_voice_samples = (size_t)nv;
        is_array = false;
        if (napi_is_array(env, argv[3], &is_array) == napi_ok && is_array && napi_get_element(env, argv[3], p, &par_v) == napi_ok) napi_typeof(env, par_v, &vt);
        if (vt != napi_null && vt != napi_undefined) {
            void *data;
            size_t len;
            if (!typed_array(env, par_v, napi_float32_array, &data, &len) || len != (size_t)pi.n_params * (size_t)ni) bad = "params must be a Float32Array of nParams * nInstances values for every part";
            else if (!(j->params[p] = (float *)malloc(len * sizeof(float) + 1))) bad = "out of host memory for a parameter table";
            else memcpy(j->params[p], data, len * sizeof(float));
        } else if (pi.n_params) bad = "a part's program needs a parameter table";
        j->parts[p].h_params = j->params[p];
    }
    const char *why = NULL;
    if (!bad && !(j->onsets = whole_samples(env, argv[5], n_voices, &why))) {
        snprintf(msg, sizeof msg, "onsets %s", why);
        bad = msg;
    }
    napi_valuetype vt = napi_undefined;
    napi_typeof(env, argv[6], &vt);
    if (!bad && vt != napi_null && vt != napi_undefined && !(j->lengths = whole_samples(env, argv[6], n_voices, &why))) {
        snprintf(msg, sizeof msg, "lengths %s", why);
        bad = msg;
    }
    napi_typeof(env, argv[7], &vt);
    if (!bad && vt != napi_null && vt != napi_undefined) {
        void *data;
        size_t len;
        if (!typed_array(env, argv[7], napi_float32_array, &data, &len) || len != n_voices) bad = "gains must be a Float32Array of one value per voice";
        else if (!(j->gains = (float *)malloc(len * sizeof(float)))) bad = "out of host memory for the gains";
        else memcpy(j->gains, data, len * sizeof(float));
    }
    if (!bad && panned) {
        void *pd, *cd;
        size_t n_p = 0, n_c = 0;
        if (!typed_array(env, argv[pans_at], napi_float32_array, &pd, &n_p) || n_p != n_voices) bad = "pans must be a Float32Array of one value per voice";
        else if (!typed_array(env, argv[pans_at + 1], napi_float64_array, &cd, &n_c) || n_c != n_voices) bad = "comp must be a Float64Array of one value per voice";
        else if (!(j->pans = (float *)malloc(n_p * sizeof(float))) || !(j->comp = (double *)malloc(n_c * sizeof(double)))) bad = "out of host memory for the pans";
        else {
            memcpy(j->pans, pd, n_p * sizeof(float));
            memcpy(j->comp, cd, n_c * sizeof(double));
        }
        n_channels = 2; /* the timeline's */
    }
    j->stereo = form == 4;
    if (!bad && with_fracs) {
        void *fd;
        size_t n_f = 0;
        if (!typed_array(env, argv[fracs_at], napi_float64_array, &fd, &n_f) || n_f != n_voices) bad = "fracs must be a Float64Array of one value per voice";
        else if (!(j->fracs = (double *)malloc(n_f * sizeof(double)))) bad = "out of host memory for the fractions";
        else memcpy(j->fracs, fd, n_f * sizeof(double));
    }
    if (!bad && form == 3) {
        void *dd, *gd;
        size_t n_d = 0, n_g = 0;
        double speakers = 0;
        if (napi_get_value_double(env, argv[space_at], &speakers) != napi_ok || !(speakers >= 1 && speakers <= 8 && speakers == (double)(size_t)speakers)) bad = "a Space has 1 .. 8 speakers";
        else if (!typed_array(env, argv[space_at + 1], napi_float64_array, &dd, &n_d) || n_d != n_voices * (size_t)speakers) bad = "delays must be a Float64Array of one value per voice and speaker";
        else if (!typed_array(env, argv[space_at + 2], napi_float64_array, &gd, &n_g) || n_g != n_d) bad = "tapGains must be a Float64Array of one value per voice and speaker";
        else if (!(j->delays = (double *)malloc(n_d * sizeof(double))) || !(j->tap_gains = (double *)malloc(n_g * sizeof(double)))) bad = "out of host memory for the taps";
        else {
            memcpy(j->delays, dd, n_d * sizeof(double));
            memcpy(j->tap_gains, gd, n_g * sizeof(double));
            j->n_speakers = (size_t)speakers;
            n_channels = (uint32_t)speakers; /* the timeline's */
        }
    }
    if (with_buses) { /* (a call with buses may have no master) */
        napi_valuetype mv = napi_undefined;
        napi_typeof(env, argv[19], &mv);
        if (mv == napi_null || mv == napi_undefined) with_master = 0;
        napi_typeof(env, argv[21], &mv);
        if ((with_tracks || with_stems) && (mv == napi_null || mv == napi_undefined)) with_buses = 0; /* (a call with tracks or stems may have no buses) */
    }
    if (!bad && with_buses) { /* the buses: programs of the parts' context, each with its table; and the levels */
        uint32_t n_buses = 0, n_tables = 0;
        bool arrays = false, tables = false;
        void *sd;
        size_t n_s = 0;
        if (napi_is_array(env, argv[21], &arrays) != napi_ok || !arrays || napi_get_array_length(env, argv[21], &n_buses) != napi_ok || n_buses < 1 || n_buses > 4)
            bad = "buses must be an array of 1 .. 4 programs";
        else if (napi_is_array(env, argv[22], &tables) != napi_ok || !tables || napi_get_array_length(env, argv[22], &n_tables) != napi_ok || n_tables != n_buses)
            bad = "busParams must be an array of one entry per bus";
        else if (with_tracks) { /* (the levels are the tracks': trackSends) */
            napi_valuetype st = napi_undefined;
            napi_typeof(env, argv[23], &st);
            if (st != napi_null && st != napi_undefined) bad = "sends must be null with tracks: the buses are fed by trackSends";
        } else if (!typed_array(env, argv[23], napi_float32_array, &sd, &n_s) || n_s != (size_t)n_buses * n_voices) bad = "sends must be a Float32Array of one value per bus and voice";
        else if (!(j->sends = (float *)malloc(n_s * sizeof(float) + 1))) bad = "out of host memory for the send levels";
        else memcpy(j->sends, sd, n_s * sizeof(float));
        for (uint32_t b = 0; b < n_buses && !bad; b++) {
            napi_value prog_v, table_v;
            napi_valuetype tt = napi_undefined;
            prog_box *pb = NULL;
            if (napi_get_element(env, argv[21], b, &prog_v) != napi_ok || napi_get_element(env, argv[22], b, &table_v) != napi_ok) { bad = "could not read a bus"; break; }
            if (!(pb = as_prog(env, prog_v))) { /* (as_prog has thrown) */
                piece_free(env, j);
                return NULL;
            }
            j->bus_pb[b] = pb;
            j->n_buses = b + 1;
            dusp_program_info bi;
            dusp_program_info_get(pb->prog, &bi);
            napi_typeof(env, table_v, &tt);
            if (pb->cb != j->pbs[0]->cb) bad = "a bus is built on the context of the piece's parts";
            else if (tt != napi_null && tt != napi_undefined) {
                void *data;
                size_t len;
                if (!typed_array(env, table_v, napi_float32_array, &data, &len) || len != (size_t)bi.n_params * n_channels) bad = "busParams holds Float32Arrays of nParams * timeline channels values";
                else if (!(j->bus_params[b] = (float *)malloc(len * sizeof(float) + 1))) bad = "out of host memory for a parameter table";
                else memcpy(j->bus_params[b], data, len * sizeof(float));
            } else if (bi.n_params) bad = "a bus's program needs a parameter table";
        }
    }
    if (!bad && with_tracks) { /* the tracks: where the voices go, the track programs with their lists and tables, the faders and levels */
        double n_tracks = 0;
        uint32_t n_tp = 0, n_lists = 0, n_tables = 0;
        bool a0 = false, a1 = false, a2 = false;
        void *od;
        size_t n_o = 0;
        napi_valuetype ft = napi_undefined, lt = napi_undefined;
        j->with_tracks = 1;
        if (napi_get_value_double(env, argv[24], &n_tracks) != napi_ok || !(n_tracks >= 1 && n_tracks <= 8 && n_tracks == (double)(size_t)n_tracks)) bad = "a call has 1 .. 8 tracks";
        else if (!typed_array(env, argv[25], napi_int32_array, &od, &n_o) || n_o != n_voices) bad = "trackOf must be an Int32Array of one value per voice";
        else if (!(j->track_of = (int32_t *)malloc(n_o * sizeof(int32_t)))) bad = "out of host memory for trackOf";
        else if (napi_is_array(env, argv[26], &a0) != napi_ok || !a0 || napi_get_array_length(env, argv[26], &n_tp) != napi_ok || n_tp > 8) bad = "trackProgs must be an array of 0 .. 8 programs";
        else if (napi_is_array(env, argv[27], &a1) != napi_ok || !a1 || napi_get_array_length(env, argv[27], &n_lists) != napi_ok || n_lists != n_tp) bad = "trackLists must be an array of one entry per track program";
        else if (napi_is_array(env, argv[28], &a2) != napi_ok || !a2 || napi_get_array_length(env, argv[28], &n_tables) != napi_ok || n_tables != n_tp) bad = "trackParams must be an array of one entry per track program";
        else {
            memcpy(j->track_of, od, n_o * sizeof(int32_t));
            j->n_tracks = (size_t)n_tracks;
        }
        for (uint32_t t = 0; t < n_tp && !bad; t++) {
            napi_value prog_v, list_v, table_v;
            napi_valuetype tt = napi_undefined;
            prog_box *pb = NULL;
            void *ld;
            size_t n_l = 0;
            if (napi_get_element(env, argv[26], t, &prog_v) != napi_ok || napi_get_element(env, argv[27], t, &list_v) != napi_ok || napi_get_element(env, argv[28], t, &table_v) != napi_ok) { bad = "could not read a track program"; break; }
            if (!(pb = as_prog(env, prog_v))) { /* (as_prog has thrown) */
                piece_free(env, j);
                return NULL;
            }
            j->tprog_pb[t] = pb;
            j->n_tprogs = t + 1;
            dusp_program_info ti;
            dusp_program_info_get(pb->prog, &ti);
            napi_typeof(env, table_v, &tt);
            if (pb->cb != j->pbs[0]->cb) bad = "a track program is built on the context of the piece's parts";
            else if (!typed_array(env, list_v, napi_uint32_array, &ld, &n_l) || n_l < 1 || n_l > 8) bad = "trackLists holds Uint32Arrays of 1 .. 8 tracks";
            else if (!(j->tprog_tracks[t] = (uint32_t *)malloc(n_l * sizeof(uint32_t)))) bad = "out of host memory for a track list";
            else {
                memcpy(j->tprog_tracks[t], ld, n_l * sizeof(uint32_t));
                j->tprog_n[t] = n_l;
                if (tt != napi_null && tt != napi_undefined) {
                    void *data;
                    size_t len;
                    if (!typed_array(env, table_v, napi_float32_array, &data, &len) || len != (size_t)ti.n_params * n_l * n_channels) bad = "trackParams holds Float32Arrays of nParams * tracks * timeline channels values";
                    else if (!(j->tprog_params[t] = (float *)malloc(len * sizeof(float) + 1))) bad = "out of host memory for a parameter table";
                    else memcpy(j->tprog_params[t], data, len * sizeof(float));
                } else if (ti.n_params) bad = "a track program needs a parameter table";
            }
        }
        napi_typeof(env, argv[29], &ft);
        if (!bad && ft != napi_null && ft != napi_undefined) {
            void *data;
            size_t len;
            if (!typed_array(env, argv[29], napi_float32_array, &data, &len) || len != j->n_tracks) bad = "faders must be a Float32Array of one value per track";
            else if (!(j->faders = (float *)malloc(len * sizeof(float)))) bad = "out of host memory for the faders";
            else memcpy(j->faders, data, len * sizeof(float));
        }
        napi_typeof(env, argv[30], &lt);
        if (!bad && lt != napi_null && lt != napi_undefined) {
            void *data;
            size_t len;
            if (!typed_array(env, argv[30], napi_float32_array, &data, &len) || len != j->n_buses * j->n_tracks || !len) bad = "trackSends must be a Float32Array of one value per bus and track";
            else if (!(j->track_sends = (float *)malloc(len * sizeof(float)))) bad = "out of host memory for the tracks' levels";
            else memcpy(j->track_sends, data, len * sizeof(float));
        }
    }
    if (!bad && with_master) { /* the master: a program of the parts' context; its table has one column a channel of the timeline */
        napi_valuetype mt = napi_undefined;
        if (!(j->master_pb = as_prog(env, argv[19]))) { /* (as_prog has thrown) */
            piece_free(env, j);
            return NULL;
        }
        dusp_program_info mi;
        dusp_program_info_get(j->master_pb->prog, &mi);
        napi_typeof(env, argv[20], &mt);
        if (j->master_pb->cb != j->pbs[0]->cb) bad = "the master is built on the context of the piece's parts";
        else if (mt != napi_null && mt != napi_undefined) {
            void *data;
            size_t len;
            if (!typed_array(env, argv[20], napi_float32_array, &data, &len) || len != (size_t)mi.n_params * n_channels) bad = "masterParams must be a Float32Array of nParams * timeline channels values";
            else if (!(j->master_params = (float *)malloc(len * sizeof(float) + 1))) bad = "out of host memory for a parameter table";
            else memcpy(j->master_params, data, len * sizeof(float));
        } else if (mi.n_params) bad = "the master's program needs a parameter table";
    }
    j->with_stems = with_stems;
    j->with_meters = with_meters;
    j->stems_asked = with_stems;
    if (with_meters) {
        bool asked = false;
        double n_blocks = -1;
        if (napi_get_value_bool(env, argv[31], &asked) != napi_ok || napi_get_value_double(env, argv[32], &n_blocks) != napi_ok || !(n_blocks >= 0 && n_blocks <= 4294967295.0) ||
            n_blocks != (double)(size_t)n_blocks)
            bad = bad ? bad : "stems is a boolean and nBlocks a whole number";
        else
            j->stems_asked = asked, j->n_blocks = (size_t)n_blocks;
    }
    j->with_loud = with_loud;
    j->l_gain = 1.0, j->l_level = 1.0f;
    if (with_loud) {
        bool deliver = false;
        if (napi_get_value_bool(env, argv[33], &deliver) != napi_ok || napi_get_value_double(env, argv[34], &j->target) != napi_ok || napi_get_value_double(env, argv[35], &j->ceiling) != napi_ok)
            bad = bad ? bad : "deliver is a boolean, targetLufs and ceilingDbtp are numbers";
        j->deliver = deliver ? 1 : 0;
    }
    j->with_limiter = with_limiter;
    j->lim_reduction = 1.0;
    if (with_limiter) { /* (the library refuses a window that is 0 or above 4096) */
        double window = -1;
        if (napi_get_value_double(env, argv[36], &window) != napi_ok || !(window >= 0 && window <= 4294967295.0) || window != (double)(size_t)window)
            bad = bad ? bad : "windowSamples is a whole number";
        else
            j->lim_window = (size_t)window;
    }
    if (with_release) { /* (the library refuses a release above 2^22; 0: the call without one) */
        double release = -1;
        if (napi_get_value_double(env, argv[37], &release) != napi_ok || !(release >= 0 && release <= 4294967295.0) || release != (double)(size_t)release)
            bad = bad ? bad : "releaseSamples is a whole number";
        else
            j->lim_release = (size_t)release;
    }
    j->n_signals = j->stems_asked ? 1 + j->n_tracks + j->n_buses + 1 : 1;
    j->n_channels = (size_t)n_channels;
    if (!bad && with_loud && !(j->m_tp = (double *)calloc(j->n_signals * j->n_channels + 1, sizeof(double)))) bad = "out of host memory for the true peaks";
    if (!bad && with_meters &&
        (!(j->m_rms = (double *)calloc(j->n_signals * j->n_channels + 1, sizeof(double))) || !(j->m_lufs = (double *)calloc(j->n_signals + 1, sizeof(double))) ||
         !(j->m_momentary = (double *)calloc(j->n_signals * j->n_blocks + 1, sizeof(double)))))
        bad = "out of host memory for the meters";
    j->n_floats = j->n_signals * (size_t)n_channels * j->n_total;
    j->n_bytes = j->n_floats * (size_t)(!j->format || j->format == DUSP_PCM_F32 ? 4 : j->format == DUSP_PCM_S16 ? 2 : 3);
    if (!bad && !(j->out = (float *)malloc(j->n_bytes + 1))) bad = "out of host memory for the PCM buffer";
    if (bad) {
        char full[320];
        snprintf(full, sizeof full, "dusp-hip: renderPiece: %s", bad);
        piece_free(env, j);
        throw_string(env, full);
        return NULL;
    }
    napi_value promise, name;
    int queued = napi_create_promise(env, &j->deferred, &promise) == napi_ok && napi_create_string_utf8(env, "dusp-hip render", NAPI_AUTO_LENGTH, &name) == napi_ok;
    for (uint32_t p = 0; p < n_parts && queued; p++) {
        napi_value prog_v;
        queued = napi_get_element(env, argv[0], p, &prog_v) == napi_ok && napi_create_reference(env, prog_v, 1, &j->refs[p]) == napi_ok;
    }
    if (queued && j->master_pb) queued = napi_create_reference(env, argv[19], 1, &j->master_ref) == napi_ok;
    for (size_t b = 0; b < j->n_buses && queued; b++) {
        napi_value prog_v;
        queued = napi_get_element(env, argv[21], (uint32_t)b, &prog_v) == napi_ok && napi_create_reference(env, prog_v, 1, &j->bus_ref[b]) == napi_ok;
    }
    for (size_t t = 0; t < j->n_tprogs && queued; t++) {
        napi_value prog_v;
        queued = napi_get_element(env, argv[26], (uint32_t)t, &prog_v) == napi_ok && napi_create_reference(env, prog_v, 1, &j->tprog_ref[t]) == napi_ok;
    }
    queued = queued && napi_create_async_work(env, NULL, name, piece_execute, piece_complete, j, &j->work) == napi_ok;
    if (queued) {
        for (uint32_t p = 0; p < n_parts; p++) j->pbs[p]->in_flight++;
        if (j->master_pb) j->master_pb->in_flight++;
        for (size_t b = 0; b < j->n_buses; b++) j->bus_pb[b]->in_flight++;
        for (size_t t = 0; t < j->n_tprogs; t++) j->tprog_pb[t]->in_flight++;
        if (napi_queue_async_work(env, j->work) != napi_ok) {
            for (uint32_t p = 0; p < n_parts; p++) j->pbs[p]->in_flight--;
            if (j->master_pb) j->master_pb->in_flight--;
            for (size_t b = 0; b < j->n_buses; b++) j->bus_pb[b]->in_flight--;
            for (size_t t = 0; t < j->n_tprogs; t++) j->tprog_pb[t]->in_flight--;
            queued = 0;
        }
    }
    if (!queued) {
        j->master_pb = NULL;
        j->n_buses = 0;
        j->n_tprogs = 0;
        piece_free(env, j);
        throw_string(env, "dusp-hip: renderPiece: could not queue the render");
        return NULL;
    }
    return promise;
}

static napi_value fn_render_piece(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 0); }
static napi_value fn_render_piece_pan(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 1); }
static napi_value fn_render_piece_frac(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 2); }
static napi_value fn_render_piece_space(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 3); }
static napi_value fn_render_piece_stereo(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 4); }
static napi_value fn_render_piece_master(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 5); }
static napi_value fn_render_piece_buses(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 6); }
static napi_value fn_render_piece_tracks(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 7); }
static napi_value fn_render_piece_stems(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 8); }
static napi_value fn_render_piece_meters(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 9); }
static napi_value fn_render_piece_loudness(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 10); }

/* meter(ctx, planar, nSignals, nChannels, nSamples, sampleRate) -> { rms: Float64Array [nSignals * nChannels], lufs: Float64Array [nSignals],
 * momentary: Float64Array [nSignals * blocks] }: the meters of f32 signals in host memory, on the device, gated in the library
 * (dusp_meter_host).  Throws the library's message. */
static napi_value fn_meter(napi_env env, napi_callback_info info) {
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return NULL;
    ctx_box *b = as_ctx(env, argv[0]);
    if (!b) return NULL;
    void *data;
    size_t len;
    double dims[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) napi_get_value_double(env, argv[2 + i], &dims[i]);
    for (int i = 0; i < 4; i++)
        if (!(dims[i] >= 1 && dims[i] <= 4294967295.0) || dims[i] != (double)(size_t)dims[i]) {
            throw_string(env, "dusp-hip: meter: nSignals, nChannels, nSamples and sampleRate are whole numbers of at least 1");
            return NULL;
        }
    const size_t n_signals = (size_t)dims[0], n_channels = (size_t)dims[1], n_samples = (size_t)dims[2];
    const uint32_t rate = (uint32_t)dims[3];
    if (!typed_array(env, argv[1], napi_float32_array, &data, &len) || (double)len != dims[0] * dims[1] * dims[2]) {
        throw_string(env, "dusp-hip: meter: planar must be a Float32Array of nSignals * nChannels * nSamples values");
        return NULL;
    }
    const size_t n_blocks = dusp_meter_blocks(n_samples, rate), counts[3] = {n_signals * n_channels, n_signals, n_signals * n_blocks};
    const char *names[3] = {"rms", "lufs", "momentary"};
    napi_value result, arrs[3];
    void *mem[3];
    NAPI_OK(napi_create_object(env, &result));
    for (int m = 0; m < 3; m++) {
        napi_value ab;
        NAPI_OK(napi_create_arraybuffer(env, counts[m] * sizeof(double), &mem[m], &ab));
        NAPI_OK(napi_create_typedarray(env, napi_float64_array, counts[m], ab, 0, &arrs[m]));
        NAPI_OK(napi_set_named_property(env, result, names[m], arrs[m]));
    }
    pthread_mutex_lock(&b->lock);
    int rc = dusp_meter_host(b->ctx, (const float *)data, n_signals, n_channels, n_samples, rate, (double *)mem[0], (double *)mem[1], n_blocks ? (double *)mem[2] : NULL);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(b->ctx));
    pthread_mutex_unlock(&b->lock);
    if (rc != DUSP_OK) {
        throw_string(env, msg);
        return NULL;
    }
    return result;
}

static napi_value fn_render_piece_limiter(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 11); }
static napi_value fn_render_piece_limiter_release(napi_env env, napi_callback_info info) { return render_piece_call(env, info, 12); }

/* limit(ctx, planar, nSignals, nChannels, nSamples, sampleRate, threshold, windowSamples) -> { data, gain, reduction }: f32 signals in host memory
 * limited on the device under ONE look-ahead gain curve (dusp_limit_host): data a Float32Array of planar's layout, gain a Float64Array [nSamples],
 * reduction the smallest gain.  Throws the library's message. */
static napi_value limit_call(napi_env env, napi_callback_info info, int with_release) {
    napi_value argv[9];
    if (!get_args(env, info, with_release ? 9 : 8, argv)) return NULL;
    ctx_box *b = as_ctx(env, argv[0]);
    if (!b) return NULL;
    void *data, *mem, *gain_mem;
    size_t len;
    double dims[4] = {0, 0, 0, 0}, threshold = 0, window = 0, release = 0;
    for (int i = 0; i < 4; i++) napi_get_value_double(env, argv[2 + i], &dims[i]);
    for (int i = 0; i < 4; i++)
        if (!(dims[i] >= 1 && dims[i] <= 4294967295.0) || dims[i] != (double)(size_t)dims[i]) {
            throw_string(env, "dusp-hip: limit: nSignals, nChannels, nSamples and sampleRate are whole numbers of at least 1");
            return NULL;
        }
    if (napi_get_value_double(env, argv[6], &threshold) != napi_ok || napi_get_value_double(env, argv[7], &window) != napi_ok || !(window >= 0 && window <= 4294967295.0) ||
        window != (double)(size_t)window) {
        throw_string(env, "dusp-hip: limit: threshold is a number and windowSamples a whole number");
        return NULL;
    }
    if (with_release && (napi_get_value_double(env, argv[8], &release) != napi_ok || !(release >= 0 && release <= 4294967295.0) || release != (double)(size_t)release)) {
        throw_string(env, "dusp-hip: limit: releaseSamples is a whole number");
        return NULL;
    }
    const size_t n_signals = (size_t)dims[0], n_channels = (size_t)dims[1], n_samples = (size_t)dims[2];
    if (!typed_array(env, argv[1], napi_float32_array, &data, &len) || (double)len != dims[0] * dims[1] * dims[2]) {
        throw_string(env, "dusp-hip: limit: planar must be a Float32Array of nSignals * nChannels * nSamples values");
        return NULL;
    }
    napi_value ab, limited, gain_ab, gain, reduced, result;
    double reduction = 1.0;
    NAPI_OK(napi_create_arraybuffer(env, len * sizeof(float), &mem, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_float32_array, len, ab, 0, &limited));
    NAPI_OK(napi_create_arraybuffer(env, n_samples * sizeof(double), &gain_mem, &gain_ab));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_samples, gain_ab, 0, &gain));
    pthread_mutex_lock(&b->lock);
    int rc = with_release ? dusp_limit_release_host(b->ctx, (const float *)data, n_signals, n_channels, n_samples, (uint32_t)dims[3], threshold, (size_t)window, (size_t)release, (float *)mem,
                                                    (double *)gain_mem, &reduction)
                          : dusp_limit_host(b->ctx, (const float *)data, n_signals, n_channels, n_samples, (uint32_t)dims[3], threshold, (size_t)window, (float *)mem, (double *)gain_mem, &reduction);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(b->ctx));
    pthread_mutex_unlock(&b->lock);
    if (rc != DUSP_OK) {
        throw_string(env, msg);
        return NULL;
    }
    NAPI_OK(napi_create_object(env, &result));
    NAPI_OK(napi_create_double(env, reduction, &reduced));
    NAPI_OK(napi_set_named_property(env, result, "data", limited));
    NAPI_OK(napi_set_named_property(env, result, "gain", gain));
    NAPI_OK(napi_set_named_property(env, result, "reduction", reduced));
    return result;
}
static napi_value fn_limit(napi_env env, napi_callback_info info) { return limit_call(env, info, 0); }
/* limitRelease(the same eight, releaseSamples): limit with a release of its own, 1 .. 2^22 samples (dusp_limit_release_host) */
static napi_value fn_limit_release(napi_env env, napi_callback_info info) { return limit_call(env, info, 1); }

/* truePeak(ctx, planar, nSignals, nChannels, nSamples, sampleRate) -> Float64Array [nSignals * nChannels]: the true peaks of f32 signals in
 * host memory, on the device, linear (dusp_true_peak_host).  Throws the library's message. */
static napi_value fn_true_peak(napi_env env, napi_callback_info info) {
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return NULL;
    ctx_box *b = as_ctx(env, argv[0]);
    if (!b) return NULL;
    void *data, *mem;
    size_t len;
    double dims[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) napi_get_value_double(env, argv[2 + i], &dims[i]);
    for (int i = 0; i < 4; i++)
        if (!(dims[i] >= 1 && dims[i] <= 4294967295.0) || dims[i] != (double)(size_t)dims[i]) {
            throw_string(env, "dusp-hip: truePeak: nSignals, nChannels, nSamples and sampleRate are whole numbers of at least 1");
            return NULL;
        }
    const size_t n_signals = (size_t)dims[0], n_channels = (size_t)dims[1], n_samples = (size_t)dims[2];
    if (!typed_array(env, argv[1], napi_float32_array, &data, &len) || (double)len != dims[0] * dims[1] * dims[2]) {
        throw_string(env, "dusp-hip: truePeak: planar must be a Float32Array of nSignals * nChannels * nSamples values");
        return NULL;
    }
    napi_value ab, result;
    NAPI_OK(napi_create_arraybuffer(env, n_signals * n_channels * sizeof(double), &mem, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, n_signals * n_channels, ab, 0, &result));
    pthread_mutex_lock(&b->lock);
    int rc = dusp_true_peak_host(b->ctx, (const float *)data, n_signals, n_channels, n_samples, (uint32_t)dims[3], (double *)mem);
    char msg[512];
    if (rc != DUSP_OK) snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(b->ctx));
    pthread_mutex_unlock(&b->lock);
    if (rc != DUSP_OK) {
        throw_string(env, msg);
        return NULL;
    }
    return result;
}

/* descriptorChannels(words) -> the output channels of the descriptor's circuit (dusp_descriptor_channels: host code only, no context) */
static napi_value fn_descriptor_channels(napi_env env, napi_callback_info info) {
    napi_value argv[1], out;
    void *data;
    size_t len;
    if (!get_args(env, info, 1, argv)) return NULL;
    if (!typed_array(env, argv[0], napi_float64_array, &data, &len)) {
        throw_string(env, "dusp-hip: descriptorChannels: the descriptor must be a Float64Array");
        return NULL;
    }
    const int n = dusp_descriptor_channels((const double *)data, len);
    if (n < 0) {
        char msg[512];
        snprintf(msg, sizeof msg, "dusp-hip: %s", dusp_last_error(NULL));
        throw_string(env, msg);
        return NULL;
    }
    NAPI_OK(napi_create_uint32(env, (uint32_t)n, &out));
    return out;
}

static napi_value init(napi_env env, napi_value exports) {
    static const struct {
        const char *name;
        napi_callback fn;
    } fns[] = {
        {"version", fn_version},          {"abiVersion", fn_abi_version},     {"ctxCreate", fn_ctx_create},
        {"ctxDestroy", fn_ctx_destroy},   {"tableUpload", fn_table_upload},   {"programBuild", fn_program_build},
        {"programDestroy", fn_program_destroy}, {"programInfo", fn_program_info}, {"stateDownload", fn_state_download},
        {"render", fn_render},            {"programContinue", fn_program_continue}, {"deviceCount", fn_device_count},
        {"renderPcm", fn_render_pcm},     {"renderMix", fn_render_mix},       {"renderScore", fn_render_score},
        {"renderPiece", fn_render_piece}, {"descriptorChannels", fn_descriptor_channels}, {"renderPiecePan", fn_render_piece_pan},
        {"renderPieceFrac", fn_render_piece_frac}, {"renderPieceSpace", fn_render_piece_space}, {"renderPieceStereo", fn_render_piece_stereo}, {"renderPieceMaster", fn_render_piece_master},
        {"renderPieceBuses", fn_render_piece_buses}, {"renderPieceTracks", fn_render_piece_tracks}, {"renderPieceStems", fn_render_piece_stems},
        {"renderPieceMeters", fn_render_piece_meters}, {"meter", fn_meter}, {"renderPieceLoudness", fn_render_piece_loudness}, {"truePeak", fn_true_peak},
        {"renderPieceLimiter", fn_render_piece_limiter}, {"limit", fn_limit},
        {"renderPieceLimiterRelease", fn_render_piece_limiter_release}, {"limitRelease", fn_limit_release},
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok ||
            napi_set_named_property(env, exports, fns[i].name, f) != napi_ok)
            return NULL;
    }
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
