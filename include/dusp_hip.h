/* dusp_hip.h — C ABI of the MI355X (gfx950) offline render path for Dusp.
 *
 * This library replaces ONE path of the reference: the chunk loop of
 *   src/renderChannelData.js:5-49  ->  src/Circuit.js:19-47 (tick/tickUntil)
 *   ->  src/Unit.js:111-119 (tick)  ->  per-unit `_tick` loops in src/components/
 * The reference has no FFI boundary on this path (it is pure in-process JS), so
 * the entry points below are the ones a Node N-API addon / ctypes stub binds in
 * order to stand in for `renderChannelData(outlet, duration)`; INTEGRATION.md
 * shows that binding.  Plain pointers and sizes only, no C++ or torch types.
 *
 * Hand-off format: a host-side extractor (dusp_amd/js/lib/extract.js, or
 * dusp_amd/descriptor.py) flattens the live Unit/Inlet/Outlet graph — in the
 * order `circuit.units` already holds (src/Circuit.js:125-131) — into an array of
 * little-endian f64 "descriptor words" (layout: DESIGN.md §3).  Many
 * structurally identical circuits (voices, a parameter sweep) are rendered by
 * ONE program plus a per-instance f32 parameter table.
 *
 * Error convention mirrors the reference's (thrown strings that surface as
 * Promise rejections, src/renderChannelData.js:12-17): every call returns 0 on
 * success or a negative dusp_status, and dusp_last_error() returns the message.
 * No C++ exception ever crosses this boundary and nothing calls abort(): sizes
 * taken from a descriptor are bounded before anything is allocated, and an
 * allocation failure inside the library comes back as a status like any other.
 * Nothing here ever falls back to a CPU implementation: without a usable HIP
 * device the calls fail with DUSP_ERR_HIP.
 *
 * Numerics: PCM and unit state are the reference's bit for bit wherever the device executes the IEEE operations JS
 * does — everything but the units that call Math.tan / Math.pow (Filter coefficients; Gain, DecibelToScaler,
 * SemitoneToRatio, Pow, Pan, MidiToFrequency), which are within 1e-5 of full scale.  One form trades
 * bits for speed inside that tolerance: a Filter whose cutoff is a constant between about 1.5 and 22.5 kHz (at 48 kHz) and
 * whose output only feeds sums, products with constants or bounded signals, delay lines and outlets is evaluated as a
 * scan over each chunk: each such Filter deviates from the reference's recurrence by at most 2^-24 (sum|h| + 2) <= 1.9e-6
 * of its own output's scale, and the form is taken only where what the circuit makes of those deviations — every unit's
 * worst-case gain, feedback loops' 1 / (1 - loop gain) included — stays within 2.5e-6 of the Filters' output scale at every
 * outlet (jit_codegen.hpp jit_filter_scan_ok).  A loop of gain 0.6 and above, a per-instance gain, a
 * product of two filtered signals keep the Filter stage.  DUSP_FILTER_SCAN=0 in the environment of dusp_ctx_create keeps
 * EVERY Filter on the stage, whose results are the reference recurrence's, operation for operation.
 *
 * Threading: a dusp_ctx is bound to one HIP device and is not thread-safe;
 * different contexts are independent (one context per GPU for multi-GPU use).
 * Streams: a program's workspaces are reused from render to render; renders of
 * one program are ordered among themselves whatever streams they are given (a
 * render on another stream than the previous one waits for it), and
 * dusp_state_download / dusp_program_destroy wait for the last render wherever
 * it ran.
 */
#ifndef DUSP_HIP_H
#define DUSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DUSP_ABI_VERSION 7

typedef struct dusp_ctx dusp_ctx;
typedef struct dusp_program dusp_program;

typedef enum {
    DUSP_OK = 0,
    DUSP_ERR_ARG = -1,         /* bad argument / malformed descriptor */
    DUSP_ERR_UNSUPPORTED = -2, /* graph uses something the GPU path does not implement */
    DUSP_ERR_HIP = -3,         /* HIP runtime error (no device, out of memory, launch failure) */
    DUSP_ERR_STATE = -4,       /* call sequence error (e.g. wave table not uploaded) */
    DUSP_ERR_NOMEM = -5        /* a host allocation failed while the call was being prepared */
} dusp_status;

/* Engine that executes a program (chosen at build time from the graph's shape):
 *   CHUNK — universal engine: one lane per instance, units ticked chunk by chunk
 *           exactly in circuit order (every opcode: feedback, filters, delay lines, CircleBuffers,
 *           envelopes).
 *   FUSED — time-parallel fused kernels for recognised voice shapes (Osc, Osc x Ramp,
 *           Osc x gain, Sum.many chains): one lane per sample, time split across waves,
 *           16-byte coalesced PCM stores.
 *   WAVE  — one wavefront per instance (or a few), wavefront-wide phase accumulation.  A circuit gets a kernel COMPILED FOR IT
 *           (units inlined in process order, operands in registers, the Filters' recurrences of a workgroup side by side on
 *           one wave with the other units beside them; dusp_circuit_kernel_source) — every unit of the path: FM, Filters,
 *           feedback edges, envelopes, the comb family, delay lines and CircleBuffer nodes lane-parallel or, where their
 *           accesses can meet inside a chunk, through ordered slot operations.  What stays on the interpreter kernel
 *           (chunk buffers in LDS) is decided by regime: circuits of more
 *           than 256 units (DUSP_JIT_MAX_UNITS), and a structure's FIRST render while its kernel compiles in the background.  Few instances and
 *           a long render are split in time when the graph allows it: oscillators, closed forms of time and stateless units by exact jumps,
 *           and — ABI v7 — circuits with constant-cutoff Filters too, in segments that warm up a segment early from rest and are checked
 *           against each other on the host (bit for bit the one long recurrence).  Refuses by regime, not by unit: channel
 *           counts that grow during the first chunks, more chunk buffers than LDS holds, an oscillator phase outside [0, sampleRate).
 * AUTO picks FUSED, else WAVE, else CHUNK.  (DUSP_ENGINE_LOOP — hand-written kernels for the feedback voice Osc -> Sum -> Delay -> Filter -> gain
 * of rounds 1 and 2 — is accepted and means AUTO since ABI v7: the kernel compiled for that circuit renders it 1.7 to 2.5 times faster.)
 *
 * DUSP_ENGINE_RESUMABLE may be OR-ed into the engine argument of dusp_program_build: the program will be
 * continued with dusp_program_continue (event-segmented rendering, src/Circuit.js:23,57-65).  Programs whose
 * circuit owns delay lines / CircleBuffers or has a feedback edge then run on the WAVE or the CHUNK engine and
 * keep their rings and chunk buffers resident between segments; a continuation never fails over the engine
 * (a WAVE program whose state leaves that engine's regime migrates to CHUNK). */
typedef enum {
    DUSP_ENGINE_AUTO = 0, DUSP_ENGINE_CHUNK = 1, DUSP_ENGINE_FUSED = 2, DUSP_ENGINE_WAVE = 3, DUSP_ENGINE_LOOP = 4,
    DUSP_ENGINE_RESUMABLE = 0x100
} dusp_engine;

typedef struct {
    uint32_t sample_rate;
    uint32_t chunk_size;
    uint32_t n_units;        /* units in the circuit */
    uint32_t n_out_channels; /* channels of the rendered outlet == result.length of renderChannelData */
    uint32_t n_params;       /* per-instance parameter slots the descriptor references */
    uint32_t engine;         /* dusp_engine actually selected */
    uint32_t n_device_ops;   /* channel-expanded ops the kernel executes per chunk */
    uint32_t n_inputs;       /* host-generated input streams the program reads (dusp_render_*_inputs) */
    char shape[64];          /* FUSED: signature of the fused kernel, e.g. "mul(osc(k),ramp)" */
} dusp_program_info;

/* Library / ABI identification. */
const char *dusp_version(void);
int dusp_abi_version(void);

/* Message of the last failing call on this context (or, with ctx == NULL, of
 * the last failing dusp_ctx_create on this thread).  Never NULL. */
const char *dusp_last_error(const dusp_ctx *ctx);

/* ABI v7.  HIP devices this process sees (what `device` of dusp_ctx_create ranges over), or a negative dusp_status
 * (message: dusp_last_error(NULL)).  A host that shards independent circuit instances over a node's GPUs creates one
 * context per device (dusp_amd/js/lib/renderChannelData.js renderMany, dusp_amd/shard.py). */
int dusp_device_count(void);

/* Create a context on HIP device `device` (-1 = current device). */
int dusp_ctx_create(int device, dusp_ctx **out);
void dusp_ctx_destroy(dusp_ctx *ctx);

/* Upload one lookup table (replaces src/components/Osc/waveTables.js:5-40 and
 * src/components/Shape/shapeTables.js:3-38: the host computes the tables exactly as the
 * reference does and hands them over as data).  table_id: 0 sin, 1 saw, 2 square,
 * 3 triangle, 4 8bit (oscillators); 5 decay, 6 attack, 7 semiSine, 8 decaySquared (Shape).
 * n must equal sample_rate + 1 of every program later built on this context. */
int dusp_table_upload(dusp_ctx *ctx, int table_id, const float *table, size_t n);

/* Compile a descriptor into a device program (replaces `new Circuit(unit)` +
 * computeOrders as the thing that fixes the schedule, src/Circuit.js:67-148 —
 * the ORDER itself comes from the descriptor).  `engine` = DUSP_ENGINE_AUTO
 * normally; tests force CHUNK to cross-check the engines. */
int dusp_program_build(dusp_ctx *ctx, const double *desc, size_t n_words, int engine, dusp_program **out);
void dusp_program_destroy(dusp_program *prog);

/* Continue a rendered program from a LATER extraction of the same circuit (replaces what
 * src/Circuit.js:23,57-65 does between two ticks: host callbacks — scheduled events — have run
 * on the unit objects, changing state fields or inlet constants).  `desc` must describe the same
 * structure (units, connections, channel counts, rings) and carry the clock the previous render
 * stopped at; unit state and constants are taken from it, ring contents and (for feedback graphs)
 * the previous chunk of every outlet stay as the device left them.  The next dusp_render_* call
 * renders the next segment.  Needs a program built with DUSP_ENGINE_RESUMABLE unless the circuit is
 * feed-forward and owns no rings; the instance count of the following render must not change. */
int dusp_program_continue(dusp_program *prog, const double *desc, size_t n_words);

int dusp_program_info_get(const dusp_program *prog, dusp_program_info *info);

/* Render n_instances independent instances of the program for n_samples samples
 * each, starting from the descriptor's initial state (replaces the loop at
 * src/renderChannelData.js:29-45; like it, ticks ceil(n_samples/chunk) chunks
 * and maps NaN / -0 to +0 on copy-out).
 *
 *   d_params  device pointer, f32 [n_params][n_instances] (slot-major); may be
 *             NULL when the program has no parameters.
 *   d_out     device pointer, f32 [n_instances][n_out_channels][n_samples].
 *   stream    hipStream_t to launch on (NULL = the context's own stream).
 *
 * Asynchronous: returns once the work is enqueued.  Inputs and outputs stay
 * resident in HBM; nothing crosses PCIe.  Three kinds of program wait for the stream inside the call, because what they launch
 * depends on a few bytes the device has to hand back first: a Delay or a Filter whose delay / cutoff is a per-instance parameter
 * (the column is looked at: one small launch, its verdict back), and a few long circuits with Filters cut into segments that warm
 * up (the segments' hand-overs are checked when the launch is done).  dusp_render_host waits anyway. */
int dusp_render_device(dusp_program *prog, size_t n_instances, size_t n_samples,
                       const float *d_params, float *d_out, void *stream);

/* One `Sum.many` dealt over several GPUs, bit for bit (replaces the single process's left-deep chain of
 * src/components/Sum.js:18-29 — ((v0 + v1) + v2) + ... with an f32 rounding per add — when the voices of the mix are sharded):
 * the program holds a CONTIGUOUS run of the chain's voices (built on the fused sum chain: every voice a constant-f oscillator,
 * bare or under the supported envelopes), and this call renders the window [first_sample, first_sample + n_samples) of the
 * render's timeline, one instance, CONTINUING the chain from d_init — the running sums the ranks before this one left for the
 * same window — instead of from zero (d_init NULL: this rank holds the chain's first voices).  raw != 0 writes the sums as
 * they stand (a partial sum another rank continues: no `x || 0`, so a NaN travels on as the reference's would); the rank with
 * the chain's last voices passes raw = 0 and gets the mix as dusp_render_device would have written it.
 *   first_sample  a multiple of 2048 (whole blocks of the kernel), at most 2^40 (DUSP_ERR_ARG beyond: 2^40 samples are 66 days at 192 kHz)
 *   n_samples     at most 65535 blocks of 2048 samples, 134215680, like every launch of the fused sum chain (DUSP_ERR_UNSUPPORTED beyond)
 *   d_init, d_out device pointers, f32 [n_out_channels = 1][n_samples], 16-byte aligned; they may be the same buffer
 * Every window in that range is exact at every sample rate: the window's place in the timeline is folded into the voices' start
 * phases on the host in 128-bit integers, and the kernel counts blocks and samples from the window's first sample.
 * Asynchronous like dusp_render_device.  DUSP_ERR_UNSUPPORTED for a program that is not on the fused sum chain. */
int dusp_render_chain_window(dusp_program *prog, uint64_t first_sample, size_t n_samples,
                             const float *d_init, int raw, float *d_out, void *stream);

/* Host callers (the N-API addon): uploads h_params, renders, downloads into h_out
 * (same layouts as above) and synchronises.  The download is what the caller
 * waits for — PCIe, hundreds of times slower than the render — so:
 *   h_out from dusp_host_alloc (pinned): one DMA at link speed straight into it;
 *   h_out pageable and large: several worker threads, each double-buffering pinned
 *   staging tiles on its own stream, copy disjoint ranges concurrently;
 *   small outputs: a plain asynchronous copy. */
int dusp_render_host(dusp_program *prog, size_t n_instances, size_t n_samples,
                     const float *h_params, float *h_out);

/* Result buffers (replaces `new TypedArray(lengthInSamples)` of src/renderChannelData.js:39 as the thing that owns the
 * returned samples): n_bytes of PINNED host memory from the context's pool.  dusp_render_host* into such a buffer is a
 * direct device-to-host DMA.  dusp_host_free hands the buffer back to the pool (it stays pinned for the next render of
 * that size; dusp_ctx_destroy releases everything).  The N-API addon wraps these in external ArrayBuffers whose
 * finalizer calls dusp_host_free. */
int dusp_host_alloc(dusp_ctx *ctx, size_t n_bytes, void **out);
int dusp_host_free(dusp_ctx *ctx, void *p);

/* Host-generated signals.  A descriptor may hold INPUT units (opcode 41, attribute = stream index): units whose
 * output the HOST computes while the rest of the circuit runs on the device — the reference's Noise
 * (src/components/Noise.js:16-27: a Math.random() per sample, which only the caller's JavaScript engine can draw in
 * the reference's order), or any source the caller ticks itself.  dusp_program_info.n_inputs says how many streams the
 * program reads; bind them at every render:
 *   inputs   f32 [n_inputs][n_instances][n_samples]  (the samples of THIS render call, i.e. of this segment)
 * The plain render calls refuse a program with inputs. */
int dusp_render_device_inputs(dusp_program *prog, size_t n_instances, size_t n_samples,
                              const float *d_params, const float *d_inputs, float *d_out, void *stream);
int dusp_render_host_inputs(dusp_program *prog, size_t n_instances, size_t n_samples,
                            const float *h_params, const float *h_inputs, float *h_out, int interleaved);

/* Wire format (replaces the per-chunk loop of src/RenderStream.js:36-57 as the thing that produces frames):
 * planar PCM f32 [n_instances][n_channels][n_samples], as the render calls write it, to interleaved frames
 * f32 [n_instances][n_samples][n_channels] — `buffer[t * numberOfChannels + c]`, 32-bit little-endian floats
 * (src/RenderStream.js:54,63-68; also the layout of a WAV data chunk).  Device pointers, asynchronous; the two
 * buffers must not overlap. */
int dusp_interleave_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples,
                           float *d_interleaved, void *stream);

/* dusp_render_host, delivering interleaved frames: h_out is f32 [n_instances][n_samples][n_out_channels]. */
int dusp_render_host_interleaved(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, float *h_out);

/* Device-side PCM delivery (additions to ABI v7: DUSP_ABI_VERSION is unchanged, a binder detects them by symbol).  Replaces
 * the host's per-sample encode loop: the peak search, the gain, the quantisation and the interleave run on the device, and
 * 2 (s16) or 3 (s24) bytes per sample are downloaded instead of 4.
 *
 * The sample contract (dusp_amd/csrc/pcm_quant.hpp; dusp_amd/wav.py and dusp_amd/js/lib/wav.js compute the same bytes), for
 * an f32 sample x, the instance's gain g (a double) and S = 32767 (s16) or 8388607 (s24):
 *     t = (double)x * g;  t = NaN ? 0 : min(max(t, -1), 1);  q = t * S rounded to the nearest integer, halves away from zero
 * as little-endian int16 / packed 3-byte int24, interleaved [instance][frame][channel].  DUSP_PCM_F32 is (float)((double)x * g),
 * interleaved, not clamped, NaN left as it is.
 *   peak  of an instance: the exact maximum of |x| over all its channels and samples, as an f32; NaN if any sample is NaN.
 *   gain  DUSP_NORMALISE_NONE: 1.  DUSP_NORMALISE_CLIP: 1 / (double)peak when the peak is finite and > 1 (shrink only what
 *         would clip), else 1.  DUSP_NORMALISE_FULL: 1 / (double)peak when the peak is finite and > 0, else 1.  One gain
 *         per instance covers all its channels. */
typedef enum { DUSP_PCM_S16 = 1, DUSP_PCM_S24 = 2, DUSP_PCM_F32 = 3 } dusp_pcm_format;
typedef enum { DUSP_NORMALISE_NONE = 0, DUSP_NORMALISE_CLIP = 1, DUSP_NORMALISE_FULL = 2 } dusp_normalise;

/* Peaks of planar PCM f32 [n_instances][n_channels][n_samples] -> d_peaks f32 [n_instances].  Device pointers, asynchronous. */
int dusp_peak_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples,
                     float *d_peaks, void *stream);

/* Planar PCM -> encoded frames: d_out receives n_instances * n_samples * n_channels * (2 | 3 | 4) bytes, exactly (any byte
 * alignment for s16 / s24, 4-byte aligned for f32; fastest from 16-byte boundaries).  Every instance's gain is derived on
 * the device from d_peaks (what dusp_peak_device wrote; NULL allowed only when normalise == 0): no host round trip, no
 * synchronisation.  Device pointers, asynchronous; the buffers must not overlap. */
int dusp_encode_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples,
                       int format, int normalise, const float *d_peaks, void *d_out, void *stream);

/* dusp_render_host, delivering encoded frames: renders, measures the peaks (when normalise != 0 or h_peaks is given),
 * encodes, and downloads n_instances * n_samples * n_out_channels * bytes into h_out by the delivery paths of
 * dusp_render_host (pinned: one DMA; large and pageable: the staged workers; small: a plain copy).
 *   h_inputs  f32 [n_inputs][n_instances][n_samples]; NULL unless the program has input streams
 *   h_peaks   f32 [n_instances], may be NULL */
int dusp_render_host_pcm(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_inputs,
                         int format, int normalise, void *h_out, float *h_peaks);

/* The mix of a batch, on the device, in Sum.many's chain order (additions to ABI v7: DUSP_ABI_VERSION is unchanged, a binder
 * detects them by symbol).  Replaces `Sum.many(voices)` as the thing that mixes rendered voices: the reference's left-deep
 * chain ((v0 + v1) + v2) + ... of Sum units, each storing an f32 (src/components/Sum.js:18-29,33-44) — one f32 rounding per
 * add, in index order.  For every channel c and sample t
 *     acc = d_init ? d_init[c][t] : term(0);   acc = (float)(acc + term(i)) for the remaining instances, in index order
 *     term(i) = d_gains ? (float)(x_i * g_i) : x_i        (a plain f32 product, as Multiply stores it, then a plain f32 add)
 * Without d_init the chain starts from the first voice itself, not from 0 + v0.
 *   d_planar       f32 [n_instances][n_channels][n_samples], as the render calls write it
 *   d_gains        f32 [n_instances], or NULL
 *   d_init, d_out  f32 [n_channels][n_samples]; d_init may be NULL, and may be d_out (in place); d_planar must not overlap d_out
 *   raw            != 0: the sums as they stand (a partial sum that is continued: NaN and -0 kept); 0: `acc || 0`, NaN and -0
 *                  leave as +0 (src/renderChannelData.js:44)
 * Any 4-byte alignment and any n_samples; 16-byte accesses where the bases are 16-byte aligned and n_channels * n_samples is a
 * multiple of 4, coalesced dword accesses elsewhere.  n_channels * n_samples must not exceed 2^31 (DUSP_ERR_ARG).  Device
 * pointers, asynchronous.
 * One divergence from the reference: a voice sample that is NaN travels through the reference's Sums and zeroes the MIX sample;
 * a batch render maps NaN to +0 per voice on copy-out, so here only that voice drops out of the sample.  (The voices' -0 -> +0
 * changes nothing after the final `|| 0`.)  The mix is the reference's wherever no voice sample is NaN. */
int dusp_mix_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_samples,
                    const float *d_gains, const float *d_init, int raw, float *d_out, void *stream);

/* Render n_instances instances and deliver their mix: instances [lo, hi) are rendered tile by tile into a scratch buffer that
 * lives with the program, and every tile continues the chain above into one [n_out_channels][n_samples] accumulator (raw for
 * all tiles but the last).  Device memory is bounded by the tile, not by n_instances, and the tiling does not change a bit of
 * the result: what a render decides from the batch and that changes bits — whether Filters run as scans, by the range of a
 * per-instance cutoff column and by whether the instance count has the render cut into warming segments — is decided from the
 * whole batch, and every tile runs on the circuit's compiled kernel, waiting for it where it is new (also under DUSP_WAVE_JIT=1,
 * where a plain short render would not wait and run on the interpreter kernel): a tile renders as one render of all instances
 * on the compiled kernel would.
 *   h_params        f32 [n_params][n_instances] (slot-major), every tile takes its own columns; NULL without parameters
 *   h_gains         f32 [n_instances], or NULL
 *   tile_instances  instances per tile; 0: the batch that fills the chip, 32 instances per compute unit, or as many of them as
 *                   fit 16 GiB and half of the device's free memory
 *   format          0: h_out receives planar f32 [n_out_channels][n_samples]; DUSP_PCM_S16 / S24 / F32: the peak and encode
 *                   kernels run over the mix as one instance and h_out receives frames, as from dusp_render_host_pcm
 *   h_peak          one f32, may be NULL (only looked at for the PCM formats)
 * Delivery paths of dusp_render_host.  DUSP_ERR_UNSUPPORTED for programs with INPUT streams and for resumable programs.  A fused
 * sum-chain program is one instance like any other: n_instances = 1 is the voice itself.  Afterwards unit state describes the
 * last tile only: dusp_state_download returns DUSP_ERR_STATE until the next plain render. */
int dusp_render_host_mix(dusp_program *prog, size_t n_instances, size_t n_samples, const float *h_params, const float *h_gains,
                         size_t tile_instances, int format, int normalise, void *h_out, float *h_peak);

/* A score: voices mixed at per-voice onsets into a timeline that is longer than a voice, on the device, in Sum.many's chain order
 * (additions to ABI v7: DUSP_ABI_VERSION is unchanged, a binder detects them by symbol).  Replaces
 * `Sum.many(voices.map((v, k) => new Delay(v, onset_k, maxDelay)))` as the thing that places rendered notes on a timeline: a Delay by
 * a whole number of samples is its input behind zeros (src/components/Delay.js:27-38), and the Sum chain adds in index order with one
 * f32 rounding per add.  Voice k covers the timeline samples onset_k .. onset_k + len_k - 1; for every channel c and timeline sample t
 *     acc = d_init ? d_init[c][t] : +0
 *     for k = 0 .. n_instances - 1:   s = t - onset_k;   if (0 <= s < len_k)  acc = (float)(acc + term_k)
 *     term_k = d_gains ? (float)(d_planar[k][c][s] * g_k) : d_planar[k][c][s]      (a plain f32 product, then a plain f32 add)
 *     d_out[c][t] = raw ? acc : (acc || 0)
 * A voice takes no part in a sample outside its span: nothing is added there, not even a zero.  A raw partial sum continued through
 * d_init is therefore the same chain wherever it is cut: tiles of voices, windows of the timeline (with the onsets shifted, negative
 * ones included), other devices.  Unlike dusp_mix_device's, the chain starts from +0 and NOT from the first voice itself: a -0 sample
 * alone on a raw timeline sample gives +0.  (Against zero-padded rows under dusp_mix_device that is the only difference, and none
 * after `|| 0`.)
 *   d_planar          f32 [n_instances][n_channels][n_voice_samples], as the render calls write it
 *   h_onsets          int64 [n_instances], in samples, any sign: a negative onset is a voice that began before the timeline.  HOST memory:
 *                     the launch's plan (which voices a block of the timeline looks at) is made on the host, and both arrays have been
 *                     read when the call returns
 *   h_lengths         int64 [n_instances], 0 <= len_k <= n_voice_samples, HOST memory; NULL: every voice counts whole
 *   d_gains           f32 [n_instances], or NULL
 *   d_init, d_out     f32 [n_channels][n_total_samples]; d_init may be NULL, and may be d_out (in place); d_planar must not overlap d_out
 *   raw               as for dusp_mix_device
 * n_instances = 0 is legal: the `|| 0` pass (or, raw, a copy) over d_init alone.  Any 4-byte alignment, any sizes with
 * n_channels * n_total_samples and n_channels * n_voice_samples at most 2^31; coalesced dword accesses.  DUSP_ERR_ARG, with a message,
 * for NULL or misaligned buffers, sizes out of range and a length outside 0 .. n_voice_samples.  The plan is uploaded into a buffer
 * that lives with the context and the launch is asynchronous on `stream`; a call may wait for the previous call's plan to have been
 * uploaded.  The NaN divergence of dusp_mix_device applies unchanged; and an infinite voice sample stays infinite here, where the
 * reference's Delay makes NaN of it (inf * 0 in its second tap). */
int dusp_score_device(dusp_ctx *ctx, const float *d_planar, size_t n_instances, size_t n_channels, size_t n_voice_samples,
                      const int64_t *h_onsets, const int64_t *h_lengths, const float *d_gains, size_t n_total_samples,
                      const float *d_init, int raw, float *d_out, void *stream);

/* Where the most recent dusp_score_device call on this context spent its time (synchronises with that launch): the kernel alone, by
 * HIP events around the launch on its stream; the plan on the host's clock (made before the call returned); and the plan's upload, by
 * events around the copy (0 when no voice reached the timeline: nothing was uploaded).  Any pointer may be NULL.  DUSP_ERR_STATE
 * before the first dusp_score_device call.  Not for two threads at once on one context, like every call on a context. */
int dusp_score_last_ms(dusp_ctx *ctx, float *kernel_ms, float *plan_ms, float *upload_ms);

/* Render n_instances instances for n_voice_samples each and deliver their score over n_total_samples: the instances are rendered tile
 * by tile, in voice order, exactly as dusp_render_host_mix renders its tiles (the same whole-batch decisions keep the tiling from
 * changing a bit), and every tile continues the chain above, raw and in place, in one [n_out_channels][n_total_samples] accumulator
 * that was zeroed once — over the union window of the tile's voices only, so a tile of notes bunched in time does not stream the whole
 * timeline; a last launch without voices applies `|| 0`.  Device memory is the tile plus the timeline plus the call's plans: all tiles'
 * plans are made up front and share ONE 16 MiB budget (a tile whose lists exceed its share takes larger blocks), beyond which only 28
 * bytes a voice and 40 a tile remain.
 *   h_params, h_gains, format, normalise, h_peak   as for dusp_render_host_mix
 *   h_onsets, h_lengths                            as for dusp_score_device
 *   tile_instances  instances per tile; 0: dusp_render_host_mix's default, sized over a voice's row
 *   h_out           planar f32 [n_out_channels][n_total_samples], or the frames of the PCM format
 * Refusals and the state afterwards are dusp_render_host_mix's. */
int dusp_render_host_score(dusp_program *prog, size_t n_instances, size_t n_voice_samples, size_t n_total_samples, const float *h_params,
                           const float *h_gains, const int64_t *h_onsets, const int64_t *h_lengths, size_t tile_instances, int format,
                           int normalise, void *h_out, float *h_peak);

/* The score's chain over voices that each lie in a buffer of their own (additions to ABI v7, detected by symbol): voice k is planar f32
 * [n_channels][h_row_samples[k]] at the DEVICE address h_rows[k] — rows of any length, rendered by any program — and
 *   out[c][t] = acc || 0,  acc = init ? init[c][t] : +0;  for k in index order: s = t - onset_k;
 *                                                           if (0 <= s < len_k) acc = f32(acc + term_k)
 * with term_k = d_gains ? f32(row_k[c][s] * g_k) : row_k[c][s]: dusp_score_device's chain word for word (dusp_amd/mix.py
 * score_chain_rows is the contract in numpy), so that a piece of several instruments, each rendered for its own note length, is ONE chain
 * over the caller's voice list, in its index order, however the instruments interleave.
 *   h_rows, h_row_samples   HOST arrays [n_voices]: the rows' device addresses (4-byte aligned; ignored, and may be NULL, where
 *                           h_row_samples[k] is 0) and their samples per channel; n_channels * h_row_samples[k] <= 2^31
 *   h_lengths               HOST array, 0 <= len_k <= h_row_samples[k], or NULL for the whole rows
 *   everything else         as dusp_score_device: asynchronous on `stream`, the plan in the context's plan buffer, n_voices = 0 legal,
 *                           d_init may be d_out, dusp_score_last_ms reports the call
 * The rows must stay as they are until the launch has run.  DUSP_ERR_ARG, with a message, for a NULL or misaligned row of a voice that
 * has samples, a length outside its row, a row beyond 2^31 floats, and dusp_score_device's timeline limits. */
int dusp_score_rows_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices, size_t n_channels,
                           const int64_t *h_onsets, const int64_t *h_lengths, const float *d_gains, size_t n_total_samples,
                           const float *d_init, int raw, float *d_out, void *stream);

/* A piece of several instruments: part p is a program, rendered for n_voice_samples per instance with the slot-major parameter table
 * h_params [n_params][n_instances].  Voice k of the chain is the NEXT UNUSED instance of part h_part_of[k]: a part's instances enter the
 * chain in their own order, parts may interleave freely (notes in time order, say), and h_part_of must name part p exactly
 * parts[p].n_instances times.  The result is dusp_score_rows_device's chain over what each program renders, bit for bit whatever the
 * tiles.  A tile is a run of the chain's voices whose rows together fit tile_bytes (0: a default derived as dusp_render_host_mix
 * derives its own, over bytes); a part's share of a tile is one contiguous instance range, rendered as one batch by that part's program
 * — with what changes bits decided from the WHOLE part, as dusp_render_host_mix decides it — and skipped where none of its voices in
 * the tile reaches the timeline; then one raw launch continues the timeline in place over the tile's union window.  All tiles' plans
 * are made up front under the one 16 MiB budget.  Device memory: one tile buffer per part, the timeline, the plans, 4 bytes a voice
 * for the gains.
 *   h_onsets, h_lengths, h_gains   [n_voices], in chain order; lengths within the voice's own part's n_voice_samples
 *   format, normalise, h_out, h_peak   as for dusp_render_host_score
 * Refused with a message: programs of different contexts or output channel counts, a program listed twice (its tile buffer would be
 * used twice), and what dusp_render_host_score refuses of any one part.  The state afterwards is dusp_render_host_mix's, for every part. */
typedef struct {
    dusp_program *prog;
    size_t n_instances;
    size_t n_voice_samples;
    const float *h_params;
} dusp_score_part;
int dusp_render_host_score_parts(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                 const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains, size_t n_total_samples,
                                 size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak);

/* Stereo placement: dusp_score_rows_device over MONO rows, every voice panned where it is added to a timeline of TWO channels
 * (additions to ABI v7, detected by symbol).  A pan that is constant over a note is a property of the placement, not of the voice; this
 * is the reference's Pan unit (src/components/Pan.js:19-25) behind every voice, without the voice becoming a two-channel circuit:
 *     accL, accR = d_init ? d_init[0][t], d_init[1][t] : +0, +0
 *     for k in index order:  s = t - onset_k;  if (0 <= s < len_k):
 *         x    = d_gains ? f32(row_k[s] * g_k) : row_k[s]
 *         accL = f32(accL + f32(((f64(x) * (1 - f64(p_k))) / 2) * comp_k))
 *         accR = f32(accR + f32(((f64(x) * (1 + f64(p_k))) / 2) * comp_k))
 *     d_out[0][t], d_out[1][t] = raw ? acc : (acc || 0)
 * every f64 operation rounded by itself (dusp_amd/mix.py score_chain_rows_panned is the contract in numpy).  Skipped adds, clipped
 * lengths, onsets of any sign, raw partial sums continued through d_init and windows of the timeline are dusp_score_rows_device's.
 *   h_rows, h_row_samples   as dusp_score_rows_device, with n_channels = 1
 *   h_pans                  f32 [n_voices], HOST memory, finite; NOT clamped to [-1, 1] (the reference does not clamp either)
 *   h_comp                  f64 [n_voices], HOST memory: comp_k.  NULL: pow(10, ((1 - |p_k|) * 1.5) / 20) by the host's pow.  The
 *                           reference computes it with the JavaScript engine's Math.pow: a JavaScript binder passes those values, so
 *                           that under Node the result is the reference's own bits
 *   d_init, d_out           f32 [2][n_total_samples], 2 * n_total_samples <= 2^31; d_init may be NULL, and may be d_out
 * The voices' coefficients (1 - p, 1 + p and comp / 2 as doubles, 32 bytes a voice) go up with the plan; dusp_score_last_ms reports
 * this call too.  DUSP_ERR_ARG, with a message, for a pan that is not finite, a comp that is NaN, and everything
 * dusp_score_rows_device refuses. */
int dusp_score_rows_pan_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices,
                               const int64_t *h_onsets, const int64_t *h_lengths, const float *d_gains, const float *h_pans,
                               const double *h_comp, size_t n_total_samples, const float *d_init, int raw, float *d_out, void *stream);

/* dusp_render_host_score_parts with a pan per voice: every part's circuit has ONE output channel (refused by message otherwise, before
 * any render), the tiles' launches are dusp_score_rows_pan_device's, and the timeline, its `|| 0`, its peak and its PCM frames have two
 * channels.  Tiles are by bytes as before: mono rows, so twice the voices of a panned two-channel circuit fit a tile.
 *   h_pans, h_comp   [n_voices], in chain order, as for dusp_score_rows_pan_device
 *   h_out            planar f32 [2][n_total_samples], or the two-channel frames of the PCM format
 * Everything else, refusals included, is dusp_render_host_score_parts'. */
int dusp_render_host_score_parts_pan(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                     const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains, const float *h_pans,
                                     const double *h_comp, size_t n_total_samples, size_t tile_bytes, int format, int normalise,
                                     void *h_out, float *h_peak);

/* Sub-sample onsets: dusp_score_rows_device and dusp_score_rows_pan_device with voice k starting at onset_k + frac_k samples,
 * 0 <= frac_k < 1 (additions to ABI v7, detected by symbol).  The reference's Delay takes any delay (src/components/Delay.js:36-38): it
 * writes every input sample to two neighbouring ring slots with the weights 1 - frac and frac.  Write x[s] for voice k's sample s after
 * the gain — f32(row_k[c][s] * g_k), or row_k[c][s]; with h_pans the Pan unit's f32 output per channel, as dusp_score_rows_pan_device
 * forms it — and len for its length.
 *   frac_k == 0: the voice is exactly dusp_score_rows_device's: span onset_k .. onset_k + len - 1, term x[s].  A call whose fractions
 *                are all zero (or h_fracs NULL) launches the kernels of those calls and gives their bits.
 *   frac_k != 0: w1 = frac_k, w0 = 1.0 - frac_k (one f64 subtraction); the voice covers the len + 1 samples onset_k .. onset_k + len,
 *                and with s = t - onset_k
 *                    c(s)      = f32(f64(x[s-1]) * w1)                 1 <= s <= len
 *                    term(0)   = f32(f64(x[0]) * w0)
 *                    term(s)   = f32(f64(c(s)) + f64(x[s]) * w0)       1 <= s <  len   (every f64 operation rounded by itself: no FMA)
 *                    term(len) = c(len)
 *                    acc       = f32(acc + term(s))                                    (in voice index order)
 *                A voice of length 0 takes no part.
 * Everything else — the skipped add outside the span, d_init, raw, `acc || 0`, lengths clipped in int64, onsets at the int64 limits,
 * windows of the timeline as the same chain with onset_k - lo — is dusp_score_rows_device's (dusp_amd/mix.py score_chain_rows and
 * score_chain_rows_panned with fracs are the contract in numpy).
 * It is what the reference renders for Sum.many(Delay(Pan(Multiply(v_k, g_k), p_k), onset_k + frac_k, maxDelay)), within three limits:
 *   1. the reference's ring drops a ceil tap that lands on ring index maxDelay, once per trip round the ring: a quirk of the ring, not
 *      of the placement, not reproduced (the reference agrees where maxDelay > timeline + largest onset + 2);
 *   2. a delay in (0, 1) puts the floor tap into the slot the unit has just read, so that it is heard a whole ring later: not
 *      reproduced (the reference agrees where onset_k >= 1);
 *   3. the reference rounds an inlet constant to f32: it agrees where onset_k + frac_k is an f32; elsewhere this call is more exact,
 *      since the fraction stays a double.
 *   h_fracs   f64 [n_voices], HOST memory, finite, in [0, 1); NULL: all zero
 *   h_pans    NULL: rows of n_channels into a timeline of n_channels, as dusp_score_rows_device.  Else n_channels must be 1 and the
 *             timeline has two channels, as dusp_score_rows_pan_device; h_comp as there
 * The voices' weights (w0 and w1 as doubles, 16 bytes a voice) go up with the plan, on top of the plan's byte budget, which counts
 * records and lists as before; dusp_score_last_ms reports this call too.  DUSP_ERR_ARG, with a message ("the fraction of voice k is
 * not finite", "... is outside [0, 1)"), checked before anything is launched, and for everything the calls without fractions refuse. */
int dusp_score_rows_frac_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices,
                                size_t n_channels, const int64_t *h_onsets, const double *h_fracs, const int64_t *h_lengths,
                                const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples,
                                const float *d_init, int raw, float *d_out, void *stream);

/* dusp_render_host_score_parts (h_pans NULL) or dusp_render_host_score_parts_pan with a fraction of a sample per voice: a tile one of
 * whose voices has a fraction is dusp_score_rows_frac_device's launch, the others are launched as before.  The fractions are checked
 * before anything is rendered.
 *   h_fracs   f64 [n_voices], in chain order, as for dusp_score_rows_frac_device; NULL: all zero
 * Everything else, refusals included, is dusp_render_host_score_parts[_pan]'s. */
int dusp_render_host_score_parts_frac(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                      const int64_t *h_onsets, const double *h_fracs, const int64_t *h_lengths, const float *h_gains,
                                      const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes, int format,
                                      int normalise, void *h_out, float *h_peak);

/* Space placement: dusp_score_rows_device over MONO rows, voice k heard by each of n_speakers speakers — the timeline's channels —
 * through a gain G_kc and a delay of D_kc samples of its own (additions to ABI v7, detected by symbol).  It is the reference's
 * SpaceChannel (src/patches/SpaceChannel.js) behind a sound, a Gain in front of a MonoDelay, done where the voice is added to the
 * timeline.  From a tap's delay the host makes i = floor(D), fr = D - i (exact in f64), w1 = fr, w0 = 1.0 - fr.  With x[s] voice k's
 * sample after the per-voice gain — f32(row_k[s] * g_k), or row_k[s] — and len its length, channel c takes
 *     y[s]      = f32(G_kc * f64(x[s]))                        (Gain.js:22: one f64 product, one rounding)
 *     fr == 0:    term(s) = y[s], 0 <= s < len, at timeline sample t = onset_k + i + s
 *     fr != 0:    dusp_score_rows_frac_device's four lines with x := y and onset := onset_k + i: the voice covers len + 1 samples
 *     acc_c     = f32(acc_c + term)                            (per channel, in voice index order; no add where the voice does not cover t)
 * Everything else — d_init, raw, `acc || 0`, a voice of length 0, clipping to the timeline, windows as the same chain with
 * onset_k - lo — is dusp_score_rows_device's (dusp_amd/mix.py score_chain_rows_placed is the contract in numpy).  onset_k + i is formed
 * in int64 without wrapping: a voice whose shifted span leaves int64 takes no part.
 * Channel c is what the reference renders for the ONE-channel circuit
 *     Sum.many(k -> MonoDelay(Gain(Delay(Multiply(v_k, g_k), onset_k, ring), dB_kc), D_kc))       with G_kc = pow(10, dB_kc / 20)
 * (a voice at onset 0 without its Delay, a tap of delay 0 without its MonoDelay), where D_kc is an f32 (the reference rounds an inlet
 * constant to f32; elsewhere this call is more exact) and the samples are finite (with fr == 0 the reference forms y + y * 0, which is
 * NaN for an infinite y; this call keeps y).  The reference's ConcatChannels hears its second inlet one chunk late; that lag is not
 * reproduced, which is why the anchor is taken channel by channel.
 *   n_speakers   1 .. 8; n_speakers * n_total_samples <= 2^31
 *   h_delays     f64 [n_voices][n_speakers], HOST memory, finite, in [0, 2^24]
 *   h_tap_gains  f64 [n_voices][n_speakers], HOST memory, finite
 *   d_init, d_out  f32 [n_speakers][n_total_samples]
 * The taps (32 bytes a voice and speaker) go up with the plan, on top of the plan's byte budget; dusp_score_last_ms reports this call
 * too.  DUSP_ERR_ARG, with a message that names the voice and the speaker, checked before anything is launched: NULL taps, n_speakers
 * outside 1 .. 8, a delay that is not finite or outside [0, 2^24], a gain that is not finite, n_speakers * n_total_samples > 2^31; and
 * for everything dusp_score_rows_device refuses. */
int dusp_score_rows_space_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices,
                                 size_t n_speakers, const int64_t *h_onsets, const int64_t *h_lengths, const float *d_gains,
                                 const double *h_delays, const double *h_tap_gains, size_t n_total_samples, const float *d_init, int raw,
                                 float *d_out, void *stream);

/* dusp_render_host_score_parts over MONO parts placed in a space: every tile is dusp_score_rows_space_device's launch and the result
 * has n_speakers channels.  The taps are per voice in chain order and checked before anything is rendered; a part that is not mono is
 * refused.  Everything else, refusals included, is dusp_render_host_score_parts'. */
int dusp_render_host_score_parts_space(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                       const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains, size_t n_speakers,
                                       const double *h_delays, const double *h_tap_gains, size_t n_total_samples, size_t tile_bytes,
                                       int format, int normalise, void *h_out, float *h_peak);

/* Stereo pieces: voices of one and of two channels side by side in a timeline of two, a mono voice panned or not (additions to ABI v7,
 * detected by symbol).  The kind of a voice is the voice's own: with x_c[s] = f32(row_k[c][s] * g_k), or row_k[c][s], voice k adds
 *     a mono row, h_pans[k] finite:  f32(((f64(x_0) * (1 - f64(p))) / 2) * comp_k) left, the same with 1 + f64(p) right
 *                                    (dusp_score_rows_pan_device's term)
 *     a mono row, h_pans[k] NaN:     x_0 left, x_0 right     (the reference's Sum reads a[channel % a.length]: Sum.js:34-38)
 *     a row of two channels:         x_0 left, x_1 right     (h_pans[k] must be NaN: the Pan unit's inlet is mono, Pan.js:6)
 * by acc = f32(acc + term) per channel in voice index order; with h_fracs, dusp_score_rows_frac_device's two taps are applied per
 * channel to those values.  Everything else is dusp_score_rows_device's (dusp_amd/mix.py score_chain_rows_stereo is the contract in
 * numpy).  It is what the reference renders for Sum.many(k -> Delay(P_k, onset_k + frac_k, maxDelay)), P_k = Pan(Multiply(v_k, g_k),
 * p_k) for a panned voice and Multiply(v_k, g_k), of one or two channels, otherwise — within dusp_score_rows_frac_device's three
 * limits where there are fractions.  All voices mono and panned gives dusp_score_rows_pan_device's bits, all voices of two channels
 * dusp_score_rows_device's.
 *   h_rows          device addresses; row k is planar f32 [h_row_channels[k]][h_row_samples[k]]
 *   h_row_channels  u32 [n_voices], HOST memory, 1 or 2
 *   h_fracs         as dusp_score_rows_frac_device's, or NULL.  A call none of whose listed voices has a fraction launches the kernel
 *                   without the two-tap form
 *   h_pans          f32 [n_voices], HOST memory; NaN: not placed.  h_comp as dusp_score_rows_pan_device's (an unplaced voice's is not read)
 *   d_init, d_out   f32 [2][n_total_samples]; n_total_samples <= 2^30
 * dusp_score_last_ms reports this call too.  DUSP_ERR_ARG, with a message that names the voice, checked before anything is launched:
 * NULL h_pans or h_row_channels, a channel count that is neither 1 nor 2, an infinite pan, a voice of two channels whose pan is not
 * NaN; and for everything dusp_score_rows_frac_device refuses. */
int dusp_score_rows_stereo_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, const uint32_t *h_row_channels,
                                  size_t n_voices, const int64_t *h_onsets, const double *h_fracs, const int64_t *h_lengths,
                                  const float *d_gains, const float *h_pans, const double *h_comp, size_t n_total_samples,
                                  const float *d_init, int raw, float *d_out, void *stream);

/* dusp_render_host_score_parts over parts of ONE OR TWO output channels into a timeline of two: every tile is
 * dusp_score_rows_stereo_device's launch, and a tile's rows take the bytes of their part's own channel count.  h_pans (never NULL) and
 * h_fracs (or NULL) are per voice in chain order and checked before anything is rendered, as is every part's channel count ("part p
 * has N output channels: a voice of a stereo piece has one or two").  Everything else, refusals included, is
 * dusp_render_host_score_parts_frac's. */
int dusp_render_host_score_parts_stereo(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                        const int64_t *h_onsets, const double *h_fracs, const int64_t *h_lengths, const float *h_gains,
                                        const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes, int format,
                                        int normalise, void *h_out, float *h_peak);

/* Master bus: the mix of a piece through a circuit, on the device (additions to ABI v7, detected by symbol).
 * dusp_render_host_score_piece is ONE entry for every placement — the five dusp_render_host_score_parts* calls above are this call
 * with the matching dusp_score_placement and no master, bit for bit and refusal for refusal (under this entry's name) — and the only one
 * that takes a master.
 *
 * A MASTER is a program with exactly one input stream (opcode INPUT, stream 0) and one output channel, built on the parts' context.
 * It is applied to every channel of the timeline by itself: channel c is instance c of the master, so its slot-major parameter table
 * is h_params [n_params][timeline channels] (an echo of 300.25 samples left and 411.5 right is one program with one parameter).
 * After the last tile the timeline's RAW running sums — no `|| 0`: in the reference a unit behind a Sum hears the Sum's own values,
 * and `|| 0` is applied at renderChannelData's copy-out only — are the master's input block as they stand ([1 stream][C instances]
 * [n_total_samples]: no copy, no transpose), the master is rendered over n_total_samples from its initial state, its own copy-out
 * applies `|| 0`, and the delivery (planar f32, or peak and encoded frames) is taken from the master's buffer:
 *     h_out = render(master, n_instances = C, n_samples = n_total_samples, input 0 of instance c = raw timeline channel c)
 * The master render decides as a tile of dusp_render_host_mix decides: it waits for its compiled kernel (two calls give the same
 * bits), and what changes bits is decided from its whole parameter table.  A stateless master is cut into time segments as any
 * render is; segments that warm up stay refused for programs with inputs, so a Filter master runs as one chain per channel.
 * Device memory: one more f32 [C][n_total_samples] (the master's output) beside the timeline.
 * The documented divergences of the chain (a NaN voice sample, Inf, the sign of a zero) reach the master unchanged.
 *   placement   NULL: plain rows.  Else its kind and the arrays of that kind, per voice in chain order, as the matching
 *               dusp_render_host_score_parts* call takes them (h_fracs with ROWS, PAN and STEREO; NULL: none)
 *   master      NULL: no master, the call is the matching dusp_render_host_score_parts* call.
 * Refused with a message before anything renders, beside what those calls refuse: a master with no input stream or more than one;
 * with more than one output channel; a resumable master; a master built on another context; a master that is also one of the parts;
 * NULL h_params where the master has parameters; C x n_total_samples beyond 2^31.  Afterwards the master's state is a mix's
 * (dusp_state_download refuses), like every part's. */
typedef enum { DUSP_PLACE_ROWS = 0, DUSP_PLACE_PAN = 1, DUSP_PLACE_SPACE = 2, DUSP_PLACE_STEREO = 3 } dusp_score_place_kind;
typedef struct dusp_score_placement {
    int kind;                    /* dusp_score_place_kind */
    const double *h_fracs;       /* ROWS, PAN, STEREO: f64 [n_voices] in [0, 1), or NULL */
    const float *h_pans;         /* PAN: finite f32 [n_voices].  STEREO: NaN for a voice that is not placed */
    const double *h_comp;        /* PAN, STEREO: f64 [n_voices], or NULL for the host's pow */
    size_t n_speakers;           /* SPACE: 1 .. 8 */
    const double *h_delays;      /* SPACE: f64 [n_voices][n_speakers] */
    const double *h_tap_gains;   /* SPACE: f64 [n_voices][n_speakers] */
} dusp_score_placement;
typedef struct dusp_score_master {
    dusp_program *prog;
    const float *h_params; /* f32 [n_params][timeline channels] or NULL */
} dusp_score_master;
int dusp_render_host_score_piece(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                 const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                 const dusp_score_placement *placement, const dusp_score_master *master, size_t n_total_samples,
                                 size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak);

/* Effect sends: per-voice send levels into bus circuits, on the device (additions to ABI v7, detected by symbol; DESIGN.md 6.15;
 * dusp_amd/mix.py score_chain_sends, master_chain and bus_return are the contract).
 *
 * A BUS is what a master is — a program with one input stream and one output channel on the parts' context, instance c of it for
 * channel c of the timeline, h_params [n_params][timeline channels] — and a call has 1 .. 4 of them.  h_sends[b][k] is what voice k
 * gives to bus b, a finite f32.  Beside the dry chain, which is untouched, every tile's launch (score_send_engine.hip: the voice's row
 * is read once) keeps one send timeline a bus:
 *     send_b[c][t] = +0; for k in chain order, where voice k covers t: send_b = f32(send_b + f32(dry_term_k[c][t] * h_sends[b][k]))
 * dry_term being the very f32 the dry chain adds (the row's sample, f32(row * g_k), or the Pan unit's two values: a send is post-fader
 * and post-pan), the product and the add plain f32 operations.  EVERY voice is in EVERY bus's chain: a level of 0 is a multiplication
 * by 0, so NaN * 0 poisons the bus and -x * 0 is -0.  After the last tile each bus is rendered over its RAW send timeline from its
 * initial state, as a master is over the mix (`|| 0` at its own copy-out), and one launch returns them:
 *     mix = f32(...f32(f32(dry + wet_0) + wet_1)... + wet_{B-1})      (Sum.many([dry, wet_0, ...]): left-deep, one rounding an add)
 * delivered as `mix || 0`, or handed raw to the master, which works as in dusp_render_host_score_piece.  Where a bus's output is NaN
 * its copy-out has made it 0 and the dry sample survives (the reference's final Sum would give NaN, delivered as 0).
 * Device memory: B send timelines and B bus outputs of f32 [C][n_total_samples], beside the timeline (and the master's output).
 *   buses   NULL: no buses, the call is dusp_render_host_score_piece (under this entry's name).
 * Refused with a message before anything renders, beside what that call refuses: every rule of a master, per bus ("bus b"); a bus
 * that is also a part, the master or another bus; n_buses outside 1 .. 4; NULL h_sends; a level that is not finite (bus and voice
 * named); h_fracs, DUSP_PLACE_SPACE or DUSP_PLACE_STEREO together with buses (DUSP_ERR_UNSUPPORTED). */
typedef struct dusp_score_buses {
    size_t n_buses;                 /* 1 .. 4 */
    const dusp_score_master *buses; /* [n_buses] */
    const float *h_sends;           /* f32 [n_buses][n_voices], HOST memory, finite */
} dusp_score_buses;
int dusp_render_host_score_piece_buses(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                       const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                       const dusp_score_placement *placement, const dusp_score_buses *buses,
                                       const dusp_score_master *master, size_t n_total_samples, size_t tile_bytes, int format,
                                       int normalise, void *h_out, float *h_peak);
/* The send chain alone: dusp_score_rows_device (h_pans NULL; rows of n_channels) or dusp_score_rows_pan_device (h_pans; n_channels
 * must be 1, the timelines have two channels) with n_buses send timelines beside the dry one.  h_sends: f32 [n_buses][n_voices], HOST
 * memory.  d_send_init (NULL: +0) and d_send_out: f32 [n_buses][C][n_total_samples], always raw; d_send_init may be d_send_out as
 * d_init may be d_out.  The levels (16 bytes a voice) go up with the plan, on top of its byte budget; dusp_score_last_ms reports this
 * call too.  Refused as dusp_score_rows_device refuses, and: n_buses outside 1 .. 4, NULL h_sends, a level that is not finite. */
int dusp_score_rows_send_device(dusp_ctx *ctx, const float *const *h_rows, const uint32_t *h_row_samples, size_t n_voices,
                                size_t n_channels, const int64_t *h_onsets, const int64_t *h_lengths, const float *d_gains,
                                const float *h_pans, const double *h_comp, size_t n_buses, const float *h_sends,
                                size_t n_total_samples, const float *d_init, int raw, float *d_out, const float *d_send_init,
                                float *d_send_out, void *stream);
/* The return of the buses alone: d_out[j] = f32(...f32(d_dry[j] + h_wets[0][j])... + h_wets[n_buses - 1][j]) over n_floats floats
 * (1 .. 2^31), `|| 0` unless raw.  h_wets: a HOST array of n_buses device addresses.  d_out may be d_dry.  Four floats a lane where
 * every buffer is on a 16-byte boundary, one a lane otherwise.  dusp_score_last_ms reports this call too. */
int dusp_score_return_device(dusp_ctx *ctx, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw,
                             float *d_out, void *stream);

/* Tracks: sub-mixes of a piece through insert circuits, on the device (additions to ABI v7, detected by symbol; DESIGN.md 6.16;
 * dusp_amd/mix.py track_mix is the contract).
 *
 * Voice k goes to track h_track_of[k] (0 .. n_tracks - 1) or, with -1, straight to the mix.  Every destination that has voices is the
 * chain of today's placement over ITS voices, in index order, raw, in a timeline of its own [C][n_total_samples]; a track without
 * voices hears zeros.  A TRACK PROGRAM is what a master is, and serves the tracks listed in h_tracks, which have isomorphic circuits:
 * its instances are (track, channel), instance j * C + c the circuit of track h_tracks[j] over channel c of that track's timeline,
 * h_params [n_params][n_tracks x C] one column an instance.  It is rendered ONCE, from its initial state, over its tracks' raw
 * timelines (`|| 0` at its own copy-out).  A track that no program lists has no circuit — a fader group — and its output is its raw
 * timeline.  Then one launch (score_tracks_engine.hip) mixes:
 *     term_g = h_faders ? f32(y_g * h_faders[g]) : y_g
 *     mix    = direct; for g in order: mix = f32(mix + term_g)                                   (left-deep, one rounding an add)
 *     feed_b = +0;     for g in order: feed_b = f32(feed_b + f32(term_g * h_track_sends[b][g]))   (with buses: every track is in every
 *                                                                                                   bus's chain, a level of 0 included)
 * and the call goes on as dusp_render_host_score_piece_buses does behind its last tile: every bus rendered over its feed, the return,
 * the master, the delivery.  With tracks the buses' h_sends must be NULL: the levels are h_track_sends.
 * Device memory on top of that call's: n_tracks timelines and the track programs' outputs, f32 [C][n_total_samples] each.
 *   tracks   NULL: the call is dusp_render_host_score_piece_buses (under this entry's name).
 * Refused with a message before anything renders, beside what that call refuses: n_tracks outside 1 .. 8; NULL h_track_of; an entry of
 * h_track_of outside -1 .. n_tracks - 1 (the voice named); a fader that is not finite (the track named); h_track_sends without buses,
 * buses without h_track_sends, buses with h_sends; a level that is not finite (bus and track named); every rule of a master, per
 * program ("track program p"); a track program that is also a part, a bus, the master or another track program; a program that lists
 * no track, a track out of range, or a track that another program (or itself) lists already; (tracks x channels) x timeline samples of
 * a program above 2^31 floats. */
typedef struct dusp_score_track_program {
    dusp_program *prog;       /* one input stream, one output channel, on the parts' context */
    size_t n_tracks;          /* how many tracks it serves, >= 1 */
    const uint32_t *h_tracks; /* [n_tracks]: which, each 0 .. the call's n_tracks - 1 */
    const float *h_params;    /* [n_params][n_tracks x timeline channels], HOST memory; NULL without parameters */
} dusp_score_track_program;
typedef struct dusp_score_tracks {
    size_t n_tracks;                          /* 1 .. 8 */
    const int32_t *h_track_of;                /* [n_voices]: -1 (straight to the mix) .. n_tracks - 1 */
    size_t n_programs;                        /* 0 .. n_tracks */
    const dusp_score_track_program *programs; /* [n_programs] */
    const float *h_faders;                    /* f32 [n_tracks], finite; NULL: none */
    const float *h_track_sends;               /* f32 [n_buses][n_tracks], finite; NULL exactly when the call has no buses */
} dusp_score_tracks;
int dusp_render_host_score_piece_tracks(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                        const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                        const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                        const dusp_score_buses *buses, const dusp_score_master *master, size_t n_total_samples,
                                        size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak);
/* The mix of the tracks alone, over flat buffers of n_floats floats (1 .. 2^31): d_out[j] = d_direct[j] + term_0[j] + ... as above,
 * `|| 0` unless raw, and d_feed_out[b][j] = (d_feed_init ? d_feed_init[b][j] : +0) + f32(term_0[j] * h_levels[b][0]) + ..., always raw.
 * h_tracks: a HOST array of n_tracks (1 .. 8) device addresses; h_faders: f32 [n_tracks] or NULL; h_levels: f32 [n_buses][n_tracks],
 * n_buses 0 .. 4 (0: no feeds; the three feed arguments are ignored); the feeds are f32 [n_buses][n_floats].  d_out may be d_direct,
 * d_feed_out may be d_feed_init.  Four floats a lane where every buffer (each feed included) is on a 16-byte boundary, one a lane
 * otherwise.  dusp_score_last_ms reports this call too. */
int dusp_score_tracks_mix_device(dusp_ctx *ctx, const float *d_direct, const float *const *h_tracks, size_t n_tracks,
                                 const float *h_faders, size_t n_buses, const float *h_levels, size_t n_floats, int raw, float *d_out,
                                 const float *d_feed_init, float *d_feed_out, void *stream);

/* Stems: the direct mix, every track and every bus return beside the mix, in the call's one delivery (additions to ABI v7, detected by
 * symbol; dusp_amd/mix.py stems is the contract).  With T tracks (0 without `tracks`) and B buses (0 without `buses`)
 * a call with stems delivers S + 1 = 1 + T + B + 1 signals of [C][n_total] f32, in this order:
 *     0            direct   direct || 0: with tracks the raw chain over the voices that go straight to the mix, else the raw dry chain
 *     1 .. T       track g  term_g || 0, term_g = faders ? f32(y_g * f_g) : y_g as the mix of the tracks forms it
 *     T+1 .. T+B   bus b    the bus's output as its own copy-out left it
 *     S            mix      the call's output exactly as without stems (behind the master where there is one; the stems are in front)
 * `|| 0`: NaN and -0 leave as +0.  Without a master and without NaN in the raw signals the first S, added left-deep in f32, `|| 0`, are
 * the mix bit for bit.  h_out: n_signals instances of what the call delivers without stems (planar f32 [C][n_total], or frames
 * [n_total][C] of `format`).  With normalise 1 or 2 ALL signals get the gain of the largest of their peaks, so delivered stems still
 * add up to the delivered mix; normalise 0 is the quantiser a signal.  h_peaks (f32 [n_signals] or NULL): every signal's own peak,
 * whatever the format, planar f32 included.  The signals take n_signals x C x n_total floats of device memory on top of the call's,
 * and as much staging for encoded frames.
 * stems NULL: dusp_render_host_score_piece_tracks under this entry's name.  Refused before anything renders, on top of that entry's
 * refusals: n_signals that is not 1 + n_tracks + n_buses + 1 (both numbers named), h_out NULL, n_signals x C x n_total beyond 2^31. */
typedef struct dusp_score_stems {
    size_t n_signals; /* must be 1 + n_tracks + n_buses + 1: the caller has sized h_out and h_peaks */
} dusp_score_stems;
int dusp_render_host_score_piece_stems(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                       const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                       const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                       const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems,
                                       size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peaks);
/* dusp_score_tracks_mix_device with n_tracks 0 .. 8, which also writes d_stems, f32 [1 + n_tracks][n_floats]: slot 0 = d_direct || 0,
 * slot 1 + g = term_g || 0.  d_stems aliases no other buffer; the wide path needs every slot on a 16-byte boundary too. */
int dusp_score_stems_mix_device(dusp_ctx *ctx, const float *d_direct, const float *const *h_tracks, size_t n_tracks,
                                const float *h_faders, size_t n_buses, const float *h_levels, size_t n_floats, int raw, float *d_out,
                                const float *d_feed_init, float *d_feed_out, float *d_stems, void *stream);
/* dusp_score_return_device which also copies wet b into d_stem_buses + b * n_floats (f32 [n_buses][n_floats]) and, d_stem_direct
 * given, writes d_dry || 0 there.  The slots alias no other buffer. */
int dusp_score_stems_return_device(dusp_ctx *ctx, const float *d_dry, const float *const *h_wets, size_t n_buses, size_t n_floats, int raw,
                                   float *d_out, float *d_stem_direct, float *d_stem_buses, void *stream);
/* d_common[i] = the largest of d_peaks[0 .. n_peaks) for every i (dusp_peak_device's words, compared as unsigned bit patterns: any NaN
 * wins), 1 <= n_peaks <= 2^24: what dusp_encode_device reads as d_peaks to give n_peaks instances one gain.  d_common is not d_peaks. */
int dusp_peak_common_device(dusp_ctx *ctx, const float *d_peaks, size_t n_peaks, float *d_common, void *stream);

/* Meters: RMS and ITU-R BS.1770-4 loudness of the mix and of every stem (additions to ABI v7, detected by symbol; DESIGN.md 6.18;
 * dusp_amd/mix.py meters is the contract).  Signals are planar f32 [n_signals][n_channels][n_samples].  Per (signal, channel) the RMS,
 * sqrt(sum f64(x)^2 / n).  Per signal the K-weighted loudness: every channel through the standard's two biquads (made for the sample
 * rate by the bilinear re-derivation libebur128 uses) in f64, EVERY channel with weight 1 (the standard for mono and stereo; a Space
 * timeline's speakers are no 5.1 layout and get weight 1 too); hop = (sample_rate + 5) / 10 samples, a block is 4 hops, block j begins
 * at sample j * hop; momentary[j] = -0.691 + 10 log10(e_j), -inf for 0; lufs the gated integrated loudness (-70 absolute, -10 relative),
 * -inf when no block is left, NaN as soon as one block's energy is not finite — which every block is that holds or follows a sample
 * that is not finite.  The meters are taken on the f32 signals in front of the PCM gain: an encoded file's loudness is
 * lufs + 20 log10(gain).  Not built: loudness range, short-term loudness, surround weights (true peak and the delivery at a loudness
 * target: the next section).
 * The sums are formed in a fixed order without floating-point atomics: two runs give the same bits.  A sample rate below 8000 is
 * refused (the shelf lies at 1682 Hz). */
/* how many blocks n_samples hold: 0 below a block, else (n_samples - block) / hop + 1; 0 for a sample rate below 8000 */
size_t dusp_meter_blocks(size_t n_samples, uint32_t sample_rate);
/* The kernels alone, on device pointers: d_sumsq f64 [n_signals][n_channels] = the sums of squares, d_hops f64
 * [n_signals][ceil(n_samples / hop)] = per hop of 100 ms the sum over the channels of the K-weighted squares (the last hop may be
 * shorter).  Both 8-byte aligned, d_planar 4-byte aligned.  Timed by dusp_score_last_ms; dusp_meter_last_ms has the four passes.  The
 * scratch is the context's: calls on one context are ordered on one stream.  n_signals x n_channels x n_samples <= 2^33. */
int dusp_meter_device(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate,
                      double *d_sumsq, double *d_hops, void *stream);
/* the last dusp_meter_device call pass by pass, by events: ms[0] the segments from rest, ms[1] the walk over the segments' states,
 * ms[2] the segments from their true states, ms[3] the reduction.  Waits for the call. */
int dusp_meter_last_ms(dusp_ctx *ctx, float ms[4]);
/* Host round trip: uploads h_planar, meters it, and gates in the library: h_rms f64 [n_signals][n_channels], h_lufs f64 [n_signals],
 * h_momentary f64 [n_signals][dusp_meter_blocks(n_samples, sample_rate)] or NULL. */
int dusp_meter_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate,
                    double *h_rms, double *h_lufs, double *h_momentary);
/* dusp_render_host_score_piece_stems which also meters what it delivers: n_signals signals (1 + n_tracks + n_buses + 1 with stems, 1 —
 * the mix — without) of the timeline's channels, at the parts' sample rate, after the last kernel that writes them and before the
 * encode.  meters NULL: that entry under this entry's name.  Refused before anything renders, each in its own words: n_signals or
 * n_blocks that is not what the call gives (both numbers named), NULL h_rms or h_lufs, a sample rate below 8000. */
typedef struct dusp_score_meters {
    size_t n_signals;    /* must be what the call delivers */
    size_t n_blocks;     /* must be dusp_meter_blocks(n_total_samples, the parts' sample rate) */
    double *h_rms;       /* [n_signals][channels] */
    double *h_lufs;      /* [n_signals] */
    double *h_momentary; /* [n_signals][n_blocks], or NULL */
} dusp_score_meters;
int dusp_render_host_score_piece_meters(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                        const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                        const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                        const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems,
                                        const dusp_score_meters *meters, size_t n_total_samples, size_t tile_bytes, int format, int normalise,
                                        void *h_out, float *h_peaks);

/* Loudness delivery: the true peak of signals, and PCM frames at a loudness target under a true-peak ceiling (additions to ABI v7,
 * detected by symbol; dusp_amd/mix.py true_peak_taps, true_peak and loudness_gain are the contract).
 * The true peak of a row of n f32 samples at a sample rate: the row oversampled F times — F = 4 below 96000 Hz, 2 below 192000 Hz, else
 * 1 — by the Hann-windowed sinc of 49 taps libebur128 interpolates with, h[j] = sinc((j - 24) / F) x 0.5 (1 - cos(2 pi j / 48)), exactly
 * 0 where F divides j - 24 != 0; phase p owns h[p], h[p + F], ..: K = ceil(49 / F) taps, a shorter phase padded with a zero tap.  With
 * x zero outside [0, n), for u in [0, n + K - 1) and every phase: acc = 0.0, acc = acc + h[p + F k] * f64(x[u - k]), k = 0 .. K - 1 in
 * that order, every product and sum rounded by itself in f64 (no FMA).  The true peak is the largest |acc| — the filter's tail behind
 * the last sample included — and NaN as soon as one acc is not finite.  F = 1: h = [1], the sample peak.  LINEAR; dBTP is 20 log10.
 * One 64-bit unsigned maximum a workgroup, no floating-point atomic: two runs give the same bits. */
/* the factor and the 49 taps at a sample rate (F = 1: h49[0] = 1, the rest 0); a rate of 0 is refused */
int dusp_true_peak_taps(uint32_t sample_rate, int *factor, double *h49);
/* the kernel alone, on device pointers: d_words [n_signals][n_channels], 8-byte aligned, one word a row: the bits of its true peak as
 * a double (the quiet NaN where an accumulator was not finite).  d_planar 4-byte aligned; rows may start on any 4-byte boundary.  The
 * shapes of dusp_meter_device, any sample rate but 0.  Timed by dusp_score_last_ms. */
int dusp_true_peak_device(dusp_ctx *ctx, const float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate,
                          uint64_t *d_words, void *stream);
/* the output positions a workgroup of that call owns (256 x 1, 2, 4 or 8: what fills the context's device), for tests and profiles; 0
 * for a call that would be refused */
size_t dusp_true_peak_tile(dusp_ctx *ctx, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate);
/* Host round trip: uploads h_planar, runs the kernel and downloads h_true_peak f64 [n_signals][n_channels]. */
int dusp_true_peak_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate,
                        double *h_true_peak);
/* dusp_render_host_score_piece_meters which also takes the true peak of every signal and channel it delivers, behind the meter kernels
 * and in front of the peak kernel, and — deliver = 1 — encodes at a loudness target: with lufs the loudness of the MIX (the last
 * signal) and tp the largest true peak of ANY delivered signal and channel,
 *     G = min(10^((target_lufs - lufs) / 20), 10^(ceiling_dbtp / 20) / tp),  level = (float)(1 / G),  gain = 1 / (double)level
 * and every signal's frames are what dusp_encode_device makes of it with `level` as its peak under DUSP_NORMALISE_FULL: ONE gain for all
 * signals, so the files still add up and none exceeds the ceiling.  The gain is unity (gain 1, level 1.0f: the samples stay as they
 * are) where lufs is -inf or NaN, where tp is 0, NaN or Inf, and where level comes out zero, subnormal or not finite.  The ceiling only
 * lowers the gain: this entry has no limiter (the _limiter entry below).  h_peaks stay the sample peaks.  deliver = 1 waits for the stream once between the meters and
 * the encode; deliver = 0 waits no more than the _meters entry and delivers its bytes.  loudness NULL: that entry under this entry's
 * name.  Refused before anything renders, behind every refusal of that entry, each in its own words: NULL h_true_peak; deliver without
 * meters, with format 0 or with normalise != 0; a target that is not finite; a ceiling that is not finite or above 0; a sample rate
 * below 8000. */
typedef struct dusp_score_loudness {
    int deliver;         /* 0: true peaks only; 1: encode at the loudness target */
    double target_lufs, ceiling_dbtp;
    double *h_true_peak; /* [n_signals][channels], required */
    double *h_gain;      /* 1, may be NULL */
    float *h_level;      /* 1, may be NULL */
} dusp_score_loudness;
int dusp_render_host_score_piece_loudness(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                          const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                          const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                          const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems,
                                          const dusp_score_meters *meters, const dusp_score_loudness *loudness, size_t n_total_samples,
                                          size_t tile_bytes, int format, int normalise, void *h_out, float *h_peaks);

/* The limiter of a delivery at a loudness target: a linked look-ahead true-peak limiter on the device (additions to ABI v7, detected by
 * symbol; dusp_amd/mix.py limiter_envelope, limiter_gain, limit and limiter_threshold are the contract).
 * Signals are planar f32 [n_signals][n_channels][n_samples]; F, h, K as for the true peak, D = (K - 1) / 2, ONE = 2^30, T the threshold
 * (linear, finite, above 0), L the window (1 .. 4096 samples).  The envelope: e[s] = the largest |acc_p[s + D]| over ALL rows and
 * phases, the accumulators formed as for the true peak; one that is not finite counts as 0.  The curve: r = T / e where e > T, else 1;
 * q = floor(r x ONE); m[j] = min(q[j .. j + L - 1]), q = ONE outside [0, n); sum[s] = m[s - L + 1] + .. + m[s], an exact integer;
 * g[s] = (double)sum[s] / (double)(L x ONE) — so g[s] <= r[s], exactly (every minimum in the mean holds q[s]), with a linear attack
 * and release of L samples.  Every row becomes (float)((double)x x g[s]), ONE curve for all: the signals of a call still add up.  reduction = min(g), 1
 * exactly where nothing exceeds T (the signals then stay bit for bit).  Integer between the two divisions: two runs, and any tiling,
 * give the same bits. */
/* 10^(ceiling_dbtp / 20) / 10^((target_lufs - lufs) / 20): the true-peak magnitude the gain of the target brings to the ceiling.  Needs
 * no device. */
double dusp_limiter_threshold(double lufs, double target_lufs, double ceiling_dbtp);
/* the samples a workgroup of both kernels owns in a call over n_samples with that window (256 x 1, 2, 4 or 8; at most 1024 above a
 * window of 512), for tests and profiles; 0 for a call that would be refused */
size_t dusp_limit_tile(dusp_ctx *ctx, size_t n_samples, size_t window_samples);
/* the two kernels alone, on device pointers, IN PLACE over d_planar (4-byte aligned; rows may start on any 4-byte boundary).  Optional,
 * NULL to leave out: d_q uint32 [n_samples], the words q; d_gain f64 [n_samples], the curve; d_smallest, one 8-byte word, the smallest
 * sum (reduction = word / (L x ONE)).  The scratch is the context's: calls on one context are ordered on one stream.  The shapes of
 * dusp_true_peak_device.  Timed by dusp_score_last_ms; dusp_limit_last_ms has the two kernels. */
int dusp_limit_device(dusp_ctx *ctx, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold,
                      size_t window_samples, uint32_t *d_q, double *d_gain, uint64_t *d_smallest, void *stream);
/* the last dusp_limit_device call kernel by kernel, by events: ms[0] the envelope kernel, ms[1] the gain / apply kernel.  Waits for the
 * call's kernels, and then checks the guard behind the context's scratch (DUSP_GUARD), which dusp_limit_device, not waiting, cannot. */
int dusp_limit_last_ms(dusp_ctx *ctx, float ms[2]);
/* Host round trip: uploads h_planar, limits it and downloads h_limited (may be h_planar); h_gain f64 [n_samples] or NULL; h_reduction
 * one double or NULL. */
int dusp_limit_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold,
                    size_t window_samples, float *h_limited, double *h_gain, double *h_reduction);
/* dusp_render_host_score_piece_loudness with a limiter in front of the one gain (limiter NULL: that entry under this entry's name).
 * After the meters, the true peaks and the one wait of a delivery at a target, on the host in f64: T = dusp_limiter_threshold(lufs of
 * the MIX, target, ceiling).  The limiter is ENGAGED where that entry's gain is not unity (level != 1.0f), T is finite and above 0 and
 * the largest true peak of any delivered signal and channel exceeds T; otherwise nothing more is launched and the delivery is that
 * entry's byte for byte.  Engaged: the limiter's kernels over every delivered signal, in place; the meter, true-peak and peak kernels
 * again over the limited signals; a second wait; then that entry's gain from the SECOND measurement and its encode.  The ceiling is
 * therefore held by the static gain as before; the delivered loudness is the target less what limiting took from the mix.  What the
 * call hands back then describes the LIMITED signals: the meters, h_true_peak, h_peaks, h_gain, h_level.  Refused behind every refusal
 * of that entry, each in its own words: a limiter without a loudness record with deliver = 1; a window of 0 or above 4096. */
typedef struct dusp_score_limiter {
    size_t window_samples; /* L, 1 .. 4096 */
    int *h_engaged;        /* each 1 value, may be NULL: whether the limiter ran ... */
    double *h_threshold;   /* ... T ... */
    double *h_reduction;   /* ... min(g), 1 when not engaged ... */
    double *h_lufs_in;     /* ... the loudness of the mix in front of the limiter ... */
    double *h_true_peak_in; /* ... and the largest true peak in front of it */
} dusp_score_limiter;
int dusp_render_host_score_piece_limiter(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                         const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                         const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                         const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems,
                                         const dusp_score_meters *meters, const dusp_score_loudness *loudness, const dusp_score_limiter *limiter,
                                         size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peaks);

/* The limiter's release of its own (additions to ABI v7, detected by symbol; dusp_amd/mix.py limiter_release_step and
 * limiter_gain_release are the contract).  q, m, L, ONE and T are the limiter's.  R is the release, 1 .. 2^22 samples, and
 * d = ceil(ONE / R) its step.  Between the minima and the mean stands the held curve, held[j] = min(m[j], held[j - 1] + d) for j from
 * -(L - 1) upwards with held[-L] = ONE — the minimum over i <= j of m[i] + d (j - i); sum[s] = held[s - L + 1] + .. + held[s];
 * g[s] = (double)sum[s] / (double)(L x ONE).  So the curve falls as the plain limiter's does and rises by at most d / ONE a sample: a
 * gain of 0 is back at 1 after at most R samples.  held <= m, so g[s] is at most the plain limiter's g[s], and R = 1 gives that curve
 * bit for bit.  All integer between the two divisions: a scan over the tiles by three launches, no workgroup waiting for another. */
/* the positions a workgroup of the release's kernels owns in a call over n_samples with that window and release: dusp_limit_tile's;
 * 0 for a call that would be refused */
size_t dusp_limit_release_tile(dusp_ctx *ctx, size_t n_samples, size_t window_samples, size_t release_samples);
/* dusp_limit_device with a release of release_samples (1 .. 2^22): the envelope kernel, then the hold, release and mean / apply kernels.
 * d_held: optional, uint32 [n_samples + window_samples - 1], the held curve; position j + (L - 1) holds held[j].  Timed by
 * dusp_score_last_ms; dusp_limit_release_last_ms has the four kernels. */
int dusp_limit_release_device(dusp_ctx *ctx, float *d_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold,
                              size_t window_samples, size_t release_samples, uint32_t *d_q, uint32_t *d_held, double *d_gain, uint64_t *d_smallest, void *stream);
/* the last dusp_limit_release_device call launch by launch, by events: ms[0] the envelope kernel, ms[1] hold, ms[2] release, ms[3]
 * mean / apply.  Waits for the call's kernels, then checks the guards behind the context's scratch (DUSP_GUARD). */
int dusp_limit_release_last_ms(dusp_ctx *ctx, float ms[4]);
/* dusp_limit_host with a release of release_samples (1 .. 2^22) */
int dusp_limit_release_host(dusp_ctx *ctx, const float *h_planar, size_t n_signals, size_t n_channels, size_t n_samples, uint32_t sample_rate, double threshold,
                            size_t window_samples, size_t release_samples, float *h_limited, double *h_gain, double *h_reduction);
/* dusp_render_host_score_piece_limiter with a release: release_samples = 0 is that entry's call byte for byte (under this entry's
 * name); 1 .. 2^22, the engaged limiter runs with that release.  Refused behind every refusal of that entry: more than 2^22 samples.
 * limiter NULL: no limiter and no release.  Scratch on the context: 4 (n + L - 1) bytes and one word a tile beside the limiter's. */
typedef struct dusp_score_limiter_release {
    dusp_score_limiter limiter;
    size_t release_samples; /* R, 1 .. 2^22; 0: no release of its own */
} dusp_score_limiter_release;
int dusp_render_host_score_piece_limiter_release(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of,
                                                 const int64_t *h_onsets, const int64_t *h_lengths, const float *h_gains,
                                                 const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                                 const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems,
                                                 const dusp_score_meters *meters, const dusp_score_loudness *loudness,
                                                 const dusp_score_limiter_release *limiter, size_t n_total_samples, size_t tile_bytes, int format,
                                                 int normalise, void *h_out, float *h_peaks);

/* State write-back (SURVEY.md §5 "checkpoint/resume"): after a render, copy the
 * state of `unit` for `instance` into out[] in the layout of the descriptor's
 * state words for that unit's opcode (Osc: phase; Ramp: t, playing; Filter:
 * has_lastF,lastF,a0,a1,a2,b1,b2,nch,(x1,x2,y1,y2)*nch; CircleBuffer nodes: t; Timer: t;
 * Shape: t,playing,finished; AHD: state,playing,t; SampleRateRedux: timeSinceLastUpdate,n,val*n).
 * Returns the number of words (>= 0) or a negative dusp_status. */
int dusp_state_download(dusp_program *prog, size_t instance, size_t unit, double *out, size_t cap);

/* How many output channels the circuit of a descriptor has, as dusp_program_build would find (dusp_program_info.n_out_channels) — on
 * the host alone: no context, no GPU.  A binder that groups voices into the parts of a piece (dusp_render_host_score_parts) refuses
 * parts of different channel counts with this, before it builds anything.  Negative: DUSP_ERR_ARG for a descriptor that does not parse
 * (dusp_last_error(NULL) has the message).  An addition to ABI v7, detected by symbol. */
int dusp_descriptor_channels(const double *desc, size_t n_words);

/* The circuit compiler, on its own (needs no device).  Programs on the WAVE engine whose units it knows are rendered by ONE
 * kernel generated for that circuit — the chunk loop of src/Circuit.js:19-41 with every unit's `_tick` inlined in process
 * order, operands in registers — compiled for gfx950 in process (hiprtc) the first time a circuit structure is rendered and
 * cached afterwards (in the process and on disk).  A circuit that is a `Sum.many` of isomorphic voices gets the voice's units
 * ONCE, in a loop over the voices, from 96 units on; other circuits are straight-line code up to 256 units.  This call returns that kernel's HIP text for a descriptor (for inspection, and so that the generator
 * and the run-time compiler can be tested without a GPU):
 *   waves      wavefronts per workgroup the text is generated for (1 .. 16)
 *   per_wave   circuit instances per wavefront (1 .. 4; renders that are split in time use 1)
 *   lds_table  bit 0: assume the oscillators' first wave table is antisymmetric (half image in LDS), as a context would find;
 *              bit 1: the text of a program built with DUSP_ENGINE_RESUMABLE (a circuit with delay lines / feedback that will be
 *              continued: outlets parked between launches, rings kept in the reference's own state);
 *              bit 2: the Filter stage's recurrence loop with 4 P values per register set (what a render falls back to when the
 *              kernel spills at 8)
 *   compile    non-zero: also compile the text for gfx950
 *   text, cap  receives at most cap - 1 characters, NUL-terminated (cap 0: nothing is copied)
 * Returns the length of the text, DUSP_ERR_UNSUPPORTED when the circuit stays on the interpreter (dusp_last_error(NULL) says
 * why), or another negative dusp_status. */
int dusp_circuit_kernel_source(const double *desc, size_t n_words, int waves, int per_wave, int lds_table, int compile, char *text, size_t cap);

/* ABI v5.  Where compiled circuit kernels (code objects) are kept across processes: $DUSP_JIT_CACHE if set ("0" / "off": no
 * disk cache), else $XDG_CACHE_HOME/dusp-hip, else $HOME/.cache/dusp-hip — read once per process.  Files are keyed by the
 * kernel text, the device library's text, the compile options, the target and the hiprtc version, and carry their length and
 * a hash of their payload; a damaged file is deleted and the kernel compiled again.  Returns "" when there is no disk cache.
 * The string lives as long as the library. */
const char *dusp_jit_cache_dir(void);

/* Duration in milliseconds of the most recent render's kernel(s) on this
 * program, measured with HIP events on the launch stream (synchronises). */
int dusp_last_kernel_ms(dusp_program *prog, float *ms);

/* Fill-kernel ceiling: writes n_floats f32 to d_out with 16-byte coalesced
 * stores and nothing else — the measured HBM write roofline the render kernels
 * are compared with. */
int dusp_fill_device(dusp_ctx *ctx, float *d_out, size_t n_floats, float value, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DUSP_HIP_H */
