// abi_render.hip — the C ABI (include/dusp_hip.h): renders into device memory.  render_device_unguarded checks the call and dispatches to
// one step per engine; the step on a compiled circuit kernel is abi_render_jit.hip.
#include <cstring>

#include "abi_internal.hpp"
#include "jit_plan.hpp"
#include "render_plan.hpp"
#include "ring_windows.hpp"

static int check_tables(dusp_program *prog) {
    dusp_ctx *ctx = prog->ctx;
    for (const auto &u : prog->P.g.units)
        if (u.op == dusp::OP_OSC || u.op == dusp::OP_MULTI_OSC || u.op == dusp::OP_SHAPE) {
            const int w = (int)u.attrs[0];
            if (!ctx->d_tables || !ctx->table_set[w])
                CTX_FAIL(ctx, DUSP_ERR_STATE, "render: wave table " + std::to_string(w) + " has not been uploaded (dusp_table_upload)");
            if (ctx->table_len != (uint32_t)prog->P.g.sample_rate + 1)
                CTX_FAIL(ctx, DUSP_ERR_STATE, "render: wave table length != sample_rate + 1");
        }
    return DUSP_OK;
}


// Rings start as zeros (Delay.js:14, CircleBuffer.js:12).  A render nothing continues fills only the slots it can reach (ring_windows.hpp);
// a program that will be continued, one whose channel counts still grow, and DUSP_RING_WINDOW=0 fill the whole rings as before.
// instance_major: rings laid out [instance][slot] (wave engine, compiled kernels), else [slot][n_pad] (chunk engine).
hipError_t zero_rings(dusp_program *prog, uint32_t n_pad, uint32_t n_chunks, bool instance_major, hipStream_t stream) {
    const dusp::Program &P = prog->P;
    float *rings = prog->d_rings.p;
    const size_t total = (size_t)P.ring_samples;
    if (prog->ctx->knobs.ring_poison) {  // (tests: what the fill leaves out holds NaN patterns, so a window cut too short shows)
        if (hipError_t e = hipMemsetAsync(rings, 0xff, total * n_pad * sizeof(float), stream)) return e;
    }
    const bool windowed = !prog->resumable && prog->ctx->knobs.ring_window != 0 && P.warm_ops.empty();
    std::vector<dusp::RingWindow> wins;
    size_t covered = 0;
    if (windowed) dusp::ring_windows(P, n_chunks, wins, covered);
    if (!windowed || wins.empty() || covered * 2 > total || wins.size() > 64)
        return hipMemsetAsync(rings, 0, total * n_pad * sizeof(float), stream);
    for (const dusp::RingWindow &w : wins) {
        hipError_t e = instance_major ? hipMemset2DAsync(rings + w.at, total * sizeof(float), 0, (size_t)w.count * sizeof(float), n_pad, stream)
                                      : hipMemsetAsync(rings + (size_t)w.at * n_pad, 0, (size_t)w.count * n_pad * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}


// The bookkeeping every render ends with: what a state download, a continuation and the next render need to know about this one
void finish_render(dusp_program *prog, uint32_t n_inst, uint32_t n_pad, uint64_t n_chunks_total) {
    prog->last_n_inst = n_inst;
    prog->last_n_pad = n_pad;
    prog->rendered = true;
    prog->h_state_valid = false;
    prog->mixed = false;
    prog->next_clock = prog->P.g.clock0 + (int64_t)n_chunks_total * dusp::kChunk;
}


// The chunk engine's arguments for n_chunks chunks of this program (workspaces as the caller has sized them)
static dusp::ChunkArgs chunk_args(dusp_program *prog, uint32_t n_inst, size_t n_samples, uint32_t n_chunks, const float *d_params, const float *d_inputs, float *d_out,
                                  uint32_t flags) {
    const dusp::Program &P = prog->P;
    dusp::ChunkArgs a{};
    a.ops = prog->d_ops.p;
    a.out_bufs = prog->d_out_bufs.p;
    a.scratch = prog->d_scratch.p;
    a.state = prog->d_state.p;
    a.rings = prog->d_rings.p;
    a.params = d_params;
    a.tables = prog->ctx->d_tables;
    a.inputs = d_inputs;
    a.out = d_out;
    a.n_samples = n_samples;
    a.clock0 = P.g.clock0;
    a.n_ops = (uint32_t)P.ops.size();
    a.n_out = (uint32_t)P.out_bufs.size();
    a.n_inst = n_inst;
    a.n_pad = (n_inst + 63u) & ~63u;
    a.n_chunks = n_chunks;
    a.sample_rate = (uint32_t)P.g.sample_rate;
    a.table_stride = prog->ctx->table_stride;
    a.flags = flags;
    a.n_warm = (uint32_t)P.warm_ops.size();
    for (uint32_t k = 0, at = a.n_ops; k < a.n_warm; k++) {
        a.warm_first[k] = at;
        a.warm_n[k] = (uint32_t)P.warm_ops[k].size();
        at += a.warm_n[k];
    }
    return a;
}


// DUSP_GUARD=1: wait for the render and look at the guard bytes behind every workspace it could have touched
int check_guards(dusp_program *prog, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    if (!g_guard_bytes) return DUSP_OK;
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    const char *hit = prog->first_overwritten();
    if (!hit && ctx->tables_guarded && ctx->d_tables && !guard_intact((const char *)ctx->d_tables + sizeof(float) * dusp::kNumTables * ctx->table_stride)) hit = "lookup tables";
    if (hit) CTX_FAIL(ctx, DUSP_ERR_HIP, std::string("render: a kernel wrote past the end of a device buffer (") + hit + "): guard bytes overwritten");
    return DUSP_OK;
}

// A render as its steps see it: the caller's arguments and the arithmetic render_device_unguarded has done on them
struct RenderCall {
    uint32_t n_inst, n_chunks, n_pad;
    size_t n_samples;
    const float *d_params, *d_inputs;
    float *d_out;
    hipStream_t stream;
};

// Sizes of the chunk engine's workspaces: every outlet's chunk [buffer][sample][n_pad], unit state [slot][n_pad], rings [slot][n_pad]
// (rows = n_inst for the wave engine's parked chunks, which are not padded)
static size_t chunk_workspace_floats(const dusp::Program &P, uint32_t rows) { return (size_t)std::max(1, P.n_bufs) * dusp::kChunk * rows; }
static size_t state_workspace_doubles(const dusp::Program &P, uint32_t n_pad) { return std::max<size_t>(1, P.init_state.size()) * n_pad; }
static size_t ring_workspace_floats(const dusp::Program &P, uint32_t n_pad) { return std::max<size_t>(1, (size_t)P.ring_samples) * n_pad; }

// Chunk buffers and the WHOLE rings as zeros (SignalChunk.js:7, Delay.js:14, CircleBuffer.js:12)
static int clear_chunk_memory(dusp_program *prog, uint32_t n_pad, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    HIP_TRY(ctx, hipMemsetAsync(prog->d_scratch.p, 0, chunk_workspace_floats(prog->P, n_pad) * sizeof(float), stream));
    if (prog->P.ring_samples) HIP_TRY(ctx, hipMemsetAsync(prog->d_rings.p, 0, (size_t)prog->P.ring_samples * n_pad * sizeof(float), stream));
    return DUSP_OK;
}

// The fused sum chain (a Sum.many of constant-f oscillators).  window: dusp_render_chain_window — this launch is a window of the
// timeline and continues another rank's sums.
static int render_sum_chain(dusp_program *prog, const RenderCall &c, dusp::FusedLaunch &L, const ChainWindow *window) {
    dusp_ctx *ctx = prog->ctx;
    const uint32_t n_inst = c.n_inst;
    hipStream_t stream = c.stream;
    if (!L.table_fx32_ok) CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, "render: wave table has entries below 2^-20; build this program with DUSP_ENGINE_CHUNK");
    const int gb = dusp::sumchain_group_blocks(n_inst, c.n_samples, ctx->n_cus);
    if (!gb) CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, "render: too many samples for the fused sum chain (at most 65535 blocks of 2048 samples: 134215680 samples a launch); use DUSP_ENGINE_CHUNK");
    if (window) {
        L.chain_first = window->first;
        L.chain_init = window->init;
        L.chain_raw = window->raw;
    }
    dusp::build_sum_voices(prog->fused, (uint32_t)prog->P.g.sample_rate, gb, L.chain_first, L.chain_first + (uint64_t)c.n_chunks * dusp::kChunk, prog->h_sum_voices, prog->h_sum_end);
    HIP_TRY(ctx, prog->d_sum_voices.ensure(prog->h_sum_voices.size()));
    HIP_TRY(ctx, hipMemcpyAsync(prog->d_sum_voices.p, prog->h_sum_voices.data(), prog->h_sum_voices.size() * sizeof(dusp::SumVoice), hipMemcpyHostToDevice, stream));
    std::vector<double> end((size_t)prog->fused.n_state_words * n_inst);
    for (int w = 0; w < prog->fused.n_state_words; w++)
        for (uint32_t i = 0; i < n_inst; i++) end[(size_t)w * n_inst + i] = prog->h_sum_end[(size_t)w];
    HIP_TRY(ctx, hipMemcpyAsync(prog->d_fused_state.p, end.data(), end.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));  // the staging vectors above are reused by the next call
    HIP_TRY(ctx, hipEventRecord(prog->ev0, stream));
    HIP_TRY(ctx, dusp::launch_sumchain(prog->fused, L, prog->d_sum_voices.p, gb, stream));
    HIP_TRY(ctx, hipEventRecord(prog->ev1, stream));
    return DUSP_OK;
}

static int render_fused(dusp_program *prog, const RenderCall &c, const ChainWindow *window) {
    dusp_ctx *ctx = prog->ctx;
    dusp::FusedLaunch L{};
    L.params = c.d_params;
    L.tables = ctx->d_tables;
    L.table_stride = ctx->table_stride;
    L.out = c.d_out;
    L.n_inst = c.n_inst;
    L.n_samples = c.n_samples;
    L.n_chunks = c.n_chunks;
    L.sample_rate = (uint32_t)prog->P.g.sample_rate;
    L.n_cus = ctx->n_cus;
    L.table_antisym = ctx->table_antisym[prog->fused.table_id];
    L.table_finite = ctx->table_finite[prog->fused.table_id];
    L.table_fx32_ok = ctx->table_fx32_ok[prog->fused.table_id];
    L.table_delta = ctx->table_delta[prog->fused.table_id];
    L.table_form = ctx->table_form[prog->fused.table_id];
    L.knobs = ctx->knobs;
    HIP_TRY(ctx, prog->d_recs.ensure(c.n_inst));
    L.recs = prog->d_recs.p;
    HIP_TRY(ctx, prog->d_fused_state.ensure((size_t)std::max(1, prog->fused.n_state_words) * c.n_inst));
    L.end_state = prog->d_fused_state.p;
    if (prog->fused.kind == dusp::FUSED_SUMCHAIN) {
        if (int rc = render_sum_chain(prog, c, L, window)) return rc;
    } else {
        HIP_TRY(ctx, hipEventRecord(prog->ev0, c.stream));
        HIP_TRY(ctx, dusp::launch_fused(prog->fused, L, c.stream));
        HIP_TRY(ctx, hipEventRecord(prog->ev1, c.stream));
    }
    finish_render(prog, c.n_inst, c.n_pad, c.n_chunks);  // (n_pad: only ever read for programs of the other engines, whose renders all set it)
    return DUSP_OK;
}

// The wave engine's interpreter kernel: every WAVE program the circuit compiler does not take, and one it takes while its kernel compiles
static int render_wave_interpreter(dusp_program *prog, const RenderCall &c) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    const uint32_t n_inst = c.n_inst, n_pad = c.n_pad, n_chunks = c.n_chunks;
    hipStream_t stream = c.stream;
    HIP_TRY(ctx, prog->d_state.ensure(state_workspace_doubles(P, n_pad)));
    dusp::WaveArgs w{};
    w.ops = prog->d_ops.p;
    w.out_bufs = prog->d_out_bufs.p;
    w.params = c.d_params;
    w.tables = ctx->d_tables;
    w.inputs = c.d_inputs;
    w.out = c.d_out;
    w.state = prog->d_state.p;
    w.init_state = prog->d_init.p;
    w.n_samples = c.n_samples;
    w.n_ops = (uint32_t)P.ops.size();
    w.n_out = (uint32_t)P.out_bufs.size();
    w.n_inst = n_inst;
    w.n_pad = n_pad;
    w.n_bufs = (uint32_t)prog->wave.n_slots;
    w.n_state_ops = (uint32_t)prog->wave.n_state_ops;
    w.n_groups = n_chunks;
    w.sample_rate = (uint32_t)P.g.sample_rate;
    w.table_stride = ctx->table_stride;
    w.vec4_ok = (c.n_samples % 4 == 0) && (((uintptr_t)c.d_out & 15) == 0);
    w.lds_table_id = prog->wave.lds_table_id;
    w.clock0 = (uint64_t)P.g.clock0;
    w.has_filter = prog->wave.has_filter ? 1u : 0u;
    w.scratch_bytes = (uint32_t)prog->wave.scratch_bytes;
    w.ring_events = prog->wave.ring_events ? 1u : 0u;
    w.ext_units = (uint32_t)prog->wave.ext_units;
    w.n_params = (uint32_t)P.g.n_params;
    w.ring_samples = (uint64_t)P.ring_samples;
    const bool resume = prog->keep_memory;
    if (resume && n_inst != prog->last_n_inst) CTX_FAIL(ctx, DUSP_ERR_STATE, "render: the instance count cannot change while a program is being continued");
    if (P.ring_samples && !resume) {  // Delay rings start as zeros (Delay.js:14); wave-engine layout [instance][slot]
        HIP_TRY(ctx, prog->d_rings.ensure(ring_workspace_floats(P, n_pad)));
        HIP_TRY(ctx, zero_rings(prog, n_pad, n_chunks, true, stream));
    }
    w.rings = prog->d_rings.p;
    w.resume = resume ? 1u : 0u;
    w.save_bufs = (prog->resumable && prog->persistent) ? 1u : 0u;
    if (w.save_bufs) {
        HIP_TRY(ctx, prog->d_saved_bufs.ensure(chunk_workspace_floats(P, n_inst)));
        w.saved_bufs = prog->d_saved_bufs.p;
    }
    prog->keep_memory = false;
    // Few instances, long render: cut time into segments so that the whole chip works on it (wave_engine.hip).
    w.n_seg = 1;
    w.seg_groups = n_chunks;
    w.max_osc_level = prog->wave.max_osc_level;
    if (prog->wave.splittable && dusp::wave_split_exact(P, ctx->table_bound, prog->param_bound.empty() ? nullptr : prog->param_bound.data())) {  // (fused_plan.hpp: only where segment totals are the reference's phases)
        dusp::jit_time_segments(ctx->n_cus, ctx->knobs.wave_segments, n_inst, n_chunks, w.n_seg, w.seg_groups);
        if (w.n_seg > 1) {
            const size_t per = (size_t)w.n_ops * n_inst * w.n_seg;
            HIP_TRY(ctx, prog->d_seg.ensure(2 * per));
            w.seg_sum = prog->d_seg.p;
            w.seg_start = prog->d_seg.p + per;
        }
    }
    prog->wave_segments = w.n_seg;
    const bool lds_ok = w.lds_table_id >= 0 && ctx->table_antisym[w.lds_table_id] && P.g.sample_rate % 2 == 0;
    HIP_TRY(ctx, hipEventRecord(prog->ev0, stream));
    HIP_TRY(ctx, dusp::launch_wave_engine(w, lds_ok, ctx->knobs.wave_max_waves, stream));
    HIP_TRY(ctx, hipEventRecord(prog->ev1, stream));
    finish_render(prog, n_inst, n_pad, n_chunks);
    return DUSP_OK;
}

// Channel counts that grow during the first chunks (Program::warm_ops): a single circuit renders those chunks here, on the chunk engine
// (with the reference's own ring protocol), and the rest on the kernel compiled for its settled op list — rings, every outlet's last
// chunk and the unit state move into that kernel's layout in between (dusp_chunk_to_wave_kernel).
// kJitLater: nothing has been rendered — no chunk of this render is past the warm-up, or (under the default knob) the structure is seen
// for the first time and its kernel compiles in the background: the caller renders on the chunk engine alone.
static int render_handoff(dusp_program *prog, const RenderCall &c) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    const uint32_t n_inst = c.n_inst, n_pad = c.n_pad, n_chunks = c.n_chunks;
    const size_t n_samples = c.n_samples, n_slots = P.init_state.size();
    hipStream_t stream = c.stream;
    const uint32_t W = dusp::handoff_warm_chunks((uint64_t)P.g.clock0, (uint32_t)P.warm_ops.size(), n_chunks);
    if (!(W > 0 && W < n_chunks)) return kJitLater;
    // (a kernel that does not compile is a failure, not a reason to render elsewhere)
    if (int rc = render_jit(prog, n_inst, n_samples - (size_t)W * dusp::kChunk, n_chunks - W, c.d_params, c.d_inputs, c.d_out, stream, W, /*probe=*/true)) return rc;
    const size_t n_ch = P.out_bufs.size(), n_head = (size_t)W * dusp::kChunk, n_rest = n_samples - n_head;
    const uint32_t n_bufs = (uint32_t)std::max(1, P.n_bufs);
    HIP_TRY(ctx, prog->d_scratch.ensure(chunk_workspace_floats(P, n_pad)));
    HIP_TRY(ctx, prog->d_state.ensure(state_workspace_doubles(P, n_pad)));
    HIP_TRY(ctx, prog->d_rings.ensure(ring_workspace_floats(P, n_pad)));
    HIP_TRY(ctx, prog->d_rings_wave.ensure(ring_workspace_floats(P, n_pad)));
    HIP_TRY(ctx, prog->d_saved_bufs.ensure(chunk_workspace_floats(P, n_inst)));
    HIP_TRY(ctx, prog->d_handoff_init.ensure(std::max<size_t>(1, n_slots)));
    HIP_TRY(ctx, prog->d_handoff_out.ensure(n_ch * std::max(n_head, n_rest)));
    if (int rc = clear_chunk_memory(prog, n_pad, stream)) return rc;
    HIP_TRY(ctx, dusp::launch_state_init(prog->d_state.p, prog->d_init.p, (uint32_t)n_slots, n_pad, stream));
    // (resumable: rings in the reference's own state — a compiled kernel continues them)
    const dusp::ChunkArgs a = chunk_args(prog, n_inst, n_head, W, c.d_params, c.d_inputs, prog->d_handoff_out.p, dusp::kChunkFlagResumable);
    HIP_TRY(ctx, hipEventRecord(prog->ev0, stream));
    HIP_TRY(ctx, dusp::launch_chunk_engine(a, stream));
    HIP_TRY(ctx, hipMemcpy2DAsync(c.d_out, n_samples * sizeof(float), prog->d_handoff_out.p, n_head * sizeof(float), n_head * sizeof(float), n_ch,
                                  hipMemcpyDeviceToDevice, stream));
    HIP_TRY(ctx, dusp::launch_chunk_to_wave(prog->d_rings.p, prog->d_rings_wave.p, (uint64_t)P.ring_samples, prog->d_scratch.p, prog->d_saved_bufs.p, n_bufs,
                                            n_inst, n_pad, prog->d_state.p, prog->d_handoff_init.p, (uint32_t)n_slots, stream));
    prog->d_rings.swap(prog->d_rings_wave);  // (same size; the compiled kernel's rings are the program's rings from here on)
    prog->last_n_inst = n_inst;
    const int rc = render_jit(prog, n_inst, n_rest, n_chunks - W, c.d_params, c.d_inputs, prog->d_handoff_out.p, stream, W);  // (ends in finish_render)
    if (rc == kJitLater) CTX_FAIL(ctx, DUSP_ERR_STATE, "render: internal error: a hand-off that does not wait for its kernel");
    if (rc != DUSP_OK) return rc;
    HIP_TRY(ctx, hipMemcpy2DAsync(c.d_out + n_head, n_samples * sizeof(float), prog->d_handoff_out.p, n_rest * sizeof(float), n_rest * sizeof(float), n_ch,
                                  hipMemcpyDeviceToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(prog->ev1, stream));
    return DUSP_OK;
}

static int render_chunk(dusp_program *prog, const RenderCall &c) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    const uint32_t n_inst = c.n_inst, n_pad = c.n_pad, n_chunks = c.n_chunks;
    hipStream_t stream = c.stream;
    if (prog->keep_memory) {  // continuing: chunk buffers and rings hold what the previous segment left
        if (n_inst != prog->last_n_inst) CTX_FAIL(ctx, DUSP_ERR_STATE, "render: the instance count cannot change while a program is being continued");
        if (prog->migrate_to_chunk) {  // the chain ran on the wave engine so far: move its memory into this engine's layout
            prog->d_rings.swap(prog->d_rings_wave);
            HIP_TRY(ctx, prog->d_scratch.ensure(chunk_workspace_floats(P, n_pad)));
            HIP_TRY(ctx, prog->d_rings.ensure(ring_workspace_floats(P, n_pad)));
            if (int rc = clear_chunk_memory(prog, n_pad, stream)) return rc;
            HIP_TRY(ctx, dusp::launch_wave_to_chunk(prog->d_rings_wave.p, prog->d_rings.p, (uint64_t)P.ring_samples, prog->d_saved_bufs.p, prog->d_scratch.p,
                                                    (uint32_t)P.n_bufs, n_inst, n_pad, stream));
            prog->migrate_to_chunk = false;
        }
    } else {
        HIP_TRY(ctx, prog->d_scratch.ensure(chunk_workspace_floats(P, n_pad)));
        HIP_TRY(ctx, prog->d_state.ensure(state_workspace_doubles(P, n_pad)));
        HIP_TRY(ctx, prog->d_rings.ensure(ring_workspace_floats(P, n_pad)));
        // outlets' chunks and all rings start as zeros (SignalChunk.js:7, Delay.js:14, CircleBuffer.js:12); the rings only where the render can reach
        HIP_TRY(ctx, hipMemsetAsync(prog->d_scratch.p, 0, chunk_workspace_floats(P, n_pad) * sizeof(float), stream));
        if (P.ring_samples) HIP_TRY(ctx, zero_rings(prog, n_pad, n_chunks, false, stream));
    }
    prog->keep_memory = false;
    HIP_TRY(ctx, dusp::launch_state_init(prog->d_state.p, prog->d_init.p, (uint32_t)P.init_state.size(), n_pad, stream));

    const dusp::ChunkArgs a = chunk_args(prog, n_inst, c.n_samples, n_chunks, c.d_params, c.d_inputs, c.d_out, (prog->resumable && prog->persistent) ? dusp::kChunkFlagResumable : 0u);
    HIP_TRY(ctx, hipEventRecord(prog->ev0, stream));
    HIP_TRY(ctx, dusp::launch_chunk_engine(a, stream));
    HIP_TRY(ctx, hipEventRecord(prog->ev1, stream));
    finish_render(prog, n_inst, n_pad, n_chunks);
    return DUSP_OK;
}

int render_device_unguarded(dusp_program *prog, size_t n_instances, size_t n_samples, const float *d_params, const float *d_inputs, float *d_out, void *stream_,
                            const ChainWindow *window) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    if (!instances_in_range(n_instances)) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: n_instances must be in [1, 2^24]");
    if (!samples_in_range(n_samples)) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: n_samples must be in [1, 2^31]");
    if (!d_out) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: d_out is NULL");
    if (P.g.n_params > 0 && !d_params) CTX_FAIL(ctx, DUSP_ERR_ARG, "render: program has parameters but d_params is NULL");
    if (int rc = check_tables(prog)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RenderCall c{};
    c.stream = stream_of(ctx, stream_);
    // A program's workspaces (state, rings, scratch, voice records) are reused from render to render: a render on ANOTHER
    // stream than the previous one first waits for what that one recorded.
    if (prog->rendered && prog->last_stream != c.stream) HIP_TRY(ctx, hipStreamWaitEvent(c.stream, prog->ev1, 0));
    prog->last_stream = c.stream;
    c.n_inst = (uint32_t)n_instances;
    c.n_chunks = (uint32_t)((n_samples + dusp::kChunk - 1) / dusp::kChunk);
    c.n_pad = (c.n_inst + 63u) & ~63u;
    c.n_samples = n_samples;
    c.d_params = d_params;
    c.d_inputs = d_inputs;
    c.d_out = d_out;

    if (prog->engine == DUSP_ENGINE_FUSED) return render_fused(prog, c, window);
    prog->jit_waves = prog->jit_per_wave = 0;
    if (prog->engine == DUSP_ENGINE_WAVE) {
        if (prog->jit_ok) {
            const int rc = render_jit(prog, c.n_inst, n_samples, c.n_chunks, d_params, d_inputs, d_out, c.stream);
            if (rc != kJitLater) return rc;
        }
        return render_wave_interpreter(prog, c);
    }
    if (prog->handoff_ok && c.n_inst == 1 && !prog->keep_memory && P.g.clock0 % dusp::kChunk == 0) {
        const int rc = render_handoff(prog, c);
        if (rc != kJitLater) return rc;
    }
    return render_chunk(prog, c);
}

static int render_device(dusp_program *prog, size_t n_instances, size_t n_samples, const float *d_params, const float *d_inputs, float *d_out, void *stream_,
                         const ChainWindow *window = nullptr) {
    return guarded(prog->ctx->err, "render", [&]() -> int {
        if (int rc = render_device_unguarded(prog, n_instances, n_samples, d_params, d_inputs, d_out, stream_, window)) return rc;
        return check_guards(prog, stream_of(prog->ctx, stream_));
    });
}

extern "C" {

int dusp_render_device(dusp_program *prog, size_t n_instances, size_t n_samples, const float *d_params, float *d_out,
                       void *stream_) {
    if (!prog) return DUSP_ERR_ARG;
    if (prog->P.g.n_inputs > 0)
        CTX_FAIL(prog->ctx, DUSP_ERR_ARG, "render: the program reads host-generated input streams; use dusp_render_device_inputs / dusp_render_host_inputs");
    return render_device(prog, n_instances, n_samples, d_params, nullptr, d_out, stream_);
}

int dusp_render_chain_window(dusp_program *prog, uint64_t first_sample, size_t n_samples, const float *d_init, int raw, float *d_out, void *stream_) {
    if (!prog) return DUSP_ERR_ARG;
    if (prog->engine != DUSP_ENGINE_FUSED || prog->fused.kind != dusp::FUSED_SUMCHAIN)
        CTX_FAIL(prog->ctx, DUSP_ERR_UNSUPPORTED, "dusp_render_chain_window: the program is not on the fused sum chain (a Sum.many of constant-f oscillators)");
    if (prog->P.g.n_params > 0) CTX_FAIL(prog->ctx, DUSP_ERR_UNSUPPORTED, "dusp_render_chain_window: programs with per-instance parameters are not chained");
    if (first_sample % 2048 != 0) CTX_FAIL(prog->ctx, DUSP_ERR_ARG, "dusp_render_chain_window: first_sample must be a multiple of 2048");
    if (first_sample > (1ull << 40)) CTX_FAIL(prog->ctx, DUSP_ERR_ARG, "dusp_render_chain_window: first_sample must be at most 2^40");
    if ((((uintptr_t)d_init | (uintptr_t)d_out) & 15) != 0) CTX_FAIL(prog->ctx, DUSP_ERR_ARG, "dusp_render_chain_window: d_init and d_out must be 16-byte aligned");
    ChainWindow window;
    window.first = first_sample;
    window.init = d_init;
    window.raw = raw != 0;
    return render_device(prog, 1, n_samples, nullptr, nullptr, d_out, stream_, &window);
}

int dusp_render_device_inputs(dusp_program *prog, size_t n_instances, size_t n_samples, const float *d_params, const float *d_inputs,
                              float *d_out, void *stream_) {
    if (!prog) return DUSP_ERR_ARG;
    if (prog->P.g.n_inputs > 0 && !d_inputs) CTX_FAIL(prog->ctx, DUSP_ERR_ARG, "render: the program has input streams but d_inputs is NULL");
    return render_device(prog, n_instances, n_samples, d_params, d_inputs, d_out, stream_);
}

}  // extern "C"
