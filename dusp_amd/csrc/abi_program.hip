// abi_program.hip — the C ABI (include/dusp_hip.h): programs from descriptors (build, continue, destroy), what a program says about itself,
// unit state after a render, and the circuit compiler's text for a descriptor.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "abi_internal.hpp"
#include "engine_select.hpp"
#include "jit_engine.hpp"

extern "C" {

// Which engine renders the program, and the plans that go with the choice (engine_select.hpp)
static int select_engine(dusp_program *prog) {
    dusp_ctx *ctx = prog->ctx;
    dusp::EngineRequest rq;
    rq.requested = prog->requested_engine;
    rq.resumable = prog->resumable;
    rq.rendered = prog->rendered;
    rq.engine_so_far = prog->engine;
    rq.delay_changed = prog->delay_changed;
    rq.wave_jit = ctx->knobs.wave_jit;
    for (int k = 0; k < dusp::kNumTables; k++) rq.table_set[k] = ctx->table_set[k], rq.table_fx32_ok[k] = ctx->table_fx32_ok[k];
    dusp::EngineChoice choice = dusp::engine_select(prog->P, rq, std::move(prog->wave.ramp_checked));
    prog->fused = std::move(choice.fused);
    prog->wave = std::move(choice.wave);
    prog->persistent = choice.persistent;
    if (choice.error) CTX_FAIL(ctx, choice.error, choice.error_text);
    prog->engine = choice.engine;
    prog->jit_src.clear();
    prog->jit_consts_uploaded = false;
    prog->jit_ok = choice.jit_ok;
    prog->jit_why = std::move(choice.jit_why);
    prog->handoff_ok = choice.handoff_ok;
    prog->handoff_why = std::move(choice.handoff_why);
    return DUSP_OK;
}

// The program constants on the device: op lists (as the chosen engine reads them), outlet buffers, start state
static int upload_constants(dusp_program *prog) {
    dusp_ctx *ctx = prog->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dusp::Program &P = prog->P;
    size_t n_all_ops = P.ops.size();  // the settled op list, then the lists of the warm-up chunks (if any)
    for (const auto &w : P.warm_ops) n_all_ops += w.size();
    HIP_TRY(ctx, prog->d_ops.ensure(n_all_ops));
    std::vector<int32_t> out_bufs = P.out_bufs;
    if (prog->engine == DUSP_ENGINE_WAVE) {  // the wave engine's view: chunk buffers renamed to their LDS slots, state blocks numbered
        std::vector<dusp::DevOp> ops = P.ops;
        const auto &slot = prog->wave.buf_slot;
        for (size_t k = 0; k < ops.size(); k++) {
            if (ops[k].out_buf >= 0) ops[k].out_buf = slot[(size_t)ops[k].out_buf];
            for (auto &in : ops[k].in)
                if (in.kind == dusp::SRC_BUF && in.idx >= 0 && in.idx < P.n_bufs) in.idx = slot[(size_t)in.idx];
            ops[k].lds_slot = prog->wave.op_state[k];
        }
        for (auto &op : ops)
            if (op.op == dusp::OP_RETRIGGER) op.pad = prog->wave.op_state[(size_t)op.pad];  // target op -> its state block
        for (auto &b : out_bufs) b = slot[(size_t)b];
        std::vector<dusp::DevOp> ordered(ops.size());
        for (size_t at = 0; at < ops.size(); at++) ordered[at] = ops[(size_t)prog->wave.order[at]];
        HIP_TRY(ctx, hipMemcpy(prog->d_ops.p, ordered.data(), ordered.size() * sizeof(dusp::DevOp), hipMemcpyHostToDevice));
    } else
    HIP_TRY(ctx, hipMemcpy(prog->d_ops.p, P.ops.data(), P.ops.size() * sizeof(dusp::DevOp), hipMemcpyHostToDevice));
    n_all_ops = P.ops.size();
    for (const auto &w : P.warm_ops) {
        if (!w.empty())
            HIP_TRY(ctx, hipMemcpy(prog->d_ops.p + n_all_ops, w.data(), w.size() * sizeof(dusp::DevOp), hipMemcpyHostToDevice));
        n_all_ops += w.size();
    }
    HIP_TRY(ctx, prog->d_out_bufs.ensure(out_bufs.size()));
    HIP_TRY(ctx, hipMemcpy(prog->d_out_bufs.p, out_bufs.data(), out_bufs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!P.init_state.empty()) {
        HIP_TRY(ctx, prog->d_init.ensure(P.init_state.size()));
        HIP_TRY(ctx, hipMemcpy(prog->d_init.p, P.init_state.data(), P.init_state.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return DUSP_OK;
}

// Shared by build and continue
static int finish_build(dusp_program *prog) {
    if (int rc = select_engine(prog)) return rc;
    return upload_constants(prog);
}

static int compile_status(dusp_ctx *ctx, const char *who, const std::string &err) {
    const bool unsupported = err.find("not supported") != std::string::npos || err.find("only ") != std::string::npos;
    CTX_FAIL(ctx, unsupported ? DUSP_ERR_UNSUPPORTED : DUSP_ERR_ARG, std::string(who) + ": " + err);
}

int dusp_program_build(dusp_ctx *ctx, const double *desc, size_t n_words, int engine, dusp_program **out) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, "dusp_program_build", [&]() -> int {
    if (!out) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_program_build: out is NULL");
    *out = nullptr;
    const bool resumable = (engine & DUSP_ENGINE_RESUMABLE) != 0;
    engine &= ~DUSP_ENGINE_RESUMABLE;
    if (engine == DUSP_ENGINE_LOOP) engine = DUSP_ENGINE_AUTO;  // (ABI v7: the loop kernels are gone; a caller that still names them gets what AUTO picks for its circuit)
    if (engine != DUSP_ENGINE_AUTO && engine != DUSP_ENGINE_CHUNK && engine != DUSP_ENGINE_FUSED && engine != DUSP_ENGINE_WAVE)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_program_build: bad engine");
    std::unique_ptr<dusp_program> prog(new dusp_program);  // (its destructor frees whatever a failing step below has allocated)
    prog->ctx = ctx;
    prog->requested_engine = engine;
    prog->resumable = resumable;
    std::string err;
    if (!dusp::compile(desc, n_words, prog->P, err, /*continuation=*/false)) return compile_status(ctx, "dusp_program_build", err);
    if (ctx->table_len && ctx->table_len != (uint32_t)prog->P.g.sample_rate + 1)
        CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_program_build: uploaded wave tables do not match the program's sample rate");
    if (int rc = finish_build(prog.get())) return rc;
    HIP_TRY(ctx, hipEventCreate(&prog->ev0));
    HIP_TRY(ctx, hipEventCreate(&prog->ev1));
    *out = prog.release();
    return DUSP_OK;
    });
}

int dusp_program_continue(dusp_program *prog, const double *desc, size_t n_words) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    return guarded(ctx->err, "dusp_program_continue", [&]() -> int {
    if (!prog->rendered) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_program_continue: nothing has been rendered yet");
    dusp::Program next;
    std::string err;
    if (!dusp::compile(desc, n_words, next, err, /*continuation=*/true)) return compile_status(ctx, "dusp_program_continue", err);
    const dusp::Program &P = prog->P;
    // same circuit: same units, wiring, channel counts, buffers, state slots and rings — only constants and state may differ
    bool same = next.g.units.size() == P.g.units.size() && next.ops.size() == P.ops.size() && next.n_bufs == P.n_bufs &&
                next.ring_samples == P.ring_samples && next.out_bufs == P.out_bufs && next.g.n_params == P.g.n_params &&
                next.g.sample_rate == P.g.sample_rate && next.init_state.size() == P.init_state.size() &&
                next.dev_rings.size() == P.dev_rings.size();
    for (size_t k = 0; same && k < P.g.units.size(); k++) same = next.g.units[k].op == P.g.units[k].op && next.g.units[k].n_out == P.g.units[k].n_out;
    for (size_t k = 0; same && k < P.ops.size(); k++) {
        const dusp::DevOp &a = P.ops[k], &b = next.ops[k];
        same = a.op == b.op && a.unit == b.unit && a.out_buf == b.out_buf && a.state_slot == b.state_slot && a.ring_base == b.ring_base &&
               a.ring_len == b.ring_len && a.n_in == b.n_in;
        for (int j = 0; same && j < dusp::kMaxIn; j++)  // connections must stay connections to the same buffer
            same = (a.in[j].kind == dusp::SRC_BUF) == (b.in[j].kind == dusp::SRC_BUF) && (a.in[j].kind != dusp::SRC_BUF || a.in[j].idx == b.in[j].idx);
    }
    if (!same) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_program_continue: the descriptor does not describe the circuit this program was built from");
    if (next.g.clock0 != prog->next_clock)
        CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_program_continue: descriptor clock " + std::to_string(next.g.clock0) + " does not follow the rendered clock " +
                                          std::to_string(prog->next_clock));
    const bool persistent = next.ring_samples != 0 || !next.feed_forward;
    if (persistent && !(prog->resumable && (prog->engine == DUSP_ENGINE_CHUNK || prog->engine == DUSP_ENGINE_WAVE)))
        CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_program_continue: a circuit with delay lines / feedback has to be built with DUSP_ENGINE_RESUMABLE");
    const int engine_before = prog->engine;
    // The wave engine writes every Delay slot once, with its final value; after a change of the delay new taps can land on
    // slots that already hold data, which only the chunk engine's read-modify-write protocol accumulates like the reference.
    bool delay_changed = prog->delay_changed;
    for (size_t k = 0; k < P.ops.size(); k++)
        if (P.ops[k].op == dusp::OP_DELAY) {
            const dusp::DevOperand &a = P.ops[k].in[1], &b = next.ops[k].in[1];
            if (a.kind != b.kind || a.idx != b.idx || std::memcmp(&a.cval, &b.cval, sizeof(float)) != 0) delay_changed = true;
        }
    // All or nothing: if planning or the upload fails, the program goes back to the circuit it was rendering (host plans AND
    // the device copies of its constants), so a later render never runs a mixture of the two.
    struct Before {
        dusp::Program P; bool delay_changed; int engine;
    } before{std::move(prog->P), prog->delay_changed, prog->engine};
    prog->P = std::move(next);
    prog->delay_changed = delay_changed;
    if (int rc = finish_build(prog)) {
        const std::string why = ctx->err;
        prog->P = std::move(before.P);
        prog->delay_changed = before.delay_changed;
        const int requested = prog->requested_engine;
        prog->requested_engine = before.engine;  // re-plan the old circuit onto the engine it was on
        const int back = finish_build(prog);
        prog->requested_engine = requested;
        ctx->err = back == DUSP_OK ? why : why + " (and the previous program could not be restored: " + ctx->err + ")";
        return rc;
    }
    prog->keep_memory = persistent;
    if (persistent && engine_before == DUSP_ENGINE_WAVE && prog->engine == DUSP_ENGINE_CHUNK) prog->migrate_to_chunk = true;
    return DUSP_OK;
    });
}

void dusp_program_destroy(dusp_program *prog) {
    if (!prog) return;
    (void)hipSetDevice(prog->ctx->device);
    // renders may have gone to a caller's stream: wait for what the last one recorded, not only for the context's own stream
    if (prog->rendered && prog->ev1) (void)hipEventSynchronize(prog->ev1);
    (void)hipStreamSynchronize(prog->ctx->stream);
    delete prog;
}

int dusp_program_info_get(const dusp_program *prog, dusp_program_info *info) {
    if (!prog || !info) return DUSP_ERR_ARG;
    std::memset(info, 0, sizeof *info);
    const dusp::Graph &g = prog->P.g;
    info->sample_rate = (uint32_t)g.sample_rate;
    info->chunk_size = (uint32_t)g.chunk;
    info->n_units = (uint32_t)g.units.size();
    info->n_out_channels = (uint32_t)prog->P.out_bufs.size();
    info->n_params = (uint32_t)g.n_params;
    info->engine = (uint32_t)prog->engine;
    info->n_device_ops = (uint32_t)prog->P.ops.size();
    info->n_inputs = (uint32_t)g.n_inputs;
    if (prog->engine == DUSP_ENGINE_FUSED) std::snprintf(info->shape, sizeof info->shape, "%s", prog->fused.shape.c_str());
    if (prog->engine == DUSP_ENGINE_WAVE && prog->jit_ok && (prog->jit_waves || !prog->rendered))
    {
        const int at = std::snprintf(info->shape, sizeof info->shape, "%s, compiled kernel: %d units, %dx%d", prog->P.feed_forward ? "feed-forward" : "feedback",
                                     (int)prog->P.ops.size(), prog->jit_waves, prog->jit_per_wave);
        if (at > 0 && (size_t)at < sizeof info->shape && (prog->jit_voices || prog->jit_segments > 1)) {
            if (prog->jit_voices && prog->jit_segments > 1) std::snprintf(info->shape + at, sizeof info->shape - (size_t)at, ", loop, %u seg", prog->jit_segments);
            else if (prog->jit_voices) std::snprintf(info->shape + at, sizeof info->shape - (size_t)at, ", voice loop");
            else if (prog->warm_redo_from) std::snprintf(info->shape + at, sizeof info->shape - (size_t)at, ", %u seg, redo@%u", prog->jit_segments, prog->warm_redo_from);
            else std::snprintf(info->shape + at, sizeof info->shape - (size_t)at, ", %u seg", prog->jit_segments);
        } else if (at > 0 && (size_t)at < sizeof info->shape && prog->jit_scan)
            std::snprintf(info->shape + at, sizeof info->shape - (size_t)at, ", scan");  // (the Filters as scans over the chunk: within the gate's bound, not bit for bit)
    }
    else if (prog->engine == DUSP_ENGINE_WAVE && prog->jit_ok)
        std::snprintf(info->shape, sizeof info->shape, "%s, %d chunk buffers in LDS (kernel compiling)", prog->P.feed_forward ? "feed-forward" : "feedback", prog->wave.n_slots);
    else if (prog->engine == DUSP_ENGINE_WAVE && prog->rendered && prog->wave_segments > 1)
        std::snprintf(info->shape, sizeof info->shape, "%s, %d chunk buffers in LDS, %u seg", prog->P.feed_forward ? "feed-forward" : "feedback", prog->wave.n_slots, prog->wave_segments);
    else if (prog->engine == DUSP_ENGINE_WAVE)
        std::snprintf(info->shape, sizeof info->shape, "%s, %d chunk buffers in LDS", prog->P.feed_forward ? "feed-forward" : "feedback", prog->wave.n_slots);
    if (prog->engine == DUSP_ENGINE_CHUNK && !prog->P.warm_ops.empty() && !prog->handoff_ok && !prog->handoff_why.empty())
        std::snprintf(info->shape, sizeof info->shape, "warm-up, then not compiled: %.34s", prog->handoff_why.c_str());
    if (prog->engine == DUSP_ENGINE_CHUNK && prog->handoff_ok && prog->jit_waves)
        std::snprintf(info->shape, sizeof info->shape, "%d warm-up chunks here, then compiled kernel: %d units, %dx%d", (int)prog->P.warm_ops.size(), (int)prog->P.ops.size(),
                      prog->jit_waves, prog->jit_per_wave);
    return DUSP_OK;
}

int dusp_state_download(dusp_program *prog, size_t instance, size_t unit, double *out, size_t cap) {
    if (!prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    return guarded(ctx->err, "dusp_state_download", [&]() -> int {
    if (!prog->rendered) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_state_download: nothing has been rendered yet");
    if (prog->mixed) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_state_download: the last render was a mix (dusp_render_host_mix, dusp_render_host_score): unit state describes its last tile only");
    const dusp::Graph &g = prog->P.g;
    if (unit >= g.units.size() || instance >= prog->last_n_inst || !out)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_state_download: unit / instance out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(prog->ev1));  // the render may have gone to a caller's stream: wait for what IT recorded
    const dusp::UnitDesc &u = g.units[unit];
    std::vector<double> words;
    auto or0 = [](double v) { return (v != v || v == 0) ? 0.0 : v; };
    // one device-to-host copy of the whole state array per render, however many units are read back afterwards
    const bool fused = prog->engine == DUSP_ENGINE_FUSED;
    const size_t stride = fused ? prog->last_n_inst : prog->last_n_pad;
    if (!prog->h_state_valid) {
        const size_t rows = fused ? (size_t)std::max(1, prog->fused.n_state_words) : std::max<size_t>(1, prog->P.init_state.size());
        prog->h_state.resize(rows * stride);
        HIP_TRY(ctx, hipMemcpy(prog->h_state.data(), fused ? prog->d_fused_state.p : prog->d_state.p, rows * stride * sizeof(double),
                               hipMemcpyDeviceToHost));
        prog->h_state_valid = true;
    }
    if (fused) {
        const int first = prog->fused.unit_state_first[unit], n = prog->fused.unit_state_count[unit];
        for (int k = 0; k < n; k++) words.push_back(prog->h_state[(size_t)(first + k) * stride + instance]);
    } else {
        auto rd = [&](int slot, double &v) {
            v = prog->h_state[(size_t)slot * stride + instance];
            return hipSuccess;
        };
        const int n_ch = (u.op == dusp::OP_FILTER) ? u.n_out : 1;
        const int per = u.op == dusp::OP_DELAY ? 0 : u.slots_per_ch;  // Delay's slot is engine-internal, not unit state
        // (FixedDelay / CombFilter / AllPass / ReadBackDelay: one word, the ring position; MonoDelay: none)
        if (u.op == dusp::OP_SAMPLE_RATE_REDUX) {  // [timeSinceLastUpdate, n, held value per channel]; `val` is `[0]` until the first update
            double since;
            HIP_TRY(ctx, rd(u.first_slot, since));
            const int n_val = std::isinf(since) ? 1 : u.n_out;
            words.push_back(since);
            words.push_back((double)n_val);
            for (int c = 0; c < n_val; c++) {
                double v;
                HIP_TRY(ctx, rd(u.first_slot + c * per + 1, v));
                words.push_back(v);
            }
        } else if (u.op == dusp::OP_MULTI_OSC) {  // [n, phase per channel]
            words.push_back((double)u.n_out);
            for (int c = 0; c < u.n_out; c++) {
                double v;
                HIP_TRY(ctx, rd(u.first_slot + c * per, v));
                words.push_back(v);
            }
        } else if (u.op == dusp::OP_FILTER) {
            for (int k = 0; k < 7; k++) {
                double v;
                HIP_TRY(ctx, rd(u.first_slot + k, v));
                words.push_back(v);
            }
            words.push_back((double)n_ch);
            for (int c = 0; c < n_ch; c++)
                for (int k = 7; k < 11; k++) {
                    double v;
                    HIP_TRY(ctx, rd(u.first_slot + c * per + k, v));
                    words.push_back(or0(v));
                }
        } else {
            for (int k = 0; k < per; k++) {
                double v;
                HIP_TRY(ctx, rd(u.first_slot + k, v));
                words.push_back(v);
            }
        }
    }
    for (size_t k = 0; k < words.size() && k < cap; k++) out[k] = words[k];
    return (int)words.size();
    });
}

int dusp_last_kernel_ms(dusp_program *prog, float *ms) {
    if (!prog || !ms) return DUSP_ERR_ARG;
    dusp_ctx *ctx = prog->ctx;
    if (!prog->rendered) CTX_FAIL(ctx, DUSP_ERR_STATE, "dusp_last_kernel_ms: nothing has been rendered yet");
    HIP_TRY(ctx, hipEventSynchronize(prog->ev1));
    HIP_TRY(ctx, hipEventElapsedTime(ms, prog->ev0, prog->ev1));
    return DUSP_OK;
}

int dusp_circuit_kernel_source(const double *desc, size_t n_words, int waves, int per_wave, int lds_table, int compile, char *text, size_t cap) {
    return guarded(g_error, "dusp_circuit_kernel_source", [&]() -> int {
    if (!desc || (cap && !text)) {
        g_error = "dusp_circuit_kernel_source: NULL argument";
        return DUSP_ERR_ARG;
    }
    if (waves < 1 || waves > 16 || per_wave < 1 || per_wave > 4) {
        g_error = "dusp_circuit_kernel_source: waves must be 1 .. 16 and per_wave 1 .. 4";
        return DUSP_ERR_ARG;
    }
    // (descriptor -> program -> plan -> options -> text: host code only, jit_codegen.hpp jit_source_from_descriptor — the same function the
    // sanitizer build of tests/native/hostcheck.cpp drives with malformed descriptors)
    dusp::JitSourceRequest rq;
    rq.waves = waves;
    rq.per_wave = per_wave;
    rq.continued = (lds_table & 2) != 0;
    rq.lean_recurrence = (lds_table & 4) != 0;  // (the Filter stage's recurrence loop with 4 P values per register set: what a render falls back to when the kernel spills)
    rq.lds_table = (lds_table & 1) != 0;
    rq.scan_knob = getenv("DUSP_FILTER_SCAN") ? atoi(getenv("DUSP_FILTER_SCAN")) : 1;
    rq.lean = !(getenv("DUSP_JIT_LEAN") && atoi(getenv("DUSP_JIT_LEAN")) == 0);
    rq.delay_line = getenv("DUSP_DELAY_LINE") ? atoi(getenv("DUSP_DELAY_LINE")) : 1;
    if (const char *range = getenv("DUSP_CUTOFF_RANGE"))  // (tests of the generator: "lo,hi" = what a renderer would have found in the Filters' cutoff columns)
        if (sscanf(range, "%lf,%lf", &rq.cutoff_lo, &rq.cutoff_hi) != 2) rq.cutoff_lo = rq.cutoff_hi = 0.0;
    dusp::JitSource src;
    std::string err;
    const int verdict = dusp::jit_source_from_descriptor(desc, n_words, rq, src, err);
    if (verdict != 0) {
        g_error = "dusp_circuit_kernel_source: " + err;
        return verdict == 1 ? DUSP_ERR_ARG : DUSP_ERR_UNSUPPORTED;
    }
    if (compile && !dusp::jit_compile_only(src.text, nullptr, err)) {
        g_error = "dusp_circuit_kernel_source: " + err;
        return DUSP_ERR_HIP;
    }
    if (cap) {
        const size_t n = std::min(cap - 1, src.text.size());
        std::memcpy(text, src.text.data(), n);
        text[n] = 0;
    }
    return (int)std::min<size_t>(src.text.size(), 0x7fffffff);
    });
}

int dusp_descriptor_channels(const double *desc, size_t n_words) {
    return guarded(g_error, "dusp_descriptor_channels", [&]() -> int {
    if (!desc) {
        g_error = "dusp_descriptor_channels: NULL argument";
        return DUSP_ERR_ARG;
    }
    dusp::Program P;  // (descriptor -> program: host code only, what dusp_program_build does first)
    std::string err;
    if (!dusp::compile(desc, n_words, P, err, /*continuation=*/false)) {
        g_error = "dusp_descriptor_channels: " + err;
        return DUSP_ERR_ARG;
    }
    return (int)P.out_bufs.size();
    });
}

}  // extern "C"
