// abi_render_jit.hip — the render of a WAVE program on the kernel compiled for its circuit, in named steps (render_jit at the end).
// WAVE programs the circuit compiler takes: ONE kernel generated for this circuit's structure (jit_codegen.hpp), compiled for
// gfx950 in process the first time the structure is seen (jit_engine.hip), cached from then on.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "abi_internal.hpp"
#include "jit_engine.hpp"
#include "jit_plan.hpp"

// What the steps of render_jit hand on to each other
struct JitRender {
    dusp::JitArgs a{};
    dusp::JitPlan plan;
    hipFunction_t render = nullptr;
    dusp::JitSource *src = nullptr;
    int scratch = 0;    // bytes of scratch per lane of the kernel at hand
    unsigned grid = 0;  // workgroups of the render launch
    DevBuf<unsigned long long> d_debug;  // diagnostic build: what wave 0 of every workgroup measured
    JitRender() = default;
    JitRender(const JitRender &) = delete;
    JitRender &operator=(const JitRender &) = delete;
    ~JitRender() { d_debug.release(); }  // (whichever step the render leaves by)
};

// Per-instance (parameter) delays: the kernel a Delay gets depends on where its instances' values lie — all of at least a chunk
// (write-once ring), all below a chunk (no ring), or neither (ordered slot operations) — so the column is looked at first
// (one small launch + a few bytes back; only programs with such a unit pay it).  The verdict lives in the operand's spare word.
// Per-instance CUTOFFS of Filters likewise: whether the Filter may run as a scan (jit_filter_scan_ok) depends on the range of the
// column — its smallest and largest value travel back with the Delays' verdicts, behind the same synchronisation.
static int jit_classify_columns(dusp_program *prog, uint32_t n_inst, const float *d_params, bool persistent, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    std::vector<int64_t> entries;
    std::vector<size_t> which, filters;
    std::vector<int> slots;
    for (size_t k = 0; k < prog->P.ops.size(); k++) {
        const dusp::DevOp &op = prog->P.ops[k];
        if ((op.op == dusp::OP_DELAY || op.op == dusp::OP_MONO_DELAY) && op.in[1].kind == dusp::SRC_PARAM) {
            entries.insert(entries.end(), {(int64_t)op.in[1].idx, op.ring_len, (int64_t)(op.op == dusp::OP_MONO_DELAY)});
            which.push_back(k);
        }
        if (op.op == dusp::OP_FILTER && op.in[1].kind == dusp::SRC_PARAM && ctx->knobs.filter_scan != 0 && !persistent) {
            slots.push_back(op.in[1].idx);
            filters.push_back(k);
        }
    }
    if (which.empty() && filters.empty()) return DUSP_OK;
    const size_t n = which.size(), nf = filters.size();
    HIP_TRY(ctx, prog->d_jit_regime.ensure(4 * n + 2 * nf + 2));  // [3 n] entries as int64, n verdicts (one int64 slot each), then nf slots (int) and 3 nf range words (unsigned)
    int64_t *d_entries = prog->d_jit_regime.p;
    int *d_bits = (int *)(prog->d_jit_regime.p + 3 * n);
    int *d_slots = (int *)(prog->d_jit_regime.p + 4 * n);
    unsigned *d_range = (unsigned *)(d_slots + nf);
    std::vector<int> bits(n, 0);
    std::vector<unsigned> range(3 * nf, 0u);
    if (n) {
        HIP_TRY(ctx, hipMemcpyAsync(d_entries, entries.data(), 3 * n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipMemsetAsync(d_bits, 0, n * sizeof(int64_t), stream));
        HIP_TRY(ctx, dusp::jit_launch_classify_delays(d_params, n_inst, d_entries, (int)n, d_bits, stream));
        HIP_TRY(ctx, hipMemcpyAsync(bits.data(), d_bits, n * sizeof(int), hipMemcpyDeviceToHost, stream));
    }
    if (nf && !prog->mix_range.empty()) {  // a tile of a mix: the range of the whole batch's column
        for (size_t i = 0; i < nf; i++)
            for (int j = 0; j < 3; j++) range[3 * i + j] = prog->mix_range[3 * (size_t)slots[i] + j];
    } else if (nf) {
        HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), nf * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipMemsetAsync(d_range, 0, 3 * nf * sizeof(unsigned), stream));
        HIP_TRY(ctx, dusp::jit_launch_column_range(d_params, n_inst, d_slots, (int)nf, d_range, stream));
        HIP_TRY(ctx, hipMemcpyAsync(range.data(), d_range, 3 * nf * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    bool changed = false;
    for (size_t i = 0; i < n; i++) {
        const int regime = bits[i] == dusp::DELAY_REGIME_LONG || bits[i] == dusp::DELAY_REGIME_SHORT ? bits[i] : dusp::DELAY_REGIME_OTHER;
        int32_t &pad = prog->P.ops[which[i]].in[1].pad;
        changed = changed || pad != regime;
        pad = regime;
    }
    for (size_t i = 0; i < nf; i++) {  // (the range itself is no part of the text: only whether the circuit's Filters scan — the key of jit_src — is)
        dusp::DevOp &op = prog->P.ops[filters[i]];
        const bool known = range[3 * i + 2] == 0u && range[3 * i] != 0u && range[3 * i + 1] != 0u;
        op.in[1].pad = known ? dusp::kFilterColumnKnown : 0;
        if (known) {
            float lo, hi;
            const unsigned lo_bits = 0x7fffffffu - range[3 * i], hi_bits = range[3 * i + 1];
            std::memcpy(&lo, &lo_bits, 4);
            std::memcpy(&hi, &hi_bits, 4);
            op.d[0] = (double)lo;
            op.d[1] = (double)hi;
        }
    }
    if (changed) {  // (another kernel text: the generated units differ)
        prog->jit_src.clear();
        prog->jit_consts_uploaded = false;
    }
    return DUSP_OK;
}

// Everything a render decides before it touches the device (jit_plan.hpp), for this context and this batch
static int jit_plan_render(dusp_program *prog, JitRender &R, uint32_t n_inst, uint32_t n_chunks, bool persistent, bool resume, bool handoff, bool inputs) {
    dusp_ctx *ctx = prog->ctx;
    if (prog->voice_loop < 0) {
        dusp::VoicePlan voices;
        prog->voice_loop = !persistent && prog->P.ops.size() > dusp::jit_loop_voices_from() && dusp::jit_find_voices(prog->P, prog->wave, voices) ? 1 : 0;
    }
    dusp::JitSite site;
    site.n_cus = ctx->n_cus;
    site.knobs = ctx->knobs;
    for (int k = 0; k < dusp::kNumTables; k++)
        site.table_form[k] = ctx->table_form[k], site.table_delta[k] = ctx->table_delta[k], site.table_bound[k] = ctx->table_bound[k], site.table_antisym[k] = ctx->table_antisym[k];
    dusp::JitBatch batch;
    batch.n_inst = n_inst;
    batch.n_chunks = n_chunks;
    batch.persistent = persistent;
    batch.resume = resume;
    batch.handoff = handoff;
    batch.inputs = inputs;
    batch.voice_loop = prog->voice_loop != 0;
    batch.whole_n_inst = prog->mix_n_inst;
    batch.param_bound = prog->param_bound.empty() ? nullptr : prog->param_bound.data();
    batch.params_unknown = prog->P.g.n_params > 0 && prog->param_bound.empty();
    R.plan = dusp::jit_plan(site, batch, prog->P, prog->wave);
    if (R.plan.error) CTX_FAIL(ctx, DUSP_ERR_ARG, R.plan.error);
    R.a.n_seg = R.plan.n_seg;
    R.a.seg_groups = R.plan.seg_groups;
    R.a.warm = R.plan.warm ? 1u : 0u;
    return DUSP_OK;
}

// The kernel for the plan's geometry: its text generated or found by jit_source_key, compiled (or, wait == false, left to a background
// thread: kJitLater), and — where it spills — the next geometry of the ladder (jit_plan.hpp jit_spill_step) until one does not.
static int jit_obtain_kernel(dusp_program *prog, JitRender &R, uint32_t n_inst, uint32_t n_chunks, bool wait) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    dusp::JitPlan &plan = R.plan;
    dusp::JitOptions &opt = plan.opt;
    auto text_of = [&](const dusp::JitOptions &o, std::string *why) -> dusp::JitSource * {  // found, or generated now (nullptr: the compiler refuses, *why says why)
        auto it = prog->jit_src.find(dusp::jit_source_key(o));
        if (it == prog->jit_src.end()) {
            dusp::JitSource gen;
            if (!dusp::jit_generate(P, prog->wave, o, gen)) {
                if (why) *why = gen.why;
                return nullptr;
            }
            it = prog->jit_src.emplace(dusp::jit_source_key(o), std::move(gen)).first;
        }
        return &it->second;
    };
    for (;;) {  // a kernel that spills (128 registers per lane at 16 wavefronts) is rebuilt for fewer instances per wave, then fewer waves
        std::string why;
        R.src = text_of(opt, &why);
        if (!R.src) CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, "render: circuit compiler: " + why);
        // A structure seen for the first time costs a compile of 0.3-0.8 s.  A render the interpreter kernel finishes sooner
        // than that does not wait for it: the compile starts in a background thread, THIS render runs on the interpreter (same
        // PCM, same state), and the next render of the structure — in this process, or in any with DUSP_JIT_CACHE set — finds
        // its kernel.  DUSP_WAVE_JIT=2 always waits (tests, benchmarks).
        if (ctx->knobs.wave_jit == 1 && !wait && !dusp::jit_code_ready(R.src->text)) {
            // interpreter: ~0.7 ns per unit and chunk with the chip full, ~1 us per unit and chunk along one wavefront's serial path
            const double units = (double)P.ops.size();
            const double est_ms = std::max(units * (double)n_inst * n_chunks * 0.7e-6, units * (double)plan.seg_groups * 1.0e-3);
            if (est_ms < 400.0) {
                dusp::jit_compile_in_background(R.src->text);
                if (plan.filter_stage && opt.filter_block == 8) {
                    // (a Filter stage's kernel at 16 wavefronts usually ends on the recurrence loop's narrower form: that text joins the
                    // queue now, so the geometry search does not cost a further render on the interpreter per step)
                    dusp::JitOptions narrow = opt;
                    narrow.filter_block = 4;
                    const dusp::JitSource *alt = text_of(narrow, nullptr);
                    if (alt && !dusp::jit_code_ready(alt->text)) dusp::jit_compile_in_background(alt->text);
                }
                return kJitLater;
            }
        }
        std::string err;
        int scratch = 0;
        if (!dusp::jit_get_kernel(ctx->device, R.src->text, "dusp_jit_render", &R.render, &scratch, err))
            CTX_FAIL(ctx, DUSP_ERR_HIP, "render: circuit compiler: " + err);
        R.scratch = scratch;
        if (ctx->knobs.jit_log) fprintf(stderr, "[dusp jit] %d waves x %d instances, filter block %d: %d bytes of scratch per lane\n", plan.waves, plan.per_wave, opt.filter_block, scratch);
        if (scratch <= ctx->knobs.jit_spill_bytes || ctx->knobs.jit_force_waves) break;  // (a few registers spilled outside the hot path is cheaper than halving the instances in flight)
        if (!dusp::jit_spill_step(plan)) break;
    }
    return DUSP_OK;
}

// (from here on the render happens on the compiled kernel) State, rings, parked outlets; the text's constants on the device
static int jit_workspaces(dusp_program *prog, JitRender &R, uint32_t n_chunks, bool persistent, bool resume, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    dusp::JitArgs &a = R.a;
    const dusp::JitSource *src = R.src;
    HIP_TRY(ctx, prog->d_state.ensure(std::max<size_t>(1, P.init_state.size()) * a.n_pad));
    a.state = prog->d_state.p;
    if (P.ring_samples && !resume) {  // Delay rings start as zeros (Delay.js:14); layout [instance][slot]
        HIP_TRY(ctx, prog->d_rings.ensure((size_t)P.ring_samples * a.n_pad));
        HIP_TRY(ctx, zero_rings(prog, a.n_pad, n_chunks, true, stream));
    }
    a.rings = prog->d_rings.p;
    a.resume = resume ? 1u : 0u;
    a.save_bufs = persistent ? 1u : 0u;
    a.n_bufs = (uint32_t)std::max(1, P.n_bufs);
    if (persistent) {  // every outlet's last chunk, parked between launches (the interpreter kernel's layout: either may continue the other)
        HIP_TRY(ctx, prog->d_saved_bufs.ensure((size_t)a.n_bufs * dusp::kChunk * a.n_inst));
        a.saved_bufs = prog->d_saved_bufs.p;
    }
    prog->keep_memory = false;
    if (!prog->jit_consts_uploaded) {
        HIP_TRY(ctx, prog->d_jit_fk.ensure(std::max<size_t>(1, src->fk.size())));
        HIP_TRY(ctx, prog->d_jit_dk.ensure(std::max<size_t>(1, src->dk.size())));
        if (!src->fk.empty()) HIP_TRY(ctx, hipMemcpyAsync(prog->d_jit_fk.p, src->fk.data(), src->fk.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        if (!src->dk.empty()) HIP_TRY(ctx, hipMemcpyAsync(prog->d_jit_dk.p, src->dk.data(), src->dk.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        std::vector<int> scan(2 * src->scans.size() + 2, 0);
        for (size_t i = 0; i < src->scans.size(); i++) {
            scan[i] = src->scans[i].state_slot;
            scan[src->scans.size() + i] = src->scans[i].level;
        }
        HIP_TRY(ctx, prog->d_jit_scan.ensure(scan.size()));
        HIP_TRY(ctx, hipMemcpyAsync(prog->d_jit_scan.p, scan.data(), scan.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));  // (the host vectors above are temporaries / may be regenerated)
        prog->jit_consts_uploaded = true;
    }
    a.fk = prog->d_jit_fk.p;
    a.dk = prog->d_jit_dk.p;
    return DUSP_OK;
}

// Time segments of a circuit with scanned oscillators: one accumulate pass + prefix per FM level that has them, in front of the render pass
static int jit_accumulate_passes(dusp_program *prog, JitRender &R, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    dusp::JitArgs &a = R.a;
    const dusp::JitSource *src = R.src;
    if (!(a.n_seg > 1 && !src->scans.empty())) return DUSP_OK;
    const size_t per = src->scans.size() * (size_t)a.n_inst * a.n_seg;
    HIP_TRY(ctx, prog->d_seg.ensure(2 * per));
    a.seg_sum = prog->d_seg.p;
    a.seg_start = prog->d_seg.p + per;
    for (int level : src->pass_levels) {
        hipFunction_t pass = nullptr;
        std::string err;
        if (!dusp::jit_get_kernel(ctx->device, src->text, "dusp_jit_pass" + std::to_string(level), &pass, nullptr, err))
            CTX_FAIL(ctx, DUSP_ERR_HIP, "render: circuit compiler: " + err);
        dusp::JitArgs own = a;
        own.warm = 0u;  // (a pass totals every segment's OWN chunks, whatever the render kernel does in front of them)
        HIP_TRY(ctx, dusp::jit_launch(pass, own, R.grid, (unsigned)R.plan.waves * 64, stream));
        HIP_TRY(ctx, dusp::jit_launch_prefix(a.seg_sum, a.seg_start, prog->d_init.p, prog->d_jit_scan.p, prog->d_jit_scan.p + src->scans.size(),
                                             (int)src->scans.size(), level, a.n_inst, a.n_seg, a.sample_rate, stream));
    }
    return DUSP_OK;
}

static int jit_launch_render(dusp_program *prog, JitRender &R, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    dusp::JitArgs &a = R.a;
    if (R.plan.opt.profile) {
        HIP_TRY(ctx, R.d_debug.ensure((size_t)R.grid * 16));
        HIP_TRY(ctx, hipMemsetAsync(R.d_debug.p, 0, (size_t)R.grid * 16 * sizeof(unsigned long long), stream));
        a.debug = R.d_debug.p;
    }
    if (a.warm) {
        HIP_TRY(ctx, prog->d_warm_records.ensure((size_t)std::max(1, R.plan.opt.filter_stages) * R.plan.n_virtual * 8));
        a.warm_records = prog->d_warm_records.p;
    }
    HIP_TRY(ctx, dusp::jit_launch(R.render, a, R.grid, (unsigned)R.plan.waves * 64, stream));
    return DUSP_OK;
}

// Segments that warmed up: does every Filter stage hold, where a segment's own chunks begin, what the segment before ended with?  Then —
// by induction from the first segment, which started from the render's true state — every stored sample is the sequential render's.
// Otherwise the render is finished sequentially from the last segment that is known to be right: one wavefront from that
// segment's first chunk on, its Filters started from the state recorded there (x1 x2 y1 y2 of every stage into a copy of the start state).
static int jit_check_warm(dusp_program *prog, JitRender &R, uint32_t n_chunks, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    const dusp::JitArgs &a = R.a;
    const dusp::JitOptions &opt = R.plan.opt;
    const uint32_t n_inst = a.n_inst;
    const uint64_t n_virtual = R.plan.n_virtual;
    const unsigned per_block = (unsigned)(R.plan.waves * R.plan.per_wave);
    const size_t n_rec = (size_t)opt.filter_stages * n_virtual * 8;
    std::vector<double> rec(n_rec);
    HIP_TRY(ctx, hipMemcpyAsync(rec.data(), prog->d_warm_records.p, n_rec * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    uint32_t bad = 0;  // first segment (of any instance) whose start differs from its predecessor's end (0: none)
    for (uint32_t i = 0; i < n_inst; i++)
        for (uint32_t s = 1; s < a.n_seg && (!bad || s < bad); s++)
            for (int st = 0; st < opt.filter_stages; st++) {
                const double *now = rec.data() + ((size_t)st * n_virtual + (size_t)i * a.n_seg + s) * 8, *before = now - 8;
                if (!(now[0] == before[2] && now[1] == before[3])) bad = s;  // (a NaN never equals: such a render is finished as written)
            }
    prog->warm_redo_from = bad;
    if (bad && (n_inst > 1 || !R.src->scans.empty())) {
        // several instances (each with a state of its own by then), or scanned oscillators (their phases are the passes' business): the whole
        // render once more, every instance as one chain from its first chunk
        dusp::JitArgs whole = a;
        whole.warm = 0u;
        whole.n_seg = 1u;
        whole.seg_groups = n_chunks;
        const unsigned blocks = (unsigned)((n_inst + per_block - 1) / per_block);
        HIP_TRY(ctx, dusp::jit_launch(R.render, whole, blocks, (unsigned)R.plan.waves * 64, stream));
        prog->warm_redo_from = 1;
    } else if (bad) {
        std::vector<double> init(P.init_state);
        int st = 0;
        for (int k : prog->wave.order) {  // (stage ordinals are dealt in the plan's execution order: jit_codegen.hpp filter_ordinal)
            const dusp::DevOp &op = P.ops[(size_t)k];
            if (op.op == dusp::OP_FILTER) {
                const double *before = rec.data() + ((size_t)st * n_virtual + (bad - 1)) * 8;
                const size_t at = (size_t)op.state_slot;
                if (at + 11 <= init.size()) init[at + 7] = before[4], init[at + 8] = before[5], init[at + 9] = before[2], init[at + 10] = before[3];
                st++;
            }
        }
        HIP_TRY(ctx, prog->d_warm_init.ensure(init.size()));
        HIP_TRY(ctx, hipMemcpyAsync(prog->d_warm_init.p, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        dusp::JitArgs rest = a;
        rest.warm = 0u;
        rest.n_seg = 1u;
        rest.g_first = bad * a.seg_groups;
        rest.seg_groups = n_chunks;
        rest.init_state = prog->d_warm_init.p;
        HIP_TRY(ctx, dusp::jit_launch(R.render, rest, 1u, (unsigned)R.plan.waves * 64, stream));
        HIP_TRY(ctx, hipStreamSynchronize(stream));  // (`init` is a temporary)
    }
    return DUSP_OK;
}

// diagnostic build: what wave 0 of the workgroups measured (mean over workgroups), to stderr
static int jit_profile_report(dusp_program *prog, JitRender &R, hipStream_t stream) {
    dusp_ctx *ctx = prog->ctx;
    const unsigned grid = R.grid;
    std::vector<unsigned long long> h((size_t)grid * 16);
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    HIP_TRY(ctx, hipMemcpy(h.data(), R.d_debug.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    double loop = 0, serial = 0, chunks = 0;
    double ph[12] = {0};
    for (unsigned b = 0; b < grid; b++) {
        loop += (double)h[b * 16], serial += (double)h[b * 16 + 1] + (double)h[b * 16 + 3], chunks += (double)h[b * 16 + 2];
        for (int i = 0; i < 12; i++) ph[i] += (double)h[b * 16 + 4 + i];
    }
    std::fprintf(stderr, "[dusp jit profile] %ux%d waves x instances (%d B of scratch per lane), %u workgroups: chunk loop %.0f cycles per chunk, of which Filter recurrences %.0f (%.1f per sample-step)\n",
                 (unsigned)R.plan.waves, R.plan.per_wave, R.scratch, grid, loop / std::max(1.0, chunks), serial / std::max(1.0, chunks), serial / std::max(1.0, chunks) / 256.0);
    std::fprintf(stderr, "[dusp jit profile]   barrier to barrier, as wave 0 sees them:");
    for (int i = 0; i < 12; i++)
        if (ph[i] > 0) std::fprintf(stderr, " %s%.0f", i == 11 ? "| tail " : "", ph[i] / std::max(1.0, chunks));
    std::fprintf(stderr, "\n");
    return DUSP_OK;
}

// handoff_chunks > 0: this launch continues a render whose first handoff_chunks chunks the chunk engine has just rendered (Program::warm_ops):
// start state in d_handoff_init, rings and outlets' last chunk already in this kernel's layout.
// probe: only find out whether the kernel is at hand (DUSP_OK) or being compiled in the background (kJitLater); nothing is launched.
int render_jit(dusp_program *prog, uint32_t n_inst, size_t n_samples, uint32_t n_chunks, const float *d_params, const float *d_inputs, float *d_out,
               hipStream_t stream, uint32_t handoff_chunks, bool probe) {
    dusp_ctx *ctx = prog->ctx;
    const dusp::Program &P = prog->P;
    const uint32_t n_pad = (n_inst + 63u) & ~63u;
    const bool persistent = (prog->resumable && prog->persistent) || handoff_chunks > 0;
    const bool resume = prog->keep_memory || handoff_chunks > 0;
    if (resume && !handoff_chunks && n_inst != prog->last_n_inst) CTX_FAIL(ctx, DUSP_ERR_STATE, "render: the instance count cannot change while a program is being continued");
    if (int rc = jit_classify_columns(prog, n_inst, d_params, persistent, stream)) return rc;
    if (prog->jit_table_generation != ctx->table_generation) {  // a table was uploaded since: forms / the LDS image may have changed
        prog->jit_src.clear();
        prog->jit_consts_uploaded = false;
        prog->jit_table_generation = ctx->table_generation;
    }

    JitRender R;
    dusp::JitArgs &a = R.a;
    a.params = d_params;
    a.tables = ctx->d_tables;
    a.inputs = d_inputs;
    a.out = d_out;
    a.state = prog->d_state.p;
    a.init_state = handoff_chunks ? prog->d_handoff_init.p : prog->d_init.p;
    a.n_samples = n_samples;
    a.ring_samples = (uint64_t)P.ring_samples;
    a.clock0 = (uint64_t)P.g.clock0 + (uint64_t)handoff_chunks * dusp::kChunk;
    a.n_inst = n_inst;
    a.n_pad = n_pad;
    a.n_groups = n_chunks;
    a.sample_rate = (uint32_t)P.g.sample_rate;
    a.table_stride = ctx->table_stride;
    a.vec4_ok = (n_samples % 4 == 0) && (((uintptr_t)d_out & 15) == 0);
    a.n_out = (uint32_t)P.out_bufs.size();
    if (int rc = jit_plan_render(prog, R, n_inst, n_chunks, persistent, resume, handoff_chunks > 0, d_inputs != nullptr)) return rc;
    // (a tile of a mix waits like a hand-off: a mix whose first tiles ran on the interpreter and whose later ones on the kernel would sum the Filter
    // stage's arithmetic and the scan's, split wherever the compile happened to finish)
    if (int rc = jit_obtain_kernel(prog, R, n_inst, n_chunks, /*wait=*/(handoff_chunks && !probe) || prog->mix_n_inst)) return rc;  // (kJitLater included)
    if (probe) return DUSP_OK;
    if (int rc = jit_workspaces(prog, R, n_chunks, persistent, resume, stream)) return rc;
    const unsigned per_block = (unsigned)(R.plan.waves * R.plan.per_wave);
    R.grid = (unsigned)((R.plan.n_virtual + per_block - 1) / per_block);
    if (!handoff_chunks) HIP_TRY(ctx, hipEventRecord(prog->ev0, stream));  // (a hand-off's clock started in front of the chunk engine's part)
    if (int rc = jit_accumulate_passes(prog, R, stream)) return rc;
    if (int rc = jit_launch_render(prog, R, stream)) return rc;
    if (a.warm)
        if (int rc = jit_check_warm(prog, R, n_chunks, stream)) return rc;
    HIP_TRY(ctx, hipEventRecord(prog->ev1, stream));
    if (R.plan.opt.profile)
        if (int rc = jit_profile_report(prog, R, stream)) return rc;
    prog->jit_waves = R.plan.waves;
    prog->jit_per_wave = R.plan.per_wave;
    prog->jit_segments = a.n_seg;
    prog->jit_voices = R.src->voice_loop;
    prog->jit_scan = R.plan.opt.filter_scan;
    if (!a.warm) prog->warm_redo_from = 0;
    finish_render(prog, n_inst, n_pad, (uint64_t)n_chunks + handoff_chunks);
    return DUSP_OK;
}
