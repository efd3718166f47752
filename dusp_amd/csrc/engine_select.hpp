// engine_select.hpp — which engine renders a program: AUTO's fused -> wave -> chunk order, the rules for resumable and continued programs,
// whether the circuit compiler takes the program, and whether a program whose channel counts still grow hands over to a compiled kernel
// behind its warm-up chunks.  Plain data in, plain data out: host code only (no HIP), so that tests/native/engine_select_check.cpp and the
// sanitizer build (tests/native/hostcheck.cpp) run the very logic dusp_program_build / dusp_program_continue run (abi_program.hip finish_build).
#pragma once
#include <string>
#include <utility>
#include <vector>

#include "../../include/dusp_hip.h"
#include "jit_codegen.hpp"

namespace dusp {

// What the caller knows besides the compiled Program
struct EngineRequest {
    int requested = DUSP_ENGINE_AUTO;  // AUTO, CHUNK, FUSED or WAVE
    bool resumable = false;            // built with DUSP_ENGINE_RESUMABLE
    bool rendered = false;             // a continuation: the program has rendered before ...
    int engine_so_far = DUSP_ENGINE_CHUNK;  // ... on this engine
    bool delay_changed = false;        // ... and a continuation changed a Delay's constant
    int wave_jit = 1;                  // Knobs::wave_jit (0: no compiled kernels)
    // the context's tables: uploaded, and no nonzero entry below 2^-20
    bool table_set[kNumTables] = {false, false, false, false, false};
    bool table_fx32_ok[kNumTables] = {false, false, false, false, false};
};

struct EngineChoice {
    int engine = DUSP_ENGINE_CHUNK;
    int error = DUSP_OK;  // DUSP_ERR_UNSUPPORTED: `requested` cannot render this program (error_text says why; nothing else is valid but the plans)
    std::string error_text;
    FusedPlan fused;
    WavePlan wave;
    bool persistent = false;  // rings / feedback edges: device memory carries over between segments
    bool jit_ok = false;      // a WAVE program the circuit compiler takes
    std::string jit_why;
    bool handoff_ok = false;  // a CHUNK program that hands over to a compiled kernel behind its warm-up chunks
    std::string handoff_why;  // when not: what keeps the settled circuit on the chunk engine
};

// A fresh WavePlan that keeps the Ramp verdicts of the one before (they survive re-planning: a continued render's t sequence is a suffix)
inline void wave_plan_reset(WavePlan &wave) {
    auto checked = std::move(wave.ramp_checked);
    wave = WavePlan();
    wave.ramp_checked = std::move(checked);
}

// What the wave plan found out goes into the op list the kernels read: an Osc's FM depth (for time-split rendering) and whether a
// Ramp's t / duration may use the verified reciprocal
inline void wave_plan_write_back(const WavePlan &wave, std::vector<DevOp> &ops) {
    for (size_t k = 0; k < wave.osc_level.size() && k < ops.size(); k++)
        if (wave.osc_level[k] >= 0) ops[k].d[0] = (double)wave.osc_level[k];
    for (size_t k = 0; k < wave.ramp_fastdiv.size() && k < ops.size(); k++)
        if (ops[k].op == OP_RAMP) ops[k].attr = wave.ramp_fastdiv[k];
}

inline void delay_rings_exact(std::vector<DevOp> &ops, bool exact) {
    for (DevOp &op : ops)
        if (op.op == OP_DELAY || op.op == OP_MONO_DELAY) op.pad = exact ? kDelayExactRing : 0;
}

// `ramp_checked`: the verdicts of the program's previous WavePlan (empty for a new program).  Edits P.ops as described above.
inline EngineChoice engine_select(Program &P, const EngineRequest &rq, std::vector<WavePlan::RampChecked> ramp_checked = {}) {
    EngineChoice c;
    auto fail = [&](const std::string &text) -> EngineChoice & {
        c.error = DUSP_ERR_UNSUPPORTED;
        c.error_text = text;
        return c;
    };
    int engine = rq.requested;
    c.wave.ramp_checked = std::move(ramp_checked);
    bool fusable = plan_fused(P, c.fused);
    // The fused sum chain keeps its phases in 32.32 fixed point: no nonzero entry of its table may lie below 2^-20.  At an odd rate the
    // sine table's middle entry is sin(pi) ~ 1.2e-16 — there AUTO goes on to the next engine instead of building a program that cannot render.
    if (fusable && c.fused.kind == FUSED_SUMCHAIN && rq.table_set[c.fused.table_id] && !rq.table_fx32_ok[c.fused.table_id]) {
        fusable = false;
        c.fused.why = "the sum chain's wave table has entries below 2^-20";
    }
    const bool wavable = plan_wave(P, c.wave, rq.resumable);
    wave_plan_write_back(c.wave, P.ops);
    // A continuation of a resumable program never fails over the engine: the circuit's state may have left the regime of the
    // engine the program was built with (an oscillator phase gone NaN, ...); the choice then falls to AUTO's rules below.
    if (rq.rendered && rq.resumable && ((engine == DUSP_ENGINE_FUSED && !fusable) || (engine == DUSP_ENGINE_WAVE && !wavable))) engine = DUSP_ENGINE_AUTO;
    if (engine == DUSP_ENGINE_FUSED && !fusable) return fail("dusp_program_build: no fused kernel for this graph shape (" + c.fused.why + ")");
    if (engine == DUSP_ENGINE_WAVE && !wavable) return fail("dusp_program_build: the wave engine cannot run this graph (" + c.wave.why + ")");
    // A circuit with rings or a feedback edge carries device memory from one segment to the next.  The chunk engine keeps
    // all of it in HBM; the wave engine parks its LDS chunk buffers in HBM between launches.  An engine, once chosen, is
    // kept for the whole chain (ring layouts differ) — except that a wave program that stops being plannable migrates to
    // the chunk engine.
    c.persistent = P.ring_samples != 0 || !P.feed_forward;
    delay_rings_exact(P.ops, rq.resumable && c.persistent);  // continued programs keep their rings in the reference's own state (jit_codegen.hpp kDelayExactRing)
    if (rq.resumable && c.persistent) {
        if (engine != DUSP_ENGINE_AUTO && engine != DUSP_ENGINE_CHUNK && engine != DUSP_ENGINE_WAVE)
            return fail("dusp_program_build: a resumable program with delay lines / feedback runs on DUSP_ENGINE_WAVE or DUSP_ENGINE_CHUNK");
        if (rq.rendered)  // continuing: stay, or fall back to the chunk engine
            engine = (rq.engine_so_far == DUSP_ENGINE_WAVE && wavable && !rq.delay_changed) ? DUSP_ENGINE_WAVE : DUSP_ENGINE_CHUNK;
        else if (engine == DUSP_ENGINE_AUTO)
            engine = wavable ? DUSP_ENGINE_WAVE : DUSP_ENGINE_CHUNK;
    }
    // (the hand-written kernels for the feedback voice of BASELINE configs[3] — a one-stage and two two-stage forms, rounds 1 and 2 — are gone since
    // round 4: the kernel compiled for the circuit renders it in 8.0 ms (scan) / 12.0 ms (stage, bit-equal) against their 20.4, and whatever delay the voice has)
    if (engine == DUSP_ENGINE_AUTO) engine = fusable ? DUSP_ENGINE_FUSED : wavable ? DUSP_ENGINE_WAVE : DUSP_ENGINE_CHUNK;
    c.engine = engine;
    c.jit_ok = engine == DUSP_ENGINE_WAVE && rq.wave_jit != 0 && jit_eligible(P, c.wave, c.jit_why);
    // Channel counts that grow during the first chunks keep a program on the chunk engine — for those chunks.  When the SETTLED op list is
    // one the circuit compiler takes, a single circuit's render hands over behind them (abi_render.hip render_handoff: rings, outlets' last
    // chunk and unit state move into the compiled kernel's layout).
    if (engine == DUSP_ENGINE_CHUNK && !P.warm_ops.empty() && !rq.resumable && rq.requested == DUSP_ENGINE_AUTO && rq.wave_jit != 0 && P.g.n_inputs == 0) {
        wave_plan_reset(c.wave);
        std::string why;
        const bool planned = plan_wave(P, c.wave, /*will_continue=*/true, /*settled_only=*/true);
        if (!planned) c.handoff_why = c.wave.why;
        else if (!jit_eligible(P, c.wave, why)) c.handoff_why = why;
        if (planned && c.handoff_why.empty()) {
            c.handoff_ok = true;
            wave_plan_write_back(c.wave, P.ops);
            delay_rings_exact(P.ops, true);  // (the kernel continues rings the chunk engine kept in the reference's state)
        }
    }
    return c;
}

}  // namespace dusp
