// jit_plan.hpp — how a compiled circuit kernel is launched: time segments and whether they warm up, the kernel's options (table image, scan
// or Filter stage, delay lines), wavefronts x instances per wavefront, and the steps down from a geometry whose kernel spills.  Everything a
// render decides before it first touches the device, as plain data in, plain data out: host code only (no HIP), so that
// tests/native/jit_plan_check.cpp and the sanitizer build (tests/native/hostcheck.cpp) run the very logic a render runs.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>

#include "jit_codegen.hpp"

namespace dusp {

// What the caller knows about this render (the site — chip, knobs, tables — is jit_codegen.hpp JitSite)
struct JitBatch {
    uint32_t n_inst = 1, n_chunks = 1;
    bool persistent = false;  // a resumable program with rings / feedback edges, or a hand-off: outlets parked between launches
    bool resume = false;      // this launch continues another
    bool handoff = false;     // ... namely the chunk engine's first chunks of this render (Program::warm_ops)
    bool inputs = false;      // the circuit reads host-generated signals
    bool voice_loop = false;  // the circuit's voices run in a loop (jit_find_voices said so, once per program)
    uint32_t whole_n_inst = 0;  // a tile of a mix (dusp_render_host_mix): the instances of the whole batch, which decide whether segments warm up
    const double *param_bound = nullptr;  // [n_params] largest magnitude of every parameter column, where the caller's table is in host memory (fused_plan.hpp wave_split_exact)
    bool params_unknown = false;          // the render has per-instance parameters and no table in host memory (a render from device memory): nothing bounds them
};

struct JitPlan {
    uint32_t n_seg = 1, seg_groups = 1;  // time segments, chunks per segment
    bool warm = false;                   // ... that start a segment early and warm up (jit_warm_chunks)
    uint64_t n_virtual = 1;              // instances x segments: what the grid is cut from
    JitOptions opt;
    int waves = 1, per_wave = 1;         // the geometry to try first (jit_spill_step: the next one)
    int per_wave_cap = 1, most = 16;
    size_t budget = 0;                   // LDS left of the 160 KiB beside the wavefronts' scratch
    bool filter_stage = false;
    const char *error = nullptr;         // DUSP_JIT_FORCE asked for a geometry that does not fit
};

// Few instances, long render: cut time into segments so that the whole chip works on it (splittable circuits; the interpreter kernel
// of the wave engine and the compiled kernels share the rule).  wave_segments: the knob (0 / 1: off; n: force n segments; -1: automatic).
inline void jit_time_segments(int n_cus, int wave_segments, uint32_t n_inst, uint32_t n_chunks, uint32_t &n_seg_out, uint32_t &seg_groups) {
    n_seg_out = 1;
    seg_groups = n_chunks;
    const uint64_t target = (uint64_t)n_cus * 8;  // wavefronts that fill the chip
    uint64_t n_seg = n_inst >= target ? 1 : std::min<uint64_t>(target / n_inst, n_chunks / 8);
    if (wave_segments >= 0) n_seg = (uint64_t)wave_segments;
    n_seg = std::max<uint64_t>(1, std::min<uint64_t>(n_seg, n_chunks));
    if (n_seg > 1) {
        seg_groups = (uint32_t)((n_chunks + n_seg - 1) / n_seg);
        n_seg_out = (uint32_t)((n_chunks + seg_groups - 1) / seg_groups);  // no empty segments
    }
}

// The one place the key of a program's generated texts is formed: (wavefronts per workgroup, everything else that changes the text
// from one render of a program to the next).
inline std::pair<int, int> jit_source_key(const JitOptions &opt) {
    return {opt.waves, opt.per_wave * 8 + opt.filter_block % 8 + (opt.voice_loop ? 64 : 0) + (opt.filter_scan ? 128 : 0) + (opt.rotate ? 0 : 256) + (opt.warm ? 512 : 0)};
}

// May this render be cut in time?  Segment totals stand for the reference's phases only where the modulated increments are bounded
// (fused_plan.hpp wave_split_exact) — for plain segments and for segments that warm up alike: both start their modulated oscillators from totals.
inline bool jit_split_exact(const JitSite &site, const JitBatch &batch, const Program &P) {
    return wave_split_exact(P, site.table_bound, batch.param_bound, /*params_assumed=*/!batch.param_bound && !batch.params_unknown);
}

// The time segments of a render on a compiled kernel: plan.n_seg, plan.seg_groups, plan.warm
inline void jit_plan_segments(JitPlan &plan, const JitSite &site, const JitBatch &batch, const Program &P, const WavePlan &wave) {
    const Knobs &knobs = site.knobs;
    const uint32_t n_inst = batch.n_inst, n_chunks = batch.n_chunks;
    // Few instances, long render: cut time into segments so that the whole chip works on it
    plan.seg_groups = n_chunks;
    if (wave.splittable && !knobs.jit_force_waves && jit_split_exact(site, batch, P)) jit_time_segments(site.n_cus, knobs.wave_segments, n_inst, n_chunks, plan.n_seg, plan.seg_groups);
    // A few circuits with Filters, long: segments that warm up (jit_codegen.hpp jit_warm_chunks) — every segment starts a segment early, from rest,
    // its Filters merge with the sequential trajectory on the way (checked after the launch), and only its own chunks are stored
    // (a Filter stage's serving wave runs 32 recurrences side by side at the price of one: the chip is full at 32 rows a CU, so up to a quarter of that many
    // instances are still worth cutting)
    // (warming segments keep the Filter stage — jit_site_options — where the unsplit render may scan: not the same bits.  The tiles of a mix
    // must all decide alike, and as one render of the whole batch would: by ITS instance count.  Few enough there means few enough in every
    // tile, and with fewer instances the segment count below only grows: every tile of such a batch warms up as well, or none does.)
    const uint32_t n_decide = batch.whole_n_inst ? batch.whole_n_inst : n_inst;
    if ((uint64_t)n_decide * 4 <= (uint64_t)site.n_cus * 32 && !batch.persistent && !batch.resume && !batch.handoff && !batch.inputs && !knobs.jit_force_waves && knobs.filter_warm != 0 && knobs.wave_segments != 0 &&
        knobs.wave_segments != 1 && jit_split_exact(site, batch, P)) {
        const uint32_t warm_chunks = jit_warm_chunks(P, wave);
        if (warm_chunks) {
            // (DUSP_FILTER_WARM=n > 1, tests: segments of n chunks whatever the Filters need — too short a warm-up shows in the check, and the render is finished sequentially)
            const uint64_t target = (uint64_t)site.n_cus * 32, per = knobs.filter_warm > 1 ? (uint64_t)knobs.filter_warm : std::max<uint64_t>(8, warm_chunks);
            uint64_t n_seg = std::min<uint64_t>(target / n_inst, n_chunks / per);
            if (knobs.wave_segments > 1) n_seg = std::min<uint64_t>((uint64_t)knobs.wave_segments, n_chunks / per);
            if (n_seg >= (knobs.filter_warm > 1 ? 2u : 4u)) {  // (below that the warm-up costs what the split gains)
                plan.seg_groups = (uint32_t)((n_chunks + n_seg - 1) / n_seg);
                plan.n_seg = (uint32_t)((n_chunks + plan.seg_groups - 1) / plan.seg_groups);
                plan.warm = true;
            }
        }
    }
}

// P and wave: the program and its plan, the Delay and Filter column verdicts already in the operands' pad / d[].
inline JitPlan jit_plan(const JitSite &site, const JitBatch &batch, const Program &P, const WavePlan &wave) {
    const Knobs &knobs = site.knobs;
    const uint32_t n_inst = batch.n_inst;
    JitPlan plan;
    JitOptions &opt = plan.opt;
    jit_plan_segments(plan, site, batch, P, wave);
    // workgroup geometry: as many wavefronts as LDS holds next to the table image, no more than gives every CU a workgroup
    opt.persistent = batch.persistent;
    // Voices in a loop (jit_codegen.hpp VoicePlan): where the circuit is a sum of isomorphic voices above jit_loop_voices_from() units
    opt.voice_loop = batch.voice_loop;
    opt.profile = knobs.jit_profile != 0;
    opt.filter_fma = knobs.filter_fma != 0;
    opt.nt_stores = knobs.jit_nt == 1 || (knobs.jit_nt == 2 && P.ring_samples != 0);
    if (!knobs.jit_rotate) opt.rotate = false;
    if (plan.warm) opt.warm = true, opt.rotate = false;  // (what a stage holds at the top of a chunk must be the chunk before's: nothing of the next one computed ahead)
    jit_site_options(opt, P, site, plan.warm, /*lines_ok=*/plan.n_seg == 1 && !opt.voice_loop && !(knobs.jit_force_waves && knobs.jit_force_per_wave > 1));
    const uint64_t n_virtual = plan.n_virtual = (uint64_t)n_inst * plan.n_seg;
    const unsigned want = (unsigned)((n_virtual + 255) / 256);
    int most = 16;
    if (knobs.wave_max_waves > 0) most = std::max(1, std::min(most, knobs.wave_max_waves));
    // the sequential-stage units' per-wave scratch comes out of the same 160 KiB: as many wavefronts as fit next to the table image
    // (a power of two; jit_place_table has left the table image out where not even one wave's scratch fits beside it)
    if (opt.scratch_floats) {
        const size_t scratch = opt.scratch_floats * 4;
        while (most > 1 && opt.table_bytes + (size_t)most * scratch > 160 * 1024) most /= 2;
    }
    const size_t budget = 160 * 1024 - (size_t)most * opt.scratch_floats * 4;
    int waves = 1, per_wave = 1;
    // (the lines are per wavefront; a wavefront walks ONE segment's chunks: the chunk loop has one counter)
    const int per_wave_cap = opt.line_floats || plan.n_seg > 1 ? 1 : knobs.wave_per_wave >= 1 ? std::min(4, knobs.wave_per_wave) : 4;
    const bool filter_stage = opt.filter_stages > 0;
    if (filter_stage) {
        // The Filter stage runs one recurrence per lane of ONE wave: a workgroup wants as many instances (rows) as that wave has
        // lanes, and every CU the same number of rounds — rows = instances per CU / rounds, spread over up to 16 wavefronts.
        const uint64_t per_cu = (n_virtual + (uint64_t)site.n_cus - 1) / (uint64_t)site.n_cus;  // (instances, or the segments of one)
        const uint64_t rounds = (per_cu + 63) / 64;
        const int rows = (int)std::max<uint64_t>(1, (per_cu + rounds - 1) / rounds);
        waves = std::min(most, rows);
        per_wave = std::min(per_wave_cap, (rows + waves - 1) / waves);
        // (16 wavefronts of FOUR instances — 128 registers a lane — spill 170-470 bytes in every Filter circuit measured, filter(osc) included, and end at 16 x 2 two
        // compiles later: start there.  A first render of such a structure: 2.1-3.3 s -> one compile)
        if (waves == 16 && per_wave == 4 && knobs.wave_per_wave < 4) per_wave = 2;
        opt.filter_sub = jit_filter_sub(waves, per_wave, opt.filter_stages, budget - opt.table_bytes, opt.filter_mod);
        // (a connected cutoff parks three values per sample in two sets of rows: fewer rows per workgroup before the table image goes)
        while (opt.filter_mod && !opt.filter_sub && (per_wave > 1 || waves > 1)) {
            if (per_wave > 1) per_wave /= 2;
            else waves /= 2;
            opt.filter_sub = jit_filter_sub(waves, per_wave, opt.filter_stages, budget - opt.table_bytes, opt.filter_mod);
        }
        if (!opt.filter_sub) {  // (cannot happen with a 99 KB image: 64 rows of 64 samples take 33 KB)
            opt.lds_table = -1, opt.table_bytes = 0;
            opt.filter_sub = jit_filter_sub(waves, per_wave, opt.filter_stages, budget, opt.filter_mod);
        }
    } else {
        while (waves < most && (unsigned)waves < want) waves *= 2;
        // instances per wavefront (unsplit renders of light circuits, jit_light): 4 or 2 while that leaves every CU a workgroup —
        // their independent unit blocks fill each other's latencies
        // (not next to the table image: since the oscillators' delta form — 17 instructions a sample instead of 26 — one instance per wave is
        // the faster: osc(k) 0.66 / 0.70 / 0.69 ms at 1 / 2 / 4, mul(osc, k) 0.68 / 0.66 / 0.70; ramp and timer graphs 0.79 / 0.66 / 0.63)
        if (plan.n_seg == 1 && ((jit_light(P) && opt.lds_table < 0) || knobs.wave_per_wave > 1))
            for (int r : {4, 2})
                if (r <= per_wave_cap && (uint64_t)site.n_cus * waves * r <= n_inst) {
                    per_wave = r;
                    break;
                }
    }

    if (knobs.jit_force_waves) {  // tests: this geometry, whatever the batch
        waves = std::min(most, knobs.jit_force_waves);
        per_wave = knobs.jit_force_per_wave;
        if (filter_stage) {
            opt.filter_sub = jit_filter_sub(waves, per_wave, opt.filter_stages, budget - opt.table_bytes, opt.filter_mod);
            if (!opt.filter_sub) plan.error = "render: DUSP_JIT_FORCE: the Filter stage's rows do not fit LDS at this geometry";
        }
    }
    plan.waves = opt.waves = waves;
    plan.per_wave = opt.per_wave = per_wave;
    plan.per_wave_cap = per_wave_cap;
    plan.most = most;
    plan.budget = budget;
    plan.filter_stage = filter_stage;
    return plan;
}

// The kernel of plan.waves x plan.per_wave (Filter block plan.opt.filter_block) spills: the next geometry to try, written into the plan
// (false: none — the kernel at hand is the one).
// 16 wavefronts: 128 registers per lane.  A Filter circuit keeps its rows if it can — half the wavefronts with twice the instances each
// have twice the registers — else instances per wave, then waves, go down.
inline bool jit_spill_step(JitPlan &plan) {
    JitOptions &opt = plan.opt;
    int &waves = plan.waves, &per_wave = plan.per_wave;
    const bool filter_stage = plan.filter_stage;
    if (filter_stage && opt.filter_block == 8) {
        opt.filter_block = 4;  // (first: the recurrence loop with half the P values in flight, 16 registers less)
        return true;
    }
    opt.filter_block = 8;
    if (filter_stage && waves > 4 && waves % 2 == 0 && per_wave * 2 <= plan.per_wave_cap) {
        waves /= 2;
        per_wave *= 2;
    } else if (filter_stage && per_wave > 1) per_wave /= 2;  // (rows stay a power of two: whole rounds on every CU)
    else if (per_wave > 1) per_wave /= 2;  // (4, 2, 1: an odd count leaves the last round of workgroups a third full at the usual batch sizes)
    else if (waves > 4) waves /= 2;
    else return false;
    opt.waves = waves;
    opt.per_wave = per_wave;
    if (filter_stage) opt.filter_sub = jit_filter_sub(waves, per_wave, opt.filter_stages, plan.budget - opt.table_bytes, opt.filter_mod);
    return true;
}

}  // namespace dusp
