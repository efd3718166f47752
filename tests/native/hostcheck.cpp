// The untrusted-input path of the library on the CPU, under AddressSanitizer and UBSan (make -C dusp_amd/csrc hostcheck): descriptor words ->
// program (program.hpp: parse, channel inference, expansion) -> plans (fused_plan.hpp: fused voice shapes, the wave engine) ->
// kernel text (jit_codegen.hpp jit_source_from_descriptor — the very function dusp_circuit_kernel_source runs in front of the run-time
// compiler; the text is generated, not compiled) and -> launch plans (jit_plan.hpp jit_plan / jit_spill_step: what a render decides before
// it touches the device, over a spread of batches and knobs, every spill ladder walked to its end) and -> the engine a build or a continuation
// chooses (engine_select.hpp engine_select, for every requested engine, plain and resumable, new and continued).  Driven with
//   * every descriptor file named on the command line (the golden descriptors the reference generated) as it stands, over a spread of
//     workgroup geometries and knob settings;
//   * its truncations (every third length) and single-word corruptions (NaN, Inf, negative, fractional, huge, small-integer values at random
//     positions: the corpus of tests/test_gpu_parity.py::test_malformed_descriptors_are_rejected_not_crashed, which needs a GPU).
// Every call must come back with a verdict — 0 text, 1 malformed, 2 unsupported — and a message; the sanitizers abort on anything else
// (-fno-sanitize-recover).  Prints one JSON line; text_hash is a 64-bit FNV-1a over every generated text in call order.
// (-DHOSTCHECK_NO_PLANNER: without jit_plan.hpp — the same driver against a tree that has no planner yet, to compare text_hash.)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../dusp_amd/csrc/jit_codegen.hpp"
#ifndef HOSTCHECK_NO_PLANNER
#include "../../dusp_amd/csrc/engine_select.hpp"
#include "../../dusp_amd/csrc/jit_plan.hpp"
#endif
#include "../../dusp_amd/csrc/ring_windows.hpp"

using namespace dusp;

static long g_text = 0, g_malformed = 0, g_unsupported = 0, g_calls = 0, g_bad = 0;
static size_t g_text_bytes = 0;
static unsigned long long g_text_hash = 1469598103934665603ull;
static long g_plans = 0, g_selects = 0;

#ifndef HOSTCHECK_NO_PLANNER
// The engine choice as dusp_program_build / dusp_program_continue would ask for it: every call ends in an engine or in a refusal with a text
static void drive_engine_select(const std::vector<double> &words, bool every_variant) {
    Program P0;
    std::string err;
    if (!compile(words.data(), words.size(), P0, err)) return;
    std::vector<WavePlan::RampChecked> checked;
    for (int requested : {DUSP_ENGINE_AUTO, DUSP_ENGINE_CHUNK, DUSP_ENGINE_FUSED, DUSP_ENGINE_WAVE})
        for (int variant = 0; variant < (every_variant ? 6 : 2); variant++) {
            if (!every_variant && requested != DUSP_ENGINE_AUTO && requested != DUSP_ENGINE_WAVE) continue;
            EngineRequest rq;
            rq.requested = requested;
            rq.resumable = variant >= 1;
            rq.rendered = variant >= 3;  // a continuation, on the wave or the chunk engine so far, a Delay's constant changed
            rq.engine_so_far = variant == 4 ? DUSP_ENGINE_CHUNK : DUSP_ENGINE_WAVE;
            rq.delay_changed = variant == 5;
            rq.wave_jit = variant == 2 ? 0 : 1;
            for (int k = 0; k < kNumTables; k++) rq.table_set[k] = variant != 2, rq.table_fx32_ok[k] = variant % 2 == 0;
            Program P = P0;
            EngineChoice c = engine_select(P, rq, checked);
            checked = c.wave.ramp_checked;  // (as a program keeps them from one plan to the next)
            g_selects++;
            const bool engine_ok = c.engine == DUSP_ENGINE_CHUNK || c.engine == DUSP_ENGINE_FUSED || c.engine == DUSP_ENGINE_WAVE;
            if (c.error ? (c.error != DUSP_ERR_UNSUPPORTED || c.error_text.empty()) : (!engine_ok || !c.error_text.empty() || (c.jit_ok && c.engine != DUSP_ENGINE_WAVE) || (c.handoff_ok && c.engine != DUSP_ENGINE_CHUNK)))
                g_bad++, std::printf("FAIL: engine_select: engine %d, error %d \"%s\"\n", c.engine, c.error, c.error_text.c_str());
        }
}

// The planner over a spread of (n_inst, n_chunks, knobs), as dusp_program_build + render_jit would call it for this descriptor
static void drive_planner(const std::vector<double> &words, bool every_variant) {
    Program P;
    std::string err, why;
    WavePlan wp;
    if (!compile(words.data(), words.size(), P, err) || !plan_wave(P, wp, false) || !jit_eligible(P, wp, why)) return;
    VoicePlan voices;
    const bool voice_loop = P.ops.size() > jit_loop_voices_from() && jit_find_voices(P, wp, voices);
    static const uint32_t insts[] = {1, 17, 64, 2048, 65536, 1u << 24}, chunks[] = {1, 9, 188, 1875, 1u << 23};
    for (int variant = 0; variant < (every_variant ? 8 : 3); variant++) {
        JitSite site;
        if (variant != 3 && P.g.sample_rate % 2 == 0) {  // the reference's tables (else: a context that knows nothing about its tables)
            site.table_form[1] = 1, site.table_form[2] = 2, site.table_form[4] = 4;
            for (int k = 0; k < 5; k++) site.table_bound[k] = 1;
            site.table_delta[0] = 1;
            site.table_antisym[0] = site.table_antisym[4] = true;
        }
        Knobs &k = site.knobs;
        if (variant == 1) k.wave_segments = 0, k.filter_scan = 0;
        if (variant == 2) k.wave_segments = 5, k.filter_warm = 3, k.delay_line = 2;
        if (variant == 3) k.filter_scan = 2, k.wave_per_wave = 4, k.jit_lds_table = 0;
        if (variant == 4) k.jit_force_waves = 16, k.jit_force_per_wave = 4;
        if (variant == 5) k.jit_force_waves = 2, k.jit_force_per_wave = 1, k.delay_line = 0;
        if (variant == 6) k.wave_max_waves = 3, k.wave_per_wave = 2, k.filter_warm = 0;
        if (variant == 7) site.n_cus = 1, k.jit_rotate = 0;
        for (uint32_t n_inst : insts)
            for (uint32_t n_chunks : chunks) {
                JitBatch b;
                b.n_inst = n_inst, b.n_chunks = n_chunks;
                b.voice_loop = voice_loop;
                b.inputs = variant == 6;
                JitPlan plan = jit_plan(site, b, P, wp);
                g_plans++;
                if (plan.error) continue;
                int steps = 0;
                do {
                    if (plan.waves < 1 || plan.waves > 16 || plan.per_wave < 1 || plan.per_wave > 4 || plan.n_seg < 1 || (uint64_t)plan.n_seg * plan.seg_groups < n_chunks ||
                        (plan.filter_stage && !plan.opt.filter_sub) || jit_source_key(plan.opt).first != plan.waves)
                        g_bad++, std::printf("FAIL: a plan out of range (%d x %d, %u segments of %u)\n", plan.waves, plan.per_wave, plan.n_seg, plan.seg_groups);
                } while (jit_spill_step(plan) && ++steps < 64);
                if (steps >= 64) g_bad++, std::printf("FAIL: a spill ladder that does not end\n");
            }
    }
}
#endif

static void drive(const std::vector<double> &words, bool every_geometry) {
    // the plans dusp_program_build consults before the circuit compiler
    {
        Program P;
        std::string err;
        if (compile(words.data(), words.size(), P, err)) {
            FusedPlan fp;
            (void)plan_fused(P, fp);
            WavePlan wp;
            (void)plan_wave(P, wp, false);
            std::vector<RingWindow> wins;
            size_t covered = 0;
            ring_windows(P, 40, wins, covered);
        } else if (err.empty()) {
            g_bad++;
            std::printf("FAIL: compile() refused a descriptor without a message\n");
        }
    }
#ifndef HOSTCHECK_NO_PLANNER
    drive_engine_select(words, every_geometry);
    drive_planner(words, every_geometry);
#endif
    static const int geo[][2] = {{4, 1}, {16, 1}, {16, 2}, {8, 4}, {1, 1}};
    const int n_geo = every_geometry ? 5 : 2;
    for (int gi = 0; gi < n_geo; gi++)
        for (int variant = 0; variant < (every_geometry ? 4 : 2); variant++) {
            JitSourceRequest rq;
            rq.waves = geo[gi][0];
            rq.per_wave = geo[gi][1];
            rq.continued = variant == 1;
            rq.scan_knob = variant == 2 ? 0 : variant == 3 ? 2 : 1;
            rq.lean_recurrence = variant == 2;
            rq.lds_table = variant != 3;
            rq.delay_line = variant == 3;
            JitSource src;
            std::string err;
            const int v = jit_source_from_descriptor(words.data(), words.size(), rq, src, err);
            g_calls++;
            if (v == 0) {
                g_text++;
                g_text_bytes += src.text.size();
                for (unsigned char c : src.text) g_text_hash = (g_text_hash ^ c) * 1099511628211ull;
                if (src.text.find("dusp_jit_render") == std::string::npos) g_bad++, std::printf("FAIL: a text without a render kernel\n");
            } else if (v == 1) g_malformed++;
            else if (v == 2) g_unsupported++;
            else g_bad++, std::printf("FAIL: verdict %d\n", v);
            if (v != 0 && err.empty()) g_bad++, std::printf("FAIL: verdict %d without a message\n", v);
        }
}

int main(int argc, char **argv) {
    std::mt19937_64 rng(7);
    const double poison[] = {NAN, INFINITY, -INFINITY, -1.0, 0.5, 1e18, -1e18, 3.0, 65536.0, 1099511627776.0, 0.0, 1.0, 2.0, 255.0, 4294967296.0, -0.0, 1e-300, 7.0, 40.0};
    const int n_poison = (int)(sizeof poison / sizeof poison[0]);
    int files = 0;
    const int corruptions = argc > 1 && std::getenv("HOSTCHECK_CORRUPTIONS") ? std::atoi(std::getenv("HOSTCHECK_CORRUPTIONS")) : 60;
    for (int a = 1; a < argc; a++) {
        FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::printf("FAIL: cannot open %s\n", argv[a]);
            g_bad++;
            continue;
        }
        std::vector<double> words;
        double w;
        while (std::fread(&w, sizeof w, 1, f) == 1) words.push_back(w);
        std::fclose(f);
        files++;
        drive(words, true);
        for (size_t k = 0; k < words.size(); k += 3) drive(std::vector<double>(words.begin(), words.begin() + (long)k), false);
        for (int c = 0; c < corruptions && !words.empty(); c++) {
            std::vector<double> d2 = words;
            d2[(size_t)(rng() % d2.size())] = poison[rng() % (unsigned)n_poison];
            if (c % 5 == 4) d2[(size_t)(rng() % d2.size())] = poison[rng() % (unsigned)n_poison];  // (two at once)
            drive(d2, false);
        }
    }
    std::printf("{\"files\": %d, \"calls\": %ld, \"text\": %ld, \"malformed\": %ld, \"unsupported\": %ld, \"text_bytes\": %zu, \"text_hash\": \"%016llx\", \"plans\": %ld, \"selects\": %ld, \"bad\": %ld}\n",
                files, g_calls, g_text, g_malformed, g_unsupported, g_text_bytes, g_text_hash, g_plans, g_selects, g_bad);
    return g_bad ? 1 : 0;
}
