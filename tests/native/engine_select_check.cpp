// dusp_amd/csrc/engine_select.hpp on the CPU: the engine dusp_program_build / dusp_program_continue choose for a program, against the rules
// written out below as a table over what plan_fused / plan_wave / jit_eligible say when called on their own.
//   engine_select_check FILE...   (descriptor words as f64: tests/golden/*.desc.f64)
// For every file: requested engine {AUTO, CHUNK, FUSED, WAVE} x {plain, resumable} x {compiled kernels on, off} as a new program, and
// x {engine so far} x {a Delay's constant changed} as a continuation of a rendered resumable one.  Prints one JSON line.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../dusp_amd/csrc/engine_select.hpp"

using namespace dusp;

static long g_cases = 0, g_bad = 0;
static long n_auto[4] = {0, 0, 0, 0};  // AUTO's choices by engine
static long n_refused = 0, n_resumable_wave = 0, n_resumable_chunk = 0, n_resumable_refused = 0, n_stays_wave = 0, n_falls_to_chunk = 0, n_back_to_auto = 0, n_handoff = 0,
            n_handoff_files = 0, n_jit = 0, n_fx32 = 0;
static long n_delay_stays = 0, n_delay_falls = 0, n_ff_stays = 0;  // the named continuation cases: a delay_* golden, a feed-forward one

static const char *kNames[] = {"AUTO", "CHUNK", "FUSED", "WAVE"};

// What the planners say about this descriptor, each asked on its own
struct Facts {
    bool fusable = false, wavable = false, persistent = false, jit = false, settled_jit = false, warm_ops = false, inputs = false, sumchain = false;
    int sum_table = 0;
    std::string fused_why, wave_why;
};

static bool facts_of(const std::vector<double> &words, bool resumable, Facts &f) {
    Program P;
    std::string err, why;
    if (!compile(words.data(), words.size(), P, err, /*continuation=*/false)) return false;
    FusedPlan fp;
    f.fusable = plan_fused(P, fp);
    f.fused_why = fp.why;
    f.sumchain = f.fusable && fp.kind == FUSED_SUMCHAIN;
    f.sum_table = fp.table_id;
    WavePlan wp;
    f.wavable = plan_wave(P, wp, resumable);
    f.wave_why = wp.why;
    f.jit = f.wavable && jit_eligible(P, wp, why);
    f.persistent = P.ring_samples != 0 || !P.feed_forward;
    f.warm_ops = !P.warm_ops.empty();
    f.inputs = P.g.n_inputs != 0;
    WavePlan settled;
    f.settled_jit = plan_wave(P, settled, /*will_continue=*/true, /*settled_only=*/true) && jit_eligible(P, settled, why);
    return true;
}

static void fail(const char *file, const EngineRequest &rq, const std::string &what) {
    g_bad++;
    std::printf("FAIL: %s, %s%s%s, so far %s%s, wave_jit %d: %s\n", file, kNames[rq.requested], rq.resumable ? " resumable" : "", rq.rendered ? " continued" : "", kNames[rq.engine_so_far],
                rq.delay_changed ? ", delay changed" : "", rq.wave_jit, what.c_str());
}

// One call of engine_select against the table.  fx32_ok: what the context says about every table it has.
static void check(const char *file, const std::vector<double> &words, const EngineRequest &rq, bool fx32_ok) {
    Facts f;
    Program P;
    std::string err;
    if (!facts_of(words, rq.resumable, f) || !compile(words.data(), words.size(), P, err, /*continuation=*/false)) return;
    g_cases++;
    if (f.sumchain && !fx32_ok) f.fusable = false, f.fused_why = "the sum chain's wave table has entries below 2^-20";
    const EngineChoice got = engine_select(P, rq);

    // ---- the rules ----
    int want = rq.requested;
    std::string refused;
    bool back_to_auto = false;
    // a continuation of a resumable program never fails over the engine: AUTO's rules instead
    if (rq.rendered && rq.resumable && ((want == DUSP_ENGINE_FUSED && !f.fusable) || (want == DUSP_ENGINE_WAVE && !f.wavable))) want = DUSP_ENGINE_AUTO, back_to_auto = true;
    if (want == DUSP_ENGINE_FUSED && !f.fusable) refused = "dusp_program_build: no fused kernel for this graph shape (" + f.fused_why + ")";
    else if (want == DUSP_ENGINE_WAVE && !f.wavable) refused = "dusp_program_build: the wave engine cannot run this graph (" + f.wave_why + ")";
    else if (rq.resumable && f.persistent) {  // rings or feedback, to be continued: wave if plannable, else chunk; never fused
        if (want == DUSP_ENGINE_FUSED) refused = "dusp_program_build: a resumable program with delay lines / feedback runs on DUSP_ENGINE_WAVE or DUSP_ENGINE_CHUNK";
        else if (rq.rendered) want = rq.engine_so_far == DUSP_ENGINE_WAVE && f.wavable && !rq.delay_changed ? DUSP_ENGINE_WAVE : DUSP_ENGINE_CHUNK;
        else if (want == DUSP_ENGINE_AUTO) want = f.wavable ? DUSP_ENGINE_WAVE : DUSP_ENGINE_CHUNK;
    }
    if (refused.empty() && want == DUSP_ENGINE_AUTO) want = f.fusable ? DUSP_ENGINE_FUSED : f.wavable ? DUSP_ENGINE_WAVE : DUSP_ENGINE_CHUNK;  // the first engine that applies
    const bool want_jit = refused.empty() && want == DUSP_ENGINE_WAVE && rq.wave_jit != 0 && f.jit;
    // channel counts that still grow keep AUTO's plain program on the chunk engine: it hands over when the settled circuit is one the compiler takes
    const bool replanned = refused.empty() && want == DUSP_ENGINE_CHUNK && f.warm_ops && rq.requested == DUSP_ENGINE_AUTO && !rq.resumable && !f.inputs && rq.wave_jit != 0;
    const bool want_handoff = replanned && f.settled_jit;

    // ---- the verdict ----
    if (!refused.empty()) {
        if (got.error != DUSP_ERR_UNSUPPORTED || got.error_text != refused) fail(file, rq, "expected DUSP_ERR_UNSUPPORTED \"" + refused + "\", got " + std::to_string(got.error) + " \"" + got.error_text + "\"");
        n_refused++;
        if (rq.resumable && f.persistent && !rq.rendered) n_resumable_refused++;
        return;
    }
    if (got.error != DUSP_OK || !got.error_text.empty()) return fail(file, rq, "refused: " + got.error_text);
    if (got.engine != want) fail(file, rq, std::string("engine ") + kNames[got.engine] + ", expected " + kNames[want]);
    if (got.persistent != f.persistent) fail(file, rq, "persistent");
    if (got.jit_ok != want_jit) fail(file, rq, got.jit_ok ? "jit_ok, unexpectedly" : "not jit_ok: " + got.jit_why);
    if (got.handoff_ok != want_handoff) fail(file, rq, got.handoff_ok ? "handoff_ok, unexpectedly" : "not handoff_ok: " + got.handoff_why);
    if (got.handoff_ok && !(rq.requested == DUSP_ENGINE_AUTO && !rq.resumable && !f.inputs && rq.wave_jit != 0 && got.engine == DUSP_ENGINE_CHUNK)) fail(file, rq, "a hand-off outside AUTO / plain / no inputs / compiled kernels on");
    if (!got.handoff_ok && replanned && got.handoff_why.empty())
        fail(file, rq, "no hand-off and no reason");
    if (got.engine == DUSP_ENGINE_FUSED && got.fused.shape.empty()) fail(file, rq, "FUSED without a fused plan");
    if (got.engine == DUSP_ENGINE_WAVE && (!got.wave.ok || got.wave.order.size() != P.ops.size())) fail(file, rq, "WAVE without a wave plan");
    // the edits to the op list: exact rings for what will be continued, the wave plan's findings written back
    const bool exact = (rq.resumable && f.persistent) || got.handoff_ok;
    const bool written_back = got.handoff_ok || (f.wavable && !replanned);  // (the plan in got.wave is the one the op list was edited from)
    for (size_t k = 0; k < P.ops.size(); k++) {
        const DevOp &op = P.ops[k];
        if ((op.op == OP_DELAY || op.op == OP_MONO_DELAY) && op.pad != (exact ? kDelayExactRing : 0)) fail(file, rq, "a Delay's ring protocol");
        if (!written_back) continue;
        if (k < got.wave.osc_level.size() && got.wave.osc_level[k] >= 0 && op.d[0] != (double)got.wave.osc_level[k]) fail(file, rq, "an Osc's FM level not written back");
        if (k < got.wave.ramp_fastdiv.size() && op.op == OP_RAMP && op.attr != got.wave.ramp_fastdiv[k]) fail(file, rq, "a Ramp's reciprocal verdict not written back");
    }
    // ---- what the cases covered ----
    const bool is_delay = std::strstr(file, "/delay_") != nullptr || std::strncmp(file, "delay_", 6) == 0;
    if (!rq.rendered && rq.requested == DUSP_ENGINE_AUTO && !rq.resumable && rq.wave_jit && fx32_ok) n_auto[got.engine]++;
    if (!rq.rendered && rq.resumable && f.persistent && rq.requested == DUSP_ENGINE_AUTO) (got.engine == DUSP_ENGINE_WAVE ? n_resumable_wave : n_resumable_chunk)++;
    if (rq.rendered && f.persistent && rq.engine_so_far == DUSP_ENGINE_WAVE && got.engine == DUSP_ENGINE_WAVE) n_stays_wave++, n_delay_stays += is_delay;
    if (rq.rendered && f.persistent && rq.engine_so_far == DUSP_ENGINE_WAVE && rq.delay_changed && got.engine == DUSP_ENGINE_CHUNK) n_falls_to_chunk++, n_delay_falls += is_delay;
    if (rq.rendered && !f.persistent && rq.requested == DUSP_ENGINE_WAVE && got.engine == DUSP_ENGINE_WAVE) n_ff_stays++;
    if (back_to_auto) n_back_to_auto++;
    if (got.handoff_ok) n_handoff++;
    if (got.jit_ok) n_jit++;
    if (!fx32_ok && f.sumchain) n_fx32++;
}

int main(int argc, char **argv) {
    int files = 0;
    for (int a = 1; a < argc; a++) {
        FILE *fh = std::fopen(argv[a], "rb");
        if (!fh) {
            std::printf("FAIL: cannot open %s\n", argv[a]);
            g_bad++;
            continue;
        }
        std::vector<double> words;
        double w;
        while (std::fread(&w, sizeof w, 1, fh) == 1) words.push_back(w);
        std::fclose(fh);
        files++;
        const long handoffs_before = n_handoff;
        for (int requested : {DUSP_ENGINE_AUTO, DUSP_ENGINE_CHUNK, DUSP_ENGINE_FUSED, DUSP_ENGINE_WAVE})
            for (int resumable = 0; resumable < 2; resumable++) {
                EngineRequest rq;
                rq.requested = requested;
                rq.resumable = resumable != 0;
                for (int k = 0; k < kNumTables; k++) rq.table_set[k] = rq.table_fx32_ok[k] = true;
                for (int wave_jit : {1, 0, 2}) {
                    rq.wave_jit = wave_jit;
                    check(argv[a], words, rq, true);
                }
                rq.wave_jit = 1;
                for (int k = 0; k < kNumTables; k++) rq.table_fx32_ok[k] = false;  // (a table with entries below 2^-20: the sum chain does not take it)
                check(argv[a], words, rq, false);
                for (int k = 0; k < kNumTables; k++) rq.table_fx32_ok[k] = true;
                if (!resumable) continue;
                rq.rendered = true;  // a continuation
                for (int so_far : {DUSP_ENGINE_CHUNK, DUSP_ENGINE_FUSED, DUSP_ENGINE_WAVE})
                    for (int changed = 0; changed < 2; changed++) {
                        rq.engine_so_far = so_far;
                        rq.delay_changed = changed != 0;
                        check(argv[a], words, rq, true);
                    }
            }
        const char *base = std::strrchr(argv[a], '/');
        base = base ? base + 1 : argv[a];
        // (of the circuits whose channel counts grow, patch_scary has warm-up chunks of its own op lists and must hand over under AUTO; the grow_*
        // vectors settle within their first chunk, compile to wave programs as they stand, and — like every file — may hand over only per the table)
        if (std::strncmp(base, "patch_scary", 11) == 0 && n_handoff == handoffs_before) g_bad++, std::printf("FAIL: %s: no hand-off under AUTO\n", base);
        n_handoff_files += n_handoff != handoffs_before;
    }
    std::printf("{\"files\": %d, \"cases\": %ld, \"bad\": %ld, \"auto_chunk\": %ld, \"auto_fused\": %ld, \"auto_wave\": %ld, \"refused\": %ld, \"resumable_wave\": %ld, \"resumable_chunk\": %ld, "
                "\"resumable_refused\": %ld, \"stays_wave\": %ld, \"falls_to_chunk\": %ld, \"delay_stays_wave\": %ld, \"delay_falls_to_chunk\": %ld, \"feed_forward_stays_wave\": %ld, "
                "\"back_to_auto\": %ld, \"handoff\": %ld, \"handoff_files\": %ld, \"jit\": %ld, \"fx32\": %ld}\n",
                files, g_cases, g_bad, n_auto[DUSP_ENGINE_CHUNK], n_auto[DUSP_ENGINE_FUSED], n_auto[DUSP_ENGINE_WAVE], n_refused, n_resumable_wave, n_resumable_chunk, n_resumable_refused,
                n_stays_wave, n_falls_to_chunk, n_delay_stays, n_delay_falls, n_ff_stays, n_back_to_auto, n_handoff, n_handoff_files, n_jit, n_fx32);
    return g_bad ? 1 : 0;
}
