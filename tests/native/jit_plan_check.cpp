// dusp_amd/csrc/jit_plan.hpp on the CPU: the launch planner of the compiled circuit kernels against what the library chose BEFORE the
// planner was a module of its own, the spill ladder, the key of a program's generated texts and the time-segment count.
//   jit_plan_check NAME=FILE ...   (descriptor words as f64; tests/test_abi.py builds the circuits and names them)
// Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../dusp_amd/csrc/jit_plan.hpp"

using namespace dusp;

static long g_cases = 0, g_bad = 0;

// "name=value" words -> knobs and batch flags (force=WxR; persistent / resume / handoff / inputs)
static void apply_words(const std::string &words, Knobs &k, bool &persistent, bool &resume, bool &handoff, bool &inputs) {
    size_t at = 0;
    while (at < words.size()) {
        size_t end = words.find(' ', at);
        if (end == std::string::npos) end = words.size();
        const std::string w = words.substr(at, end - at);
        at = end + 1;
        const size_t eq = w.find('=');
        const std::string name = w.substr(0, eq), val = eq == std::string::npos ? "" : w.substr(eq + 1);
        const int v = std::atoi(val.c_str());
        if (name == "persistent") persistent = true;
        else if (name == "resume") resume = true;
        else if (name == "handoff") handoff = persistent = resume = true;
        else if (name == "inputs") inputs = true;
        else if (name == "force") std::sscanf(val.c_str(), "%dx%d", &k.jit_force_waves, &k.jit_force_per_wave);
        else if (name == "wave_segments") k.wave_segments = v;
        else if (name == "filter_warm") k.filter_warm = v;
        else if (name == "wave_per_wave") k.wave_per_wave = v;
        else if (name == "wave_max_waves") k.wave_max_waves = v;
        else if (name == "delay_line") k.delay_line = v;
        else if (name == "filter_scan") k.filter_scan = v;
        else if (name == "jit_lds_table") k.jit_lds_table = v;
        else if (name == "jit_rotate") k.jit_rotate = v;
        else if (!name.empty()) std::printf("FAIL: unknown word %s\n", name.c_str()), std::exit(2);
    }
}

// descriptor words -> the program and plan dusp_program_build hands a render
static bool load_circuit(const std::vector<double> &words, Program &P, WavePlan &wave) {
    std::string err;
    if (!compile(words.data(), words.size(), P, err, /*continuation=*/false) || !plan_wave(P, wave, false)) return false;
    for (size_t k = 0; k < wave.osc_level.size() && k < P.ops.size(); k++)
        if (wave.osc_level[k] >= 0) P.ops[k].d[0] = (double)wave.osc_level[k];
    for (size_t k = 0; k < wave.ramp_fastdiv.size() && k < P.ops.size(); k++)
        if (P.ops[k].op == OP_RAMP) P.ops[k].attr = wave.ramp_fastdiv[k];
    std::string why;
    return jit_eligible(P, wave, why);
}

static std::string describe(uint32_t n_seg, uint32_t seg_groups, bool warm, const JitOptions &opt, int most, int cap, size_t budget, bool filter_stage, bool error) {
    char s[400];
    std::snprintf(s, sizeof s, "seg %ux%u warm %d | image %d/%zu scan %d stages %d mod %d rotate %d optwarm %d voices %d lines %zu/%d scratch %zu | most %d cap %d budget %zu stage %d | err %d", n_seg, seg_groups,
                  (int)warm, opt.lds_table, opt.table_bytes, (int)opt.filter_scan, opt.filter_stages, (int)opt.filter_mod, (int)opt.rotate, (int)opt.warm, (int)opt.voice_loop, opt.line_floats,
                  (int)opt.line_whole_only, opt.scratch_floats, most, cap, budget, (int)filter_stage, (int)error);
    return s;
}
static std::string step_name(const JitOptions &opt) {
    char s[64];
    std::snprintf(s, sizeof s, "%dx%d/b%d/s%d", opt.waves, opt.per_wave, opt.filter_block, opt.filter_sub);
    return s;
}

// Recorded plans, 256 CUs, a context with the reference's tables (sine .. 8bit antisymmetric and within [-1, 1], saw / square / triangle
// closed forms, 8bit derived from sine, the sine's differences exact in f64).  HOW EVERY ROW WAS OBTAINED: from the commit before the
// planner existed, never from jit_plan.hpp — the lines of its render_jit from "Few instances, long render" to the end of the
// DUSP_JIT_FORCE block were copied verbatim into a function of a host-only program (a struct with the context's fields the lines
// name standing in for dusp_ctx), followed by a loop around its spill chain ("if (filter_stage && opt.filter_block == 8)" .. "else break",
// verbatim as well) that takes every kernel to have spilled; that program printed these rows for these circuits.
//   plan:   what stood in a / opt / most / per_wave_cap / budget / filter_stage behind the geometry search (err: the DUSP_JIT_FORCE failure)
//   ladder: waves x per_wave / Filter block / filter_sub of the first decision and of every step after a spill, to the end
//           (a forced geometry is never stepped down: one entry)
struct Row {
    const char *circuit;
    uint32_t n_inst, n_chunks;
    const char *words;  // knobs and batch flags (apply_words)
    const char *plan, *ladder;
};
static const Row kRows[] = {
    {"light", 1u, 188u, "",
     "seg 21x9 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"light", 17u, 188u, "",
     "seg 21x9 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "2x1/b8/s256"},
    {"light", 65u, 188u, "",
     "seg 21x9 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "8x1/b8/s256 4x1/b8/s256"},
    {"light", 16383u, 188u, "",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x2/b8/s256 16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"light", 65536u, 188u, "",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x4/b8/s256 16x2/b8/s256 16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"osc", 1u, 188u, "",
     "seg 21x9 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"osc", 17u, 188u, "",
     "seg 21x9 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "2x1/b8/s256"},
    {"osc", 65u, 188u, "",
     "seg 21x9 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "8x1/b8/s256 4x1/b8/s256"},
    {"osc", 16383u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"osc", 65536u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"filter_stage", 1u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "1x1/b8/s64 1x1/b4/s64"},
    {"filter_stage", 17u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "1x1/b8/s64 1x1/b4/s64"},
    {"filter_stage", 65u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "1x1/b8/s64 1x1/b4/s64"},
    {"filter_stage", 16383u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x2/b8/s64 16x2/b4/s64 8x4/b8/s64 8x4/b4/s64 8x2/b8/s64 8x2/b4/s64 4x4/b8/s64 4x4/b4/s64 4x2/b8/s64 4x2/b4/s64 4x1/b8/s64 4x1/b4/s64"},
    {"filter_stage", 65536u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x2/b8/s64 16x2/b4/s64 8x4/b8/s64 8x4/b4/s64 8x2/b8/s64 8x2/b4/s64 4x4/b8/s64 4x4/b4/s64 4x2/b8/s64 4x2/b4/s64 4x1/b8/s64 4x1/b4/s64"},
    {"cfg4", 8192u, 1875u, "",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 768/0 scratch 768 | most 16 cap 1 budget 114688 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"cfg4", 8192u, 1875u, "filter_scan=0",
     "seg 1x1875 warm 0 | image 0/99024 scan 0 stages 1 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x2/b8/s128 16x2/b4/s128 8x4/b8/s128 8x4/b4/s128 8x2/b8/s256 8x2/b4/s256 4x4/b8/s256 4x4/b4/s256 4x2/b8/s256 4x2/b4/s256 4x1/b8/s256 4x1/b4/s256"},
    {"cfg4", 8192u, 1875u, "filter_scan=2",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 768/0 scratch 768 | most 16 cap 1 budget 114688 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"cfg4", 8192u, 4u, "persistent resume",
     "seg 1x4 warm 0 | image 0/99024 scan 0 stages 1 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x2/b8/s128 16x2/b4/s128 8x4/b8/s128 8x4/b4/s128 8x2/b8/s256 8x2/b4/s256 4x4/b8/s256 4x4/b4/s256 4x2/b8/s256 4x2/b4/s256 4x1/b8/s256 4x1/b4/s256"},
    {"cfg4", 1u, 40u, "handoff",
     "seg 1x40 warm 0 | image 0/99024 scan 0 stages 1 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "1x1/b8/s256 1x1/b4/s256"},
    {"filter_long", 1u, 1875u, "",
     "seg 209x9 warm 1 | image 0/99024 scan 0 stages 1 mod 0 rotate 0 optwarm 1 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 1 | err 0",
     "1x1/b8/s256 1x1/b4/s256"},
    {"filter_long", 1u, 1875u, "filter_warm=0",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"filter_long", 1u, 1875u, "filter_warm=3",
     "seg 625x3 warm 1 | image 0/99024 scan 0 stages 1 mod 0 rotate 0 optwarm 1 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 1 | err 0",
     "3x1/b8/s256 3x1/b4/s256"},
    {"filter_long", 1u, 1875u, "wave_segments=0",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"filter_long", 1u, 1875u, "wave_segments=1",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"filter_long", 1u, 1875u, "wave_segments=5",
     "seg 5x375 warm 1 | image 0/99024 scan 0 stages 1 mod 0 rotate 0 optwarm 1 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 1 | err 0",
     "1x1/b8/s256 1x1/b4/s256"},
    {"filter_long", 1u, 1875u, "inputs",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"filter_long", 4096u, 1875u, "",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"fm", 5u, 1875u, "",
     "seg 209x9 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "8x1/b8/s256 4x1/b8/s256"},
    {"fm", 5u, 1875u, "wave_segments=0",
     "seg 1x1875 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"fm", 5u, 1875u, "wave_segments=1",
     "seg 1x1875 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"fm", 5u, 1875u, "wave_segments=7",
     "seg 7x268 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "1x1/b8/s256"},
    {"fm", 65536u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"osc96k", 1u, 3750u, "",
     "seg 417x9 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 0 | err 0",
     "2x1/b8/s256"},
    {"osc96k", 65536u, 375u, "",
     "seg 1x375 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x4/b8/s256 16x2/b8/s256 16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"delay", 8192u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 768/0 scratch 768 | most 16 cap 1 budget 114688 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"delay", 8192u, 188u, "delay_line=0",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"delay", 8192u, 188u, "delay_line=2",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/1 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"light", 65536u, 188u, "force=2x1",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "2x1/b8/s256"},
    {"light", 65536u, 188u, "force=16x4",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x4/b8/s256"},
    {"filter_stage", 8192u, 188u, "force=16x4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x4/b8/s32"},
    {"filter_stage", 8192u, 188u, "force=4x2",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "4x2/b8/s64"},
    {"filter_stage", 16384u, 188u, "wave_per_wave=4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x4/b8/s32 16x4/b4/s32 16x2/b8/s64 16x2/b4/s64 8x4/b8/s64 8x4/b4/s64 8x2/b8/s64 8x2/b4/s64 4x4/b8/s64 4x4/b4/s64 4x2/b8/s64 4x2/b4/s64 4x1/b8/s64 4x1/b4/s64"},
    {"filter_stage", 16384u, 188u, "wave_per_wave=1",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 1 budget 163840 stage 1 | err 0",
     "16x1/b8/s64 16x1/b4/s64 8x1/b8/s64 8x1/b4/s64 4x1/b8/s64 4x1/b4/s64"},
    {"light", 65536u, 188u, "wave_per_wave=2",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 2 budget 163840 stage 0 | err 0",
     "16x2/b8/s256 16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"osc", 65536u, 188u, "wave_per_wave=4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x4/b8/s256 16x2/b8/s256 16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"osc", 65536u, 188u, "wave_max_waves=4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 4 cap 4 budget 163840 stage 0 | err 0",
     "4x1/b8/s256"},
    {"filter_stage", 65536u, 188u, "wave_max_waves=4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 4 cap 4 budget 163840 stage 1 | err 0",
     "4x4/b8/s64 4x4/b4/s64 4x2/b8/s64 4x2/b4/s64 4x1/b8/s64 4x1/b4/s64"},
    {"filter_stage", 65536u, 188u, "wave_max_waves=3",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 3 cap 4 budget 163840 stage 1 | err 0",
     "3x4/b8/s64 3x4/b4/s64 3x2/b8/s64 3x2/b4/s64 3x1/b8/s64 3x1/b4/s64"},
    {"osc", 65536u, 188u, "jit_lds_table=0",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 0 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 0 | err 0",
     "16x4/b8/s256 16x2/b8/s256 16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"cfg4", 8192u, 1875u, "jit_rotate=0",
     "seg 1x1875 warm 0 | image 0/99024 scan 1 stages 0 mod 0 rotate 0 optwarm 0 voices 0 lines 768/0 scratch 768 | most 16 cap 1 budget 114688 stage 0 | err 0",
     "16x1/b8/s256 8x1/b8/s256 4x1/b8/s256"},
    {"cfg4", 8192u, 1875u, "filter_scan=0 force=16x4",
     "seg 1x1875 warm 0 | image 0/99024 scan 0 stages 1 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x4/b8/s64"},
    {"cfg4", 8192u, 1875u, "filter_scan=0 delay_line=0 force=16x4",
     "seg 1x1875 warm 0 | image 0/99024 scan 0 stages 1 mod 0 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x4/b8/s64"},
    {"filter_stage", 8192u, 188u, "jit_lds_table=0 force=16x4",
     "seg 1x188 warm 0 | image -1/0 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 0 | most 16 cap 4 budget 163840 stage 1 | err 0",
     "16x4/b8/s64"},
    {"comb_filter", 8192u, 188u, "",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 768 | most 16 cap 4 budget 114688 stage 1 | err 0",
     "16x1/b8/s32 16x1/b4/s32 8x2/b8/s32 8x2/b4/s32 4x4/b8/s32 4x4/b4/s32 4x2/b8/s64 4x2/b4/s64 4x1/b8/s64 4x1/b4/s64"},
    {"comb_filter", 8192u, 188u, "force=16x4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 768 | most 16 cap 4 budget 114688 stage 1 | err 1",
     ""},
    {"comb_filter", 8192u, 188u, "force=16x1",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 768 | most 16 cap 4 budget 114688 stage 1 | err 0",
     "16x1/b8/s32"},
    {"comb_filter", 8192u, 188u, "wave_max_waves=4",
     "seg 1x188 warm 0 | image 0/99024 scan 0 stages 1 mod 1 rotate 1 optwarm 0 voices 0 lines 0/0 scratch 768 | most 4 cap 4 budget 151552 stage 1 | err 0",
     "4x4/b8/s64 4x4/b4/s64 4x2/b8/s64 4x2/b4/s64 4x1/b8/s64 4x1/b4/s64"},
};

static JitSite reference_site(const Program &P) {
    JitSite site;
    site.n_cus = 256;
    if (P.g.sample_rate % 2 == 0) {
        site.table_form[1] = 1, site.table_form[2] = 2, site.table_form[4] = 4;
        if (P.g.sample_rate % 4 == 0) site.table_form[3] = 3;
        for (int k = 0; k < 5; k++) site.table_bound[k] = 1, site.table_antisym[k] = true;
        site.table_delta[0] = 1;
    }
    return site;
}

static void fail(const char *what, const std::string &detail) {
    g_bad++;
    std::printf("FAIL: %s: %s\n", what, detail.c_str());
}

static void check_rows(std::map<std::string, std::vector<double>> &circuits) {
    for (const Row &row : kRows) {
        g_cases++;
        const std::string id = std::string(row.circuit) + " " + std::to_string(row.n_inst) + " x " + std::to_string(row.n_chunks) + " [" + row.words + "]";
        Program P;
        WavePlan wave;
        if (!circuits.count(row.circuit) || !load_circuit(circuits[row.circuit], P, wave)) {
            fail("no such circuit", id);
            continue;
        }
        JitSite site = reference_site(P);
        JitBatch batch;
        batch.n_inst = row.n_inst;
        batch.n_chunks = row.n_chunks;
        apply_words(row.words, site.knobs, batch.persistent, batch.resume, batch.handoff, batch.inputs);
        VoicePlan voices;  // (as render_jit finds the verdict it caches)
        batch.voice_loop = !batch.persistent && P.ops.size() > jit_loop_voices_from() && jit_find_voices(P, wave, voices);
        JitPlan plan = jit_plan(site, batch, P, wave);
        const std::string got = describe(plan.n_seg, plan.seg_groups, plan.warm, plan.opt, plan.most, plan.per_wave_cap, plan.budget, plan.filter_stage, plan.error != nullptr);
        if (got != row.plan) fail(id.c_str(), "plan\n    got  " + got + "\n    want " + row.plan);
        if (plan.n_virtual != (uint64_t)row.n_inst * plan.n_seg) fail(id.c_str(), "n_virtual");
        std::string ladder;
        if (!plan.error) {
            int steps = 0;
            do {
                if (plan.waves != plan.opt.waves || plan.per_wave != plan.opt.per_wave) fail(id.c_str(), "the plan's geometry and its options' differ");
                if (plan.filter_stage && !plan.opt.filter_sub) fail(id.c_str(), "a Filter step without rows");
                if (plan.waves * plan.per_wave < 1) fail(id.c_str(), "an empty workgroup");
                ladder += (ladder.empty() ? "" : " ") + step_name(plan.opt);
            } while (!site.knobs.jit_force_waves && jit_spill_step(plan) && ++steps < 64);
            if (steps >= 64) fail(id.c_str(), "the ladder does not end");
        }
        if (ladder != row.ladder) fail(id.c_str(), "ladder\n    got  " + ladder + "\n    want " + row.ladder);
    }
}

// Two option sets that differ in exactly one of the fields a text depends on from render to render get different keys
static void check_keys() {
    JitOptions base;
    base.waves = 16, base.per_wave = 2;
    for (int field = 0; field < 7; field++) {
        JitOptions o = base;
        const char *name = "";
        switch (field) {
            case 0: o.waves = 8, name = "waves"; break;
            case 1: o.per_wave = 4, name = "per_wave"; break;
            case 2: o.filter_block = 4, name = "filter_block"; break;
            case 3: o.voice_loop = true, name = "voice_loop"; break;
            case 4: o.filter_scan = true, name = "filter_scan"; break;
            case 5: o.rotate = false, name = "rotate"; break;
            case 6: o.warm = true, name = "warm"; break;
        }
        g_cases++;
        if (jit_source_key(o) == jit_source_key(base)) fail("two texts under one key", name);
    }
    // ... and all combinations of them, over every geometry: no two of them share a key
    std::map<std::pair<int, int>, int> seen;
    for (int waves = 1; waves <= 16; waves++)
        for (int per_wave = 1; per_wave <= 4; per_wave++)
            for (int bits = 0; bits < 32; bits++) {
                JitOptions o;
                o.waves = waves, o.per_wave = per_wave;
                o.filter_block = bits & 1 ? 4 : 8, o.voice_loop = bits & 2, o.filter_scan = bits & 4, o.rotate = !(bits & 8), o.warm = bits & 16;
                g_cases++;
                if (seen[jit_source_key(o)]++) fail("two texts under one key", std::to_string(waves) + " x " + std::to_string(per_wave) + ", bits " + std::to_string(bits));
            }
}

// The shared segment count against the expression both engines carried before (restated: the reference here is the arithmetic)
static void check_segments() {
    const uint32_t insts[] = {1, 2, 7, 64, 2047, 2048, 2049, 1u << 24}, chunks[] = {1, 7, 8, 9, 188, 1875, 1u << 23};
    const int knobs[] = {-1, 0, 1, 2, 5, 1000000};
    const int n_cus = 256;
    for (uint32_t n_inst : insts)
        for (uint32_t n_chunks : chunks)
            for (int knob : knobs) {
                uint32_t want_seg = 1, want_groups = n_chunks;
                const uint64_t target = (uint64_t)n_cus * 8;
                uint64_t n_seg = n_inst >= target ? 1 : std::min<uint64_t>(target / n_inst, n_chunks / 8);
                if (knob >= 0) n_seg = (uint64_t)knob;
                n_seg = std::max<uint64_t>(1, std::min<uint64_t>(n_seg, n_chunks));
                if (n_seg > 1) want_groups = (uint32_t)((n_chunks + n_seg - 1) / n_seg), want_seg = (uint32_t)((n_chunks + want_groups - 1) / want_groups);
                uint32_t got_seg = 0, got_groups = 0;
                jit_time_segments(n_cus, knob, n_inst, n_chunks, got_seg, got_groups);
                g_cases++;
                const std::string id = std::to_string(n_inst) + " x " + std::to_string(n_chunks) + ", knob " + std::to_string(knob);
                if (got_seg != want_seg || got_groups != want_groups) fail("segment count", id);
                if (got_seg < 1 || (uint64_t)got_seg * got_groups < n_chunks) fail("segments do not cover the render", id);
                if ((uint64_t)(got_seg - 1) * got_groups >= n_chunks) fail("an empty segment", id);
            }
}

int main(int argc, char **argv) {
    std::map<std::string, std::vector<double>> circuits;
    for (int a = 1; a < argc; a++) {
        const std::string arg = argv[a];
        const size_t eq = arg.find('=');
        FILE *f = eq == std::string::npos ? nullptr : std::fopen(arg.substr(eq + 1).c_str(), "rb");
        if (!f) {
            fail("cannot open", arg);
            continue;
        }
        double w;
        std::vector<double> &words = circuits[arg.substr(0, eq)];
        while (std::fread(&w, sizeof w, 1, f) == 1) words.push_back(w);
        std::fclose(f);
    }
    check_rows(circuits);
    check_keys();
    check_segments();
    std::printf("{\"cases\": %ld, \"rows\": %zu, \"bad\": %ld}\n", g_cases, sizeof kRows / sizeof kRows[0], g_bad);
    return g_bad ? 1 : 0;
}
