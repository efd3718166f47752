// dusp_amd/csrc/jit_plan.hpp on the CPU: a tile of a mix (JitBatch::whole_n_inst) decides what changes BITS as one render of the whole
// batch does — whether the render is cut into warming segments (the Filter stage's arithmetic) and with it whether the Filters scan.
//   mix_plan_check FILE   (the descriptor words of a long feed-forward Filter circuit, as f64)
// Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../dusp_amd/csrc/jit_plan.hpp"

using namespace dusp;

int main(int argc, char **argv) {
    std::vector<double> words;
    FILE *f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    double w;
    while (std::fread(&w, sizeof w, 1, f) == 1) words.push_back(w);
    std::fclose(f);
    Program P;
    WavePlan wave;
    std::string err, why;
    if (!compile(words.data(), words.size(), P, err, /*continuation=*/false) || !plan_wave(P, wave, false) || !jit_eligible(P, wave, why)) return 2;
    JitSite site;
    site.n_cus = 256;
    for (int k = 0; k < 5; k++) site.table_bound[k] = 1, site.table_antisym[k] = true;
    long cases = 0, bad = 0, warm_wholes = 0, scan_wholes = 0, tiles_that_alone_differ = 0;
    const uint32_t wholes[] = {1, 2, 37, 100, 2047, 2048, 2049, 4096, 8192, 65536}, tiles[] = {1, 3, 64, 1024, 2048, 2049, 8192};
    const uint32_t chunks[] = {6, 31, 32, 33, 188, 1875};
    const int warm_knobs[] = {1, 3, 0};  // DUSP_FILTER_WARM: by the Filters, segments of 3 chunks (a threshold of two segments), off
    for (int knob : warm_knobs)
        for (uint32_t n_chunks : chunks)
            for (uint32_t whole : wholes) {
                site.knobs.filter_warm = knob;
                JitBatch b;
                b.n_inst = whole;
                b.n_chunks = n_chunks;
                const JitPlan want = jit_plan(site, b, P, wave);
                warm_wholes += want.warm;
                scan_wholes += want.opt.filter_scan;
                if (want.warm && want.opt.filter_scan) bad++, std::printf("FAIL: warming segments that scan\n");
                for (uint32_t tile : tiles) {
                    if (tile > whole) continue;
                    for (uint32_t n : {tile, whole % tile}) {  // the full tiles and the ragged last one
                        if (!n) continue;
                        JitBatch t = b;
                        t.n_inst = n;
                        const JitPlan alone = jit_plan(site, t, P, wave);
                        t.whole_n_inst = whole;
                        const JitPlan got = jit_plan(site, t, P, wave);
                        cases++;
                        tiles_that_alone_differ += alone.opt.filter_scan != want.opt.filter_scan;
                        if (got.warm != want.warm || got.opt.filter_scan != want.opt.filter_scan) {
                            bad++;
                            std::printf("FAIL: %u of %u instances x %u chunks, DUSP_FILTER_WARM=%d: warm %d scan %d, the whole batch %d %d\n", n, whole, n_chunks, knob, (int)got.warm,
                                        (int)got.opt.filter_scan, (int)want.warm, (int)want.opt.filter_scan);
                        }
                    }
                }
            }
    std::printf("{\"cases\": %ld, \"bad\": %ld, \"warm_wholes\": %ld, \"scan_wholes\": %ld, \"tiles_that_alone_differ\": %ld}\n", cases, bad, warm_wholes, scan_wholes, tiles_that_alone_differ);
    return bad ? 1 : 0;
}
