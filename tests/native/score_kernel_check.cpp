// score_kernel_check.cpp — the text of dusp_amd/csrc/score_engine.hip compiled for the HOST (hip_host_stub/: lanes one after the other), fed the
// plan of score_plan.hpp, and held to a plain loop over the contract (dusp_amd/mix.py score_chain) on bit patterns: gains, init (a second
// buffer, in place), raw, no voices at all, bases off the 16-byte boundaries, n_total and n_voice at every residue mod 4, one and two
// channels, onsets of every residue mod 4 and both signs, 1 / 9 / 37 voices (9 and 37 are no multiples of the kernel's depth), spans that
// end inside a unit, inside a block and on a block boundary, blocks no voice reaches, windows of the timeline (a tile's union window: what
// lies outside must stay as it was), and plans whose block was doubled.  Every buffer is exactly as long as the call says, between sentinels
// where the kernel writes: built with -fsanitize=address,undefined by tests/test_score_host.py, an index past a buffer is an error here, not a
// fault on a shared GPU.  Prints {"cases": n, "bad": m, "doubled": plans with a doubled block, "windows": launches over part of the timeline}.
#include "../../dusp_amd/csrc/score_engine.hip"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
static float or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }
int main() {
    std::mt19937 rng(9);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, doubled = 0, windows = 0;
    const int totals[] = {1, 255, 256, 257, 1022, 2317};
    const int voices_len[] = {1, 4, 253, 254, 255, 256, 773};
    for (int NT : totals) for (int NV : voices_len) for (int C : {1, 2}) for (int N : {0, 1, 9, 37})
    for (int variant = 0; variant < 12; variant++) {
        const int gains = variant & 1, init = (variant >> 1) % 3, raw = variant >= 6;
        for (int layout : {0, 1, 2, 3}) {  // 0 scattered onsets, 1 onsets at block boundaries and in front of 0, 2 bunched (empty blocks, a window), 3 a small plan budget
            if (N == 0 && layout) continue;
            const int off = (int)(rng() % 4), inoff = (int)(rng() % 4);
            std::vector<int64_t> onsets(N), lens(N);
            for (int k = 0; k < N; k++) {
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4;
                else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4;  // both signs, every residue, past the end too
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                if (layout == 1 && k % 3 == 0 && onsets[k] >= 0) lens[k] = std::min<int64_t>(NV, 256 - onsets[k] % 256);  // a span that ends on a block boundary
            }
            const bool with_lens = variant % 4 != 3;
            const size_t row = (size_t)C * NV, trow = (size_t)C * NT;
            // exact-size buffers (heap: the sanitizer sees one float past them), the output between sentinels
            std::vector<float> in_s((size_t)N * row + inoff), g(N), ini(trow), out_s(trow + 128 + off);
            float *in = in_s.data() + inoff;  // (the allocator's 16-byte boundary + inoff floats)
            for (size_t k = 0; k < (size_t)N * row; k++) in[k] = nd(rng) * std::pow(10.f, (float)(k / row % 7) - 3);
            for (size_t k = 0; k < (size_t)N * row; k += 29) in[k] = (k & 1) ? -0.0f : (k % 3 ? INFINITY : 1e-41f);
            if (N > 2 && row > 3) in[(N / 2) * row + 3] = NAN;
            if (N) for (size_t k = 0; k < row; k++) if (k % 11 == 5) in[k] = -0.0f;
            for (auto &x : g) x = 0.05f + 1.9f * (rng() % 1000) / 1000.f;
            if (N > 2) g[1] = -g[1];
            for (size_t k = 0; k < trow; k++) ini[k] = (k % 13 == 0) ? -0.0f : 30 * nd(rng);
            const float S = -12345.678f;
            for (auto &x : out_s) x = S;
            float *out = out_s.data() + 64 + off;
            dusp::ScorePlan P;
            const bool whole = layout != 2 || init != 2;  // a window only in place: outside it nothing is written
            const int64_t rc = dusp::score_plan(onsets.data(), with_lens ? lens.data() : nullptr, (size_t)N, NV, NT, whole, layout == 3 ? 600 : dusp::kScorePlanBytes, P);
            if (rc != -1) { bad++; continue; }
            doubled += P.block_shift > dusp::kScoreGroupShift;
            windows += !whole && P.w_hi > P.w_lo && (P.w_lo > 0 || P.w_hi < NT);
            const float *pinit = nullptr;
            if (init == 1) pinit = ini.data();
            if (init == 2) { memcpy(out, ini.data(), trow * 4); pinit = out; }
            // the contract
            std::vector<float> want(trow);
            for (int c = 0; c < C; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) { want[o] = ini[o]; continue; }  // (only with init == 2: out as it was)
                volatile float acc = init ? ini[o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const int64_t s = t - onsets[k], len = with_lens ? lens[k] : NV;
                    if (s < 0 || s >= len) continue;
                    volatile float term = in[(size_t)k * row + (size_t)c * NV + s];
                    if (gains) term = term * g[k];
                    acc = acc + term;
                }
                want[o] = raw ? (float)acc : or0(acc);
            }
            if (P.w_hi > P.w_lo) {
                // the plan's image, exact size on the heap
                std::vector<unsigned char> image;
                const size_t at = dusp::score_plan_pack(P, image);
                const dusp::ScoreVoice *dv = (const dusp::ScoreVoice *)(image.data() + at);
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                const bool any = N > 0;
                dusp::launch_score(in, gains ? g.data() : nullptr, any ? dv : nullptr, any ? bf : nullptr, any ? en : nullptr, pinit, out, (uint32_t)C, NV, NT,
                                   (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
            }
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t p = 0; p < trow; p++) {
                if (want[p] != want[p]) ok &= out[p] != out[p];
                else ok &= memcmp(&out[p], &want[p], 4) == 0;
            }
            checked++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d NV %d C %d N %d variant %d layout %d off %d inoff %d shift %u\n", NT, NV, C, N, variant, layout, off, inoff, P.block_shift); }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"windows\": %ld}\n", checked, bad, doubled, windows);
    return bad != 0;
}
