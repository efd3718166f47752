// score_rows_kernel_check.cpp — the text of dusp_amd/csrc/score_rows_engine.hip compiled for the HOST (hip_host_stub/: lanes one after the
// other), fed score_rows_plan's plans, and held to a plain loop over the contract (dusp_amd/mix.py score_chain_rows) on bit patterns.
// EVERY ROW IS A HEAP ALLOCATION OF ITS OWN, exactly channels x samples floats (none at all for an empty row), so under AddressSanitizer
// one float read outside a row — the unpredicated load of a lane an entry does not cover, a padded entry that names voice 0 — is reported.
// Covered: gains, init (a second buffer, in place), raw; no voices; one and two channels; 1, 9 and 37 voices (no multiples of the
// kernel's depth); rows of 1, 3, 255, 256, 257 and 773 samples mixed in one list; a first voice of length 0 (with a row, and with no row
// at all); onsets of every residue mod 4 and both signs; spans that end inside a block and on a block boundary; blocks no voice reaches;
// windows of the timeline (what lies outside stays as it was); plans whose block was doubled.  The output lies between sentinels, the
// plan's image is an exact-size allocation on a 32-byte boundary.  Built with -fsanitize=address,undefined by tests/test_piece_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "windows": w, "zero_first": z}.
#include "../../dusp_amd/csrc/score_rows_engine.hip"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
static float or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }
int main() {
    std::mt19937 rng(10);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, doubled = 0, windows = 0, zero_first = 0;
    const int totals[] = {1, 255, 256, 257, 1022, 2317};
    const int row_lens[] = {1, 3, 255, 256, 257, 773};
    for (int NT : totals) for (int C : {1, 2}) for (int N : {0, 1, 9, 37})
    for (int variant = 0; variant < 12; variant++) {
        const int gains = variant & 1, init = (variant >> 1) % 3, raw = variant >= 6;
        for (int layout : {0, 1, 2, 3}) for (int first : {0, 1, 2}) {  // first: 0 any voice 0; 1 voice 0 has a row but length 0; 2 voice 0 has no row at all
            // layout: 0 scattered onsets, 1 onsets at block boundaries and in front of 0, 2 bunched (empty blocks, a window), 3 a small plan budget
            if (N == 0 && (layout || first)) continue;
            const int off = (int)(rng() % 4);
            std::vector<int64_t> onsets(N), lens(N);
            std::vector<uint32_t> samples(N);
            std::vector<std::unique_ptr<float[]>> rows(N);
            std::vector<uint64_t> addr(N);
            for (int k = 0; k < N; k++) {
                const int NV = row_lens[(k + rng() % 6) % 6];
                samples[k] = (uint32_t)NV;
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4;
                else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4;  // both signs, every residue, past the end too
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                if (layout == 1 && k % 3 == 0 && onsets[k] >= 0) lens[k] = std::min<int64_t>(NV, 256 - onsets[k] % 256);  // a span that ends on a block boundary
            }
            bool with_lens = variant % 4 != 3;
            if (first == 1) { lens[0] = 0; with_lens = true; }
            if (first == 2) { samples[0] = 0; lens[0] = 0; }
            zero_first += first != 0;
            for (int k = 0; k < N; k++) {
                const size_t row = (size_t)C * samples[k];
                if (!row) continue;  // (no row at all: a NULL address, which nothing may read)
                rows[k].reset(new float[row]);  // exactly its size: one float past it is the sanitizer's
                addr[k] = (uint64_t)(uintptr_t)rows[k].get();
                for (size_t j = 0; j < row; j++) rows[k][j] = nd(rng) * std::pow(10.f, (float)(k % 7) - 3);
                for (size_t j = (size_t)k % 29; j < row; j += 29) rows[k][j] = (j & 1) ? -0.0f : (j % 3 ? INFINITY : 1e-41f);
                if (k == N / 2 && row > 3) rows[k][3] = NAN;
            }
            const size_t trow = (size_t)C * NT;
            std::vector<float> g(N), ini(trow), out_s(trow + 128 + off);
            for (auto &x : g) x = 0.05f + 1.9f * (rng() % 1000) / 1000.f;
            if (N > 2) g[1] = -g[1];
            for (size_t k = 0; k < trow; k++) ini[k] = (k % 13 == 0) ? -0.0f : 30 * nd(rng);
            const float S = -12345.678f;
            for (auto &x : out_s) x = S;
            float *out = out_s.data() + 64 + off;
            dusp::ScoreRowsPlan P;
            const bool whole = layout != 2 || init != 2;  // a window only in place: outside it nothing is written
            const int64_t rc = dusp::score_rows_plan(onsets.data(), with_lens ? lens.data() : nullptr, samples.data(), addr.data(), (size_t)N, NT, whole,
                                                     layout == 3 ? 600 : dusp::kScorePlanBytes, P, {});
            if (rc != -1) { bad++; continue; }
            doubled += P.block_shift > dusp::kScoreGroupShift;
            windows += !whole && P.w_hi > P.w_lo && (P.w_lo > 0 || P.w_hi < NT);
            const float *pinit = nullptr;
            if (init == 1) pinit = ini.data();
            if (init == 2) { memcpy(out, ini.data(), trow * 4); pinit = out; }
            std::vector<float> want(trow);  // the contract
            for (int c = 0; c < C; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) { want[o] = ini[o]; continue; }  // (only with init == 2: out as it was)
                volatile float acc = init ? ini[o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const int64_t s = t - onsets[k], len = with_lens ? lens[k] : (int64_t)samples[k];
                    if (s < 0 || s >= len) continue;
                    volatile float term = rows[k][(size_t)c * samples[k] + s];
                    if (gains) term = term * g[k];
                    acc = acc + term;
                }
                want[o] = raw ? (float)acc : or0(acc);
            }
            if (P.w_hi > P.w_lo) {
                std::vector<unsigned char> packed;
                const size_t at = dusp::score_plan_pack(P, packed);
                void *image = nullptr;  // exact size, on the 32-byte boundary the device's buffer gives it
                if (at != 0 || posix_memalign(&image, 32, std::max<size_t>(packed.size(), 1)) != 0) { bad++; continue; }
                memcpy(image, packed.data(), packed.size());
                const dusp::ScoreRow *dv = (const dusp::ScoreRow *)image;
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                const bool any = P.n_entries() > 0;  // (as the ABI: no listed voice, no plan)
                dusp::launch_score_rows(gains ? g.data() : nullptr, any ? dv : nullptr, any ? bf : nullptr, any ? en : nullptr, pinit, out, (uint32_t)C, NT, (uint64_t)P.w_lo,
                                        (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
                free(image);
            }
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t p = 0; p < trow; p++) {
                if (want[p] != want[p]) ok &= out[p] != out[p];
                else ok &= memcmp(&out[p], &want[p], 4) == 0;
            }
            checked++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d C %d N %d variant %d layout %d first %d off %d shift %u\n", NT, C, N, variant, layout, first, off, P.block_shift); }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"windows\": %ld, \"zero_first\": %ld}\n", checked, bad, doubled, windows, zero_first);
    return bad != 0;
}
