// score_space_kernel_check.cpp — the text of dusp_amd/csrc/score_space_engine.hip compiled for the HOST (hip_host_stub/: lanes one after
// the other), fed score_rows_plan's plans WITH TAPS and score_space_tap's records, and held to a plain loop per timeline sample over the
// contract (dusp_amd/mix.py score_chain_rows_placed) on bit patterns.  The brute-force chain forms a tap the way the reference's Gain
// and MonoDelay do (Gain.js:22, MonoDelay.js:24-26) — y = f32(G * f64(x)); the ceil tap of sample s - 1 rounded to f32 alone in its
// slot, the floor tap of sample s added to it in f64, every operation rounded by itself (volatile).  EVERY ROW IS A HEAP ALLOCATION OF
// ITS OWN, exactly its samples (none at all for an empty row), so under AddressSanitizer a read of row[len] (the tail tap's lane must
// not load x[len]) or of row[-1] (the first lane must not load x[-1]) is reported; so is the tap array, an exact-size allocation on its
// 32-byte boundary.
// Covered: both instantiations (gains or none); init (a second buffer, in place), raw; lists of 1, 8, 9 and 37 voices; C = 1, 2, 3 and
// 6 speakers; whole and fractional taps mixed in one voice and in one list, lists of whole taps only and of fractional ones only;
// delays 0, 0.5, 2^-24, 1 - 2^-53, 255, 256.25 and one past the timeline; shifts that put one channel's span wholly outside the window
// while another's is inside; rows of 1, 3, 255, 256, 257 and 773 samples; len = 1; spans that end inside a group, on a group boundary
// and on n_total; a first voice of length 0 (with a row, and with none); output bases 0 .. 3 floats past the buffer's start; windows of
// the timeline; plans whose block was doubled.  Built with -fsanitize=address,undefined by tests/test_space_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "windows": w, "two_taps": t, "one_taps": o, "outside": x, "whole_lists": l}.
#include "../../dusp_amd/csrc/score_space_engine.hip"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
static float or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }
int main() {
    std::mt19937 rng(23);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, doubled = 0, windows = 0, two_taps = 0, one_taps = 0, outside = 0, whole_lists = 0;
    const int totals[] = {1, 256, 257, 1301};
    const int row_lens[] = {1, 3, 255, 256, 257, 773};
    for (int NT : totals) for (int N : {1, 8, 9, 37})
    for (int variant = 0; variant < 12; variant++) for (int C : {1, 2, 3, 6}) {
        const int gains = variant & 1, init = (variant >> 1) % 3, raw = variant >= 6;
        const double edge_delays[] = {0.0, 0.5, 0x1p-24, 1.0 - 0x1p-53, 255.0, 256.25, (double)NT - 0.5};
        for (int layout : {0, 1, 2, 3, 4}) for (int first : {0, 1, 2}) {  // first: 0 any voice 0; 1 voice 0 has a row but length 0; 2 voice 0 has no row at all
            // layout: 0 scattered onsets, 1 onsets at block boundaries and in front of 0, 2 bunched (empty blocks, a window), 3 a small plan budget,
            //         4 the edge placements in turn (a span ending on a group boundary, on n_total, the tail tap on a boundary, onset -len - shift)
            if (first && (N == 1 || (layout != 0 && layout != 3 && layout != 4))) continue;
            const int off = (int)(rng() % 4);
            const int tap_mode = (int)(rng() % 8);  // 0: whole taps only; 1: every tap fractional; else mixed
            std::vector<int64_t> onsets(N), lens(N);
            std::vector<uint32_t> samples(N);
            std::vector<std::unique_ptr<float[]>> rows(N);
            std::vector<uint64_t> addr(N);
            std::vector<double> delays((size_t)N * C), tg((size_t)N * C);
            bool with_lens = variant % 4 != 3;
            for (int k = 0; k < N; k++) {
                const int NV = row_lens[(k + rng() % 6) % 6];
                samples[k] = (uint32_t)NV;
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                const int64_t len = with_lens ? lens[k] : NV;
                for (int c = 0; c < C; c++) {
                    const unsigned dk = rng() % 10;
                    double D = dk < 4 ? edge_delays[rng() % 7] : dk == 4 ? (double)(NT + 3 * NV + (int)(rng() % 50)) : (double)(rng() % 700) + (double)(rng() % 1024) / 1024.0;
                    if (dk == 5) D = (double)(rng() % 3) * 256.0;                     // whole, on a group boundary
                    if (tap_mode == 0) D = std::floor(D);
                    if (tap_mode == 1 && D == std::floor(D)) D += 0.375;
                    delays[(size_t)k * C + c] = D;
                    tg[(size_t)k * C + c] = (rng() % 7 == 0) ? 1.0 : (rng() % 7 == 1) ? -0.0 : std::pow(10.0, -3.0 * (double)(rng() % 1000) / 1000.0 / 20.0 * 8.0);
                }
                const int64_t shift0 = (int64_t)std::floor(delays[(size_t)k * C]);
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4 - shift0;
                else if (layout == 4) {
                    const int ek = (k + variant) % 6;
                    onsets[k] = (ek == 0 ? -1 : ek == 1 ? -len : ek == 2 ? NT - len : ek == 3 ? NT - 1 : ek == 4 ? (int64_t)(1 + rng() % 4) * 256 - len : 256 - len - 1) - shift0;
                } else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4 - (rng() % 3 == 0 ? shift0 : 0);  // both signs, every residue, past the end too
            }
            if (first == 1) { lens[0] = 0; with_lens = true; }
            if (first == 2) { samples[0] = 0; lens[0] = 0; }
            for (int k = 0; k < N; k++) {
                const size_t row = samples[k];
                if (!row) continue;  // (no row at all: a NULL address, which nothing may read)
                rows[k].reset(new float[row]);  // exactly its size: one float past it, or in front of it, is the sanitizer's
                addr[k] = (uint64_t)(uintptr_t)rows[k].get();
                for (size_t j = 0; j < row; j++) rows[k][j] = nd(rng) * std::pow(10.f, (float)(k % 7) - 3);
                for (size_t j = (size_t)k % 29; j < row; j += 29) rows[k][j] = (j & 1) ? -0.0f : (j % 3 ? INFINITY : (j % 5 ? 1e-41f : FLT_MAX));
                if (k == N / 2 && row > 3) rows[k][3] = NAN;
                if (row > 5) rows[k][5] = 5e-39f;
            }
            const size_t trow = (size_t)C * NT;
            std::vector<float> g(N), ini(trow), out_s(trow + 128 + off);
            for (auto &x : g) x = 0.05f + 1.9f * (rng() % 1000) / 1000.f;
            if (N > 2) g[1] = -g[1];
            for (size_t k = 0; k < trow; k++) ini[k] = (k % 13 == 0) ? -0.0f : 30 * nd(rng);
            const float S = -12345.678f;
            for (auto &x : out_s) x = S;
            float *out = out_s.data() + 64 + off;
            void *tapmem = nullptr;  // exactly its size, on the boundary the device's image gives it
            if (posix_memalign(&tapmem, 32, (size_t)N * C * sizeof(dusp::ScoreSpaceTap)) != 0) { bad++; continue; }
            dusp::ScoreSpaceTap *taps = (dusp::ScoreSpaceTap *)tapmem;
            for (size_t j = 0; j < (size_t)N * C; j++) taps[j] = dusp::score_space_tap(delays[j], tg[j]);
            dusp::ScoreRowsPlan P;
            const bool whole = layout != 2 || init != 2;  // a window only in place: outside it nothing is written
            const int64_t rc = dusp::score_rows_plan(onsets.data(), with_lens ? lens.data() : nullptr, samples.data(), addr.data(), (size_t)N, NT, whole,
                                                     layout == 3 ? 600 : dusp::kScorePlanBytes, P, {nullptr, taps, (size_t)C});
            if (rc != -1) { bad++; free(tapmem); continue; }
            if (P.n_entries() == 0) { free(tapmem); continue; }  // (no listed voice: the launch is the rows kernel's)
            doubled += P.block_shift > dusp::kScoreGroupShift;
            windows += !whole && (P.w_lo > 0 || P.w_hi < NT);
            whole_lists += tap_mode == 0;
            const float *pinit = nullptr;
            if (init == 1) pinit = ini.data();
            if (init == 2) { memcpy(out, ini.data(), trow * 4); pinit = out; }
            std::vector<float> want(trow);  // the contract, sample by sample
            for (int c = 0; c < C; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) { want[o] = ini[o]; continue; }  // (only with init == 2: out as it was)
                volatile float acc = init ? ini[o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const double D = delays[(size_t)k * C + c], G = tg[(size_t)k * C + c];
                    const double whole_d = std::floor(D);
                    const double w1 = D - whole_d;
                    const int64_t s = t - onsets[k] - (int64_t)whole_d, len = with_lens ? lens[k] : (int64_t)samples[k];
                    auto y_of = [&](int64_t at) {  // the voice's sample after its gain and the tap's Gain; at is within [0, len)
                        volatile float x = rows[k][(size_t)at];
                        if (gains) x = x * g[k];
                        volatile double y = G * (double)x;
                        return (float)y;
                    };
                    if (c == 0 && t == 0 && len > 0) {  // (counted once a voice: a channel wholly outside the window beside one inside it)
                        bool any_in = false, any_out = false;
                        for (int cc = 0; cc < C; cc++) {
                            const int64_t a = onsets[k] + (int64_t)std::floor(delays[(size_t)k * C + cc]);
                            (a < P.w_hi && a + len > P.w_lo ? any_in : any_out) = true;
                        }
                        outside += any_in && any_out;
                    }
                    if (w1 == 0.0) {
                        if (s < 0 || s >= len) continue;
                        one_taps++;
                        volatile float term = y_of(s);
                        acc = acc + term;
                        continue;
                    }
                    if (len == 0 || s < 0 || s > len) continue;
                    two_taps++;
                    volatile double w0 = 1.0 - w1;
                    volatile float ceil_tap = 0.0f, term;
                    if (s >= 1) { volatile double y = (double)y_of(s - 1) * w1; ceil_tap = (float)y; }
                    if (s >= 1 && s < len) { volatile double y = (double)y_of(s) * w0; volatile double z = (double)ceil_tap + y; term = (float)z; }
                    else if (s >= 1) term = ceil_tap;
                    else { volatile double y = (double)y_of(0) * w0; term = (float)y; }
                    acc = acc + term;
                }
                want[o] = raw ? (float)acc : or0(acc);
            }
            {
                std::vector<unsigned char> packed;
                const size_t at = dusp::score_plan_pack(P, packed);
                void *image = nullptr;
                if (at != 0 || posix_memalign(&image, 32, std::max<size_t>(packed.size(), 1)) != 0) { bad++; free(tapmem); continue; }
                memcpy(image, packed.data(), packed.size());
                const dusp::ScoreRow *dv = (const dusp::ScoreRow *)image;
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                dusp::launch_score_space(gains ? g.data() : nullptr, taps, dv, bf, en, pinit, out, (uint32_t)C, NT, (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift,
                                         P.first_block, raw, nullptr);
                free(image);
            }
            free(tapmem);
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t p = 0; p < trow; p++) {
                if (want[p] != want[p]) ok &= out[p] != out[p];
                else ok &= memcmp(&out[p], &want[p], 4) == 0;
            }
            checked++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d N %d variant %d C %d layout %d first %d off %d shift %u\n", NT, N, variant, C, layout, first, off, P.block_shift); }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"windows\": %ld, \"two_taps\": %ld, \"one_taps\": %ld, \"outside\": %ld, \"whole_lists\": %ld}\n", checked, bad, doubled,
           windows, two_taps, one_taps, outside, whole_lists);
    return bad != 0;
}
