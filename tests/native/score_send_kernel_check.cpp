// score_send_kernel_check.cpp — the text of dusp_amd/csrc/score_send_engine.hip compiled for the HOST (hip_host_stub/: lanes one after
// the other), fed score_rows_plan's plans and a parallel array of ScoreSend, and held on bit patterns (a) to a plain loop over the
// contract (dusp_amd/mix.py score_chain_sends): the dry chain, and for every bus f32(send + f32(term * level)) over EVERY covering
// voice, a level of 0 included; (b) in its dry output to dusp_score_rows_kernel / dusp_score_pan_kernel over the same plan, whose text is
// compiled in beside it.  EVERY ROW IS A HEAP ALLOCATION OF ITS OWN, exactly its samples (none at all for an empty row), so under
// AddressSanitizer one float read outside a row is reported; so are the plan's image, the levels and the pan coefficients, exact-size
// allocations on the boundaries the device gives them.
// Covered: B = 1 .. 4; rows of 1 and of 2 channels, and panned mono rows; with and without gains; init and send_init (none, a second
// buffer, in place); raw; a launch without voices; lists of 1, 8, 9 and 37 voices; rows of 1, 3, 255, 256, 257 and 773 samples in one
// list; voice 0 of length 0, with a row and with none (unlisted: the padding's zeros name it); windows of the timeline that begin and
// end inside a group; plans whose block was doubled; levels 0, -0, 1, negative, tiny and huge over rows that hold NaN, Inf, -0 and
// subnormals.  Then dusp_score_return_kernel against a plain loop at 1, 3, 4, 5 and 4634 floats, B = 0 .. 4, in place and out of
// place, raw and not, on buffers that are 16-byte aligned (four floats a lane) and on ones that are not (one a lane).
// Built with -fsanitize=address,undefined by tests/test_sends_host.py.
// Prints {"cases": n, "bad": m, "dry_bad": d, "doubled": d, "windows": w, "zero_first": z, "returns": r}.
#include "../../dusp_amd/csrc/score_rows_engine.hip"
#include "../../dusp_amd/csrc/score_pan_engine.hip"
#include "../../dusp_amd/csrc/score_send_engine.hip"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
static float or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }
static double comp_of(float p) { return std::pow(10.0, ((1.0 - std::fabs((double)p)) * 1.5) / 20.0); }
static float pan_term(float x, double side, double comp) {  // the reference's term: Pan.js:21-22
    volatile double y = (double)x * side;
    volatile double h = y / 2.0;
    volatile double z = h * comp;
    return (float)z;
}
static bool same_bits(const float *a, const float *b, size_t n) {
    bool ok = true;
    for (size_t p = 0; p < n; p++) ok &= (b[p] != b[p]) ? (a[p] != a[p]) : memcmp(&a[p], &b[p], 4) == 0;
    return ok;
}
int main() {
    std::mt19937 rng(15);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, dry_bad = 0, doubled = 0, windows = 0, zero_first = 0, returns = 0;
    const float fixed_levels[] = {0.0f, -0.0f, 1.0f, -0.75f, 1e-30f, 3e20f, 0.6f};
    const int totals[] = {1, 255, 257, 1022, 2317};
    const int row_lens[] = {1, 3, 255, 256, 257, 773};
    for (int NT : totals) for (int N : {0, 1, 8, 9, 37})
    for (int B = 1; B <= 4; B++) for (int mode : {0, 1, 2})  // mode: 0 rows of one channel, 1 rows of two, 2 panned mono rows
    for (int variant = 0; variant < 12; variant++) {
        const int gains = variant & 1, init = (variant >> 1) % 3, raw = variant >= 6;
        const bool pan = mode == 2;
        const int RC = mode == 1 ? 2 : 1, C = mode == 0 ? 1 : 2;  // a row's channels, the timeline's
        for (int layout : {0, 1, 2, 3}) for (int first : {0, 1, 2}) {
            if (N == 0 && (layout || first)) continue;
            if ((layout + first + variant + B + mode) % 3 != 0 && N != 0) continue;  // (a third of the grid: every axis still meets every other)
            const int off = (int)(rng() % 4);
            std::vector<int64_t> onsets(N), lens(N);
            std::vector<uint32_t> samples(N);
            std::vector<std::unique_ptr<float[]>> rows(N);
            std::vector<uint64_t> addr(N);
            std::vector<float> pans(N);
            std::vector<double> comp(N);
            for (int k = 0; k < N; k++) {
                const int NV = row_lens[(k + rng() % 6) % 6];
                samples[k] = (uint32_t)NV;
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4;
                else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4;
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                if (layout == 1 && k % 3 == 0 && onsets[k] >= 0) lens[k] = std::min<int64_t>(NV, 256 - onsets[k] % 256);
                pans[k] = (float)(rng() % 20001) / 10000.f - 1.0f;
                comp[k] = comp_of(pans[k]);
            }
            bool with_lens = variant % 4 != 3;
            if (first == 1) { lens[0] = 0; with_lens = true; }
            if (first == 2) { samples[0] = 0; lens[0] = 0; }
            zero_first += first != 0;
            for (int k = 0; k < N; k++) {
                const size_t row = (size_t)RC * samples[k];
                if (!row) continue;
                rows[k].reset(new float[row]);  // exactly its size: one float past it is the sanitizer's
                addr[k] = (uint64_t)(uintptr_t)rows[k].get();
                for (size_t j = 0; j < row; j++) rows[k][j] = nd(rng) * std::pow(10.f, (float)(k % 7) - 3);
                for (size_t j = (size_t)k % 29; j < row; j += 29) rows[k][j] = (j & 1) ? -0.0f : (j % 3 ? INFINITY : (j % 5 ? 1e-41f : FLT_MAX));
                if (k == N / 2 && row > 3) rows[k][3] = NAN;
                if (row > 5) rows[k][5] = 5e-39f;
            }
            const size_t trow = (size_t)C * NT, srow = (size_t)B * trow;
            std::vector<float> g(N), ini(trow), sini(srow), out_s(trow + 128 + off), snd_s(srow + 128 + off), base_s(trow);
            for (auto &x : g) x = 0.05f + 1.9f * (rng() % 1000) / 1000.f;
            if (N > 2) g[1] = -g[1];
            for (size_t k = 0; k < trow; k++) ini[k] = (k % 13 == 0) ? -0.0f : 30 * nd(rng);
            for (size_t k = 0; k < srow; k++) sini[k] = (k % 11 == 0) ? -0.0f : 20 * nd(rng);
            void *levels_v = nullptr;
            if (posix_memalign(&levels_v, 16, std::max<size_t>((size_t)N * sizeof(dusp::ScoreSend), 1)) != 0) { bad++; continue; }
            dusp::ScoreSend *levels = (dusp::ScoreSend *)levels_v;
            for (int k = 0; k < N; k++)
                for (int b = 0; b < 4; b++) {
                    const unsigned lk = rng() % 12;
                    levels[k].level[b] = b >= B ? 0.0f : lk < 7 ? fixed_levels[lk] : (float)(rng() % 2001) / 1000.f - 1.0f;
                }
            const float S = -12345.678f;
            for (auto &x : out_s) x = S;
            for (auto &x : snd_s) x = S;
            float *out = out_s.data() + 64 + off, *snd = snd_s.data() + 64 + off;
            dusp::ScoreRowsPlan P;
            const bool whole = layout != 2 || init != 2;  // a window only in place: outside it nothing is written
            const int64_t rc = dusp::score_rows_plan(onsets.data(), with_lens ? lens.data() : nullptr, samples.data(), addr.data(), (size_t)N, NT, whole,
                                                     layout == 3 ? 600 : dusp::kScorePlanBytes, P, {});
            if (rc != -1) { bad++; free(levels_v); continue; }
            doubled += P.block_shift > dusp::kScoreGroupShift;
            windows += !whole && P.w_hi > P.w_lo && (P.w_lo > 0 || P.w_hi < NT);
            const float *pinit = nullptr, *psinit = nullptr;
            if (init == 1) { pinit = ini.data(); psinit = sini.data(); }
            if (init == 2) { memcpy(out, ini.data(), trow * 4); pinit = out; memcpy(snd, sini.data(), srow * 4); psinit = snd; }
            std::vector<float> want(trow), swant(srow);  // the contract
            for (int c = 0; c < C; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) {  // (only with init == 2: both as they were)
                    want[o] = ini[o];
                    for (int b = 0; b < B; b++) swant[(size_t)b * trow + o] = sini[(size_t)b * trow + o];
                    continue;
                }
                volatile float acc = init ? ini[o] : 0.0f;
                volatile float sacc[4];
                for (int b = 0; b < B; b++) sacc[b] = init ? sini[(size_t)b * trow + o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const int64_t s = t - onsets[k], len = with_lens ? lens[k] : (int64_t)samples[k];
                    if (s < 0 || s >= len) continue;
                    volatile float x = rows[k][pan ? s : (int64_t)c * samples[k] + s];
                    if (gains) x = x * g[k];
                    volatile float term = pan ? pan_term(x, c == 0 ? 1.0 - (double)pans[k] : 1.0 + (double)pans[k], comp[k]) : (float)x;
                    acc = acc + term;
                    for (int b = 0; b < B; b++) {
                        volatile float part = term * levels[k].level[b];
                        sacc[b] = sacc[b] + part;
                    }
                }
                want[o] = raw ? (float)acc : or0(acc);
                for (int b = 0; b < B; b++) swant[(size_t)b * trow + o] = sacc[b];
            }
            bool dry_ok = true;
            if (P.w_hi > P.w_lo) {
                std::vector<unsigned char> packed;
                const size_t at = dusp::score_plan_pack(P, packed);
                void *image = nullptr, *coeff = nullptr;
                if (at != 0 || posix_memalign(&image, 32, std::max<size_t>(packed.size(), 1)) != 0) { bad++; free(levels_v); continue; }
                if (posix_memalign(&coeff, 32, std::max<size_t>((size_t)N * sizeof(dusp::ScorePan), 1)) != 0) { bad++; free(image); free(levels_v); continue; }
                memcpy(image, packed.data(), packed.size());
                for (int k = 0; k < N; k++) ((dusp::ScorePan *)coeff)[k] = dusp::score_pan_coefficients(pans[k], comp[k]);
                const dusp::ScoreRow *dv = (const dusp::ScoreRow *)image;
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                const bool any = P.n_entries() > 0;  // (as the ABI: no listed voice, no plan)
                const dusp::ScorePan *dp = any && pan ? (const dusp::ScorePan *)coeff : nullptr;
                // the dry chain by the kernels that stand: out of place from the same start
                const float *binit = init ? ini.data() : nullptr;
                if (init == 2) memcpy(base_s.data(), ini.data(), trow * 4);  // (a window: outside it as it was)
                if (pan)
                    dusp::launch_score_pan(gains ? g.data() : nullptr, dp, any ? dv : nullptr, any ? bf : nullptr, any ? en : nullptr, binit, base_s.data(), NT, (uint64_t)P.w_lo,
                                           (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
                else
                    dusp::launch_score_rows(gains ? g.data() : nullptr, any ? dv : nullptr, any ? bf : nullptr, any ? en : nullptr, binit, base_s.data(), (uint32_t)C, NT,
                                            (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
                const hipError_t err = dusp::launch_score_send(gains ? g.data() : nullptr, any ? levels : nullptr, dp, any ? dv : nullptr, any ? bf : nullptr, any ? en : nullptr, pinit, out,
                                                               psinit, snd, (uint32_t)B, (uint32_t)C, NT, (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, pan,
                                                               nullptr);
                if (err != hipSuccess) bad++;
                for (int c = 0; c < C; c++)
                    for (int64_t t = P.w_lo; t < P.w_hi; t++) dry_ok &= memcmp(&out[(size_t)c * NT + t], &base_s[(size_t)c * NT + t], 4) == 0;  // (bit for bit, NaNs too: one text)
                free(image);
                free(coeff);
            } else if (init != 2) {
                free(levels_v);
                continue;  // (nothing launched, nothing written)
            }
            free(levels_v);
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0 && memcmp(&snd_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + srow; k < snd_s.size(); k++) ok &= memcmp(&snd_s[k], &S, 4) == 0;
            ok &= same_bits(out, want.data(), trow) && same_bits(snd, swant.data(), srow);
            checked++;
            if (!dry_ok) dry_bad++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d N %d B %d mode %d variant %d layout %d first %d off %d shift %u\n", NT, N, B, mode, variant, layout, first, off, P.block_shift); }
        }
    }
    // the return of the buses
    for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)4634})
        for (int B = 0; B <= 4; B++) for (int raw : {0, 1}) for (int in_place : {0, 1}) for (int aligned : {0, 1}) {
            void *mem[6];
            float *buf[6];  // dry, four wets, out: exactly n floats each behind the offset
            bool got = true;
            for (int j = 0; j < 6; j++) {
                const size_t skip = aligned ? 0 : 1 + j % 3;  // (exactly n floats behind it: one past them is the sanitizer's)
                got &= posix_memalign(&mem[j], 16, (n + skip) * 4) == 0;
                buf[j] = (float *)mem[j] + skip;
            }
            if (!got) { bad++; continue; }
            for (int j = 0; j < 6; j++)
                for (size_t p = 0; p < n; p++) buf[j][p] = p % 17 == 3 ? -0.0f : p % 19 == 4 ? NAN : p % 23 == 5 ? (j & 1 ? INFINITY : -INFINITY) : nd(rng);
            if (n > 2) { buf[0][2] = 1.0f; buf[1][2] = -1.0f; }  // (a sum that is -0 or +0 by the order)
            std::vector<float> want(n);
            for (size_t p = 0; p < n; p++) {
                volatile float a = buf[0][p];
                for (int b = 0; b < B; b++) a = a + buf[1 + b][p];
                want[p] = raw ? (float)a : or0(a);
            }
            float *out = in_place ? buf[0] : buf[5];
            const float *wets[4] = {buf[1], buf[2], buf[3], buf[4]};
            const hipError_t err = dusp::launch_score_return(buf[0], wets, (uint32_t)B, out, nullptr, nullptr, n, raw, nullptr);
            const bool ok = err == hipSuccess && same_bits(out, want.data(), n);
            returns++;
            if (!ok) { bad++; if (bad < 20) printf("RETURN MISMATCH n %zu B %d raw %d in_place %d aligned %d\n", n, B, raw, in_place, aligned); }
            for (int j = 0; j < 6; j++) free(mem[j]);
        }
    printf("{\"cases\": %ld, \"bad\": %ld, \"dry_bad\": %ld, \"doubled\": %ld, \"windows\": %ld, \"zero_first\": %ld, \"returns\": %ld}\n", checked, bad, dry_bad, doubled, windows,
           zero_first, returns);
    return bad != 0 || dry_bad != 0;
}
