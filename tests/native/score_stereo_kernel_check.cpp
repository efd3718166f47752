// score_stereo_kernel_check.cpp — the text of dusp_amd/csrc/score_stereo_engine.hip compiled for the HOST (hip_host_stub/: lanes one
// after the other), fed score_rows_plan's plans over rows of ONE AND TWO channels (row_channels, pans with NaN for "not placed") and held
// to a plain loop over the contract (dusp_amd/mix.py score_chain_rows_stereo) on bit patterns of both channels.  The brute-force chain
// computes a panned term the way the reference's Pan unit does, ((f64(x) * (1 -+ f64(p))) / 2) * comp, and the two taps of a voice with
// a fraction the way two_tap_terms does, every operation rounded by itself (volatile).  EVERY ROW IS A HEAP ALLOCATION OF ITS OWN, exactly
// channels x samples floats (none at all for an empty row), so under AddressSanitizer one float read outside a row — the unpredicated
// load of a lane an entry does not cover, a padded entry that names voice 0, row[len] or row[-1] of a voice with a fraction, the second
// channel of a row that has one — is reported; so are the coefficient and weight arrays, exact-size allocations on their boundaries.
// Covered: the three kinds mixed inside one batch, and lists all of one kind; gains, init (a second buffer, in place), raw; lists of 1,
// 8, 9 and 37 voices; rows of 1, 3, 255, 256, 257 and 773 samples mixed in one list; a first voice of length 0 (with a row, and with no
// row at all); onsets of both signs; spans that end inside a group, on a group boundary and on n_total; windows of the timeline; plans
// whose block was doubled; launches without any fraction (the FRAC = false kernel) and with fractions 0, 0.5, 2^-24 and 1 - 2^-53 mixed.
// Also: the record's stride says the kind, and a plan made WITHOUT row_channels is byte for byte the plan it was.
// Built with -fsanitize=address,undefined by tests/test_stereo_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "windows": w, "zero_first": z, "frac_launches": f, "mixed_batches": x, "plans_same": p}.
#include "../../dusp_amd/csrc/score_stereo_engine.hip"
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
// the reference's term: Pan.js:21-22
static float pan_term(float x, double side, double comp) {
    volatile double y = (double)x * side;
    volatile double h = y / 2.0;
    volatile double z = h * comp;
    return (float)z;
}
int main() {
    std::mt19937 rng(13);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, doubled = 0, windows = 0, zero_first = 0, frac_launches = 0, mixed_batches = 0, plans_same = 0;
    const float fixed_pans[] = {-1.0f, 1.0f, 0.0f, 1e-40f, 0.3f, 1.5f};
    const double fixed_fracs[] = {0.0, 0.5, 0x1p-24, 1.0 - 0x1p-53};
    const int totals[] = {1, 255, 256, 257, 1022, 2317};
    const int row_lens[] = {1, 3, 255, 256, 257, 773};
    for (int NT : totals) for (int N : {1, 8, 9, 37})
    for (int variant = 0; variant < 12; variant++) {
        const int gains = variant & 1, init = (variant >> 1) % 3, raw = variant >= 6;
        for (int layout : {0, 1, 2, 3}) for (int first : {0, 1, 2}) for (int kinds : {0, 1, 2, 3}) for (int with_fracs : {0, 1}) {
            // layout: 0 scattered onsets, 1 onsets at block boundaries and in front of 0, 2 bunched (empty blocks, a window), 3 a small plan budget
            // kinds: 0 the three in turn (mixed inside every batch), 1 all panned mono, 2 all plain mono, 3 all two-channel
            if ((kinds != 0 || first != 0) && (variant % 3 != (layout + kinds) % 3)) continue;  // (the full product only for the mixed lists)
            const int off = (int)(rng() % 4);
            std::vector<int64_t> onsets(N), lens(N);
            std::vector<uint32_t> samples(N), channels(N);
            std::vector<std::unique_ptr<float[]>> rows(N);
            std::vector<uint64_t> addr(N);
            std::vector<float> pans(N);
            std::vector<double> comp(N), fracs(N);
            for (int k = 0; k < N; k++) {
                const int NV = row_lens[(k + rng() % 6) % 6];
                samples[k] = (uint32_t)NV;
                const int kind = kinds == 0 ? (k + first) % 3 : kinds - 1;  // 0 panned mono, 1 plain mono, 2 two channels
                channels[k] = kind == 2 ? 2u : 1u;
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4;
                else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4;  // both signs, every residue, past the end too
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                if (layout == 1 && k % 3 == 0 && onsets[k] >= 0) lens[k] = std::min<int64_t>(NV, 256 - onsets[k] % 256);  // a span that ends on a group boundary
                if (layout == 0 && k % 7 == 3 && onsets[k] >= 0 && onsets[k] < NT) lens[k] = std::min<int64_t>(NV, NT - onsets[k]);  // ... and one that ends on n_total
                const unsigned pk = rng() % 12;
                pans[k] = kind != 0 ? NAN : pk < 6 ? fixed_pans[pk] : (float)(rng() % 20001) / 10000.f - 1.0f;
                comp[k] = kind != 0 ? NAN : comp_of(pans[k]);  // (an unplaced voice's compensation is nobody's)
                fracs[k] = with_fracs ? fixed_fracs[(k + rng() % 2) % 4] : 0.0;
            }
            bool with_lens = variant % 4 != 3;
            if (first == 1) { lens[0] = 0; with_lens = true; }
            if (first == 2) { samples[0] = 0; lens[0] = 0; }
            zero_first += first != 0;
            for (int k = 0; k < N; k++) {
                const size_t row = (size_t)samples[k] * channels[k];
                if (!row) continue;  // (no row at all: a NULL address, which nothing may read)
                rows[k].reset(new float[row]);  // exactly its size: one float past it is the sanitizer's
                addr[k] = (uint64_t)(uintptr_t)rows[k].get();
                for (size_t j = 0; j < row; j++) rows[k][j] = nd(rng) * std::pow(10.f, (float)(k % 7) - 3);
                for (size_t j = (size_t)k % 29; j < row; j += 29) rows[k][j] = (j & 1) ? -0.0f : (j % 3 ? INFINITY : (j % 5 ? 1e-41f : FLT_MAX));
                if (k == N / 2 && row > 3) rows[k][3] = NAN;
                if (row > 5) rows[k][5] = 5e-39f;
            }
            const size_t trow = (size_t)2 * NT;
            std::vector<float> g(N), ini(trow), out_s(trow + 128 + off);
            for (auto &x : g) x = 0.05f + 1.9f * (rng() % 1000) / 1000.f;
            if (N > 2) g[1] = -g[1];
            for (size_t k = 0; k < trow; k++) ini[k] = (k % 13 == 0) ? -0.0f : (k % 101 == 7) ? INFINITY : (k % 211 == 9) ? NAN : 30 * nd(rng);
            const float S = -12345.678f;
            for (auto &x : out_s) x = S;
            float *out = out_s.data() + 64 + off;
            dusp::ScoreRowsPlan P;
            const bool whole = layout != 2 || init != 2;  // a window only in place: outside it nothing is written
            const size_t budget = layout == 3 ? 600 : dusp::kScorePlanBytes;
            const int64_t rc = dusp::score_rows_plan(onsets.data(), with_lens ? lens.data() : nullptr, samples.data(), addr.data(), (size_t)N, NT, whole, budget, P,
                                                     {with_fracs ? fracs.data() : nullptr, nullptr, 0, channels.data(), pans.data()});
            if (rc != -1) { bad++; continue; }
            {   // the same call without row_channels: the plan it always was, but for the strides of the mono rows
                dusp::ScoreRowsPlan Q;
                dusp::score_rows_plan(onsets.data(), with_lens ? lens.data() : nullptr, samples.data(), addr.data(), (size_t)N, NT, whole, budget, Q, {with_fracs ? fracs.data() : nullptr});
                bool same = Q.block_first == P.block_first && Q.entries == P.entries && Q.w_lo == P.w_lo && Q.w_hi == P.w_hi && Q.block_shift == P.block_shift && Q.voices.size() == P.voices.size();
                for (int k = 0; same && k < N; k++) {
                    const dusp::ScoreRow &a = P.voices[k], &b = Q.voices[k];
                    same = a.onset == b.onset && a.lo == b.lo && a.hi == b.hi && a.row == b.row && a.pad == b.pad;
                    if (a.hi > a.lo) {
                        same &= b.stride == samples[k];
                        same &= a.stride == (channels[k] == 2 ? samples[k] : std::isnan(pans[k]) ? dusp::kScoreStrideMono : dusp::kScoreStridePanned);
                    }
                }
                plans_same += same;
                if (!same) bad++;
            }
            doubled += P.block_shift > dusp::kScoreGroupShift;
            windows += !whole && P.w_hi > P.w_lo && (P.w_lo > 0 || P.w_hi < NT);
            bool any_frac = false;
            for (int k = 0; k < N; k++) any_frac |= P.voices[k].hi > P.voices[k].lo && P.voices[k].pad != 0;
            frac_launches += any_frac;
            for (size_t b = 0; b + 1 < P.block_first.size(); b++)
                for (uint32_t e = P.block_first[b]; e + 2 < P.block_first[b + 1] && e + 2 < P.block_first[b] + 8; e++) {
                    const uint32_t s0 = P.voices[P.entries[e]].stride, s1 = P.voices[P.entries[e + 1]].stride, s2 = P.voices[P.entries[e + 2]].stride;
                    if ((s0 == dusp::kScoreStrideMono) + (s1 == dusp::kScoreStrideMono) + (s2 == dusp::kScoreStrideMono) == 1 &&
                        (s0 == dusp::kScoreStridePanned) + (s1 == dusp::kScoreStridePanned) + (s2 == dusp::kScoreStridePanned) == 1) { mixed_batches++; break; }
                }
            const float *pinit = nullptr;
            if (init == 1) pinit = ini.data();
            if (init == 2) { memcpy(out, ini.data(), trow * 4); pinit = out; }
            std::vector<float> want(trow);  // the contract
            for (int c = 0; c < 2; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) { want[o] = ini[o]; continue; }  // (only with init == 2: out as it was)
                volatile float acc = init ? ini[o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const int64_t s = t - onsets[k], len = with_lens ? lens[k] : (int64_t)samples[k];
                    const double fr = fracs[k];
                    if (len == 0 || s < 0 || s >= len + (fr != 0.0 ? 1 : 0)) continue;
                    auto placed = [&](int64_t at) -> float {  // the voice's sample after gain and placement, channel c
                        volatile float x = rows[k][(channels[k] == 2 ? (size_t)c * samples[k] : 0) + (size_t)at];
                        if (gains) x = x * g[k];
                        if (channels[k] == 1 && !std::isnan(pans[k])) return pan_term(x, c == 0 ? 1.0 - (double)pans[k] : 1.0 + (double)pans[k], comp[k]);
                        return x;
                    };
                    volatile float term;
                    if (fr == 0.0) {
                        term = placed(s);
                    } else {
                        volatile double w1 = fr, w0 = 1.0 - w1;
                        volatile float ceil_tap = 0.0f;
                        if (s >= 1) { volatile double cd = (double)placed(s - 1) * w1; ceil_tap = (float)cd; }
                        if (s == len) term = ceil_tap;
                        else {
                            volatile double floor_tap = (double)placed(s) * w0;
                            if (s == 0) term = (float)floor_tap;
                            else { volatile double both = (double)ceil_tap + floor_tap; term = (float)both; }
                        }
                    }
                    acc = acc + term;
                }
                want[o] = raw ? (float)acc : or0(acc);
            }
            if (P.w_hi > P.w_lo && P.n_entries() > 0) {  // (as the ABI: no listed voice, no plan, and the launch is the pan kernel's)
                std::vector<unsigned char> packed;
                const size_t at = dusp::score_plan_pack(P, packed);
                void *image = nullptr, *coeff = nullptr, *weights = nullptr;  // exact sizes, on the boundaries the device's buffer gives them
                if (at != 0 || posix_memalign(&image, 32, std::max<size_t>(packed.size(), 1)) != 0) { bad++; continue; }
                if (posix_memalign(&coeff, 32, (size_t)N * sizeof(dusp::ScorePan)) != 0) { bad++; free(image); continue; }
                if (posix_memalign(&weights, 16, (size_t)N * sizeof(dusp::ScoreFrac)) != 0) { bad++; free(image); free(coeff); continue; }
                memcpy(image, packed.data(), packed.size());
                for (int k = 0; k < N; k++) {
                    ((dusp::ScorePan *)coeff)[k] = std::isnan(pans[k]) ? dusp::ScorePan{0.0, 0.0, 0.0, 0.0} : dusp::score_pan_coefficients(pans[k], comp[k]);
                    ((dusp::ScoreFrac *)weights)[k] = dusp::score_frac_weights(fracs[k]);
                }
                const dusp::ScoreRow *dv = (const dusp::ScoreRow *)image;
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                dusp::launch_score_stereo(gains ? g.data() : nullptr, (const dusp::ScorePan *)coeff, any_frac ? (const dusp::ScoreFrac *)weights : nullptr, dv, bf, en, pinit, out, NT,
                                          (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
                free(image);
                free(coeff);
                free(weights);
            } else if (P.w_hi > P.w_lo) {  // (no voice reaches the window: init -> out alone, which is not this kernel's)
                for (size_t o = 0; o < trow; o++) out[o] = want[o];
            }
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            if (P.w_hi > P.w_lo || init == 2)
                for (size_t p = 0; p < trow; p++) {
                    if (want[p] != want[p]) ok &= out[p] != out[p];
                    else ok &= memcmp(&out[p], &want[p], 4) == 0;
                }
            checked++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d N %d variant %d layout %d first %d kinds %d fracs %d off %d shift %u\n", NT, N, variant, layout, first, kinds, with_fracs, off, P.block_shift); }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"windows\": %ld, \"zero_first\": %ld, \"frac_launches\": %ld, \"mixed_batches\": %ld, \"plans_same\": %ld}\n", checked, bad,
           doubled, windows, zero_first, frac_launches, mixed_batches, plans_same);
    return bad != 0;
}
