// score_frac_kernel_check.cpp — the text of dusp_amd/csrc/score_frac_engine.hip compiled for the HOST (hip_host_stub/: lanes one after
// the other), fed score_rows_plan's plans WITH FRACTIONS, score_frac_weights' and score_pan_coefficients' records, and held to a plain
// loop per timeline sample over the contract (dusp_amd/mix.py score_chain_rows / score_chain_rows_panned with fracs) on bit patterns.
// The brute-force chain forms the two taps the way the reference's Delay does (Delay.js:36-38) — the ceil tap of sample s - 1 rounded to
// f32 alone in its slot, the floor tap of sample s added to it in f64, every operation rounded by itself (volatile) — and a panned
// sample the way the reference's Pan does, ((f64(x) * (1 -+ f64(p))) / 2) * comp.  EVERY ROW IS A HEAP ALLOCATION OF ITS OWN, exactly
// channels x samples floats (none at all for an empty row), so under AddressSanitizer a read of row[len] (the tail tap's lane must not
// load x[len]) or of row[-1] (the first lane must not load x[-1]) is reported; so are the weight and coefficient arrays, exact-size
// allocations on their 16- and 32-byte boundaries.
// Covered: the four instantiations (gains x pan); init (a second buffer, in place), raw; lists of 1, 8, 9 and 37 voices; voices with
// and without a fraction mixed in one list, and lists without any; fractions 0.5, 2^-24, 1 - 2^-53, the smallest subnormal double and
// random ones; rows of 1, 3, 255, 256, 257 and 773 samples of one and two channels; len = 1; onset = -1, onset = -len (the tail tap
// alone), onset + len = n_total (the tail tap clipped off), onset = n_total - 1; spans that end inside a group, on a group boundary and
// on n_total; a first voice of length 0 (with a row, and with none); output bases 0 .. 3 floats past the buffer's start; windows of the
// timeline; plans whose block was doubled.  Built with -fsanitize=address,undefined by tests/test_frac_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "windows": w, "two_taps": t, "tail_only": o, "whole_lists": l}.
#include "../../dusp_amd/csrc/score_frac_engine.hip"
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
// the reference's Pan term: Pan.js:21-22
static float pan_of(float x, double side, double comp) {
    volatile double y = (double)x * side;
    volatile double h = y / 2.0;
    volatile double z = h * comp;
    return (float)z;
}
int main() {
    std::mt19937 rng(17);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, doubled = 0, windows = 0, two_taps = 0, tail_only = 0, whole_lists = 0;
    const float fixed_pans[] = {-1.0f, 1.0f, 0.0f, 1e-40f, 0.3f, 1.5f};
    const double edge_fracs[] = {0.5, 0x1p-24, 1.0 - 0x1p-53, 0x1p-1074, 0.3};
    const int totals[] = {1, 255, 256, 257, 1022, 1301};
    const int row_lens[] = {1, 3, 255, 256, 257, 773};
    for (int NT : totals) for (int N : {1, 8, 9, 37})
    for (int variant = 0; variant < 12; variant++) for (int pan = 0; pan < 2; pan++) {
        const int gains = variant & 1, init = (variant >> 1) % 3, raw = variant >= 6;
        for (int layout : {0, 1, 2, 3, 4}) for (int first : {0, 1, 2}) {  // first: 0 any voice 0; 1 voice 0 has a row but length 0; 2 voice 0 has no row at all
            // layout: 0 scattered onsets, 1 onsets at block boundaries and in front of 0, 2 bunched (empty blocks, a window), 3 a small plan budget,
            //         4 the edge placements in turn (onset -1, -len, n_total - len, n_total - 1, a tail tap on a group boundary)
            if (first && (N == 1 || (layout != 0 && layout != 3 && layout != 4))) continue;
            const int C = pan ? 1 : 1 + (variant / 3) % 2;  // channels of a row
            const int CT = pan ? 2 : C;                     // channels of the timeline
            const int off = (int)(rng() % 4);
            const int frac_mode = (int)(rng() % 8);         // 0: no fraction anywhere (yet the kernel is launched); 1: every voice has one; else mixed
            std::vector<int64_t> onsets(N), lens(N);
            std::vector<uint32_t> samples(N);
            std::vector<std::unique_ptr<float[]>> rows(N);
            std::vector<uint64_t> addr(N);
            std::vector<float> pans(N);
            std::vector<double> comp(N), fracs(N);
            bool with_lens = variant % 4 != 3;
            for (int k = 0; k < N; k++) {
                const int NV = row_lens[(k + rng() % 6) % 6];
                samples[k] = (uint32_t)NV;
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                const int64_t len = with_lens ? lens[k] : NV;
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4;
                else if (layout == 4) {
                    const int ek = (k + variant) % 6;
                    onsets[k] = ek == 0 ? -1 : ek == 1 ? -len : ek == 2 ? NT - len : ek == 3 ? NT - 1 : ek == 4 ? (int64_t)(1 + rng() % 4) * 256 - len : 256 - len - 1;
                } else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4;  // both signs, every residue, past the end too
                if (layout == 1 && k % 3 == 0 && onsets[k] >= 0 && with_lens) lens[k] = std::min<int64_t>(NV, 256 - onsets[k] % 256);  // a span that ends on a block boundary
                const unsigned pk = rng() % 12;
                pans[k] = pk < 6 ? fixed_pans[pk] : (float)(rng() % 20001) / 10000.f - 1.0f;
                comp[k] = comp_of(pans[k]);
                const unsigned fk = rng() % 8;
                fracs[k] = frac_mode == 0 ? 0.0 : (frac_mode != 1 && fk < 3) ? 0.0 : fk < 5 ? edge_fracs[rng() % 5] : (double)(1 + rng() % 1023) / 1024.0;
            }
            if (first == 1) { lens[0] = 0; with_lens = true; }
            if (first == 2) { samples[0] = 0; lens[0] = 0; }
            for (int k = 0; k < N; k++) {
                const size_t row = (size_t)C * samples[k];
                if (!row) continue;  // (no row at all: a NULL address, which nothing may read)
                rows[k].reset(new float[row]);  // exactly its size: one float past it, or in front of it, is the sanitizer's
                addr[k] = (uint64_t)(uintptr_t)rows[k].get();
                for (size_t j = 0; j < row; j++) rows[k][j] = nd(rng) * std::pow(10.f, (float)(k % 7) - 3);
                for (size_t j = (size_t)k % 29; j < row; j += 29) rows[k][j] = (j & 1) ? -0.0f : (j % 3 ? INFINITY : (j % 5 ? 1e-41f : FLT_MAX));
                if (k == N / 2 && row > 3) rows[k][3] = NAN;
                if (row > 5) rows[k][5] = 5e-39f;
            }
            const size_t trow = (size_t)CT * NT;
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
                                                     layout == 3 ? 600 : dusp::kScorePlanBytes, P, {fracs.data()});
            if (rc != -1) { bad++; continue; }
            if (P.n_entries() == 0) continue;  // (no listed voice: the launch is the existing kernels')
            doubled += P.block_shift > dusp::kScoreGroupShift;
            windows += !whole && (P.w_lo > 0 || P.w_hi < NT);
            whole_lists += frac_mode == 0;
            const float *pinit = nullptr;
            if (init == 1) pinit = ini.data();
            if (init == 2) { memcpy(out, ini.data(), trow * 4); pinit = out; }
            std::vector<float> want(trow);  // the contract, sample by sample
            for (int c = 0; c < CT; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) { want[o] = ini[o]; continue; }  // (only with init == 2: out as it was)
                volatile float acc = init ? ini[o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const int64_t s = t - onsets[k], len = with_lens ? lens[k] : (int64_t)samples[k];
                    auto x_of = [&](int64_t at) {  // the voice's sample after gain (and pan); at is within [0, len)
                        volatile float x = rows[k][(pan ? 0 : (size_t)c * samples[k]) + (size_t)at];
                        if (gains) x = x * g[k];
                        if (pan) x = pan_of(x, c == 0 ? 1.0 - (double)pans[k] : 1.0 + (double)pans[k], comp[k]);
                        return (float)x;
                    };
                    if (fracs[k] == 0.0) {
                        if (s < 0 || s >= len) continue;
                        volatile float term = x_of(s);
                        acc = acc + term;
                        continue;
                    }
                    if (len == 0 || s < 0 || s > len) continue;
                    two_taps += c == 0;
                    tail_only += c == 0 && onsets[k] == -len;
                    const double w1 = fracs[k];
                    volatile double w0 = 1.0 - w1;
                    volatile float ceil_tap = 0.0f, term;
                    if (s >= 1) { volatile double y = (double)x_of(s - 1) * w1; ceil_tap = (float)y; }
                    if (s >= 1 && s < len) { volatile double y = (double)x_of(s) * w0; volatile double z = (double)ceil_tap + y; term = (float)z; }
                    else if (s >= 1) term = ceil_tap;
                    else { volatile double y = (double)x_of(0) * w0; term = (float)y; }
                    acc = acc + term;
                }
                want[o] = raw ? (float)acc : or0(acc);
            }
            {
                std::vector<unsigned char> packed;
                const size_t at = dusp::score_plan_pack(P, packed);
                void *image = nullptr, *coeff = nullptr, *weights = nullptr;  // exact sizes, on the boundaries the device's buffer gives them
                if (at != 0 || posix_memalign(&image, 32, std::max<size_t>(packed.size(), 1)) != 0) { bad++; continue; }
                if (posix_memalign(&coeff, 32, (size_t)N * sizeof(dusp::ScorePan)) != 0) { bad++; free(image); continue; }
                if (posix_memalign(&weights, 16, (size_t)N * sizeof(dusp::ScoreFrac)) != 0) { bad++; free(image); free(coeff); continue; }
                memcpy(image, packed.data(), packed.size());
                for (int k = 0; k < N; k++) ((dusp::ScorePan *)coeff)[k] = dusp::score_pan_coefficients(pans[k], comp[k]);
                for (int k = 0; k < N; k++) ((dusp::ScoreFrac *)weights)[k] = dusp::score_frac_weights(fracs[k]);
                const dusp::ScoreRow *dv = (const dusp::ScoreRow *)image;
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                dusp::launch_score_frac(gains ? g.data() : nullptr, pan ? (const dusp::ScorePan *)coeff : nullptr, (const dusp::ScoreFrac *)weights, dv, bf, en, pinit, out,
                                        (uint32_t)C, NT, (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
                free(image);
                free(coeff);
                free(weights);
            }
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t p = 0; p < trow; p++) {
                if (want[p] != want[p]) ok &= out[p] != out[p];
                else ok &= memcmp(&out[p], &want[p], 4) == 0;
            }
            checked++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d N %d variant %d pan %d layout %d first %d off %d shift %u\n", NT, N, variant, pan, layout, first, off, P.block_shift); }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"windows\": %ld, \"two_taps\": %ld, \"tail_only\": %ld, \"whole_lists\": %ld}\n", checked, bad, doubled, windows,
           two_taps, tail_only, whole_lists);
    return bad != 0;
}
