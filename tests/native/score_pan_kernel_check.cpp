// score_pan_kernel_check.cpp — the text of dusp_amd/csrc/score_pan_engine.hip compiled for the HOST (hip_host_stub/: lanes one after the
// other), fed score_rows_plan's plans over MONO rows and score_pan_coefficients' records, and held to a plain loop over the contract
// (dusp_amd/mix.py score_chain_rows_panned) on bit patterns of both channels.  The brute-force chain computes a term the way the
// reference's Pan unit does, ((f64(x) * (1 -+ f64(p))) / 2) * comp, every operation rounded by itself (volatile doubles); the kernel
// multiplies by comp / 2.  EVERY ROW IS A HEAP ALLOCATION OF ITS OWN, exactly its samples (none at all for an empty row), so under
// AddressSanitizer one float read outside a row — the unpredicated load of a lane an entry does not cover, a padded entry that names
// voice 0 — is reported; so is the coefficient array, an exact-size allocation on a 32-byte boundary.
// Covered: gains, init (a second buffer, in place), raw; no voices; lists of 1, 8, 9 and 37 voices; rows of 1, 3, 255, 256, 257 and 773
// samples mixed in one list; a first voice of length 0 (with a row, and with no row at all); onsets of both signs; windows of the
// timeline; plans whose block was doubled; pans -1, +1, 0, 1e-40, 0.3, 1.5, random ones, and pans far outside [-1, 1] whose
// compensation is subnormal or 0.  Then the identity the kernel rests on, (y / 2) * comp == y * (comp / 2) as DOUBLES, over the planted
// f32 values times the pans whose compensation is a normal double, and as the f32 it rounds to over all of them.
// Built with -fsanitize=address,undefined by tests/test_pan_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "windows": w, "zero_first": z, "identity": i, "identity_bad": b}.
#include "../../dusp_amd/csrc/score_pan_engine.hip"
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
static float term_of(float x, double side, double comp) {
    volatile double y = (double)x * side;
    volatile double h = y / 2.0;
    volatile double z = h * comp;
    return (float)z;
}
int main() {
    std::mt19937 rng(11);
    std::normal_distribution<float> nd;
    long checked = 0, bad = 0, doubled = 0, windows = 0, zero_first = 0, identity = 0, identity_bad = 0;
    const float fixed_pans[] = {-1.0f, 1.0f, 0.0f, 1e-40f, 0.3f, 1.5f};
    const float far_pans[] = {4200.0f, -4150.0f, 1e6f, -3e38f, 17.0f, -250.0f};
    const int totals[] = {1, 255, 256, 257, 1022, 2317};
    const int row_lens[] = {1, 3, 255, 256, 257, 773};
    for (int NT : totals) for (int N : {0, 1, 8, 9, 37})
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
            std::vector<float> pans(N);
            std::vector<double> comp(N);
            for (int k = 0; k < N; k++) {
                const int NV = row_lens[(k + rng() % 6) % 6];
                samples[k] = (uint32_t)NV;
                if (layout == 1) onsets[k] = (int64_t)(rng() % 6) * 256 - (int64_t)(k % 4) - (k % 5 == 0 ? NV : 0);
                else if (layout == 2) onsets[k] = NT / 2 + (int64_t)(rng() % 9) - 4;
                else onsets[k] = (int64_t)(rng() % (unsigned)(NT + 2 * NV + 8)) - NV - 4;  // both signs, every residue, past the end too
                const unsigned lk = rng() % 6;
                lens[k] = lk == 0 ? 0 : lk == 1 ? 1 : lk == 2 ? NV : (int64_t)(rng() % (unsigned)(NV + 1));
                if (layout == 1 && k % 3 == 0 && onsets[k] >= 0) lens[k] = std::min<int64_t>(NV, 256 - onsets[k] % 256);  // a span that ends on a block boundary
                const unsigned pk = rng() % 16;
                pans[k] = pk < 6 ? fixed_pans[pk] : pk == 6 ? far_pans[rng() % 6] : (float)(rng() % 20001) / 10000.f - 1.0f;
                comp[k] = comp_of(pans[k]);
            }
            bool with_lens = variant % 4 != 3;
            if (first == 1) { lens[0] = 0; with_lens = true; }
            if (first == 2) { samples[0] = 0; lens[0] = 0; }
            zero_first += first != 0;
            for (int k = 0; k < N; k++) {
                const size_t row = samples[k];
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
            for (int c = 0; c < 2; c++) for (int t = 0; t < NT; t++) {
                const size_t o = (size_t)c * NT + t;
                if (t < P.w_lo || t >= P.w_hi) { want[o] = ini[o]; continue; }  // (only with init == 2: out as it was)
                volatile float acc = init ? ini[o] : 0.0f;
                for (int k = 0; k < N; k++) {
                    const int64_t s = t - onsets[k], len = with_lens ? lens[k] : (int64_t)samples[k];
                    if (s < 0 || s >= len) continue;
                    volatile float x = rows[k][s];
                    if (gains) x = x * g[k];
                    volatile float term = term_of(x, c == 0 ? 1.0 - (double)pans[k] : 1.0 + (double)pans[k], comp[k]);
                    acc = acc + term;
                }
                want[o] = raw ? (float)acc : or0(acc);
            }
            if (P.w_hi > P.w_lo) {
                std::vector<unsigned char> packed;
                const size_t at = dusp::score_plan_pack(P, packed);
                void *image = nullptr, *coeff = nullptr;  // exact sizes, on the 32-byte boundaries the device's buffer gives them
                if (at != 0 || posix_memalign(&image, 32, std::max<size_t>(packed.size(), 1)) != 0) { bad++; continue; }
                if (posix_memalign(&coeff, 32, std::max<size_t>((size_t)N * sizeof(dusp::ScorePan), 1)) != 0) { bad++; free(image); continue; }
                memcpy(image, packed.data(), packed.size());
                for (int k = 0; k < N; k++) ((dusp::ScorePan *)coeff)[k] = dusp::score_pan_coefficients(pans[k], comp[k]);
                const dusp::ScoreRow *dv = (const dusp::ScoreRow *)image;
                const uint32_t *bf = (const uint32_t *)(dv + N), *en = bf + P.block_first.size();
                const bool any = P.n_entries() > 0;  // (as the ABI: no listed voice, no plan)
                dusp::launch_score_pan(gains ? g.data() : nullptr, any ? (const dusp::ScorePan *)coeff : nullptr, any ? dv : nullptr, any ? bf : nullptr, any ? en : nullptr, pinit,
                                       out, NT, (uint64_t)P.w_lo, (uint64_t)P.w_hi, P.block_shift, P.first_block, raw, nullptr);
                free(image);
                free(coeff);
            }
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t k = 64 + off + trow; k < out_s.size(); k++) ok &= memcmp(&out_s[k], &S, 4) == 0;
            for (size_t p = 0; p < trow; p++) {
                if (want[p] != want[p]) ok &= out[p] != out[p];
                else ok &= memcmp(&out[p], &want[p], 4) == 0;
            }
            checked++;
            if (!ok) { bad++; if (bad < 20) printf("MISMATCH NT %d N %d variant %d layout %d first %d off %d shift %u\n", NT, N, variant, layout, first, off, P.block_shift); }
        }
    }
    // (y / 2) * comp == y * (comp / 2): the same double where comp is a normal double, the same f32 everywhere
    {
        std::vector<float> xs = {0.0f, -0.0f, INFINITY, -INFINITY, FLT_MAX, -FLT_MAX, 1e-45f, -1e-40f, 5e-39f, 1.0f, -1.0f, NAN, FLT_MIN, 0.1f, -3.3e-7f, 2.5e38f};
        for (int j = 0; j < 4000; j++) {
            uint32_t b = (uint32_t)rng();
            float x;
            memcpy(&x, &b, 4);
            xs.push_back(x);
        }
        std::vector<float> ps(fixed_pans, fixed_pans + 6);
        ps.insert(ps.end(), far_pans, far_pans + 6);
        for (int j = 0; j < 200; j++) ps.push_back((float)(rng() % 20001) / 10000.f - 1.0f);
        ps.push_back(std::nextafter(1.0f, 0.0f));
        ps.push_back(-std::nextafter(1.0f, 0.0f));
        for (float p : ps) {
            const double comp = comp_of(p);
            const dusp::ScorePan c = dusp::score_pan_coefficients(p, comp);
            for (float x : xs) for (double side : {c.lm, c.rp}) {
                volatile double y = (double)x * side;
                volatile double a = y / 2.0;
                volatile double ref = a * comp, fast = y * c.ch;
                const double r = ref, f = fast;
                const float rf = (float)r, ff = (float)f;
                bool same = (rf != rf) ? (ff != ff) : memcmp(&rf, &ff, 4) == 0;
                if (std::fpclassify(comp) == FP_NORMAL) same &= (r != r) ? (f != f) : memcmp(&r, &f, 8) == 0;
                identity++;
                if (!same) { identity_bad++; if (identity_bad < 10) printf("IDENTITY x %a p %a: %a vs %a\n", x, p, r, f); }
            }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"windows\": %ld, \"zero_first\": %ld, \"identity\": %ld, \"identity_bad\": %ld}\n", checked, bad, doubled, windows,
           zero_first, identity, identity_bad);
    return bad != 0 || identity_bad != 0;
}
