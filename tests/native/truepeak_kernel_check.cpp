// truepeak_kernel_check.cpp — the text of dusp_amd/csrc/truepeak_engine.hip compiled for the HOST (hip_host_stub_lds/: the lanes of a
// workgroup as threads, LDS as statics, __syncthreads a barrier; the wave's shuffle and the 64-bit atomicMax that stub lacks are defined
// here) and held BIT FOR BIT to the contract's loop (dusp_amd/mix.py true_peak), written out below with every product and sum rounded by
// itself; and truepeak_plan.hpp's grid rule and gain on the way.
// EVERY BUFFER IS A HEAP ALLOCATION OF EXACTLY ITS SIZE — the signals, the words — so under AddressSanitizer one element read or
// written outside a buffer is reported.
// Covered: F = 4 (44100 Hz), 2 (96000 Hz) and 1 (192000 Hz); per_lane 1 (few rows on 256 CUs) and — one row of about four tiles on a
// device of ONE CU — 2, 4 and 8; n = 1, 5, W - 1, W, W + 1, W + K - 2, W + K - 1 and 2 W + 3; 1 x 1, 1 x 2 (odd n: the second row unaligned)
// and 3 x 2; noise, the largest value last (the peak in the tail), the largest value first, a planted NaN and a planted Inf (that row
// NaN, the others as the loop's); two runs give equal words.
// Built with -fsanitize=address,undefined by tests/test_loudness_host.py.  Prints {"cases": n, "bad": m, "groups": g, "per_lane": mask}.
#include <hip/hip_runtime.h>  // (hip_host_stub_lds: included first, so that the kernel's own include is this one)

#include <cstring>
#include <mutex>
// ---- what the kernel needs beyond that stub ----
static inline long long __double_as_longlong(double v) {
    long long b;
    memcpy(&b, &v, 8);
    return b;
}
// the wave's xor shuffle: every lane of the workgroup parks its value, a barrier, reads its partner's (within its wave of 64), a barrier
static unsigned long long g_shuffle_slots[256];
static inline unsigned long long __shfl_xor(unsigned long long v, int off) {
    g_shuffle_slots[threadIdx.x] = v;
    __syncthreads();
    const unsigned long long other = g_shuffle_slots[threadIdx.x ^ (unsigned)off];
    __syncthreads();
    return other;
}
static std::mutex g_atomic_mutex;
static inline unsigned long long atomicMax(unsigned long long *at, unsigned long long v) {
    std::lock_guard<std::mutex> hold(g_atomic_mutex);
    const unsigned long long old = *at;
    if (v > old) *at = v;
    return old;
}
static inline hipError_t hipMemsetAsync(void *p, int value, size_t bytes, hipStream_t) {
    memset(p, value, bytes);
    return 0;
}

#include "../../dusp_amd/csrc/truepeak_engine.hip"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
using namespace dusp;
static long cases = 0, bad = 0;
static unsigned per_lane_seen = 0;
template <class T>
struct Heap {  // exactly n elements
    T *p;
    explicit Heap(size_t n) : p((T *)malloc(n ? n * sizeof(T) : 1)) {}
    ~Heap() { free(p); }
};
// the contract's loop over one row -> the word
static uint64_t want_word(const float *x, size_t n, uint32_t F, const TruePeakTaps &taps) {
    const uint32_t K = true_peak_phase_taps(F);
    uint64_t most = 0;
    bool finite = true;
    for (size_t u = 0; u < n + K - 1; u++)
        for (uint32_t p = 0; p < F; p++) {
            volatile double acc = 0.0;
            for (uint32_t k = 0; k < K; k++) {
                const double v = u >= k && u - k < n ? (double)x[u - k] : 0.0;
                volatile double prod = (p + F * k < kTruePeakTaps ? taps.h[p + F * k] : 0.0) * v;
                acc = acc + prod;
            }
            const double a = std::fabs(acc);
            uint64_t bits;
            memcpy(&bits, &a, 8);
            finite = finite && std::isfinite(a);
            most = bits > most ? bits : most;
        }
    return finite ? most : 0x7ff8000000000000ull;
}
// kind 0: noise; 1: the largest value last; 2: the largest value first; 3: a NaN planted in the last row; 4: an Inf there
static void run(uint32_t rate, uint32_t S, uint32_t C, size_t n, int kind, int n_cus) {
    const uint32_t F = true_peak_factor(rate);
    const TruePeakTaps taps = true_peak_taps(F);
    const size_t rows = (size_t)S * C;
    Heap<float> x(rows * n);
    Heap<uint64_t> words(rows), again(rows);
    std::mt19937 rng((unsigned)(n * 31 + rows * 7 + kind + F));
    std::normal_distribution<float> nd;
    for (size_t i = 0; i < rows * n; i++) x.p[i] = 0.1f * nd(rng);
    for (size_t r = 0; r < rows && kind == 1; r++) x.p[r * n + n - 1] = 0.9f;
    for (size_t r = 0; r < rows && kind == 2; r++) x.p[r * n] = -0.9f;
    if (kind == 3) x.p[(rows - 1) * n + n / 2] = NAN;
    if (kind == 4) x.p[(rows - 1) * n + n / 2] = -INFINITY;
    per_lane_seen |= true_peak_grid(rows, n, true_peak_phase_taps(F), n_cus).per_lane;
    for (size_t r = 0; r < rows; r++) words.p[r] = again.p[r] = 0xdeadbeefull;
    if (launch_true_peak(x.p, rows, n, F, taps, n_cus, words.p, nullptr) != 0 || launch_true_peak(x.p, rows, n, F, taps, n_cus, again.p, nullptr) != 0) { bad++; return; }
    for (size_t r = 0; r < rows; r++) {
        cases++;
        const uint64_t want = want_word(x.p + r * n, n, F, taps);
        const bool planted = kind >= 3 && r == rows - 1;
        if (words.p[r] != want || again.p[r] != want || planted != std::isnan(true_peak_of_word(words.p[r]))) {
            bad++;
            printf("rate %u %ux%u n %zu kind %d cus %d row %zu: %016llx and %016llx, the loop %016llx\n", rate, S, C, n, kind, n_cus, r, (unsigned long long)words.p[r],
                   (unsigned long long)again.p[r], (unsigned long long)want);
        }
    }
}
static void plan_checks() {
    // the taps: what the issue states, to 1e-12
    const TruePeakTaps t4 = true_peak_taps(4), t2 = true_peak_taps(2), t1 = true_peak_taps(1);
    const double sums4[4] = {1.0, 1.0004797919518407, 1.0009044839413876, 1.0004797919518404};
    for (int p = 0; p < 4; p++) {
        double s = 0;
        for (int j = p; j < 49; j += 4) s += t4.h[j];
        cases++;
        if (std::fabs(s - sums4[p]) > 1e-12) bad++, printf("phase %d of F = 4 sums to %.17g\n", p, s);
    }
    double odd = 0;
    for (int j = 1; j < 49; j += 2) odd += t2.h[j];
    cases++;
    if (std::fabs(odd - 1.000113462147264) > 1e-12 || t4.h[0] != 0 || t4.h[48] != 0 || t4.h[24] != 1 || t1.h[0] != 1 || t1.h[1] != 0) bad++, printf("taps\n");
    // the grid: no workgroup without a position, every position in a workgroup, per_lane falls until the chip is full
    for (uint64_t rows : {1ull, 2ull, 6ull, 1000ull})
        for (uint64_t n : {1ull, 255ull, 256ull, 2048ull, 2049ull, 100000ull, 3000000ull})
            for (uint32_t K : {1u, 13u, 25u})
                for (int cus : {1, 256}) {
                    const TruePeakGrid G = true_peak_grid(rows, n, K, cus);
                    cases++;
                    const bool ok = G.W == 256 * G.per_lane && G.per_lane >= 1 && G.per_lane <= kTruePeakPerLaneMax && G.tiles * G.W >= n + K - 1 && (G.tiles - 1) * G.W < n + K - 1 &&
                                    G.groups == rows * G.tiles && (G.per_lane == 1 || G.groups >= (uint64_t)cus * kTruePeakGroupsPerCu) &&
                                    (G.per_lane == kTruePeakPerLaneMax || rows * ((n + K - 1 + 2 * G.W - 1) / (2 * G.W)) < (uint64_t)cus * kTruePeakGroupsPerCu);
                    if (!ok) bad++, printf("grid rows %llu n %llu K %u cus %d: per_lane %u tiles %llu\n", (unsigned long long)rows, (unsigned long long)n, K, cus, G.per_lane, (unsigned long long)G.tiles);
                }
    // the gain: loudness-limited, ceiling-limited, the unity cases
    double g;
    float l;
    true_peak_loudness_gain(-20.0, 0.5, -23.0, -1.0, g, l);
    cases++;
    if (!(l == (float)(1.0 / std::pow(10.0, -3.0 / 20.0)) && g == 1.0 / (double)l)) bad++, printf("gain by loudness %.17g %.9g\n", g, l);
    true_peak_loudness_gain(-30.0, 1.2, 0.0, -1.0, g, l);
    cases++;
    if (!(l == (float)(1.2 / std::pow(10.0, -1.0 / 20.0)) && g == 1.0 / (double)l && g * 1.2 <= std::pow(10.0, -1.0 / 20.0) * (1 + 1e-7))) bad++, printf("gain by ceiling %.17g %.9g\n", g, l);
    const double lufs[] = {-INFINITY, NAN, -20, -20, -20, 1e9, -1e9}, tps[] = {0.5, 0.5, 0.0, NAN, INFINITY, 0.5, 1e-300};
    for (int i = 0; i < 7; i++) {
        true_peak_loudness_gain(lufs[i], tps[i], -23.0, -1.0, g, l);
        cases++;
        if (g != 1.0 || l != 1.0f) bad++, printf("unity case %d: %.17g %.9g\n", i, g, l);
    }
}
int main() {
    plan_checks();
    const uint32_t rates[] = {44100, 96000, 192000};
    for (uint32_t rate : rates) {
        const uint32_t K = true_peak_phase_taps(true_peak_factor(rate));
        const size_t W = 256;  // (few rows on 256 CUs: a position a lane)
        const size_t ns[] = {1, 5, W - 1, W, W + 1, W + K - 2, W + K - 1, 2 * W + 3};
        for (size_t n : ns)
            for (int kind = 0; kind < 5; kind++) {
                if (n < 2 && kind >= 1 && kind <= 2) continue;
                run(rate, 1, 1, n, kind, 256);
                if (n & 1) run(rate, 1, 2, n, kind, 256);
                if (kind == 0 || kind >= 3) run(rate, 3, 2, n, kind, 256);
            }
        // a lane takes 2, 4 and 8 positions where that still gives a device of ONE CU its 4 workgroups: one row of about 4 tiles
        for (size_t per : {2, 4, 8}) {
            const size_t Wp = 256 * per;
            for (size_t n : {4 * Wp - 1, 4 * Wp + 1, 4 * Wp + K - 1}) {
                if (true_peak_grid(1, n, K, 1).per_lane != per) bad++, printf("per_lane at n %zu K %u is not %zu\n", n, K, per);
                run(rate, 1, 1, n, (int)(n % 3), 1);
            }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"groups\": %lu, \"per_lane\": %u}\n", cases, bad, g_groups_run, per_lane_seen);
    return bad ? 1 : 0;
}
