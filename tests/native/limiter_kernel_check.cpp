// limiter_kernel_check.cpp — the text of dusp_amd/csrc/limiter_engine.hip compiled for the HOST (hip_host_stub_lds/: the lanes of a
// workgroup as threads, LDS as statics, __syncthreads a barrier; the wave's shuffle and the 64-bit atomicMin that stub lacks are defined
// here) and held BIT FOR BIT to the contract's loop (dusp_amd/mix.py limiter_envelope, limiter_gain, limit), written out below with every
// product and sum rounded by itself, the sliding minimum and the sliding sum as the plain double loops; and limiter_plan.hpp's grid rule
// and threshold on the way.
// EVERY BUFFER IS A HEAP ALLOCATION OF EXACTLY ITS SIZE — the signals, the words q, the curve, the smallest sum — so under
// AddressSanitizer one element read or written outside a buffer is reported.
// Covered: F = 4 (44100 Hz), 2 (96000 Hz) and 1 (192000 Hz); L = 1, 2, 3, 64 and 4096; per_lane 1 (256 CUs) and — about four tiles on a
// device of ONE CU — 2, 4 and 8 (8 at L <= 512 only: a longer window caps the tile at 1024); n = 1, 5, W - 1, W, W + 1 and 2 W + 3;
// 1 x 1, 1 x 2 (odd n: the second row unaligned) and 3 x 2; noise over the threshold, a lone peak at sample 0, n - 1, W - 1 and W, and
// L - 1 and L samples on either side of the first tile edge, a planted NaN and Inf, a threshold above everything (the rows stay bit for
// bit, the sum stays L x ONE); two runs give equal bits.
// Built with -fsanitize=address,undefined by tests/test_limiter_host.py.  Prints {"cases": n, "bad": m, "groups": g, "per_lane": mask}.
#include <hip/hip_runtime.h>  // (hip_host_stub_lds: included first, so that the kernel's own include is this one)

#include <cstring>
#include <mutex>
// ---- what the kernels need beyond that stub ----
static inline long long __double_as_longlong(double v) {
    long long b;
    memcpy(&b, &v, 8);
    return b;
}
static inline double __longlong_as_double(long long b) {
    double v;
    memcpy(&v, &b, 8);
    return v;
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
static inline unsigned long long atomicMin(unsigned long long *at, unsigned long long v) {
    std::lock_guard<std::mutex> hold(g_atomic_mutex);
    const unsigned long long old = *at;
    if (v < old) *at = v;
    return old;
}

#include "../../dusp_amd/csrc/limiter_engine.hip"
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
// the contract's loops: x [rows][n] -> q [n], g [n], y [rows][n], the smallest sum
static void want(const float *x, size_t rows, size_t n, uint32_t F, const TruePeakTaps &taps, double T, uint32_t L, std::vector<uint32_t> &q, std::vector<double> &g, std::vector<float> &y,
                 uint64_t &smallest) {
    const uint32_t K = true_peak_phase_taps(F), D = limiter_delay(F);
    q.assign(n, 0), g.assign(n, 0.0), y.assign(rows * n, 0.0f);
    for (size_t s = 0; s < n; s++) {
        double e = 0.0;
        for (size_t r = 0; r < rows; r++)
            for (uint32_t p = 0; p < F; p++) {
                volatile double acc = 0.0;
                const size_t u = s + D;
                for (uint32_t k = 0; k < K; k++) {
                    const double v = u >= k && u - k < n ? (double)x[r * n + u - k] : 0.0;
                    volatile double prod = (p + F * k < kTruePeakTaps ? taps.h[p + F * k] : 0.0) * v;
                    acc = acc + prod;
                }
                const double a = std::fabs(acc);
                if (std::isfinite(a) && a > e) e = a;
            }
        volatile double ratio = e > T ? T / e : 1.0;
        q[s] = (uint32_t)std::floor(ratio * 1073741824.0);
    }
    auto q_at = [&](long long j) -> uint64_t { return j >= 0 && j < (long long)n ? q[(size_t)j] : kLimiterOne; };
    std::vector<uint64_t> m(n + L - 1);  // m[j + (L - 1)] = min(q[j .. j + L - 1])
    for (size_t i = 0; i < m.size(); i++) {
        uint64_t least = kLimiterOne;
        for (uint32_t k = 0; k < L; k++) least = std::min(least, q_at((long long)i - (long long)(L - 1) + k));
        m[i] = least;
    }
    smallest = (uint64_t)L * kLimiterOne;
    for (size_t s = 0; s < n; s++) {
        uint64_t sum = 0;
        for (uint32_t k = 0; k < L; k++) sum += m[s + k];
        smallest = std::min(smallest, sum);
        g[s] = (double)sum / (double)((uint64_t)L * kLimiterOne);
        for (size_t r = 0; r < rows; r++) {
            volatile double prod = (double)x[r * n + s] * g[s];
            y[r * n + s] = (float)prod;
        }
    }
}
// kind 0: noise; 1: a threshold above everything; 2: a NaN planted in the last row; 3: an Inf there; 10 + : a lone peak at sample `at`
static void run(uint32_t rate, uint32_t S, uint32_t C, size_t n, uint32_t L, int kind, size_t at, int n_cus) {
    const uint32_t F = true_peak_factor(rate);
    const TruePeakTaps taps = true_peak_taps(F);
    const size_t rows = (size_t)S * C;
    Heap<float> x(rows * n), first(rows * n), again(rows * n);
    Heap<uint32_t> q1(n), q2(n);
    Heap<double> g1(n), g2(n);
    Heap<uint64_t> w1(1), w2(1);
    std::mt19937 rng((unsigned)(n * 31 + rows * 7 + kind + F + L));
    std::normal_distribution<float> nd;
    const bool lone = kind >= 10;
    for (size_t i = 0; i < rows * n; i++) x.p[i] = (lone ? 0.05f : 0.4f) * nd(rng);
    if (lone && at < n) x.p[((at + L) % rows) * n + at] = at & 1 ? -3.0f : 2.5f;  // (the peak in a different row each time)
    if (kind == 2) x.p[(rows - 1) * n + n / 2] = NAN;
    if (kind == 3) x.p[(rows - 1) * n + n / 2] = -INFINITY;
    const double T = kind == 1 ? 100.0 : 0.5;
    per_lane_seen |= limiter_grid(n, L, n_cus).per_lane;
    memcpy(first.p, x.p, rows * n * sizeof(float)), memcpy(again.p, x.p, rows * n * sizeof(float));
    *w1.p = *w2.p = 0xdeadbeefull;
    if (launch_limit_envelope(first.p, rows, n, F, taps, T, L, n_cus, q1.p, w1.p, nullptr) != 0 || launch_limit_apply(first.p, rows, n, L, n_cus, q1.p, w1.p, g1.p, nullptr) != 0 ||
        launch_limit_envelope(again.p, rows, n, F, taps, T, L, n_cus, q2.p, w2.p, nullptr) != 0 || launch_limit_apply(again.p, rows, n, L, n_cus, q2.p, w2.p, g2.p, nullptr) != 0) {
        bad++;
        return;
    }
    std::vector<uint32_t> q;
    std::vector<double> g;
    std::vector<float> y;
    uint64_t smallest;
    want(x.p, rows, n, F, taps, T, L, q, g, y, smallest);
    cases++;
    bool ok = *w1.p == smallest && *w2.p == smallest && !memcmp(q1.p, q.data(), n * 4) && !memcmp(q2.p, q.data(), n * 4) && !memcmp(g1.p, g.data(), n * 8) && !memcmp(g2.p, g.data(), n * 8) &&
              !memcmp(first.p, y.data(), rows * n * 4) && !memcmp(again.p, y.data(), rows * n * 4);
    if (kind == 1) ok = ok && smallest == (uint64_t)L * kLimiterOne && !memcmp(first.p, x.p, rows * n * 4);
    if ((kind == 0 && n >= 64) || lone) ok = ok && (at >= n || smallest < (uint64_t)L * kLimiterOne);  // (the case does limit)
    if (!ok) {
        bad++;
        printf("rate %u %ux%u n %zu L %u kind %d at %zu cus %d: smallest %llx and %llx, the loop %llx\n", rate, S, C, n, L, kind, at, n_cus, (unsigned long long)*w1.p, (unsigned long long)*w2.p,
               (unsigned long long)smallest);
    }
}
static void plan_checks() {
    for (uint64_t n : {1ull, 255ull, 256ull, 2048ull, 2049ull, 100000ull, 3000000ull})
        for (uint32_t L : {1u, 240u, 512u, 513u, 4096u})
            for (int cus : {1, 256}) {
                const LimiterGrid G = limiter_grid(n, L, cus);
                const uint32_t cap = L > kLimiterWindowShort ? kLimiterPerLaneLong : kTruePeakPerLaneMax;
                cases++;
                const bool ok = G.W == 256 * G.per_lane && G.per_lane >= 1 && G.per_lane <= cap && G.tiles * G.W >= n && (G.tiles - 1) * G.W < n &&
                                (G.per_lane == 1 || G.tiles >= (uint64_t)cus * kLimiterGroupsPerCu) && (G.per_lane == cap || (n + 2 * G.W - 1) / (2 * G.W) < (uint64_t)cus * kLimiterGroupsPerCu) &&
                                G.W + 2 * (L - 1) <= 256 * cap + 2 * ((L > kLimiterWindowShort ? kLimiterWindowMax : kLimiterWindowShort) - 1);
                if (!ok) bad++, printf("grid n %llu L %u cus %d: per_lane %u tiles %llu\n", (unsigned long long)n, L, cus, G.per_lane, (unsigned long long)G.tiles);
            }
    cases++;
    if (limiter_threshold(-20.0, -16.0, -1.0) != std::pow(10.0, -1.0 / 20.0) / std::pow(10.0, 4.0 / 20.0) || limiter_delay(4) != 6 || limiter_delay(2) != 12 || limiter_delay(1) != 0 ||
        limiter_reduction((uint64_t)3 << 29, 3) != 0.5)
        bad++, printf("threshold, delay or reduction\n");
}
int main() {
    plan_checks();
    const uint32_t rates[] = {44100, 96000, 192000}, windows[] = {1, 2, 3, 64, 4096};
    const size_t W = 256;  // (256 CUs: a sample a lane)
    for (uint32_t rate : rates)
        for (uint32_t L : windows) {
            const size_t ns[] = {1, 5, W - 1, W, W + 1, 2 * W + 3};
            for (size_t n : ns) {
                if (L == 4096 && n != 5 && n != 2 * W + 3) continue;  // (the long window costs the loop L^2 a sample: two lengths)
                run(rate, 1, 1, n, L, 0, 0, 256);
                if (n & 1) run(rate, 1, 2, n, L, (int)(n % 4), 0, 256);
                if (rate == 44100 || n == 2 * W + 3) run(rate, 3, 2, n, L, n == 2 * W + 3 ? 2 : 3, 0, 256);
            }
            // a lone peak where a short halo shows: the ends, the tile's edge, and L - 1 and L samples on either side of it
            const size_t n = 2 * W + 3;
            if (rate == 96000 && L == 4096) continue;
            for (size_t at : {(size_t)0, n - 1, W - 1, W, W - L, W - L + 1, W - 1 + L, W + L, W - 1 - (L - 1), W + (L - 1)})
                if (at < n && (rate == 44100 || at == W - 1 || at == W)) run(rate, 3, 2, n, L, 10, at, 256);
        }
    // a lane takes 2, 4 and 8 samples where that still gives a device of ONE CU its 4 workgroups
    for (uint32_t L : {3u, 64u, 4096u})
        for (size_t per : {2, 4, 8}) {
            const size_t Wp = 256 * per;
            if (L > kLimiterWindowShort && per > kLimiterPerLaneLong) continue;
            for (size_t n : {4 * Wp - 1, 4 * Wp + 1}) {
                if (limiter_grid(n, L, 1).per_lane != per) bad++, printf("per_lane at n %zu L %u is not %zu\n", n, L, per);
                if (L == 4096 && n > 4 * Wp) continue;
                run(L == 64 ? 96000 : 44100, 1, n & 2 ? 2 : 1, n, L, n % 4 == 1 ? 10 : 0, Wp - 1 + (n % 7), 1);
            }
        }
    printf("{\"cases\": %ld, \"bad\": %ld, \"groups\": %lu, \"per_lane\": %u}\n", cases, bad, g_groups_run, per_lane_seen);
    return bad ? 1 : 0;
}
