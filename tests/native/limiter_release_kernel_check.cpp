// limiter_release_kernel_check.cpp — the text of dusp_amd/csrc/limiter_release_engine.hip compiled for the HOST (hip_host_stub_lds/: the
// lanes of a workgroup as threads, LDS as statics, __syncthreads a barrier; the wave's shuffles and the 64-bit atomicMin that stub lacks
// are defined here) and held BIT FOR BIT to the contract's loops (dusp_amd/mix.py limiter_gain_release), written out below as the plain
// double loop for the minima, the sequential recurrence held[j] = min(m[j], held[j - 1] + d) and the plain sum; and
// limiter_release_plan.hpp's step, grid and look-back on the way.
// EVERY BUFFER IS A HEAP ALLOCATION OF EXACTLY ITS SIZE — the signals, the words q, the held curve, the summaries, the gain, the smallest
// sum — so under AddressSanitizer one element read or written outside a buffer is reported.
// Covered: L = 1, 3, 64, 513 and 4096; R = 1, 2, L, W - 1, W, W + 1, 3 W + 1, 100000 and 2^22; n = 1, 5, W - 1, W, W + 1, 2 W + 3 and
// 9 W + 7 at per_lane 1 (256 CUs), and about four tiles on a device of ONE CU at per_lane 2, 4 and 8 (8 at L <= 512 only); rows 1 and 3;
// words of noise, a lone dip at sample 0, n - 1, and L - 1 and L positions either side of a tile's edge, a deep dip whose release
// crosses more than three tiles with a shallower and a deeper one inside it and tiles of ONE between, and words that are all ONE
// (the rows stay bit for bit, the sum stays L x ONE); two runs of the noise give equal bits.
// Built with -fsanitize=address,undefined by tests/test_limiter_release_host.py.  Prints {"cases": n, "bad": m, "groups": g, "per_lane": mask}.
#include <hip/hip_runtime.h>  // (hip_host_stub_lds: included first, so that the kernel's own include is this one)

#include <cstring>
#include <mutex>
// ---- what the kernels need beyond that stub: the wave's shuffles (every lane of the workgroup parks its value, a barrier, reads its
// partner's within its wave of 64, a barrier) and the 64-bit atomicMin ----
static unsigned long long g_shuffle_slots[256];
static inline unsigned long long __shfl_xor(unsigned long long v, int off) {
    g_shuffle_slots[threadIdx.x] = v;
    __syncthreads();
    const unsigned long long other = g_shuffle_slots[threadIdx.x ^ (unsigned)off];
    __syncthreads();
    return other;
}
static inline unsigned long long __shfl_up(unsigned long long v, int off) {  // (a lane without a partner below it keeps its own)
    g_shuffle_slots[threadIdx.x] = v;
    __syncthreads();
    const unsigned long long other = (threadIdx.x & 63) >= (unsigned)off ? g_shuffle_slots[threadIdx.x - (unsigned)off] : v;
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

#include "../../dusp_amd/csrc/limiter_release_engine.hip"
#include <algorithm>
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
// the contract's loops: q [n], x [rows][n] -> held [n + L - 1], g [n], y [rows][n], the smallest sum
static void want(const uint32_t *q, const float *x, size_t rows, size_t n, uint32_t L, uint32_t R, std::vector<uint32_t> &held, std::vector<double> &g, std::vector<float> &y,
                 uint64_t &smallest) {
    const uint64_t d = (kLimiterOne + (uint64_t)R - 1) / R;
    auto q_at = [&](long long j) -> uint64_t { return j >= 0 && j < (long long)n ? q[(size_t)j] : kLimiterOne; };
    held.assign(n + L - 1, 0), g.assign(n, 0.0), y.assign(rows * n, 0.0f);
    uint64_t last = kLimiterOne;  // held[-L]
    for (size_t i = 0; i < held.size(); i++) {
        uint64_t least = kLimiterOne;  // m[j], j = i - (L - 1)
        for (uint32_t k = 0; k < L; k++) least = std::min(least, q_at((long long)i - (long long)(L - 1) + k));
        last = std::min(least, last + d);
        held[i] = (uint32_t)last;
    }
    smallest = (uint64_t)L * kLimiterOne;
    for (size_t s = 0; s < n; s++) {
        uint64_t sum = 0;
        for (uint32_t k = 0; k < L; k++) sum += held[s + k];
        smallest = std::min(smallest, sum);
        g[s] = (double)sum / (double)((uint64_t)L * kLimiterOne);
        for (size_t r = 0; r < rows; r++) {
            volatile double prod = (double)x[r * n + s] * g[s];
            y[r * n + s] = (float)prod;
        }
    }
}
// kind 0: words of noise; 1: all ONE; 2: a deep dip at `at`, a shallower one W / 2 behind it and a deeper one 2 W behind it, ONE elsewhere;
// 10: a lone dip at `at`
static void run(size_t rows, size_t n, uint32_t L, uint32_t R, int kind, size_t at, int n_cus) {
    const LimiterReleaseGrid P = limiter_release_grid(n, L, R, n_cus);
    Heap<float> x(rows * n), first(rows * n), again(rows * n);
    Heap<uint32_t> q(n), h1(n + L - 1), h2(n + L - 1), a1(P.hold_tiles), a2(P.hold_tiles);
    Heap<double> g1(n), g2(n);
    Heap<uint64_t> w1(1), w2(1);
    std::mt19937 rng((unsigned)(n * 31 + rows * 7 + kind + L + R));
    std::normal_distribution<float> nd;
    for (size_t i = 0; i < rows * n; i++) x.p[i] = 0.4f * nd(rng);
    for (size_t s = 0; s < n; s++) q.p[s] = kind == 0 ? (rng() % 4 ? kLimiterOne : rng() % (kLimiterOne + 1u)) : kLimiterOne;
    if (kind == 10 && at < n) q.p[at] = kLimiterOne / 3;
    if (kind == 2) {
        if (at < n) q.p[at] = 1000;
        if (at + P.W / 2 < n) q.p[at + P.W / 2] = kLimiterOne / 2;  // (inside the first one's release where R is long: must not show)
        if (at + 2 * P.W < n) q.p[at + 2 * P.W] = 3;                // (deeper: takes over)
    }
    per_lane_seen |= P.per_lane;
    memcpy(first.p, x.p, rows * n * sizeof(float)), memcpy(again.p, x.p, rows * n * sizeof(float));
    *w1.p = *w2.p = (uint64_t)L * kLimiterOne;  // (what the envelope kernel leaves)
    const bool twice = kind == 0 && (n == 2 * 256 + 3 || n_cus == 1);  // (the second run: where there is noise and more than one tile)
    if (launch_limit_hold(n, L, R, n_cus, q.p, h1.p, a1.p, nullptr) != 0 || launch_limit_release(n, L, R, n_cus, h1.p, a1.p, nullptr) != 0 ||
        launch_limit_mean_apply(first.p, rows, n, L, n_cus, h1.p, w1.p, g1.p, nullptr) != 0 ||
        (twice && (launch_limit_hold(n, L, R, n_cus, q.p, h2.p, a2.p, nullptr) != 0 || launch_limit_release(n, L, R, n_cus, h2.p, a2.p, nullptr) != 0 ||
                   launch_limit_mean_apply(again.p, rows, n, L, n_cus, h2.p, w2.p, g2.p, nullptr) != 0))) {
        bad++;
        return;
    }
    if (!twice) *w2.p = *w1.p, memcpy(h2.p, h1.p, (n + L - 1) * 4), memcpy(g2.p, g1.p, n * 8), memcpy(again.p, first.p, rows * n * 4);
    std::vector<uint32_t> held;
    std::vector<double> g;
    std::vector<float> y;
    uint64_t smallest;
    want(q.p, x.p, rows, n, L, R, held, g, y, smallest);
    cases++;
    bool ok = *w1.p == smallest && *w2.p == smallest && !memcmp(h1.p, held.data(), held.size() * 4) && !memcmp(h2.p, held.data(), held.size() * 4) && !memcmp(g1.p, g.data(), n * 8) &&
              !memcmp(g2.p, g.data(), n * 8) && !memcmp(first.p, y.data(), rows * n * 4) && !memcmp(again.p, y.data(), rows * n * 4);
    if (kind == 1) ok = ok && smallest == (uint64_t)L * kLimiterOne && !memcmp(first.p, x.p, rows * n * 4);
    if (kind == 10 || kind == 2) ok = ok && (at >= n || smallest < (uint64_t)L * kLimiterOne);  // (the case does limit)
    if (!ok) {
        bad++;
        printf("rows %zu n %zu L %u R %u kind %d at %zu cus %d: smallest %llx and %llx, the loop %llx\n", rows, n, L, R, kind, at, n_cus, (unsigned long long)*w1.p, (unsigned long long)*w2.p,
               (unsigned long long)smallest);
    }
}
static void plan_checks() {
    cases++;
    if (limiter_release_step(1) != kLimiterOne || limiter_release_step(16) != (1u << 26) || limiter_release_step(3) != 357913942u || limiter_release_step(kLimiterReleaseMax) != 256)
        bad++, printf("the step\n");
    for (uint64_t n : {1ull, 255ull, 2049ull, 3000000ull})
        for (uint32_t L : {1u, 240u, 513u, 4096u})
            for (uint32_t R : {1u, 7u, 2400u, kLimiterReleaseMax})
                for (int cus : {1, 256}) {
                    const LimiterReleaseGrid P = limiter_release_grid(n, L, R, cus);
                    const LimiterGrid G = limiter_grid(n, L, cus);
                    cases++;
                    const uint64_t dW = (uint64_t)P.d * P.W;
                    const bool ok = P.W == G.W && P.per_lane == G.per_lane && P.tiles == G.tiles && P.positions == n + L - 1 && P.hold_tiles * P.W >= P.positions &&
                                    (P.hold_tiles - 1) * P.W < P.positions && P.positions + P.hold_tiles <= limiter_release_words(n, L) && dW * (P.look_back - 1) >= kLimiterOne &&
                                    dW * (P.look_back - 1) < kLimiterOne + dW;
                    if (!ok) bad++, printf("grid n %llu L %u R %u cus %d\n", (unsigned long long)n, L, R, cus);
                }
}
int main() {
    plan_checks();
    const size_t W = 256;  // (256 CUs: a position a lane)
    for (uint32_t L : {1u, 3u, 64u, 513u, 4096u}) {
        const uint32_t releases[] = {1, 2, L, (uint32_t)W - 1, (uint32_t)W, (uint32_t)W + 1, 3 * (uint32_t)W + 1, 100000, kLimiterReleaseMax};
        const size_t ns[] = {1, 5, W - 1, W, W + 1, 2 * W + 3, 9 * W + 7};
        int turn = 0;
        for (size_t n : ns) {
            if (L == 4096 && n != 5 && n != 2 * W + 3) continue;  // (the long window costs the loop L a position: two lengths)
            for (uint32_t R : releases) {  // (every release at 2 W + 3; elsewhere every third, and under a long window every fourth)
                if (n != 2 * W + 3 ? turn++ % 3 != 0 : L >= 513 && turn++ % 4 != 0) continue;
                run(n & 1 ? 3 : 1, n, L, R, 0, 0, 256);
            }
            if (n == 5 || n == W + 1) run(1, n, L, 1000, 1, 0, 256);
        }
        // a lone dip where a short halo or a wrong carry shows: the ends, and L - 1 and L positions either side of a tile's edge
        const size_t n = 2 * W + 3;
        for (size_t at : {(size_t)0, n - 1, W - 1, W, W - L, W - L + 1, W - 1 + L, W + L, W - 1 - (L - 1), W + (L - 1)})
            if (at < n && (L < 513 || at == W - 1 || at == W)) {
                run(2, n, L, L == 3 ? 2 * W : 7, 10, at, 256);
                if (at == 0 || at == W - 1 || at == W) run(1, n, L, 1u << 20, 10, at, 256);
            }
        // a release across more than three tiles, a shallower and a deeper dip inside it, tiles of ONE between
        if (L <= 64) run(2, 9 * W + 7, L, 5 * W, 2, W / 2, 256), run(1, 9 * W + 7, L, kLimiterReleaseMax, 2, W - 1, 256);
    }
    // a lane takes 2, 4 and 8 positions where that still gives a device of ONE CU its 4 workgroups
    for (uint32_t L : {3u, 64u, 4096u})
        for (size_t per : {2, 4, 8}) {
            const size_t Wp = 256 * per;
            if (L > kLimiterWindowShort && per > kLimiterPerLaneLong) continue;
            for (size_t n : {4 * Wp - 1, 4 * Wp + 1}) {
                if (limiter_grid(n, L, 1).per_lane != per) bad++, printf("per_lane at n %zu L %u is not %zu\n", n, L, per);
                if (L == 4096 && n > 4 * Wp) continue;
                run(n & 2 ? 2 : 1, n, L, n % 4 == 1 ? 3 * Wp + 1 : 777, n % 4 == 1 ? 2 : 0, Wp - 1, 1);
            }
        }
    printf("{\"cases\": %ld, \"bad\": %ld, \"groups\": %lu, \"per_lane\": %u}\n", cases, bad, g_groups_run, per_lane_seen);
    return bad ? 1 : 0;
}
