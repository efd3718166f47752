// meter_kernel_check.cpp — the text of dusp_amd/csrc/meter_engine.hip compiled for the HOST (hip_host_stub_lds/: the lanes of a workgroup
// as threads, LDS as statics, __syncthreads a barrier) and held to the ONE sequential loop of the contract (dusp_amd/mix.py k_weighted):
// every hop's sum over the channels of z^2 within the bound the cut in time may differ by, every row's sum of squares within n 2^-52
// relative, and what meter_plan.hpp makes of the hop sums (blocks, gates) against the same over the loop's sums.
// EVERY BUFFER IS A HEAP ALLOCATION OF EXACTLY ITS SIZE — the signals, the scratch (meter_geometry's doubles), the sums — so under
// AddressSanitizer one element read or written outside a buffer is reported.
// Covered: 8000 Hz (hop 800, L 400: two segments a hop), 8010 Hz (hop 801, L 267: three), 11025 Hz (hop 1103, a prime: L is the hop);
// n = 1, L - 1, L, L + 1, hop - 1, hop, hop + 1, block - 1, block, block + 1 and 3 blocks + 17 (a last short segment, a last short
// hop); S x C = 1 x 1 and 3 x 2, and 5 x 8 once (more segments than a workgroup has lanes); noise, noise on a DC offset of 0.5, a
// planted Inf (hops before it as the loop's, hops from it on not finite in both).
// Built with -fsanitize=address,undefined by tests/test_meters_host.py.  Prints {"cases": n, "bad": m, "groups": g, "worst": r}:
// worst = the largest observed difference of a hop sum over its bound.
#include "../../dusp_amd/csrc/meter_engine.hip"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
using namespace dusp;
static long cases = 0, bad = 0;
static double worst = 0.0;
template <class T>
struct Heap {  // exactly n elements
    T *p;
    explicit Heap(size_t n) : p((T *)malloc(n ? n * sizeof(T) : 1)) {}
    ~Heap() { free(p); }
};
// sum |g_k| of the impulse response of 1 / (1 + a1 z^-1 + a2 z^-2), until it stops growing
static double gain_of(double a1, double a2) {
    double g1 = 0.0, g2 = 0.0, sum = 0.0;
    for (long k = 0; k < 100000000; k++) {
        const double g = (k == 0 ? 1.0 : 0.0) - a1 * g1 - a2 * g2;
        const double next = sum + std::fabs(g);
        if (k > 16 && next == sum) break;
        sum = next, g2 = g1, g1 = g;
    }
    return sum;
}
static void run(uint32_t rate, uint32_t S, uint32_t C, size_t n, int kind) {
    const uint32_t hop = meter_hop(rate);
    const size_t rows = (size_t)S * C, n_hops = (n + hop - 1) / hop;
    const MeterCoef k = meter_k_weighting(rate);
    const MeterGeometry G = meter_geometry(rows, n, hop);
    Heap<float> x(rows * n);
    Heap<double> scratch(G.doubles), sumsq(rows), hops(S * n_hops);
    std::mt19937 rng((unsigned)(n * 31 + rows * 7 + kind));
    std::normal_distribution<float> nd;
    double peak = 0.0;
    for (size_t i = 0; i < rows * n; i++) {
        x.p[i] = 0.1f * nd(rng) + (kind == 1 ? 0.5f : 0.0f);
        peak = std::fmax(peak, std::fabs((double)x.p[i]));
    }
    const size_t inf_at = n / 2 + 3 < n ? n / 2 + 3 : n - 1;  // (in the last row)
    if (kind == 2) x.p[(rows - 1) * n + inf_at] = INFINITY;
    for (size_t i = 0; i < G.doubles; i++) scratch.p[i] = NAN;
    if (launch_meter(x.p, S, C, n, hop, k, scratch.p, sumsq.p, hops.p, nullptr, nullptr) != 0) { bad++; return; }
    // the one sequential loop, and per hop the bound: a sample of z differs by at most delta, so z^2 by 2 |z| delta + delta^2
    const double delta = 2.0 * 8.0 * std::ldexp(1.0, -53) * gain_of(k.s[0][3], k.s[0][4]) * gain_of(k.s[1][3], k.s[1][4]) * peak;
    std::vector<double> want(S * n_hops, 0.0), bound(S * n_hops, 0.0);
    for (size_t r = 0; r < rows; r++) {
        double x1 = 0, x2 = 0, y1 = 0, y2 = 0, z1 = 0, z2 = 0, sq = 0;
        for (size_t t = 0; t < n; t++) {
            const double v = (double)x.p[r * n + t];
            volatile double y = k.s[0][0] * v;
            y = y + k.s[0][1] * x1; y = y + k.s[0][2] * x2; y = y - k.s[0][3] * y1; y = y - k.s[0][4] * y2;
            volatile double z = k.s[1][0] * y;
            z = z + k.s[1][1] * y1; z = z + k.s[1][2] * y2; z = z - k.s[1][3] * z1; z = z - k.s[1][4] * z2;
            x2 = x1, x1 = v, y2 = y1, y1 = y, z2 = z1, z1 = z;
            want[(r / C) * n_hops + t / hop] += z * z;
            bound[(r / C) * n_hops + t / hop] += 2.0 * std::fabs(z) * delta + delta * delta;
            sq += v * v;
        }
        cases++;
        const bool row_inf = kind == 2 && r == rows - 1;
        if (row_inf ? std::isfinite(sumsq.p[r]) : !(std::fabs(sumsq.p[r] - sq) <= (double)n * std::ldexp(1.0, -52) * sq)) {
            bad++;
            printf("sumsq rate %u %ux%u n %zu kind %d row %zu: %.17g, the loop %.17g\n", rate, S, C, n, kind, r, sumsq.p[r], sq);
        }
    }
    for (size_t i = 0; i < S * n_hops; i++) {
        cases++;
        const double got = hops.p[i];
        bool ok;
        if (!std::isfinite(want[i])) {
            ok = !std::isfinite(got);
        } else {
            const double limit = bound[i] + 1e-13 * want[i];
            ok = std::fabs(got - want[i]) <= limit;
            if (limit > 0) worst = std::fmax(worst, std::fabs(got - want[i]) / limit);
        }
        if (kind == 2 && i / n_hops == S - 1 && i % n_hops >= inf_at / hop) ok = ok && !std::isfinite(got);  // (holds or follows the Inf)
        if (!ok) {
            bad++;
            printf("hop rate %u %ux%u n %zu kind %d signal %zu hop %zu: %.17g, the loop %.17g\n", rate, S, C, n, kind, i / n_hops, i % n_hops, got, want[i]);
        }
    }
    // the gates over the kernels' sums and over the loop's: the same blocks, the same loudness to 1e-9
    const size_t n_blocks = meter_blocks(n, rate);
    for (uint32_t s = 0; s < S && n_blocks; s++) {
        std::vector<double> m0(n_blocks), m1(n_blocks);
        const double l0 = meter_loudness(hops.p + s * n_hops, n_blocks, 4 * (size_t)hop, m0.data()), l1 = meter_loudness(want.data() + s * n_hops, n_blocks, 4 * (size_t)hop, m1.data());
        cases++;
        if (!(l0 == l1 || (std::isnan(l0) && std::isnan(l1)) || std::fabs(l0 - l1) <= 1e-9)) {
            bad++;
            printf("lufs rate %u %ux%u n %zu kind %d signal %u: %.17g, the loop %.17g\n", rate, S, C, n, kind, s, l0, l1);
        }
    }
}
int main() {
    const uint32_t rates[] = {8000, 8010, 11025};
    for (uint32_t rate : rates) {
        const size_t hop = meter_hop(rate), L = meter_segment((uint32_t)hop), block = 4 * hop;
        if ((rate == 8000 && L != 400) || (rate == 8010 && L != 267) || (rate == 11025 && L != hop)) { printf("L at %u Hz is %zu\n", rate, L); bad++; }
        const size_t ns[] = {1, L - 1, L, L + 1, hop - 1, hop, hop + 1, block - 1, block, block + 1, 3 * block + 17};
        for (size_t n : ns)
            for (int kind = 0; kind < 3; kind++) {
                run(rate, 1, 1, n, kind);
                if (rate == 8000 || n >= block) run(rate, 3, 2, n, kind);
            }
    }
    run(8000, 5, 8, 3 * 3200 + 17, 0);
    printf("{\"cases\": %ld, \"bad\": %ld, \"groups\": %lu, \"worst\": %.3g}\n", cases, bad, g_groups_run, worst);
    return bad ? 1 : 0;
}
