// CPU check of dusp_amd/csrc/pcm_quant.hpp (the PCM sample contract the device encoder, dusp_amd/wav.py and wav.js share) against
// the same steps evaluated in integers: both IEEE multiplies as exact 128-bit products rounded to nearest even by hand, the
// rounding to an integer (halves away from zero) on the mantissa.  Nothing here depends on how the compiler schedules or
// contracts floating-point operations.  Build with -ffp-contract=off (the header keeps contraction off for itself under clang).
//   every f32 next to a rounding boundary (k + 0.5) / (S g), two neighbours on both sides, both signs: all k of s16, a stride of s24;
//   a few million random values; zeros, +-1, beyond +-1, NaN, infinities, subnormals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../dusp_amd/csrc/pcm_quant.hpp"

typedef unsigned __int128 u128;

static void decompose(double d, uint64_t &M, int &E) {  // |d| = M 2^E, M < 2^53 (d finite, non-zero)
    int e;
    const double m = std::frexp(std::fabs(d), &e);
    M = (uint64_t)std::ldexp(m, 53);
    E = e - 53;
}

static double mul_rne(double a, double b) {  // fl(a * b), round to nearest even, from the exact product
    if (a != a || b != b) return NAN;
    const bool neg = std::signbit(a) != std::signbit(b);
    if (std::isinf(a) || std::isinf(b)) return (a == 0.0 || b == 0.0) ? NAN : (neg ? -INFINITY : INFINITY);
    if (a == 0.0 || b == 0.0) return neg ? -0.0 : 0.0;
    uint64_t Ma, Mb;
    int Ea, Eb;
    decompose(a, Ma, Ea);
    decompose(b, Mb, Eb);
    u128 P = (u128)Ma * Mb;
    int E = Ea + Eb, bits = 0;
    for (u128 q = P; q; q >>= 1) bits++;
    if (E + bits < -900) return neg ? -0.0 : 0.0;  // (far below anything that rounds to a non-zero sample; keeps ldexp exact)
    if (bits > 53) {
        const int sh = bits - 53;
        const u128 rem = P & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
        P >>= sh;
        if (rem > half || (rem == half && (P & 1))) P++;
        E += sh;
    }
    const double r = std::ldexp((double)(uint64_t)P, E);
    return neg ? -r : r;
}

static int32_t reference(float x, double g, double S) {
    double t = mul_rne((double)x, g);
    if (t != t) t = 0.0;
    if (t < -1.0) t = -1.0;
    if (t > 1.0) t = 1.0;
    const double v = mul_rne(t, S);
    if (v == 0.0) return 0;
    uint64_t M;
    int E;
    decompose(v, M, E);
    int64_t q;
    if (E >= 0) q = (int64_t)(M << E);
    else if (-E > 62) q = 0;
    else {
        const int sh = -E;
        q = (int64_t)(M >> sh) + ((M & ((1ull << sh) - 1)) >= (1ull << (sh - 1)) ? 1 : 0);
    }
    return (int32_t)(v < 0.0 ? -q : q);
}

static long cases = 0, bad = 0;
static void check(float x, double g, double S) {
    const int32_t want = reference(x, g, S), got = dusp::pcm_quantise(x, g, S);
    cases++;
    if (want != got) {
        if (bad < 8) std::fprintf(stderr, "x %a g %a S %.0f: want %d got %d\n", x, g, S, want, got);
        bad++;
    }
}
static void around(float f, double g, double S) {
    float lo = f, hi = f;
    check(f, g, S);
    check(-f, g, S);
    for (int k = 0; k < 2; k++) {
        lo = std::nextafterf(lo, -INFINITY);
        hi = std::nextafterf(hi, INFINITY);
        check(lo, g, S), check(-lo, g, S), check(hi, g, S), check(-hi, g, S);
    }
}
static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t xr() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 3000000;
    const float peaks[] = {1.0000001f, 1.7f, 3.25f, 0.3f, 1.0e-3f, 7.0f};
    double gains[8] = {1.0, 0.5};
    int n_gains = 2;
    for (float p : peaks) {
        uint32_t b;
        std::memcpy(&b, &p, 4);
        gains[n_gains++] = dusp::pcm_gain(b, dusp::kNormaliseFull);
    }
    const double scales[2] = {dusp::kPcmScaleS16, dusp::kPcmScaleS24};
    for (int si = 0; si < 2; si++) {
        const double S = scales[si];
        const long K = (long)S, stride = si == 0 ? 1 : 257;
        for (int gi = 0; gi < n_gains; gi++) {
            const double g = gains[gi];
            for (long k = 0; k <= K; k += (k > K - 4 * stride || k < 4 * stride) ? 1 : stride) around((float)(((double)k + 0.5) / S / g), g, S);
            const float specials[] = {0.f, -0.f, 1.f, -1.f, 2.f, -2.f, 1e30f, NAN, INFINITY, -INFINITY, 1e-45f, 1.17549435e-38f, (float)(1.0 / g), (float)(0.5 / S)};
            for (float s : specials) around(s, g, S);
            for (long i = 0; i < n_random / (2 * n_gains); i++) {
                uint32_t b = (uint32_t)xr();
                if (i & 1) b = (b & 0x807fffffu) | ((uint32_t)(100 + xr() % 30) << 23);  // 2^-27 .. 2^2: where the samples are
                float x;
                std::memcpy(&x, &b, 4);
                check(x, g, S);
            }
        }
    }
    // the gains themselves: none / clip / full, at and around 1, zero, NaN, infinity
    const float ps[] = {0.f, 0.5f, 1.f, 1.0000001f, 3.f, INFINITY, NAN};
    for (float p : ps)
        for (int mode = 0; mode < 3; mode++) {
            uint32_t b;
            std::memcpy(&b, &p, 4);
            const double want = mode == 0 || !(p == p) || std::isinf(p) || !(p > (mode == 1 ? 1.f : 0.f)) ? 1.0 : 1.0 / (double)p;
            cases++;
            if (dusp::pcm_gain(b, mode) != want) bad++;
        }
    std::printf("{\"cases\": %ld, \"bad\": %ld}\n", cases, bad);
    return bad ? 1 : 0;
}
