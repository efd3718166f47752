// score_tracks_kernel_check.cpp — the text of dusp_amd/csrc/score_tracks_engine.hip compiled for the HOST (hip_host_stub/: lanes one
// after the other) and held on bit patterns to a plain loop over the contract (dusp_amd/mix.py track_mix): mix = direct, then for every
// track in order term = y * fader (or y), mix = f32(mix + term), feed_b = f32(feed_b + f32(term * level[b][g])) — a level of 0
// included — `|| 0` on the mix unless raw, the feeds raw.  EVERY BUFFER IS A HEAP ALLOCATION OF EXACTLY ITS SIZE behind its offset, so
// under AddressSanitizer one float read or written outside a buffer is reported.
// Covered: n = 1, 3, 4, 5, 1027 and 4634 floats; T = 1 .. 8; B = 0 .. 4; with and without faders; raw and not; out of place and in
// place (out = direct, feed_out = feed_init); feeds that start at +0, from a second buffer and in place; buffers on 16-byte boundaries
// (four floats a lane and a scalar tail; with B > 0 and n % 4 != 0 the feeds behind the first are not aligned and the launch must see
// it) and off them (one float a lane); planted NaN, Inf, -0 and subnormals; levels and faders 0, -0, 1, negative, tiny and huge.  Then
// two launches of more items than the grid has lanes (the stride), wide and narrow.
// Built with -fsanitize=address,undefined by tests/test_tracks_host.py.
// Prints {"cases": n, "bad": m, "wide": w, "narrow": s, "strided": g}.
#include "../../dusp_amd/csrc/score_tracks_engine.hip"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
static float or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }
static bool same_bits(const float *a, const float *b, size_t n) {
    bool ok = true;
    for (size_t p = 0; p < n; p++) ok &= (b[p] != b[p]) ? (a[p] != a[p]) : memcmp(&a[p], &b[p], 4) == 0;
    return ok;
}
struct Buf {  // exactly n floats behind `skip` floats of a 16-byte aligned allocation: one float past them is the sanitizer's
    void *mem = nullptr;
    float *p = nullptr;
    bool make(size_t n, size_t skip) {
        if (posix_memalign(&mem, 16, (n + skip) * 4) != 0) return false;
        p = (float *)mem + skip;
        return true;
    }
    ~Buf() { free(mem); }
};
static long checked = 0, bad = 0, wide = 0, narrow = 0, strided = 0;
static std::mt19937 rng(16);

static void one_case(size_t n, int T, int B, int faders, int raw, int in_place, int feed_mode, int aligned) {
    std::normal_distribution<float> nd;
    const float fixed[] = {0.0f, -0.0f, 1.0f, -0.75f, 1e-30f, 3e20f, 0.6f};
    Buf direct, out, tracks[8], feed_in, feed_out;
    bool got = direct.make(n, aligned ? 0 : 1) && out.make(n, aligned ? 0 : 2);
    for (int g = 0; g < T; g++) got &= tracks[g].make(n, aligned ? 0 : (size_t)(1 + g % 3));
    got &= feed_in.make((size_t)std::max(B, 1) * n, aligned ? 0 : 3) && feed_out.make((size_t)std::max(B, 1) * n, aligned ? 0 : 1);
    if (!got) { bad++; return; }
    auto plant = [&](float *p, size_t len, int j) {
        for (size_t k = 0; k < len; k++)
            p[k] = k % 17 == 3 ? -0.0f : k % 19 == 4 ? NAN : k % 23 == 5 ? ((j & 1) ? INFINITY : -INFINITY) : k % 29 == 6 ? 5e-39f : k % 31 == 7 ? FLT_MAX : nd(rng);
    };
    plant(direct.p, n, 0);
    for (int g = 0; g < T; g++) plant(tracks[g].p, n, g + 1);
    plant(feed_in.p, (size_t)std::max(B, 1) * n, 9);
    if (n > 2) { direct.p[2] = 1.0f; tracks[0].p[2] = -1.0f; }  // (a sum that is -0 or +0 by the order)
    float fader[8], level[4 * 8];
    for (int g = 0; g < T; g++) {
        const unsigned lk = rng() % 12;
        fader[g] = lk < 7 ? fixed[lk] : (float)(rng() % 2001) / 1000.f - 1.0f;
    }
    for (int j = 0; j < B * T; j++) {
        const unsigned lk = rng() % 12;
        level[j] = lk < 7 ? fixed[lk] : (float)(rng() % 2001) / 1000.f - 1.0f;
    }
    std::vector<float> want(n), fwant((size_t)std::max(B, 1) * n);
    for (size_t p = 0; p < n; p++) {
        volatile float acc = direct.p[p];
        volatile float f[4];
        for (int b = 0; b < B; b++) f[b] = feed_mode ? feed_in.p[(size_t)b * n + p] : 0.0f;
        for (int g = 0; g < T; g++) {
            volatile float term = tracks[g].p[p];
            if (faders) term = term * fader[g];
            acc = acc + term;
            for (int b = 0; b < B; b++) {
                volatile float part = term * level[b * T + g];
                f[b] = f[b] + part;
            }
        }
        want[p] = raw ? (float)acc : or0(acc);
        for (int b = 0; b < B; b++) fwant[(size_t)b * n + p] = f[b];
    }
    const float *ptrs[8];
    for (int g = 0; g < T; g++) ptrs[g] = tracks[g].p;
    float *o = in_place ? direct.p : out.p;
    const float *fi = feed_mode == 0 ? nullptr : feed_in.p;
    float *fo = B == 0 ? nullptr : feed_mode == 2 ? feed_in.p : feed_out.p;
    const hipError_t err = dusp::launch_score_tracks(direct.p, ptrs, faders ? fader : nullptr, B ? level : nullptr, (uint32_t)T, (uint32_t)B, o, B ? fi : nullptr, fo, nullptr, nullptr, n, raw, nullptr);
    const bool ok = err == hipSuccess && same_bits(o, want.data(), n) && (B == 0 || same_bits(fo, fwant.data(), (size_t)B * n));
    checked++;
    // which path the launch took: the wide one needs every buffer, each feed included, on a 16-byte boundary
    const bool all_aligned = aligned && (B <= 1 || n % 4 == 0);
    (all_aligned && n >= 4 ? wide : narrow)++;
    strided += (uint64_t)g_last_grid * 256 < (all_aligned ? n / 4 + n % 4 : n);
    if (!ok) { bad++; if (bad < 20) printf("MISMATCH n %zu T %d B %d faders %d raw %d in_place %d feed %d aligned %d\n", n, T, B, faders, raw, in_place, feed_mode, aligned); }
}

int main() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)1027, (size_t)4634, (size_t)4636})
        for (int T = 1; T <= 8; T++) for (int B = 0; B <= 4; B++) for (int faders : {0, 1}) for (int raw : {0, 1})
            for (int in_place : {0, 1}) for (int feed_mode : {0, 1, 2}) for (int aligned : {0, 1}) {
                if (B == 0 && feed_mode) continue;
                if (n > 1000 && (T + B + faders + raw + in_place + feed_mode + aligned) % 3 != 0) continue;  // (a third of the long ones: every axis still meets every other)
                one_case(n, T, B, faders, raw, in_place, feed_mode, aligned);
            }
    // more items than the grid's 2048 x 256 lanes: a lane takes a second item a stride away, four floats (and the tail) and one
    one_case((size_t)4 * 2048 * 256 + 4 * 300 + 3, 2, 1, 1, 0, 1, 2, 1);
    one_case((size_t)2048 * 256 + 77, 3, 2, 0, 1, 0, 0, 0);
    printf("{\"cases\": %ld, \"bad\": %ld, \"wide\": %ld, \"narrow\": %ld, \"strided\": %ld}\n", checked, bad, wide, narrow, strided);
    return bad != 0;
}
