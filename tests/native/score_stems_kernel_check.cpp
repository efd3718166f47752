// score_stems_kernel_check.cpp — the text of the STEMS instances of dusp_amd/csrc/score_tracks_engine.hip's mix kernel and of
// score_send_engine.hip's return kernel, and of pcm_peak_common.hpp, compiled for the HOST (hip_host_stub/: lanes one after the other)
// and held on bit patterns
//   * to a plain loop over the contract (dusp_amd/mix.py track_terms, track_mix, bus_return, stems): the slots are direct || 0,
//     term_g || 0 and every wet as it is, the mix and the feeds what they were;
//   * to the instances WITHOUT stems of the same two templates (a launch without slots) over the same inputs: mix and feeds bit for bit.
// EVERY BUFFER IS A HEAP ALLOCATION OF EXACTLY ITS SIZE behind its offset, so under AddressSanitizer one float read or written outside
// a buffer is reported.
// Covered, mix kernel: n = 1, 3, 4, 5, 1027, 4636 floats; T = 0 .. 8; B = 0 .. 4; with and without faders; raw and not; out of place
// and in place (out = direct); feeds from +0; every buffer on a 16-byte boundary (four floats a lane and a scalar tail — with n % 4 != 0
// the slots behind the first are off it and the launch must see that) and off (one float a lane); planted NaN, Inf, -0, subnormals.
// Return kernel: the same n; B = 0 .. 4; with and without a direct slot; raw and not; in place (out = dry) and not; on and off
// boundaries.  Then two launches of the mix kernel with more items than the grid has lanes (the stride), wide and narrow.  The common
// peak: n = 1 .. 70 words, NaN patterns included.
// Built with -fsanitize=address,undefined by tests/test_stems_host.py.
// Prints {"cases": n, "bad": m, "wide": w, "narrow": s, "strided": g, "old": o}.
#include "../../dusp_amd/csrc/score_tracks_engine.hip"
#include "../../dusp_amd/csrc/score_send_engine.hip"
#include "../../dusp_amd/csrc/pcm_peak_common.hpp"
#include <algorithm>
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
static long checked = 0, bad = 0, wide = 0, narrow = 0, strided = 0, old_held = 0;
static std::mt19937 rng(17);
static std::normal_distribution<float> nd;
static void plant(float *p, size_t len, int j) {
    for (size_t k = 0; k < len; k++)
        p[k] = k % 17 == 3 ? -0.0f : k % 19 == 4 ? NAN : k % 23 == 5 ? ((j & 1) ? INFINITY : -INFINITY) : k % 29 == 6 ? 5e-39f : k % 31 == 7 ? FLT_MAX : nd(rng);
}

static void mix_case(size_t n, int T, int B, int faders, int raw, int in_place, int aligned) {
    const float fixed[] = {0.0f, -0.0f, 1.0f, -0.75f, 1e-30f, 3e20f, 0.6f};
    Buf direct, direct_old, out, out_old, tracks[8], feed_out, feed_old, stems;
    bool got = direct.make(n, aligned ? 0 : 1) && direct_old.make(n, aligned ? 0 : 1) && out.make(n, aligned ? 0 : 2) && out_old.make(n, aligned ? 0 : 2);
    for (int g = 0; g < T; g++) got &= tracks[g].make(n, aligned ? 0 : (size_t)(1 + g % 3));
    got &= feed_out.make((size_t)std::max(B, 1) * n, aligned ? 0 : 1) && feed_old.make((size_t)std::max(B, 1) * n, aligned ? 0 : 1) && stems.make((size_t)(1 + T) * n, aligned ? 0 : 3);
    if (!got) { bad++; return; }
    plant(direct.p, n, 0);
    for (int g = 0; g < T; g++) plant(tracks[g].p, n, g + 1);
    if (n > 2 && T > 0) { direct.p[2] = 1.0f; tracks[0].p[2] = -1.0f; }  // (a sum that is -0 or +0 by the order)
    memcpy(direct_old.p, direct.p, n * 4);
    float fader[8], level[4 * 8];
    for (int g = 0; g < T; g++) {
        const unsigned lk = rng() % 12;
        fader[g] = lk < 7 ? fixed[lk] : (float)(rng() % 2001) / 1000.f - 1.0f;
    }
    for (int j = 0; j < B * T; j++) {
        const unsigned lk = rng() % 12;
        level[j] = lk < 7 ? fixed[lk] : (float)(rng() % 2001) / 1000.f - 1.0f;
    }
    std::vector<float> want(n), fwant((size_t)std::max(B, 1) * n), swant((size_t)(1 + T) * n);
    for (size_t p = 0; p < n; p++) {
        volatile float acc = direct.p[p];
        swant[p] = or0(acc);
        volatile float f[4];
        for (int b = 0; b < B; b++) f[b] = 0.0f;
        for (int g = 0; g < T; g++) {
            volatile float term = tracks[g].p[p];
            if (faders) term = term * fader[g];
            swant[(size_t)(1 + g) * n + p] = or0(term);
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
    float *slots[8];
    for (int g = 0; g < T; g++) ptrs[g] = tracks[g].p, slots[g] = stems.p + (size_t)(1 + g) * n;
    float *o = in_place ? direct.p : out.p;
    const hipError_t err = dusp::launch_score_tracks(direct.p, ptrs, faders ? fader : nullptr, B ? level : nullptr, (uint32_t)T, (uint32_t)B, o, nullptr, B ? feed_out.p : nullptr,
                                                     stems.p, slots, n, raw, nullptr);
    const unsigned grid = g_last_grid;
    bool ok = err == hipSuccess && same_bits(o, want.data(), n) && (B == 0 || same_bits(feed_out.p, fwant.data(), (size_t)B * n)) && same_bits(stems.p, swant.data(), (size_t)(1 + T) * n);
    if (T > 0) {  // the instance without stems over the same inputs: its mix and feeds, bit for bit (memcmp: NaN payloads too)
        float *oo = in_place ? direct_old.p : out_old.p;
        const hipError_t e2 = dusp::launch_score_tracks(direct_old.p, ptrs, faders ? fader : nullptr, B ? level : nullptr, (uint32_t)T, (uint32_t)B, oo, nullptr, B ? feed_old.p : nullptr, nullptr, nullptr, n, raw, nullptr);
        ok &= e2 == hipSuccess && memcmp(oo, o, n * 4) == 0 && (B == 0 || memcmp(feed_old.p, feed_out.p, (size_t)B * n * 4) == 0);
        old_held++;
    }
    checked++;
    // which path the launch took: the wide one needs every buffer, each feed and each slot included, on a 16-byte boundary
    const bool all_aligned = aligned && ((B <= 1 && T == 0) || n % 4 == 0);
    (all_aligned && n >= 4 ? wide : narrow)++;
    strided += (uint64_t)grid * 256 < (all_aligned ? n / 4 + n % 4 : n);
    if (!ok) { bad++; if (bad < 20) printf("MISMATCH mix n %zu T %d B %d faders %d raw %d in_place %d aligned %d\n", n, T, B, faders, raw, in_place, aligned); }
}

static void return_case(size_t n, int B, int with_direct, int raw, int in_place, int aligned) {
    Buf dry, dry_old, out, out_old, wets[4], slot_direct, slot_buses;
    bool got = dry.make(n, aligned ? 0 : 1) && dry_old.make(n, aligned ? 0 : 1) && out.make(n, aligned ? 0 : 2) && out_old.make(n, aligned ? 0 : 2) && slot_direct.make(n, aligned ? 0 : 3) &&
               slot_buses.make((size_t)std::max(B, 1) * n, aligned ? 0 : 1);
    for (int b = 0; b < B; b++) got &= wets[b].make(n, aligned ? 0 : (size_t)(1 + b % 3));
    if (!got) { bad++; return; }
    plant(dry.p, n, 0);
    for (int b = 0; b < B; b++) plant(wets[b].p, n, b + 1);
    memcpy(dry_old.p, dry.p, n * 4);
    std::vector<float> want(n), dwant(n);
    for (size_t p = 0; p < n; p++) {
        volatile float acc = dry.p[p];
        dwant[p] = or0(acc);
        for (int b = 0; b < B; b++) acc = acc + wets[b].p[p];
        want[p] = raw ? (float)acc : or0(acc);
    }
    const float *ptrs[4];
    float *slots[4];
    for (int b = 0; b < B; b++) ptrs[b] = wets[b].p, slots[b] = slot_buses.p + (size_t)b * n;
    float *o = in_place ? dry.p : out.p, *oo = in_place ? dry_old.p : out_old.p;
    const hipError_t err = dusp::launch_score_return(dry.p, ptrs, (uint32_t)B, o, with_direct ? slot_direct.p : nullptr, slots, n, raw, nullptr);
    const hipError_t e2 = dusp::launch_score_return(dry_old.p, ptrs, (uint32_t)B, oo, nullptr, nullptr, n, raw, nullptr);
    bool ok = err == hipSuccess && e2 == hipSuccess && same_bits(o, want.data(), n) && memcmp(o, oo, n * 4) == 0 && (!with_direct || same_bits(slot_direct.p, dwant.data(), n));
    for (int b = 0; b < B; b++) ok &= memcmp(slots[b], wets[b].p, n * 4) == 0;  // (a copy: NaN payloads and -0 as they are)
    old_held++;
    checked++;
    const bool all_aligned = aligned && (B <= 1 || n % 4 == 0);
    (all_aligned && n >= 4 ? wide : narrow)++;
    if (!ok) { bad++; if (bad < 20) printf("MISMATCH return n %zu B %d direct %d raw %d in_place %d aligned %d\n", n, B, with_direct, raw, in_place, aligned); }
}

static void common_case(uint32_t n) {
    Buf peaks, common;
    if (!peaks.make(n, 0) || !common.make(n, 1)) { bad++; return; }
    uint32_t want = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t w = (rng() % 5 == 0 ? 0x7fc00000u | (rng() & 0xffff) : rng()) & 0x7fffffffu;  // (NaN patterns sort above infinity)
        memcpy(&peaks.p[i], &w, 4);
        want = std::max(want, w);
    }
    const hipError_t err = dusp::launch_pcm_peak_common(peaks.p, common.p, n, nullptr);
    bool ok = err == hipSuccess;
    for (uint32_t i = 0; i < n; i++) ok &= memcmp(&common.p[i], &want, 4) == 0;
    checked++;
    if (!ok) { bad++; printf("MISMATCH common n %u\n", n); }
}

int main() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)1027, (size_t)4636})
        for (int T = 0; T <= 8; T++) for (int B = 0; B <= 4; B++) for (int faders : {0, 1}) for (int raw : {0, 1}) for (int in_place : {0, 1}) for (int aligned : {0, 1}) {
            if (T == 0 && faders) continue;
            if (n > 1000 && (T + B + faders + raw + in_place + aligned) % 3 != 0) continue;  // (a third of the long ones: every axis still meets every other)
            mix_case(n, T, B, faders, raw, in_place, aligned);
        }
    for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)1027, (size_t)4636})
        for (int B = 0; B <= 4; B++) for (int with_direct : {0, 1}) for (int raw : {0, 1}) for (int in_place : {0, 1}) for (int aligned : {0, 1})
            return_case(n, B, with_direct, raw, in_place, aligned);
    // more items than the grid's 2048 x 256 lanes: a lane takes a second item a stride away, four floats (and the tail) and one
    mix_case((size_t)4 * 2048 * 256 + 4 * 300, 2, 1, 1, 0, 1, 1);
    mix_case((size_t)2048 * 256 + 77, 0, 0, 0, 1, 0, 0);
    for (uint32_t n = 1; n <= 70; n += (n < 16 ? 1 : 9)) common_case(n);
    printf("{\"cases\": %ld, \"bad\": %ld, \"wide\": %ld, \"narrow\": %ld, \"strided\": %ld, \"old\": %ld}\n", checked, bad, wide, narrow, strided, old_held);
    return bad != 0;
}
