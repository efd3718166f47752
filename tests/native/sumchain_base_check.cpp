// dusp_amd/csrc/modmath.hpp on the CPU: the integer helpers every jump-ahead path shares (addmod, mulmod, mod_u32, mod_u64, jit_mulmod)
// and the sum chain's block base, each against unsigned __int128 — at every modulus in use (sampleRate << 32 and sampleRate << 36 for the
// rates of the sample-rate matrix, plus 2^17) and with operands at the edges: x next to 2^64, next to multiples of m, block counts at and
// around 2^32 / sampleRate, 65535 and 2^30.  Then the sum chain's voice records as the host builds them (fused_plan.hpp build_sum_voices)
// followed through the kernel's own steps to the phase of (window, block, lane), against (P0 + (t + 1) F) mod S in 128-bit integers.
// Prints one JSON line.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dusp_amd/csrc/fused_plan.hpp"
#include "../../dusp_amd/csrc/modmath.hpp"

using namespace dusp;
typedef unsigned __int128 u128;

static long g_cases = 0, g_bad = 0;
static long n_mod64 = 0, n_mod32 = 0, n_mulmod = 0, n_jit = 0, n_base = 0, n_base_int = 0, n_voice = 0, n_product_past_64 = 0;

static void expect(const char *what, uint64_t got, uint64_t want, uint64_t a, uint64_t b, uint64_t m) {
    g_cases++;
    if (got != want && g_bad++ < 40)
        std::printf("FAIL: %s(%llu, %llu; m = %llu): %llu, expected %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)m,
                    (unsigned long long)got, (unsigned long long)want);
}

static const uint32_t kRates[] = {8000, 11025, 22050, 32000, 44100, 48000, 88200, 96000, 131072, 192000};

// values around v: v - 2 .. v + 2 (wrapping at 2^64: the edge itself is a case)
static void around(std::vector<uint64_t> &out, uint64_t v) {
    for (int d = -2; d <= 2; d++) out.push_back(v + (uint64_t)(int64_t)d);
}

// x at the edges for a modulus m: small, next to 2^32, 2^53, 2^63 and 2^64, next to multiples of m — the largest ones below 2^64 included
static std::vector<uint64_t> edge_x(uint64_t m) {
    std::vector<uint64_t> x;
    around(x, 2);
    around(x, (uint64_t)1 << 32);
    around(x, (uint64_t)1 << 53);
    around(x, (uint64_t)1 << 63);
    around(x, ~(uint64_t)0 - 2);  // ... 2^64 - 1, and past it 0 and 1
    for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)255, (uint64_t)65535, (uint64_t)1 << 20}) {
        const u128 p = (u128)m * k;
        if (p < ((u128)1 << 64)) around(x, (uint64_t)p);
    }
    const uint64_t top = ~(uint64_t)0 / m;  // the largest multiples of m below 2^64
    for (uint64_t k = 0; k < 3 && k < top; k++) around(x, (top - k) * m);
    for (int s = 1; s < 64; s += 3) x.push_back(((uint64_t)0x9e3779b97f4a7c15ull >> s) | 1);
    return x;
}

static void check_modulus(uint64_t m, bool jit) {
    const double inv_m = 1.0 / (double)m;
    const std::vector<uint64_t> xs = edge_x(m);
    for (uint64_t x : xs) {
        expect("mod_u64", mod_u64(x, m, inv_m), x % m, x, 0, m);
        n_mod64++;
    }
    // residues at the edges, for the functions that take operands below m
    std::vector<uint64_t> rs = {0, 1, 2, m / 2 - 1, m / 2, m / 2 + 1, m - 2, m - 1, (m / 3) | 1, (uint64_t)(((u128)m * 0x9e3779b9u) >> 32)};
    std::vector<uint64_t> ns = {0, 1, 2, 3, 4, 255, 256, 257, 65535, 65536, (uint64_t)1 << 30, ((uint64_t)1 << 32) - 1};
    for (uint32_t sr : kRates) around(ns, ((uint64_t)1 << 32) / sr);
    for (uint64_t a : rs) {
        for (uint64_t b : rs) expect("addmod", addmod(a, b, m), (uint64_t)(((u128)a + b) % m), a, b, m);
        for (uint64_t n : ns) {
            const uint64_t want = (uint64_t)(((u128)a * n) % m);
            expect("mulmod", mulmod(a, n, m), want, a, n, m);
            n_mulmod++;
            if (jit) {
                expect("jit_mulmod", jit_mulmod(a, n, m, inv_m), want, a, n, m);
                n_jit++;
            }
        }
        for (uint64_t n : {(uint64_t)1 << 40, ((uint64_t)1 << 40) + 2048, ~(uint64_t)0}) expect("mulmod", mulmod(a, n, m), (uint64_t)(((u128)a * n) % m), a, n, m);
    }
}

static void check_mod_u32(uint32_t m) {
    const double inv_m = 1.0 / (double)m;
    std::vector<uint64_t> xs;
    around(xs, 2);
    around(xs, (uint64_t)1 << 31);
    around(xs, ((uint64_t)1 << 32) - 3);
    for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)64, (uint64_t)65535}) around(xs, (uint64_t)m * k);
    around(xs, (uint64_t)(0xffffffffu / m) * m);
    for (uint64_t x : xs) {
        if (x >> 32) continue;
        expect("mod_u32", mod_u32((uint32_t)x, m, inv_m), (uint32_t)x % m, x, 0, m);
        n_mod32++;
    }
}

// The block base at the edges of its operands: B0, bs below S = sr << 32, every block count a launch can have (below 2^16), first the
// function alone, then the INT path's 32-bit form inside the range its launch condition admits — and one block past it the condition
// must say no.
static void check_block_base(uint32_t sr) {
    const uint64_t S = (uint64_t)sr << 32;
    const double inv_S = 1.0 / (double)S, inv_sr = 1.0 / (double)sr;
    const std::vector<uint64_t> rs = {0, 1, S / 2, S - 1, S - 2, ((uint64_t)(sr - 1) << 32) | 0x80000000u, (uint64_t)(((u128)S * 0x9e3779b9u) >> 32)};
    std::vector<uint64_t> blks = {0, 1, 255, 256, 257, 511, 512, 32767, 32768, 65279, 65280, 65534, 65535};
    for (int d = -2; d <= 2; d++) {
        const uint64_t w = ((uint64_t)1 << 32) / sr + (uint64_t)(int64_t)d;
        if (w < 65536) blks.push_back(w);
    }
    for (uint64_t B0 : rs)
        for (uint64_t bs : rs) {
            const uint64_t bs256 = (uint64_t)(((u128)bs * 256) % S);
            for (uint64_t blk : blks) {
                const u128 exact = (u128)B0 + (u128)blk * bs;
                if (exact >> 64) n_product_past_64++;  // what the plain 64-bit product would have lost
                expect("sum_block_base", sum_block_base(B0, bs, bs256, (uint32_t)blk, S, inv_S), (uint64_t)(exact % S), B0, blk, S);
                n_base++;
            }
        }
    uint32_t most = 0;  // the most blocks the INT path takes at this rate
    for (uint32_t n = 65535; n > 0 && !most; n--)
        if (sum_int_blocks_ok(n, sr)) most = n;
    g_cases++;
    if (!most || ((uint64_t)most + 1) * sr >= ((uint64_t)1 << 32) || (most < 65535 && ((uint64_t)most + 2) * sr < ((uint64_t)1 << 32)))
        g_bad++, std::printf("FAIL: sum_int_blocks_ok at %u Hz turns at %u blocks\n", sr, most);
    for (uint32_t B0 : {0u, 1u, sr / 2, sr - 1})
        for (uint32_t bs : {0u, 1u, sr / 2, sr - 1})
            for (uint32_t blk : {0u, 1u, most / 2, most - 2, most - 1}) {
                expect("sum_block_base_int", sum_block_base_int(B0, bs, blk, sr, inv_sr), (uint32_t)(((uint64_t)B0 + (uint64_t)blk * bs) % sr), B0, blk, sr);
                n_base_int++;
            }
}

// A voice of a chain from its plan to the phase of one sample, the way sumchain_engine.hip's 32.32 path gets there: build_sum_voices,
// the block base, the lane's offset, c increments of Fm.
static void check_voice(uint32_t sr, double f, int gb, uint64_t first, uint32_t blk) {
    FusedPlan plan;
    plan.kind = FUSED_SUMCHAIN;
    plan.sum_f.push_back(std::fmod(f, (double)sr));
    plan.sum_phase0.push_back(0.0);
    std::vector<SumVoice> voices;
    std::vector<double> end;
    const uint64_t T_end = first + ((uint64_t)blk + 1) * (uint64_t)gb * kChunk;
    build_sum_voices(plan, sr, gb, first, T_end, voices, end);
    g_cases++;
    if (voices.size() != sum_voice_slots(1)) g_bad++, std::printf("FAIL: %zu slots for one voice\n", voices.size());
    uint64_t bs256;  // behind the records
    std::memcpy(&bs256, voices.data() + 1, sizeof bs256);
    const SumVoice &rc = voices[0];
    const uint64_t S = (uint64_t)sr << 32;
    const double inv_S = 1.0 / (double)S;
    const long long F = (long long)std::ldexp(plan.sum_f[0], 32);
    const uint64_t Fm = F >= 0 ? (uint64_t)F : S - (uint64_t)(-F);
    const uint64_t base = sum_block_base(rc.B0, rc.bs, bs256, blk, S, inv_S);
    for (uint32_t lane : {0u, 1u, 31u, 63u}) {
        uint64_t P = mod_u64(base + (uint64_t)lane * rc.step4, S, inv_S);
        for (uint32_t c = 0; c < 4; c++) {
            const u128 t = (u128)first + (u128)blk * (uint64_t)(gb * kChunk) + lane * 4 + c;
            expect("voice phase", P, (uint64_t)(((u128)Fm * (t + 1)) % S), first, blk, S);
            n_voice++;
            P += rc.Fm;
            if (P >= S) P -= S;
        }
    }
    g_cases++;
    if (end[0] != std::ldexp((double)(uint64_t)(((u128)Fm * T_end) % S), -32)) g_bad++, std::printf("FAIL: end phase at %u Hz, f = %g\n", sr, f);
}

int main() {
    for (uint32_t sr : kRates) {
        check_modulus((uint64_t)sr << 32, true);
        check_modulus((uint64_t)sr << 36, sr <= 131072);  // (jit_mulmod: S <= 2^53, the compiled kernels' rates)
        check_mod_u32(sr);
        check_block_base(sr);
    }
    check_modulus((uint64_t)1 << 17, true);
    check_mod_u32(1u << 17);

    for (uint32_t sr : kRates)
        for (double f : {10.0, 20.125, 440.5, (double)12345.678f, -3.25, (double)sr - 0.5})
            for (int gb : {4, 8}) {
                const uint64_t S = (uint64_t)sr << 32, B = (uint64_t)gb * kChunk;
                const double fr = std::fmod(f, (double)sr);
                const long long F = (long long)std::ldexp(fr, 32);
                const uint64_t bs = (uint64_t)(((u128)(F >= 0 ? (uint64_t)F : S - (uint64_t)(-F)) * B) % S);
                std::vector<uint64_t> firsts = {0, 2048, (uint64_t)1 << 24, (uint64_t)1 << 32, (uint64_t)1 << 36, ((uint64_t)1 << 40) - 2048, (uint64_t)1 << 40};
                if (bs) {  // where the 64-bit product blk * bs of blocks counted from sample 0 passed 2^64
                    const uint64_t wrap = (uint64_t)((((u128)1 << 64) / bs));
                    if (wrap >= 2 && wrap < ((uint64_t)1 << 30)) firsts.push_back((wrap - 2) * B / 2048 * 2048), firsts.push_back((wrap + 1) * B / 2048 * 2048);
                }
                for (uint64_t first : firsts)
                    for (uint32_t blk : {0u, 1u, 2u, 255u, 256u, (uint32_t)(((uint64_t)1 << 32) / sr), 65535u})
                        if (blk < 65536) check_voice(sr, f, gb, first, blk);
            }

    std::printf("{\"cases\": %ld, \"bad\": %ld, \"mod_u64\": %ld, \"mod_u32\": %ld, \"mulmod\": %ld, \"jit_mulmod\": %ld, \"block_base\": %ld, \"block_base_int\": %ld, "
                "\"voice_phases\": %ld, \"products_past_2_64\": %ld}\n",
                g_cases, g_bad, n_mod64, n_mod32, n_mulmod, n_jit, n_base, n_base_int, n_voice, n_product_past_64);
    return g_bad ? 1 : 0;
}
