// modmath.hpp — exact modular arithmetic on fixed-point phases: what every jump-ahead path (the fused voices, the sum chain, the wave
// engine's time segments, the compiled circuit kernels) stands on when it goes to sample t without walking there.  Host and device,
// like repeat_add.hpp: hipcc compiles it into the library's kernels, hiprtc compiles it again at run time into the per-circuit
// kernels (jit_engine.hip embeds this file's text), and tests/native/sumchain_base_check.cpp pins every function against
// unsigned __int128 on the CPU.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <cstdint>
#endif

#if !defined(DUSP_HOST_DEVICE)
#if defined(__HIPCC__)
#define DUSP_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define DUSP_HOST_DEVICE inline
#endif
#endif

namespace dusp {
namespace {

DUSP_HOST_DEVICE uint64_t addmod(uint64_t a, uint64_t b, uint64_t S) {  // a, b < S < 2^63
    const uint64_t s = a + b;
    return s >= S ? s - S : s;
}
DUSP_HOST_DEVICE uint64_t mulmod(uint64_t a, uint64_t n, uint64_t S) {  // a < S
    uint64_t acc = 0;
    for (int bit = 63 - __builtin_clzll(n | 1); bit >= 0; --bit) {
        acc = addmod(acc, acc, S);
        if ((n >> bit) & 1) acc = addmod(acc, a, S);
    }
    return acc;
}

DUSP_HOST_DEVICE uint32_t mod_u32(uint32_t x, uint32_t m, double inv_m) {
    const uint32_t q = (uint32_t)((double)x * inv_m);
    uint32_t r = x - q * m;
    if ((int32_t)r < 0) r += m;
    if (r >= m) r -= m;
    return r;
}
// x mod m for any x < 2^64 and 2^16 <= m < 2^54 (inv_m = RN(1 / m)): the quotient estimated in f64 is off by at most 2 either way —
// (double)x and inv_m carry a relative error of 2^-53 each and the product one more, together below 2^-51 of a quotient below 2^48
// — and the two corrections each way take that up.  (The moduli in use are sampleRate << 32 and sampleRate << 36: up to 2^53.6.)
DUSP_HOST_DEVICE uint64_t mod_u64(uint64_t x, uint64_t m, double inv_m) {
    const uint64_t q = (uint64_t)((double)x * inv_m);
    uint64_t r = x - q * m;
    if ((int64_t)r < 0) r += m;
    if ((int64_t)r < 0) r += m;
    if (r >= m) r -= m;
    if (r >= m) r -= m;
    return r;
}

// (a * n) mod S for a < S <= 2^53 and n < 2^32, exactly: the product is cut into pieces that mod_u64 (x < 2^64) can take.  (S = sampleRate
// << 36 of the compiled kernels, whose rates end at 2^17; at 192 kHz r << 11 below would pass 2^64.)
DUSP_HOST_DEVICE unsigned long long jit_mulmod(unsigned long long a, unsigned long long n, unsigned long long S, double inv_S) {
    const unsigned long long ah = a >> 32, al = a & 0xffffffffull;  // ah < 2^21
    unsigned long long r = mod_u64(ah * n, S, inv_S);               // (ah n) < 2^53; now r 2^32 mod S in three shifts of <= 11 bits
    r = mod_u64(r << 11, S, inv_S);
    r = mod_u64(r << 11, S, inv_S);
    r = mod_u64(r << 10, S, inv_S);
    return addmod(r, mod_u64(al * n, S, inv_S), S);
}

// The sum chain's block base: the 32.32 phase (B0 + blk * bs) mod S of a voice at block blk of a launch, for B0, bs < S < 2^50 and
// blk < 2^16 counted from the LAUNCH's first block (the host has folded the window's place in the timeline into B0).  blk * bs alone
// passes 2^64 from blk ~ 2^32 / sampleRate on, so the block count goes in as two digits of 8 bits: bs256 = (256 bs) mod S comes
// from the host beside the voice's record, both products stay below 2^58 and the sum below 2^60.
DUSP_HOST_DEVICE uint64_t sum_block_base(uint64_t B0, uint64_t bs, uint64_t bs256, uint32_t blk, uint64_t S, double inv_S) {
    return mod_u64(B0 + (uint64_t)(blk >> 8) * bs256 + (uint64_t)(blk & 255u) * bs, S, inv_S);
}
// ... and on the INT path (every phase a whole table step: the records' high words), (B0 + blk * bs) mod sampleRate in 32 bits: the
// launch takes it only while (n_blocks + 1) * sampleRate < 2^32 (sum_int_blocks_ok).
DUSP_HOST_DEVICE uint32_t sum_block_base_int(uint32_t B0, uint32_t bs, uint32_t blk, uint32_t sr, double inv_sr) {
    return mod_u32(B0 + blk * bs, sr, inv_sr);
}
DUSP_HOST_DEVICE bool sum_int_blocks_ok(uint32_t n_blocks, uint32_t sr) { return ((uint64_t)n_blocks + 1) * sr < (1ull << 32); }

}  // namespace
}  // namespace dusp
