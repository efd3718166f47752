// mix_engine.hip — the mix of a batch of rendered voices, on the device, in Sum.many's chain order.
//
// The reference mixes voices with `Sum.many(voices)`: a left-deep chain ((v0 + v1) + v2) + ... of Sum units, every one of
// which stores its result in a Float32Array (src/components/Sum.js:18-29,33-44) — one f32 rounding per add, in index order.
// That order IS the result (at 37 voices a sum rounded once differs in 70 to 80 % of the samples), so the reduction over
// instances is sequential by contract and all the parallelism is across channel x sample:
//
//   * planar PCM [instance][channel][sample] is, per instance, one row of n_channels * n_samples floats, and the output is one
//     such row: a lane owns one unit of the row (one float, or four where 16-byte accesses are possible) and walks the
//     instances.  Only the adds depend on each other; the loads of DEPTH instances are issued before the first of them is
//     needed, so a lane keeps that many rows in flight: 8 where the grid fills the chip, 32 where it cannot (below).
//   * 16-byte accesses need every row to start on a 16-byte boundary: bases aligned and a row length that is a multiple of 4.
//     An odd row length puts the instances' rows at four different phases; those (and unaligned bases) take the dword form,
//     whose wave-wide accesses are still whole contiguous 256-byte runs.
//   * a short render with many voices has few units: at four floats a lane most of the chip would have no lane at all.  The
//     launcher takes the dword form whenever the float4 grid would not give every CU a workgroup, and — when even the dword
//     grid does not — workgroups of one wavefront that each keep 32 rows in flight instead of 8: the few wavefronts there are
//     must cover the memory latency by themselves (launch_mix).
//
// term(i) = gains ? f32(x_i * g_i) : x_i — a plain f32 product, as Multiply stores it (Multiply.js:23-34), then a plain f32
// add: the project's flags (-ffp-contract=off -fno-fast-math) keep the two apart.  The chain starts from init when there is
// one (a partial sum: an earlier tile's, another device's) and from term(0) itself otherwise — not from 0 + term(0), which
// would turn a -0 into +0 one add early.  raw stores the sum as it stands; otherwise NaN and -0 leave as +0, the `x || 0` of
// renderChannelData.js:44.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dusp {

constexpr int kMixDepth = 8, kMixDepthNarrow = 32;  // rows a lane has in flight: a grid that fills the chip / one that cannot

template <int VEC>
struct MixUnit;
template <>
struct MixUnit<1> {
    using T = float;
    static __device__ __forceinline__ T scale(T x, float g) { return x * g; }
    static __device__ __forceinline__ T add(T a, T b) { return a + b; }
    static __device__ __forceinline__ T or0(T a) { return (a != a || a == 0.0f) ? 0.0f : a; }
};
template <>
struct MixUnit<4> {
    using T = float4;
    static __device__ __forceinline__ T scale(T x, float g) { return make_float4(x.x * g, x.y * g, x.z * g, x.w * g); }
    static __device__ __forceinline__ T add(T a, T b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
    static __device__ __forceinline__ T or0(T a) {
        return make_float4(MixUnit<1>::or0(a.x), MixUnit<1>::or0(a.y), MixUnit<1>::or0(a.z), MixUnit<1>::or0(a.w));
    }
};

// rows: n_inst rows of n_units units, one behind the other.  init and out may be the same buffer (a lane reads its unit of init
// before it writes that unit of out, and no other lane touches it): neither is __restrict__.
template <int VEC, int DEPTH, bool GAINS>
__global__ void __launch_bounds__(256) dusp_mix_kernel(const typename MixUnit<VEC>::T *__restrict__ rows, const float *__restrict__ gains,
                                                        const typename MixUnit<VEC>::T *init, typename MixUnit<VEC>::T *out, uint64_t n_units, uint32_t n_inst,
                                                        int raw) {
    using M = MixUnit<VEC>;
    using T = typename M::T;
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_units) return;
    const T *src = rows + u;
    T acc;
    uint32_t i = 0;
    if (init) {
        acc = init[u];
    } else {
        acc = src[0];
        if (GAINS) acc = M::scale(acc, gains[0]);
        i = 1;
    }
    for (; i + DEPTH <= n_inst; i += DEPTH) {
        T v[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; k++) v[k] = src[(uint64_t)(i + k) * n_units];
#pragma unroll
        for (int k = 0; k < DEPTH; k++) acc = M::add(acc, GAINS ? M::scale(v[k], gains[i + k]) : v[k]);
    }
    for (; i < n_inst; i++) {
        const T v = src[(uint64_t)i * n_units];
        acc = M::add(acc, GAINS ? M::scale(v, gains[i]) : v);
    }
    out[u] = raw ? acc : M::or0(acc);
}

template <int VEC, int DEPTH>
static hipError_t launch_mix_as(const float *d_planar, const float *d_gains, const float *d_init, float *d_out, uint64_t row_len, uint32_t n_inst, int raw,
                                uint32_t threads, hipStream_t stream) {
    using T = typename MixUnit<VEC>::T;
    const uint64_t n_units = row_len / VEC;
    const dim3 grid((uint32_t)((n_units + threads - 1) / threads)), block(threads);
    if (d_gains)
        hipLaunchKernelGGL((dusp_mix_kernel<VEC, DEPTH, true>), grid, block, 0, stream, (const T *)d_planar, d_gains, (const T *)d_init, (T *)d_out, n_units, n_inst, raw);
    else
        hipLaunchKernelGGL((dusp_mix_kernel<VEC, DEPTH, false>), grid, block, 0, stream, (const T *)d_planar, d_gains, (const T *)d_init, (T *)d_out, n_units, n_inst, raw);
    return hipGetLastError();
}

// row_len = n_channels * n_samples.  The caller bounds it at 2^31 floats (abi_internal.hpp kMixRowMax): with one lane per float at the
// most, the grid stays below the 2^32 threads in x that a launch may have.
// width_knob (Knobs::mix_width): 1 the dword form everywhere, 4 the float4 form wherever it is possible, else the choice below.
// depth_knob (Knobs::mix_depth): 8 / 32 rows in flight in the dword form whatever the grid, else the choice below.
hipError_t launch_mix(const float *d_planar, const float *d_gains, const float *d_init, float *d_out, uint64_t row_len, uint32_t n_inst, int raw, int n_cus,
                      int width_knob, int depth_knob, hipStream_t stream) {
    const bool can16 = row_len % 4 == 0 && (((uintptr_t)d_planar | (uintptr_t)d_out | (uintptr_t)d_init) & 15) == 0;
    // four floats a lane only while that still gives every CU a workgroup of 256; else one float a lane, and workgroups of one
    // wavefront with more rows in flight when even those are fewer than the CUs
    const bool wide = can16 && width_knob != 1 && (width_knob == 4 || (row_len / 4 + 255) / 256 >= (uint64_t)n_cus);
    if (wide) return launch_mix_as<4, kMixDepth>(d_planar, d_gains, d_init, d_out, row_len, n_inst, raw, 256, stream);
    const bool narrow = (row_len + 255) / 256 < (uint64_t)n_cus;
    if (depth_knob ? depth_knob >= kMixDepthNarrow : narrow)
        return launch_mix_as<1, kMixDepthNarrow>(d_planar, d_gains, d_init, d_out, row_len, n_inst, raw, narrow ? 64 : 256, stream);
    return launch_mix_as<1, kMixDepth>(d_planar, d_gains, d_init, d_out, row_len, n_inst, raw, narrow ? 64 : 256, stream);
}

}  // namespace dusp
