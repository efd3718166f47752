// pcm_engine.hip — device-side PCM delivery: the peak of every instance, and planar f32 -> peak-normalised interleaved
// s16 / packed s24 / f32 frames (pcm_quant.hpp is the sample contract).  What a caller downloads is then 2 or 3 bytes per
// sample instead of 4, and no host thread walks the samples again (dusp_amd/js/lib/wav.js did, one sample at a time).
//
// Peak: a pure streaming read.  An instance's channels are one contiguous run of n_channels * n_samples floats; several
// workgroups share it (one long instance still fills the chip), each with 16-byte loads over the aligned middle — workgroup 0
// of the instance also takes the scalar head and tail — then a maximum of `bits & 0x7fffffff` within the wave, within the
// workgroup, and ONE unsigned atomic max per workgroup into the instance's zeroed word.  Integer maxima commute: the result
// is exact and the same on every run, and any NaN sample wins (pcm_abs_bits).
//
// Encode: the output of the WHOLE batch is one byte stream ([instance][frame][channel], 2 / 3 / 4 bytes a sample).  An
// instance starts at byte i * n_samples * n_channels * bytes of it — not a multiple of 4 for s24, nor for s16 when
// n_samples * n_channels is odd — so the stream is cut into tiles counted from the 16-byte boundary at or below d_out, not per
// instance: every tile starts 16-byte aligned, leaves as whole 16-byte stores, and only the very first and last 16 bytes of
// the batch are written byte by byte.  A workgroup reads each channel's run of its tile's frames coalesced, quantises, and
// parks the sample bits in LDS as [channel][frame] (odd pitch: the transposing reads stay off one bank); then every lane
// assembles 16 output bytes from the 4 to 9 samples that touch them.  One channel from and to 16-byte aligned buffers needs no
// transpose: 8 samples go from two 16-byte loads to one 16-byte store of 8 shorts (24 bytes for s24, 32 for f32).
//
// Gains are derived here, on the device, from the peaks (pcm_gain): no host round trip between the two kernels.
//
// One peak for all signals of a block (a call with stems): pcm_peak_common.hpp, a kernel of this object over the peak kernel's words, in
// a header of its own because its text also compiles for the host under tests/native/hip_host_stub, which the kernels here do not.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm_peak_common.hpp"
#include "pcm_quant.hpp"

namespace dusp {

constexpr int kPcmThreads = 256;
constexpr int kGainSlots = 64;  // gains of the first instances a tile touches, computed once per workgroup

__global__ void __launch_bounds__(kPcmThreads) dusp_pcm_peak_kernel(const float *__restrict__ in, uint32_t *__restrict__ peaks, uint64_t len,
                                                                    uint32_t blocks_per_instance) {
    __shared__ uint32_t wave_max[kPcmThreads / 64];
    const uint64_t inst = blockIdx.x / blocks_per_instance;
    const uint32_t b = blockIdx.x % blocks_per_instance;
    const float *row = in + inst * len;
    uint64_t head = ((16 - ((uintptr_t)row & 15)) & 15) / 4;  // floats in front of the first 16-byte boundary
    if (head > len) head = len;
    const uint64_t n_vec = (len - head) / 4;
    const uint4 *vec = (const uint4 *)(row + head);
    uint32_t m = 0;
#pragma unroll 4
    for (uint64_t i = (uint64_t)b * kPcmThreads + threadIdx.x; i < n_vec; i += (uint64_t)blocks_per_instance * kPcmThreads) {
        const uint4 w = vec[i];
        m = max(max(m, w.x & 0x7fffffffu), max(w.y & 0x7fffffffu, max(w.z & 0x7fffffffu, w.w & 0x7fffffffu)));
    }
    if (b == 0) {
        const uint64_t tail_at = head + 4 * n_vec;
        if (threadIdx.x < head) m = max(m, pcm_abs_bits(row[threadIdx.x]));
        if (tail_at + threadIdx.x < len) m = max(m, pcm_abs_bits(row[tail_at + threadIdx.x]));  // (at most 3)
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kPcmThreads / 64; w++) m = max(m, wave_max[w]);
        if (m) atomicMax(&peaks[inst], m);
    }
}

template <int FORMAT>
struct PcmFormat {
    static constexpr int kBytes = FORMAT == kPcmS16 ? 2 : FORMAT == kPcmS24 ? 3 : 4;
};

// One channel, both buffers 16-byte aligned: planar IS interleaved, the batch is one run of n_total samples.
template <int FORMAT>
__global__ void __launch_bounds__(kPcmThreads) dusp_pcm_encode_flat_kernel(const float *__restrict__ in, const uint32_t *__restrict__ peaks, int normalise,
                                                                           unsigned char *__restrict__ out, uint64_t n_total, uint64_t n_samples) {
    constexpr int kBytes = PcmFormat<FORMAT>::kBytes;
    const uint64_t n_units = n_total / 8;
    for (uint64_t u = (uint64_t)blockIdx.x * kPcmThreads + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * kPcmThreads) {
        const float4 lo = ((const float4 *)in)[2 * u], hi = ((const float4 *)in)[2 * u + 1];
        const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        double g = 1.0;
        uint64_t inst = 0, left = 8;  // samples of this unit that still belong to `inst`
        if (normalise) {
            inst = (8 * u) / n_samples;
            left = (inst + 1) * n_samples - 8 * u;
            g = pcm_gain(peaks[inst], normalise);
        }
        uint32_t s[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (normalise && (uint64_t)j >= left) {  // the next instance begins inside the unit
                inst++;
                left += n_samples;
                g = pcm_gain(peaks[inst], normalise);
            }
            s[j] = pcm_sample_bits(x[j], g, FORMAT);
        }
        if (FORMAT == kPcmS16) {
            ((uint4 *)out)[u] = make_uint4(s[0] | s[1] << 16, s[2] | s[3] << 16, s[4] | s[5] << 16, s[6] | s[7] << 16);
        } else if (FORMAT == kPcmS24) {  // 4 samples are 3 whole dwords
            uint2 *dst = (uint2 *)(out + 24 * u);
            dst[0] = make_uint2(s[0] | s[1] << 24, s[1] >> 8 | s[2] << 16);
            dst[1] = make_uint2(s[2] >> 16 | s[3] << 8, s[4] | s[5] << 24);
            dst[2] = make_uint2(s[5] >> 8 | s[6] << 16, s[6] >> 16 | s[7] << 8);
        } else {
            ((uint4 *)out)[2 * u] = make_uint4(s[0], s[1], s[2], s[3]);
            ((uint4 *)out)[2 * u + 1] = make_uint4(s[4], s[5], s[6], s[7]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)  // the batch's last 0..7 samples
        for (uint64_t e = 8 * n_units; e < n_total; e++) {
            const uint32_t bits = pcm_sample_bits(in[e], pcm_gain(normalise ? peaks[e / n_samples] : 0u, normalise), FORMAT);
            for (int k = 0; k < kBytes; k++) out[e * kBytes + k] = (unsigned char)(bits >> (8 * k));
        }
}

// The general form.  `base` is the 16-byte boundary at or below d_out and a0 = d_out - base (0..15); positions p count bytes
// from base, the PCM stream occupies [a0, a0 + total bytes).  Workgroup k owns positions [k T, (k + 1) T), T = tile_frames *
// n_channels * bytes (a multiple of 16): the frames that touch them number at most tile_frames + 1.
template <int FORMAT>
__global__ void __launch_bounds__(kPcmThreads)
    dusp_pcm_encode_tile_kernel(const float *__restrict__ in, const uint32_t *__restrict__ peaks, int normalise, unsigned char *__restrict__ base, uint32_t a0,
                                uint32_t n_channels, uint64_t n_samples, uint64_t n_frames_total, uint32_t tile_frames, uint32_t pitch) {
    constexpr uint32_t kBytes = PcmFormat<FORMAT>::kBytes;
    extern __shared__ uint32_t tile[];  // [n_channels][pitch]: sample bits (pcm_sample_bits)
    __shared__ double gains[kGainSlots];
    const uint32_t frame_bytes = n_channels * kBytes, T = tile_frames * frame_bytes;
    const uint64_t p0 = (uint64_t)blockIdx.x * T, p_end = a0 + n_frames_total * frame_bytes;
    const uint64_t s_lo = p0 > a0 ? p0 - a0 : 0;                                // this tile's bytes of the stream: [s_lo, s_hi)
    const uint64_t s_hi = p0 + T < p_end ? p0 + T - a0 : p_end - a0;
    const uint64_t f_lo = s_lo / frame_bytes;                                   // ... and the frames that touch them: [f_lo, f_lo + nf)
    const uint32_t nf = (uint32_t)((s_hi + frame_bytes - 1) / frame_bytes - f_lo);
    const uint64_t inst_lo = f_lo / n_samples, t_lo = f_lo - inst_lo * n_samples;
    if (normalise) {
        const uint64_t n_inst = (f_lo + nf - 1) / n_samples - inst_lo + 1;
        if (threadIdx.x < kGainSlots && threadIdx.x < n_inst) gains[threadIdx.x] = pcm_gain(peaks[inst_lo + threadIdx.x], normalise);
        __syncthreads();
    }
    for (uint32_t k = threadIdx.x; k < nf; k += kPcmThreads) {  // one frame per lane: every channel's run is read coalesced
        uint64_t t = t_lo + k, di = 0;
        if (t >= n_samples) {  // the tile runs into later instances
            di = t / n_samples;
            t -= di * n_samples;
        }
        double g = 1.0;
        if (normalise) g = di < kGainSlots ? gains[di] : pcm_gain(peaks[inst_lo + di], normalise);
        const float *src = in + (inst_lo + di) * n_channels * n_samples + t;
        for (uint32_t c = 0; c < n_channels; c++) tile[c * pitch + k] = pcm_sample_bits(src[(uint64_t)c * n_samples], g, FORMAT);
    }
    __syncthreads();
    const int32_t rel0 = (int32_t)((int64_t)p0 - (int64_t)a0 - (int64_t)(f_lo * frame_bytes));  // stream byte of position p0, relative to frame f_lo's first byte
    for (uint32_t ch = threadIdx.x; ch < T / 16; ch += kPcmThreads) {  // 16 output bytes per lane
        const uint64_t p = p0 + 16 * (uint64_t)ch;
        if (p >= p_end) break;
        const int lo = p < a0 ? (int)(a0 - p) : 0, hi = p_end - p < 16 ? (int)(p_end - p) : 16;  // the chunk's bytes that belong to the stream
        const int32_t rel = rel0 + 16 * (int32_t)ch;       // stream byte of the chunk's byte 0, relative to frame f_lo (negative only in front of the stream)
        const uint32_t e = (uint32_t)(rel + lo) / kBytes;  // first sample with a byte in [lo, hi), counted from frame f_lo's channel 0
        uint32_t k = e / n_channels, c = e - k * n_channels;
        unsigned __int128 acc = 0;
        for (int o = (int32_t)(e * kBytes) - rel; o < hi; o += (int)kBytes) {  // o: where in the chunk the sample's byte 0 lands (-kBytes < o)
            const unsigned __int128 v = tile[c * pitch + k];
            acc |= o >= 0 ? v << (8 * o) : v >> (-8 * o);
            if (++c == n_channels) {
                c = 0;
                k++;
            }
        }
        if (lo == 0 && hi == 16) {
            *(uint4 *)(base + p) = make_uint4((uint32_t)acc, (uint32_t)(acc >> 32), (uint32_t)(acc >> 64), (uint32_t)(acc >> 96));
        } else {  // the batch's first and last chunk
            for (int i = lo; i < hi; i++) base[p + i] = (unsigned char)(acc >> (8 * i));
        }
    }
}

hipError_t launch_pcm_peak(const float *d_planar, float *d_peaks, uint32_t n_instances, uint32_t n_channels, uint64_t n_samples, int n_cus, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_peaks, 0, (size_t)n_instances * sizeof(float), stream);
    if (e != hipSuccess) return e;
    const uint64_t len = (uint64_t)n_channels * n_samples;
    // enough workgroups to fill the chip (8 per CU), but none with fewer than 4 loads a lane
    const uint64_t want = ((uint64_t)n_cus * 8 + n_instances - 1) / n_instances, useful = (len + 4 * 4 * kPcmThreads - 1) / (4 * 4 * kPcmThreads);
    const uint32_t per = (uint32_t)(want < useful ? want : useful);
    hipLaunchKernelGGL(dusp_pcm_peak_kernel, dim3(n_instances * per), dim3(kPcmThreads), 0, stream, d_planar, (uint32_t *)d_peaks, len, per);
    return hipGetLastError();
}

uint32_t pcm_tile_frames(uint32_t n_channels) {
    if (n_channels > 32) return 128;  // (the tile stays under 64 KB of LDS)
    const uint32_t f = (4096 / n_channels) & ~15u;  // whole 16-byte chunks whatever the sample width
    return f < 256 ? 256 : f;
}

template <int FORMAT>
static hipError_t launch_encode_as(const float *d_planar, const float *d_peaks, int normalise, void *d_out, uint32_t n_instances, uint32_t n_channels, uint64_t n_samples,
                                   int n_cus, hipStream_t stream) {
    const uint32_t *peaks = (const uint32_t *)d_peaks;
    const uint64_t n_frames = (uint64_t)n_instances * n_samples;
    if (n_channels == 1 && (((uintptr_t)d_planar | (uintptr_t)d_out) & 15) == 0) {
        const uint64_t blocks = (n_frames / 8 + kPcmThreads - 1) / kPcmThreads, cap = (uint64_t)n_cus * 16;
        hipLaunchKernelGGL(dusp_pcm_encode_flat_kernel<FORMAT>, dim3((uint32_t)(blocks < 1 ? 1 : blocks < cap ? blocks : cap)), dim3(kPcmThreads), 0, stream, d_planar,
                           peaks, normalise, (unsigned char *)d_out, n_frames, n_samples);
        return hipGetLastError();
    }
    const uint32_t a0 = (uint32_t)((uintptr_t)d_out & 15), tile_frames = pcm_tile_frames(n_channels), pitch = (tile_frames + 2) | 1;
    const uint64_t T = (uint64_t)tile_frames * n_channels * PcmFormat<FORMAT>::kBytes;
    const uint64_t tiles = (a0 + n_frames * n_channels * PcmFormat<FORMAT>::kBytes + T - 1) / T;
    hipLaunchKernelGGL(dusp_pcm_encode_tile_kernel<FORMAT>, dim3((uint32_t)tiles), dim3(kPcmThreads), (size_t)n_channels * pitch * sizeof(uint32_t), stream, d_planar,
                       peaks, normalise, (unsigned char *)d_out - a0, a0, n_channels, n_samples, n_frames, tile_frames, pitch);
    return hipGetLastError();
}

// the number of workgroups launch_pcm_encode would start in the general form (the caller bounds it)
uint64_t pcm_encode_tiles(uint64_t n_instances, uint32_t n_channels, uint64_t n_samples, int format) {
    const uint64_t T = (uint64_t)pcm_tile_frames(n_channels) * n_channels * pcm_bytes_per_sample(format);
    return (15 + n_instances * n_samples * n_channels * pcm_bytes_per_sample(format) + T - 1) / T;
}

hipError_t launch_pcm_encode(const float *d_planar, const float *d_peaks, int format, int normalise, void *d_out, uint32_t n_instances, uint32_t n_channels,
                             uint64_t n_samples, int n_cus, hipStream_t stream) {
    if (format == kPcmS16) return launch_encode_as<kPcmS16>(d_planar, d_peaks, normalise, d_out, n_instances, n_channels, n_samples, n_cus, stream);
    if (format == kPcmS24) return launch_encode_as<kPcmS24>(d_planar, d_peaks, normalise, d_out, n_instances, n_channels, n_samples, n_cus, stream);
    return launch_encode_as<kPcmF32>(d_planar, d_peaks, normalise, d_out, n_instances, n_channels, n_samples, n_cus, stream);
}

}  // namespace dusp
