// render_plan.hpp — a few small decisions a render takes between its HIP calls, as plain data in, plain data out: host code only (no HIP),
// checked at their boundary values on the CPU (tests/native/render_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "device_types.hpp"

namespace dusp {

// The fused sum chain's blocks of chunk groups: 8 groups a block when that still leaves every wave slot (16 a CU) an item, else 4;
// 8 as well where 4 would need more than 65535 blocks; 0 where even 8 would (too many samples for the sum chain).
inline int sumchain_group_blocks(uint32_t n_inst, uint64_t n_samples, int n_cus) {
    const uint64_t groups = (n_samples + kChunk - 1) / kChunk;
    const uint64_t slots = (uint64_t)n_cus * 16;
    int gb = (uint64_t)n_inst * ((groups + 7) / 8) >= slots ? 8 : 4;
    if ((groups + gb - 1) / gb > 65535) gb = 8;
    if ((groups + gb - 1) / gb > 65535) return 0;
    return gb;
}

// The tile of dusp_render_host_mix.  The engines that take any voice are parallel over INSTANCES: the wave engine and its compiled
// kernels run one wavefront per instance and fill the chip at 32 instances a CU, and below that a tile's render costs
// about what the whole batch's would, since one instance's dependent steps are the floor.  So the default (tile_instances == 0) is that
// many instances, cut down only where their PCM would not fit kMixTileBytes or half of the device's free memory — what the program's
// staging already holds (staged_bytes) is not free, but is the call's to use.  DUSP_MIX_TILE_MB=n in the environment of
// dusp_ctx_create (mix_tile_mb) makes it what fits n MiB instead (tools/mix_bench.py sweeps that).
constexpr size_t kMixTileBytes = (size_t)16 << 30;
constexpr size_t kMixTileRowsPerCu = 32;

inline size_t mix_tile_instances(size_t tile_instances, int mix_tile_mb, size_t free_bytes, size_t staged_bytes, int n_cus, size_t row_floats, size_t n_instances) {
    size_t tile = tile_instances;
    if (tile == 0 && mix_tile_mb > 0) tile = ((size_t)mix_tile_mb << 20) / (row_floats * sizeof(float));
    else if (tile == 0) {
        const size_t budget = std::min(kMixTileBytes, (free_bytes + staged_bytes) / 2);
        tile = std::min((size_t)n_cus * kMixTileRowsPerCu, budget / (row_floats * sizeof(float)));
    }
    return std::min(std::max<size_t>(1, tile), n_instances);
}

// The tiles of dusp_render_host_score_parts: runs [starts[i], starts[i + 1]) of the chain's voices whose rows (row_bytes[k] each: the
// voices are of several programs and several lengths) together fit tile_bytes, at most max_voices voices and at least one voice a tile.
// tile_bytes == 0: the default, derived as mix_tile_instances derives its own but over bytes — what fits mix_tile_mb MiB, else
// kMixTileBytes or half of the device's free memory (staged_bytes counted as the call's own) and no more voices than fill the chip.
inline std::vector<size_t> piece_tile_starts(const uint64_t *row_bytes, size_t n_voices, size_t tile_bytes, int mix_tile_mb, size_t free_bytes, size_t staged_bytes,
                                             int n_cus) {
    uint64_t budget = tile_bytes;
    size_t max_voices = n_voices;
    if (budget == 0 && mix_tile_mb > 0) budget = (uint64_t)mix_tile_mb << 20;
    else if (budget == 0) {
        budget = std::min(kMixTileBytes, (free_bytes + staged_bytes) / 2);
        max_voices = (size_t)n_cus * kMixTileRowsPerCu;
    }
    std::vector<size_t> starts{0};
    uint64_t used = 0;
    for (size_t k = 0; k < n_voices; k++) {
        if (k > starts.back() && (used + row_bytes[k] > budget || k - starts.back() >= max_voices)) {
            starts.push_back(k);
            used = 0;
        }
        used += row_bytes[k];
    }
    starts.push_back(n_voices);
    return starts;
}

// Of a render's n_chunks chunks from circuit clock clock0 (a multiple of the chunk), how many are among the program's n_warm warm-up
// chunks (Program::warm_ops) and stay on the chunk engine.  The caller hands over only when the answer is above 0 and below n_chunks.
inline uint32_t handoff_warm_chunks(uint64_t clock0, uint32_t n_warm, uint32_t n_chunks) {
    const uint64_t first_chunk = clock0 / kChunk;
    return first_chunk < n_warm ? (uint32_t)std::min<uint64_t>(n_chunks, n_warm - first_chunk) : 0u;
}

}  // namespace dusp
