// dusp_amd/csrc/render_plan.hpp on the CPU: the three small decisions a render takes between its HIP calls, at their boundary values.
// Every expected value is worked out by hand from the rule as the header states it.  Prints one JSON line.
#include <cstdio>

#include "../../dusp_amd/csrc/render_plan.hpp"

using namespace dusp;

static long g_cases = 0, g_bad = 0;

static void expect(const char *what, unsigned long long got, unsigned long long want) {
    g_cases++;
    if (got != want) g_bad++, std::printf("FAIL: %s: %llu, expected %llu\n", what, got, want);
}

int main() {
    const uint64_t C = kChunk;
    // sumchain_group_blocks(n_inst, n_samples, n_cus): 8 groups a block when n_inst * ceil(groups / 8) reaches the 16 * n_cus wave slots, else 4;
    // 8 when 4 would need more than 65535 blocks; 0 when 8 would
    expect("256 CUs, 1 instance, 11250 groups", sumchain_group_blocks(1, 11250 * C, 256), 4);          // 1407 items < 4096 slots; 2813 blocks
    expect("256 CUs, 1 instance, 32768 groups", sumchain_group_blocks(1, 32768 * C, 256), 8);          // 4096 items reach the 4096 slots
    expect("256 CUs, 1 instance, 32760 groups", sumchain_group_blocks(1, 32760 * C, 256), 4);          // 4095 items do not
    expect("256 CUs, 2 instances, 16384 groups", sumchain_group_blocks(2, 16384 * C, 256), 8);         // 2 x 2048 items
    expect("4096 CUs, 1 instance, 400000 groups", sumchain_group_blocks(1, 400000 * C, 4096), 8);      // 50000 items < 65536 slots, but 4 would need 100000 blocks
    expect("4096 CUs, 1 instance, 262140 groups", sumchain_group_blocks(1, 262140 * C, 4096), 4);      // exactly 65535 blocks of 4
    expect("4096 CUs, 1 instance, 262141 groups", sumchain_group_blocks(1, 262141 * C, 4096), 8);      // 65536 blocks of 4
    expect("256 CUs, 524280 groups", sumchain_group_blocks(1, 524280 * C, 256), 8);                    // exactly 8 x 65535
    expect("256 CUs, 524281 groups", sumchain_group_blocks(1, 524281 * C, 256), 0);                    // over 8 x 65535: too long
    expect("4096 CUs, 7 instances, 524281 groups", sumchain_group_blocks(7, 524281 * C, 4096), 0);     // ... whatever the chip and the batch
    expect("a ragged last chunk counts", sumchain_group_blocks(1, 32767 * C + 1, 256), 8);             // 32768 groups
    expect("one sample", sumchain_group_blocks(1, 1, 256), 4);

    // mix_tile_instances(tile_instances, mix_tile_mb, free_bytes, staged_bytes, n_cus, row_floats, n_instances)
    const size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
    expect("the caller's tile, cut to the batch", mix_tile_instances(5, 0, 64 * GiB, 0, 256, MiB, 3), 3);
    expect("the caller's tile wins over the knob", mix_tile_instances(5, 64, 64 * GiB, 0, 256, MiB, 100), 5);
    expect("knob 64 MiB, 4 MiB row", mix_tile_instances(0, 64, 0, 0, 256, MiB, 100000), 16);
    expect("knob below a row", mix_tile_instances(0, 1, 0, 0, 256, MiB, 100000), 1);
    expect("default: 32 rows a CU", mix_tile_instances(0, 0, 64 * GiB, 0, 256, 48000, 100000), 8192);  // 192 000-byte rows: 8192 of them are 1.5 GiB
    expect("default, small batch", mix_tile_instances(0, 0, 64 * GiB, 0, 256, 48000, 100), 100);
    expect("half of 1 GiB free, 4 MiB row", mix_tile_instances(0, 0, 1 * GiB, 0, 256, MiB, 100000), 128);
    expect("what is staged counts as free", mix_tile_instances(0, 0, 1 * GiB, 1 * GiB, 256, MiB, 100000), 256);
    expect("at most 16 GiB", mix_tile_instances(0, 0, 256 * GiB, 0, 4096, 64 * MiB, 100000), 64);      // 256 MiB rows
    expect("free memory below two rows", mix_tile_instances(0, 0, 7 * MiB, 0, 256, MiB, 100000), 1);
    expect("no free memory", mix_tile_instances(0, 0, 0, 0, 256, MiB, 100000), 1);

    // handoff_warm_chunks(clock0, n_warm, n_chunks): chunks of this render among the program's warm-up chunks
    expect("from the start", handoff_warm_chunks(0, 3, 10), 3);
    expect("one chunk in", handoff_warm_chunks(256, 3, 10), 2);
    expect("behind the warm-up", handoff_warm_chunks(768, 3, 10), 0);
    expect("far behind the warm-up", handoff_warm_chunks((uint64_t)1 << 40, 3, 10), 0);
    expect("a render that ends inside the warm-up", handoff_warm_chunks(0, 3, 3), 3);  // (W == n_chunks: the caller does not hand off)
    expect("... or before its end", handoff_warm_chunks(256, 3, 1), 1);
    expect("no warm-up", handoff_warm_chunks(0, 0, 10), 0);

    std::printf("{\"cases\": %ld, \"bad\": %ld}\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
