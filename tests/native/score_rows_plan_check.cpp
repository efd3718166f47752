// score_rows_plan_check.cpp — score_rows_plan of dusp_amd/csrc/score_plan.hpp against brute force, on the CPU, in score_plan_check.cpp's
// style: voices of their OWN row lengths (0 and 1 among them).  Over some thousands of random tiles every block's list is exactly the
// ascending set of the voices whose span, clipped to the timeline, intersects the block; the union window is the clipped spans' hull;
// onsets near +-2^62 and the int64 limits take part (-fsanitize=undefined: an overflow is an error); a listed voice's record carries its
// own row and stride, a record in no list the first listed voice's row (what the kernel's unpredicated loads rely on); a bad length is
// reported by index; a small byte budget is honoured by doubling the block, and the block is the smallest that fits; the packed image
// starts on a 32-byte boundary.  Equal rows give score_plan's lists.  Built with -fsanitize=address,undefined by tests/test_piece_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "far_onsets": f, "empty_tiles": e, "empty_rows": z}.
#include "../../dusp_amd/csrc/score_plan.hpp"

#include <cstdio>
#include <random>

using namespace dusp;

int main() {
    std::mt19937_64 rng(12);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    long cases = 0, bad = 0, doubled = 0, far_onsets = 0, empty_tiles = 0, empty_rows = 0;
    const int64_t far[] = {INT64_MAX, INT64_MIN, INT64_MAX - 5, INT64_MIN + 5, (int64_t)1 << 62, -((int64_t)1 << 62), ((int64_t)1 << 62) + 777, -((int64_t)1 << 62) - 777};
    for (int round = 0; round < 6000; round++) {
        const size_t n = (size_t)pick(0, round % 7 == 0 ? 300 : 40);
        const uint64_t max_row = (uint64_t)pick(1, round % 5 == 0 ? 5000 : 700), n_total = (uint64_t)pick(1, round % 3 == 0 ? 20000 : 3000);
        const bool with_lengths = round % 2 == 0, whole = round % 4 < 2, equal_rows = round % 11 == 0;
        const size_t budget = round % 6 == 0 ? (size_t)pick(0, 2000) : round % 6 == 1 ? n * sizeof(ScoreRow) + (size_t)pick(8, 4000) : kScorePlanBytes;
        std::vector<int64_t> onsets(n), lengths(n);
        std::vector<uint32_t> samples(n);
        std::vector<uint64_t> rows(n);
        for (size_t k = 0; k < n; k++) {
            const int rk = (int)pick(0, 7);
            samples[k] = equal_rows ? (uint32_t)max_row : rk == 0 ? 0u : rk == 1 ? 1u : rk == 2 ? (uint32_t)max_row : (uint32_t)pick(0, (int64_t)max_row);
            empty_rows += samples[k] == 0;
            rows[k] = samples[k] ? 0x1000 + 0x100 * (uint64_t)k : 0;  // (an empty row has no address)
            const int kind = (int)pick(0, 11);
            if (kind == 0) { onsets[k] = far[rng() % 8]; far_onsets++; }
            else if (kind == 1) onsets[k] = pick(-(int64_t)samples[k] - 3, 3);
            else if (kind == 2) onsets[k] = pick((int64_t)n_total - 3, (int64_t)n_total + 3);
            else if (kind == 3) onsets[k] = pick(0, 8) * 256 - pick(0, 1);
            else onsets[k] = pick(-(int64_t)max_row, (int64_t)n_total);
            const int lk = (int)pick(0, 9);
            lengths[k] = lk == 0 ? 0 : lk == 1 ? std::min<int64_t>(1, samples[k]) : lk == 2 ? (int64_t)samples[k] : pick(0, (int64_t)samples[k]);
        }
        ScoreRowsPlan P;
        const int64_t rc = score_rows_plan(onsets.data(), with_lengths ? lengths.data() : nullptr, samples.data(), rows.data(), n, n_total, whole, budget, P, {});
        cases++;
        bool ok = rc == -1;
        auto span = [&](size_t k, int64_t &lo, int64_t &hi) {  // brute force, in __int128 so that the check itself cannot overflow
            const __int128 on = onsets[k], len = with_lengths ? lengths[k] : (int64_t)samples[k];
            __int128 a = on < 0 ? (__int128)0 : on, b = on + len < (__int128)n_total ? on + len : (__int128)n_total;
            if (b <= a) { lo = hi = 0; return false; }
            lo = (int64_t)a; hi = (int64_t)b;
            return true;
        };
        int64_t u_lo = (int64_t)n_total, u_hi = 0;
        size_t first_listed = n;
        for (size_t k = 0; k < n; k++) { int64_t lo, hi; if (span(k, lo, hi)) { first_listed = k; break; } }
        for (size_t k = 0; k < n; k++) {
            int64_t lo, hi;
            const bool on = span(k, lo, hi);
            if (on) { u_lo = std::min(u_lo, lo); u_hi = std::max(u_hi, hi); }
            ok &= P.voices.size() == n && P.voices[k].lo == (uint32_t)lo && P.voices[k].hi == (uint32_t)hi;
            if (on) ok &= P.voices[k].onset == onsets[k] && P.voices[k].row == rows[k] && rows[k] != 0 && P.voices[k].stride == samples[k] && samples[k] >= 1;
            else if (first_listed < n) ok &= P.voices[k].row == rows[first_listed];  // readable, whatever voice k's own row is
        }
        if (u_hi <= u_lo) { u_lo = u_hi = 0; empty_tiles++; }
        ok &= P.t_lo == u_lo && P.t_hi == u_hi;
        ok &= whole ? (P.w_lo == 0 && P.w_hi == (int64_t)n_total) : (P.w_lo == u_lo && P.w_hi == u_hi);
        if (P.w_hi > P.w_lo) {
            const uint64_t B = (uint64_t)1 << P.block_shift;
            ok &= P.block_shift >= kScoreGroupShift && P.first_block == (uint64_t)P.w_lo / B;
            const uint64_t want_blocks = ((uint64_t)P.w_hi - 1) / B - P.first_block + 1;
            ok &= P.n_blocks() == want_blocks && P.block_first[0] == 0 && P.block_first.back() + kScoreEntryPad == P.entries.size();
            ok &= P.bytes() <= budget || want_blocks == 1;
            if (P.block_shift > kScoreGroupShift) {
                doubled++;
                const uint64_t Bh = B / 2, first_h = (uint64_t)P.w_lo / Bh, blocks_h = ((uint64_t)P.w_hi - 1) / Bh - first_h + 1;
                uint64_t entries_h = 0;
                for (size_t k = 0; k < n; k++) { int64_t lo, hi; if (span(k, lo, hi)) entries_h += (uint64_t)(hi - 1) / Bh - (uint64_t)lo / Bh + 1; }
                ok &= n * sizeof(ScoreRow) + (blocks_h + 1 + entries_h + kScoreEntryPad) * 4 > budget;  // half the block would not have fitted
            }
            for (uint64_t b = 0; ok && b < want_blocks; b++) {
                const int64_t b_lo = (int64_t)((P.first_block + b) * B), b_hi = b_lo + (int64_t)B;
                std::vector<uint32_t> want;
                for (size_t k = 0; k < n; k++) { int64_t lo, hi; if (span(k, lo, hi) && lo < b_hi && hi > b_lo) want.push_back((uint32_t)k); }
                ok &= P.block_first[b] <= P.block_first[b + 1] && P.block_first[b + 1] <= P.n_entries() &&
                      std::vector<uint32_t>(P.entries.begin() + P.block_first[b], P.entries.begin() + P.block_first[b + 1]) == want;
            }
            std::vector<unsigned char> image(3);  // the packed image: 32-byte aligned, the three arrays one behind the other
            const size_t at = score_plan_pack(P, image);
            ok &= at == 32 && image.size() == at + P.bytes();
            for (size_t k = 0; k < kScoreEntryPad; k++) ok &= P.entries[P.n_entries() + k] == 0;
            if (equal_rows && budget == kScorePlanBytes) {  // rows of one length: score_plan's lists and window
                ScorePlan Q;
                ok &= score_plan(onsets.data(), with_lengths ? lengths.data() : nullptr, n, max_row, n_total, whole, budget, Q) == -1;
                ok &= Q.block_first == P.block_first && Q.entries == P.entries && Q.w_lo == P.w_lo && Q.w_hi == P.w_hi && Q.block_shift == P.block_shift;
            }
        } else {
            ok &= P.entries.empty() && P.n_blocks() == 0 && P.n_entries() == 0;
        }
        if (!ok) { bad++; printf("MISMATCH round %d n %zu max_row %llu n_total %llu whole %d budget %zu\n", round, n, (unsigned long long)max_row, (unsigned long long)n_total, (int)whole, budget); }
    }
    {   // a bad length is reported by its index, against the voice's OWN row, whatever the onsets
        int64_t on[3] = {0, 5, INT64_MAX}, len[3] = {4, 9, 2};
        uint32_t samples[3] = {4, 8, 2};
        ScoreRowsPlan P;
        cases += 4;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {}) != 1;
        len[1] = -1;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {}) != 1;
        len[1] = 8;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {}) != -1;
        len[2] = 3;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {}) != 2;
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"far_onsets\": %ld, \"empty_tiles\": %ld, \"empty_rows\": %ld}\n", cases, bad, doubled, far_onsets, empty_tiles, empty_rows);
    return bad != 0;
}
