// score_rows_plan_frac_check.cpp — score_rows_plan of dusp_amd/csrc/score_plan.hpp WITH FRACTIONS against brute force, on the CPU, in
// score_rows_plan_check.cpp's style.  A voice whose fraction is not 0 covers one more sample, the ceil tap of its last: over some
// thousands of random tiles every block's list is exactly the ascending set of the voices whose span — [onset, onset + len + 1) with a
// fraction, [onset, onset + len) without — clipped to the timeline intersects the block; the union window is the clipped spans' hull;
// a voice that ends exactly at sample 0 is listed for its tail tap alone when it has a fraction and dropped when it has none; a record
// carries pad = len (the UNCLIPPED length, never 0) with a fraction and 0 without; onsets near +-2^62 and the int64 limits take part
// (-fsanitize=undefined: an overflow is an error); a record in no list carries the first listed voice's row; a small byte budget is
// honoured by doubling the block, and the block is the smallest that fits; fractions that are all zero, and no fractions, give one and
// the same plan.  Built with -fsanitize=address,undefined by tests/test_frac_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "far_onsets": f, "tail_only": t, "two_taps": w, "zero_fracs": z}.
#include "../../dusp_amd/csrc/score_plan.hpp"

#include <cstdio>
#include <cstring>
#include <random>

using namespace dusp;

int main() {
    std::mt19937_64 rng(13);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    long cases = 0, bad = 0, doubled = 0, far_onsets = 0, tail_only = 0, two_taps = 0, zero_fracs = 0;
    const int64_t far[] = {INT64_MAX, INT64_MIN, INT64_MAX - 5, INT64_MIN + 5, (int64_t)1 << 62, -((int64_t)1 << 62), ((int64_t)1 << 62) + 777, -((int64_t)1 << 62) - 777};
    const double edge[] = {0.5, 0x1p-24, 1.0 - 0x1p-53, 0x1p-1074, 0.3};
    for (int round = 0; round < 6000; round++) {
        const size_t n = (size_t)pick(0, round % 7 == 0 ? 300 : 40);
        const uint64_t max_row = (uint64_t)pick(1, round % 5 == 0 ? 5000 : 700), n_total = (uint64_t)pick(1, round % 3 == 0 ? 20000 : 3000);
        const bool with_lengths = round % 2 == 0, whole = round % 4 < 2, all_zero = round % 13 == 0;
        const size_t budget = round % 6 == 0 ? (size_t)pick(0, 2000) : round % 6 == 1 ? n * sizeof(ScoreRow) + (size_t)pick(8, 4000) : kScorePlanBytes;
        std::vector<int64_t> onsets(n), lengths(n);
        std::vector<uint32_t> samples(n);
        std::vector<uint64_t> rows(n);
        std::vector<double> fracs(n);
        for (size_t k = 0; k < n; k++) {
            const int rk = (int)pick(0, 7);
            samples[k] = rk == 0 ? 0u : rk == 1 ? 1u : rk == 2 ? (uint32_t)max_row : (uint32_t)pick(0, (int64_t)max_row);
            rows[k] = samples[k] ? 0x1000 + 0x100 * (uint64_t)k : 0;  // (an empty row has no address)
            const int lk = (int)pick(0, 9);
            lengths[k] = lk == 0 ? 0 : lk == 1 ? std::min<int64_t>(1, samples[k]) : lk == 2 ? (int64_t)samples[k] : pick(0, (int64_t)samples[k]);
            const int64_t len = with_lengths ? lengths[k] : (int64_t)samples[k];
            const int kind = (int)pick(0, 13);
            if (kind == 0) { onsets[k] = far[rng() % 8]; far_onsets++; }
            else if (kind == 1) onsets[k] = pick(-(int64_t)samples[k] - 3, 3);
            else if (kind == 2) onsets[k] = pick((int64_t)n_total - 3, (int64_t)n_total + 3);
            else if (kind == 3) onsets[k] = pick(0, 8) * 256 - pick(0, 1);
            else if (kind == 4) onsets[k] = -len;                              // ends exactly at sample 0: only the tail tap is on the timeline
            else if (kind == 5) onsets[k] = (int64_t)n_total - len;            // the tail tap is clipped off
            else if (kind == 6) onsets[k] = pick(0, 8) * 256 - len;            // the tail tap is the first sample of a block
            else onsets[k] = pick(-(int64_t)max_row, (int64_t)n_total);
            const int fk = (int)pick(0, 7);
            fracs[k] = all_zero || fk == 0 ? 0.0 : fk == 1 ? edge[rng() % 5] : (double)pick(1, 1023) / 1024.0;
        }
        zero_fracs += all_zero;
        ScoreRowsPlan P;
        const int64_t rc = score_rows_plan(onsets.data(), with_lengths ? lengths.data() : nullptr, samples.data(), rows.data(), n, n_total, whole, budget, P, {fracs.data()});
        cases++;
        bool ok = rc == -1;
        auto length = [&](size_t k) { return with_lengths ? lengths[k] : (int64_t)samples[k]; };
        auto span = [&](size_t k, int64_t &lo, int64_t &hi) {  // brute force, in __int128 so that the check itself cannot overflow
            const __int128 on = onsets[k], len = length(k), end = on + len + (fracs[k] != 0.0 && len > 0 ? 1 : 0);
            __int128 a = on < 0 ? (__int128)0 : on, b = end < (__int128)n_total ? end : (__int128)n_total;
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
            if (on) {
                ok &= P.voices[k].onset == onsets[k] && P.voices[k].row == rows[k] && rows[k] != 0 && P.voices[k].stride == samples[k] && samples[k] >= 1;
                ok &= P.voices[k].pad == (fracs[k] != 0.0 ? (uint32_t)length(k) : 0u) && (fracs[k] == 0.0 || P.voices[k].pad >= 1);
                two_taps += fracs[k] != 0.0;
                if (fracs[k] != 0.0 && onsets[k] == -length(k)) { tail_only++; ok &= lo == 0 && hi == 1; }
            } else if (first_listed < n) ok &= P.voices[k].row == rows[first_listed];  // readable, whatever voice k's own row is
            if (!on && fracs[k] == 0.0 && length(k) > 0) ok &= onsets[k] >= (int64_t)n_total || onsets[k] <= -length(k);
        }
        if (u_hi <= u_lo) u_lo = u_hi = 0;
        ok &= P.t_lo == u_lo && P.t_hi == u_hi;
        ok &= whole ? (P.w_lo == 0 && P.w_hi == (int64_t)n_total) : (P.w_lo == u_lo && P.w_hi == u_hi);
        if (P.w_hi > P.w_lo) {
            const uint64_t B = (uint64_t)1 << P.block_shift;
            ok &= P.block_shift >= kScoreGroupShift && P.first_block == (uint64_t)P.w_lo / B;
            const uint64_t want_blocks = ((uint64_t)P.w_hi - 1) / B - P.first_block + 1;
            ok &= P.n_blocks() == want_blocks && P.block_first[0] == 0 && P.block_first.back() + kScoreEntryPad == P.entries.size();
            ok &= P.bytes() <= budget || want_blocks == 1;  // (the weights, 16 bytes a voice, come on top: not counted)
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
            for (size_t k = 0; k < kScoreEntryPad; k++) ok &= P.entries[P.n_entries() + k] == 0;
        } else {
            ok &= P.entries.empty() && P.n_blocks() == 0 && P.n_entries() == 0;
        }
        if (all_zero) {  // all fractions zero: the plan made without fractions, record for record
            ScoreRowsPlan Q;
            ok &= score_rows_plan(onsets.data(), with_lengths ? lengths.data() : nullptr, samples.data(), rows.data(), n, n_total, whole, budget, Q, {}) == -1;
            ok &= Q.block_first == P.block_first && Q.entries == P.entries && Q.w_lo == P.w_lo && Q.w_hi == P.w_hi && Q.t_lo == P.t_lo && Q.t_hi == P.t_hi &&
                  Q.block_shift == P.block_shift && Q.first_block == P.first_block && Q.voices.size() == P.voices.size() &&
                  (n == 0 || memcmp(Q.voices.data(), P.voices.data(), n * sizeof(ScoreRow)) == 0);
        }
        if (!ok) { bad++; printf("MISMATCH round %d n %zu max_row %llu n_total %llu whole %d budget %zu\n", round, n, (unsigned long long)max_row, (unsigned long long)n_total, (int)whole, budget); }
    }
    {   // the weights: w0 is the IEEE subtraction, 16 bytes a voice; a bad length is still reported by its index
        const ScoreFrac w = score_frac_weights(0x1p-53), h = score_frac_weights(0.5), z = score_frac_weights(1.0 - 0x1p-53);
        cases += 4;
        bad += !(w.w1 == 0x1p-53 && w.w0 == 1.0 - 0x1p-53 && h.w0 == 0.5 && h.w1 == 0.5 && z.w0 == 0x1p-53 && sizeof(ScoreFrac) == 16 && alignof(ScoreFrac) == 16);
        int64_t on[3] = {0, 5, INT64_MAX}, len[3] = {4, 9, 2};
        uint32_t samples[3] = {4, 8, 2};
        double fr[3] = {0.25, 0.5, 0.75};
        ScoreRowsPlan P;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {fr}) != 1;
        len[1] = 8;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {fr}) != -1;
        bad += !(P.voices[0].hi == 5 && P.voices[0].pad == 4 && P.voices[1].hi == 14 && P.voices[2].hi == 0 && P.t_hi == 14);
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"far_onsets\": %ld, \"tail_only\": %ld, \"two_taps\": %ld, \"zero_fracs\": %ld}\n", cases, bad, doubled, far_onsets,
           tail_only, two_taps, zero_fracs);
    return bad != 0;
}
