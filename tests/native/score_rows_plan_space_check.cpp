// score_rows_plan_space_check.cpp — score_rows_plan of dusp_amd/csrc/score_plan.hpp WITH TAPS (a whole shift and a two-tap flag per voice
// and channel: Space placement) against brute force, on the CPU, in score_rows_plan_frac_check.cpp's style.  Over some thousands of
// random tiles every block's list is exactly the ascending set of the voices whose span — the hull of the channels' spans,
// [onset + min shift, onset + max(shift + len + (w1 != 0))) — clipped to the timeline intersects the block; the union window is the
// clipped spans' hull; a record carries pad = len (the UNCLIPPED length) whether or not a tap has a fraction; onsets near +-2^62 and at
// the int64 limits take part with shifts up to 2^24 on top (-fsanitize=undefined: an overflow is an error); channels whose spans are
// disjoint (one in front of the timeline or behind it, shifts 2^24 apart) are listed by their hull; a record in no list carries the
// first listed voice's row; a small byte budget is honoured by doubling the block, and the block is the smallest that fits; taps that
// are all zero shifts without fractions list exactly what the plan without taps lists; a call without taps is untouched.  Built with
// -fsanitize=address,undefined by tests/test_space_host.py.
// Prints {"cases": n, "bad": m, "doubled": d, "far_onsets": f, "disjoint": j, "two_taps": w, "zero_taps": z}.
#include "../../dusp_amd/csrc/score_plan.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>

using namespace dusp;

int main() {
    std::mt19937_64 rng(29);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    long cases = 0, bad = 0, doubled = 0, far_onsets = 0, disjoint = 0, two_taps = 0, zero_taps = 0;
    const int64_t far[] = {INT64_MAX, INT64_MIN, INT64_MAX - 5, INT64_MIN + 5, (int64_t)1 << 62, -((int64_t)1 << 62), INT64_MAX - kScoreSpaceShiftMax, INT64_MIN + kScoreSpaceShiftMax};
    const double edge[] = {0.5, 0x1p-24, 1.0 - 0x1p-53, 0.25};
    for (int round = 0; round < 6000; round++) {
        const size_t n = (size_t)pick(0, round % 7 == 0 ? 300 : 40), C = (size_t)pick(1, 8);
        const uint64_t max_row = (uint64_t)pick(1, round % 5 == 0 ? 5000 : 700), n_total = (uint64_t)pick(1, round % 3 == 0 ? 20000 : 3000);
        const bool with_lengths = round % 2 == 0, whole = round % 4 < 2, all_zero = round % 13 == 0;
        const size_t budget = round % 6 == 0 ? (size_t)pick(0, 2000) : round % 6 == 1 ? n * sizeof(ScoreRow) + (size_t)pick(8, 4000) : kScorePlanBytes;
        std::vector<int64_t> onsets(n), lengths(n);
        std::vector<uint32_t> samples(n);
        std::vector<uint64_t> rows(n);
        std::vector<ScoreSpaceTap> taps(n * C);
        for (size_t k = 0; k < n; k++) {
            const int rk = (int)pick(0, 7);
            samples[k] = rk == 0 ? 0u : rk == 1 ? 1u : rk == 2 ? (uint32_t)max_row : (uint32_t)pick(0, (int64_t)max_row);
            rows[k] = samples[k] ? 0x1000 + 0x100 * (uint64_t)k : 0;
            const int lk = (int)pick(0, 9);
            lengths[k] = lk == 0 ? 0 : lk == 1 ? std::min<int64_t>(1, samples[k]) : lk == 2 ? (int64_t)samples[k] : pick(0, (int64_t)samples[k]);
            const int64_t len = with_lengths ? lengths[k] : (int64_t)samples[k];
            const int kind = (int)pick(0, 13);
            if (kind == 0) { onsets[k] = far[rng() % 8]; far_onsets++; }
            else if (kind == 1) onsets[k] = pick(-(int64_t)samples[k] - 3, 3);
            else if (kind == 2) onsets[k] = pick((int64_t)n_total - 3, (int64_t)n_total + 3);
            else if (kind == 3) onsets[k] = pick(0, 8) * 256 - pick(0, 1);
            else if (kind == 4) onsets[k] = -len - pick(0, 700);                  // in front of the timeline: only a shift brings it back
            else if (kind == 5) onsets[k] = (int64_t)n_total - len - pick(0, 3);
            else if (kind == 6) onsets[k] = -kScoreSpaceShiftMax - len + pick(-2, 2);  // only the largest shift reaches sample 0
            else onsets[k] = pick(-(int64_t)max_row, (int64_t)n_total);
            const int tk = (int)pick(0, 5);  // how the channels' shifts lie: 0 all zero, 1 small, 2 one channel 2^24 away (disjoint spans), 3 spread over the timeline, else mixed
            for (size_t c = 0; c < C; c++) {
                int64_t shift = tk == 0 ? 0 : tk == 1 ? pick(0, 700) : tk == 2 ? (c == C - 1 ? kScoreSpaceShiftMax - pick(0, 1) : pick(0, 3)) : tk == 3 ? pick(0, (int64_t)n_total + 5) : pick(0, 1) * pick(0, 2000);
                const int fk = (int)pick(0, 5);
                double frac = all_zero || fk == 0 ? 0.0 : fk == 1 ? edge[rng() % 4] : (double)pick(1, 1023) / 1024.0;
                if (all_zero) shift = 0;
                if (shift == kScoreSpaceShiftMax) frac = 0.0;  // (a delay is at most 2^24)
                const double D = (double)shift + frac;  // (rounded where shift + frac is no double: the tap is made from D, as on the host)
                const ScoreSpaceTap T = score_space_tap(D, 0.5);
                if (T.shift != (int64_t)std::floor(D) || T.w1 != D - std::floor(D) || T.w0 != 1.0 - T.w1 || T.shift < 0 || T.shift > kScoreSpaceShiftMax || T.w1 < 0.0 || T.w1 >= 1.0) bad++;
                taps[k * C + c] = T;
            }
        }
        zero_taps += all_zero;
        ScoreRowsPlan P;
        const int64_t rc = score_rows_plan(onsets.data(), with_lengths ? lengths.data() : nullptr, samples.data(), rows.data(), n, n_total, whole, budget, P, {nullptr, taps.data(), C});
        cases++;
        bool ok = rc == -1;
        auto length = [&](size_t k) { return with_lengths ? lengths[k] : (int64_t)samples[k]; };
        auto span = [&](size_t k, int64_t &lo, int64_t &hi) {  // brute force, in __int128 so that the check itself cannot overflow
            const __int128 on = onsets[k], len = length(k);
            lo = hi = 0;
            if (len == 0) return false;
            __int128 a = 0, b = 0;
            bool covered = false;  // does any CHANNEL reach the timeline?  (the hull may, where no channel does: then the voice may be listed or not)
            for (size_t c = 0; c < C; c++) {
                const ScoreSpaceTap &T = taps[k * C + c];
                const __int128 ca = on + T.shift, cb = ca + len + (T.w1 != 0.0 ? 1 : 0);
                if (c == 0 || ca < a) a = ca;
                if (c == 0 || cb > b) b = cb;
                covered |= ca < (__int128)n_total && cb > 0;
            }
            (void)covered;
            if (a < 0) a = 0;
            if (b > (__int128)n_total) b = (__int128)n_total;
            if (b <= a) return false;
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
                ok &= P.voices[k].pad == (uint32_t)length(k) && P.voices[k].pad >= 1;
                int64_t lo_shift = INT64_MAX, hi_shift = 0;
                for (size_t c = 0; c < C; c++) {
                    two_taps += taps[k * C + c].w1 != 0.0;
                    lo_shift = std::min(lo_shift, taps[k * C + c].shift);
                    hi_shift = std::max(hi_shift, taps[k * C + c].shift);
                }
                disjoint += hi_shift - lo_shift > length(k) + 1;
            } else {
                ok &= P.voices[k].onset == 0 && P.voices[k].pad == 0;  // (a record in no list: the kernel finds it covers nothing)
                if (first_listed < n) ok &= P.voices[k].row == rows[first_listed];
            }
        }
        if (u_hi <= u_lo) u_lo = u_hi = 0;
        ok &= P.t_lo == u_lo && P.t_hi == u_hi;
        ok &= whole ? (P.w_lo == 0 && P.w_hi == (int64_t)n_total) : (P.w_lo == u_lo && P.w_hi == u_hi);
        if (P.w_hi > P.w_lo) {
            const uint64_t B = (uint64_t)1 << P.block_shift;
            ok &= P.block_shift >= kScoreGroupShift && P.first_block == (uint64_t)P.w_lo / B;
            const uint64_t want_blocks = ((uint64_t)P.w_hi - 1) / B - P.first_block + 1;
            ok &= P.n_blocks() == want_blocks && P.block_first[0] == 0 && P.block_first.back() + kScoreEntryPad == P.entries.size();
            ok &= P.bytes() <= budget || want_blocks == 1;  // (the taps, 32 bytes a voice and channel, come on top: not counted)
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
        if (all_zero) {  // no shift and no fraction anywhere: the lists of the plan made without taps; only pad differs (len, not 0)
            ScoreRowsPlan Q;
            ok &= score_rows_plan(onsets.data(), with_lengths ? lengths.data() : nullptr, samples.data(), rows.data(), n, n_total, whole, budget, Q, {}) == -1;
            ok &= Q.block_first == P.block_first && Q.entries == P.entries && Q.w_lo == P.w_lo && Q.w_hi == P.w_hi && Q.t_lo == P.t_lo && Q.t_hi == P.t_hi &&
                  Q.block_shift == P.block_shift && Q.first_block == P.first_block && Q.voices.size() == P.voices.size();
            for (size_t k = 0; ok && k < n; k++)
                ok &= Q.voices[k].onset == P.voices[k].onset && Q.voices[k].lo == P.voices[k].lo && Q.voices[k].hi == P.voices[k].hi && Q.voices[k].row == P.voices[k].row &&
                      Q.voices[k].pad == 0;
        }
        if (!ok) { bad++; printf("MISMATCH round %d n %zu C %zu max_row %llu n_total %llu whole %d budget %zu\n", round, n, C, (unsigned long long)max_row, (unsigned long long)n_total, (int)whole, budget); }
    }
    {   // the tap: the half the addresses need is the second 16 bytes; a bad length is still reported by its index
        const ScoreSpaceTap t = score_space_tap(256.25, -0.75), z = score_space_tap(0.0, 1.0), top = score_space_tap(16777216.0, 2.0), tiny = score_space_tap(0x1p-24, 1.0);
        cases += 5;
        bad += !(t.shift == 256 && t.w1 == 0.25 && t.w0 == 0.75 && t.gain == -0.75 && z.shift == 0 && z.w1 == 0.0 && z.w0 == 1.0);
        bad += !(top.shift == kScoreSpaceShiftMax && top.w1 == 0.0 && tiny.shift == 0 && tiny.w1 == 0x1p-24 && tiny.w0 == 1.0 - 0x1p-24);
        bad += !(sizeof(ScoreSpaceTap) == 32 && alignof(ScoreSpaceTap) == 32 && offsetof(ScoreSpaceTap, w1) == 16 && offsetof(ScoreSpaceTap, shift) == 24);
        int64_t on[3] = {0, 5, INT64_MAX}, len[3] = {4, 9, 2};
        uint32_t samples[3] = {4, 8, 2};
        const ScoreSpaceTap T[6] = {score_space_tap(0.0, 1.0), score_space_tap(10.5, 1.0), score_space_tap(1.0, 1.0), score_space_tap(2.0, 1.0), score_space_tap(0.0, 1.0), score_space_tap(16777216.0, 1.0)};
        ScoreRowsPlan P;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {nullptr, T, 2}) != 1;
        len[1] = 8;
        bad += score_rows_plan(on, len, samples, nullptr, 3, 100, true, kScorePlanBytes, P, {nullptr, T, 2}) != -1;
        bad += !(P.voices[0].lo == 0 && P.voices[0].hi == 15 && P.voices[0].pad == 4 && P.voices[1].lo == 6 && P.voices[1].hi == 15 && P.voices[2].hi == 0 && P.t_hi == 15);
    }
    printf("{\"cases\": %ld, \"bad\": %ld, \"doubled\": %ld, \"far_onsets\": %ld, \"disjoint\": %ld, \"two_taps\": %ld, \"zero_taps\": %ld}\n", cases, bad, doubled, far_onsets,
           disjoint, two_taps, zero_taps);
    return bad != 0;
}
