// abi_piece.hip — the C ABI (include/dusp_hip.h): the host renders of a PIECE — the voices of several instruments (parts) placed into one
// timeline: dusp_render_host_score_parts and its pan, frac, space and stereo forms, and dusp_render_host_score_piece, which is all of
// them and takes a master, with _buses (effect sends, 6.15), _tracks (sub-mixes, 6.16), _stems (every signal beside the
// mix, 6.17), _meters (6.18) and _loudness (true peaks, and a delivery at a loudness target: 6.19).  One record of the call (PieceCall) and one driver, render_host_score_parts, that reads as its stages:
// check, tiles, plans, buffers, render, finish.  Behind them what a master, the buses, the tracks and the stems are held to and do.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <memory>

#include "abi_score.hpp"
#include "render_plan.hpp"

namespace {  // (nothing of this file but its entries is a symbol of the library)

// ---- the call ----

// What an entry was called with.  The optional features are here and nowhere else: a stage takes the call, not a pointer a feature
struct PieceCall {
    const char *who;
    const dusp_score_part *parts;
    size_t n_parts, n_voices;
    const uint32_t *h_part_of;  // voice k of the chain: the next unused instance of part h_part_of[k]
    const int64_t *h_onsets, *h_lengths;
    const float *h_gains;
    ScorePlacement place;  // (with per-voice sends: their levels too; a stereo piece: the voices' channels, made from the parts')
    size_t n_total, tile_bytes;
    int format, normalise;
    void *h_out;
    float *h_peak;  // (with stems: one a signal)
    const dusp_score_master *master = nullptr;  // dusp_render_host_score_piece: a mono circuit over every channel of the raw timeline
    const dusp_score_buses *buses = nullptr;    // ..._buses
    const dusp_score_tracks *tracks = nullptr;  // ..._tracks
    const dusp_score_stems *stems = nullptr;    // ..._stems: h_out takes 1 + tracks + buses + 1 signals and h_peak as many peaks
    const dusp_score_meters *meters = nullptr;  // ..._meters
    const dusp_score_loudness *loud = nullptr;  // ..._loudness: the true peak of every delivered (signal, channel), and with deliver the one gain
    const dusp_score_limiter *limiter = nullptr;  // ..._limiter: the delivered signals limited to the ceiling in front of that gain
    size_t release = 0;                           // ..._limiter_release: the limiter's release in samples (0: none of its own)

    dusp_program *prog0() const { return parts[0].prog; }  // (its buffers hold what belongs to the piece: the timeline, the gains, the encoded frames)
    dusp_ctx *ctx() const { return parts[0].prog->ctx; }
    size_t n_buses() const { return buses ? buses->n_buses : 0; }
    size_t n_tracks() const { return tracks ? tracks->n_tracks : 0; }
};

// What the checks of a call yield beside their verdict
struct PieceFacts {
    size_t n_out_ch = 0, timeline = 0;  // the timeline's channels, and its floats
    std::vector<size_t> part_ch;        // a part's own channels (they differ in a stereo piece only)
    std::vector<size_t> instance_of;    // voice k is instance instance_of[k] of its part
    std::vector<uint32_t> row_channels; // (a stereo piece: the voices' own)
    std::vector<size_t> slot_of;        // (with tracks: where track g's timeline lies in d_mix_tracks)
    size_t n_signals = 0;               // (with stems: the direct mix, the tracks, the buses' returns, and the mix last)
    uint32_t sample_rate = 0;           // the parts': what a call with meters is metered at
};

// the batches of a call, which stand until the delivery has waited for the stream: the parts' first — part p's is batches[p], decided
// from the WHOLE part — then the track programs', the buses', the master's
using PieceBatches = std::vector<std::unique_ptr<TiledBatch>>;

// ---- the master of a piece: one mono circuit over every channel of the timeline ----

// how the messages name what is held to a master's rules ("bus 2", "a bus"), and whose timeline it reads ("send ", "track "; a master: "")
struct ScoreNoun {
    std::string the, a, heard;
};

// What a piece's master is held to before anything renders; n_ch: the timeline's channels, each an instance of the master.  A bus and
// a track program are held to the same rules in the same words but for the noun
static int score_master_check(const PieceCall &call, const dusp_score_master *master, size_t n_ch, const ScoreNoun &noun) {
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who), &the = noun.the, &a = noun.a, &heard = noun.heard;
    const size_t n_total = call.n_total;
    dusp_program *m = master->prog;
    if (!m) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + "'s program is NULL");
    if (m->ctx != ctx) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " was built on another context: it shares the one of the piece's parts");
    for (size_t p = 0; p < call.n_parts; p++)
        if (call.parts[p].prog == m)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also part " + std::to_string(p) + ": its buffers would be used twice; build it on its own");
    if (m->P.g.n_inputs != 1)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + a + " reads exactly one input stream (the " + heard + "timeline's channel), this program has " + std::to_string(m->P.g.n_inputs));
    if (m->P.out_bufs.size() != 1)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + a + " has one output channel, this program has " + std::to_string(m->P.out_bufs.size()) +
                                        ": it is applied to every channel of the timeline by itself");
    if (m->resumable)
        CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": a resumable program (DUSP_ENGINE_RESUMABLE) is not " + a + ": every call renders it from its initial state");
    if (m->P.g.n_params > 0 && !master->h_params) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " has parameters but its h_params is NULL");
    if (!samples_in_range(n_total) || n_ch * n_total > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " renders channels x timeline samples, which must not exceed 2^31: render such a piece in windows of the timeline without " + a);
    return DUSP_OK;
}

// What the buses of a piece are held to before anything renders: their number and levels (and what sends do not go with), every
// rule of a master per bus, and a bus that is also the master or another bus
static int score_buses_check(const PieceCall &call, size_t n_ch) {
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who);
    const dusp_score_buses *buses = call.buses;
    const dusp_score_master *master = call.master;
    if (!call.tracks) {  // (per-voice levels, which travel with the placement)
        if (int rc = call.place.check_sends(ctx, call.who, call.n_voices)) return rc;
    } else if (buses->n_buses < 1 || buses->n_buses > dusp::kScoreBusMax) {  // (a call with tracks: the levels are the tracks', score_tracks_check)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 4 buses, not " + std::to_string(buses->n_buses));
    }
    if (!buses->buses) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the buses' programs are NULL");
    for (size_t b = 0; b < buses->n_buses; b++) {
        const std::string the = "bus " + std::to_string(b);
        if (int rc = score_master_check(call, &buses->buses[b], n_ch, ScoreNoun{the, "a bus", "send "})) return rc;
        if (master && master->prog == buses->buses[b].prog)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also the master: its buffers would be used twice; build it on its own");
        for (size_t q = 0; q < b; q++)
            if (buses->buses[q].prog == buses->buses[b].prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": buses " + std::to_string(q) + " and " + std::to_string(b) + " are the same program: its buffers would be used twice; build it twice");
    }
    return DUSP_OK;
}

// What a host render with buses does between its last tile and its delivery: every bus in turn rendered over its RAW send timeline
// (d_mix_sends [b], [n_ch][n_total]: channel c the one input stream of instance c) from its initial state into its own d_host_out, as a
// master is (`|| 0` at its own copy-out), then ONE return launch that adds the buses' outputs onto the dry sums in d_mix, left-deep:
// raw where a master follows (which reads the sums as they stand), else with the `|| 0` a delivery without buses applies by a launch
// of its own.  rendered: the buses' batches.
// With stems (d_stem_buses given): the same sum into d_out (nullptr: d_mix in place), every bus's output kept in its slot, d_stem_buses +
// b * the timeline, and — d_stem_direct given: per-note sends, whose dry timeline has no slot yet — dry || 0.
static int score_buses_return(dusp_program *prog, const dusp_score_buses *buses, size_t n_ch, size_t n_total, int raw, PieceBatches &rendered, float *d_out,
                              float *d_stem_direct, float *d_stem_buses) {
    dusp_ctx *ctx = prog->ctx;
    const float *wets[dusp::kScoreBusMax] = {nullptr, nullptr, nullptr, nullptr};
    float *slots[dusp::kScoreBusMax] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t b = 0; b < buses->n_buses; b++) {
        rendered.emplace_back(new TiledBatch(buses->buses[b].prog, n_ch, buses->buses[b].h_params, nullptr, n_ch));  // (one tile: all channels)
        if (int rc = rendered.back()->render_tile(0, n_ch, n_total, prog->d_mix_sends.p + b * n_ch * n_total)) return rc;
        wets[b] = buses->buses[b].prog->d_host_out.p;
        if (d_stem_buses) slots[b] = d_stem_buses + b * n_ch * n_total;
    }
    HIP_TRY(ctx, dusp::launch_score_return(prog->d_mix.p, wets, (uint32_t)buses->n_buses, d_out ? d_out : prog->d_mix.p, d_stem_direct, d_stem_buses ? slots : nullptr,
                                           (uint64_t)n_ch * n_total, raw, ctx->stream));
    return DUSP_OK;
}

// ---- the tracks of a piece: sub-mixes through circuits of their own (dusp_amd/mix.py track_mix) ----

// What the tracks of a piece are held to before anything renders: their number, where every voice goes, the faders and levels, what
// tracks do not go with, every rule of a master per track program ("track program p"), a program that is used twice, and the tracks
// every program lists.  slot_of[g]: where track g's timeline lies in d_mix_tracks — the tracks of one program adjacent, in the
// program's order, the tracks without a circuit behind them
static int score_tracks_check(const PieceCall &call, size_t n_ch, std::vector<size_t> &slot_of) {
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who);
    const dusp_score_tracks *tracks = call.tracks;
    const dusp_score_buses *buses = call.buses;
    const dusp_score_master *master = call.master;
    const size_t n_voices = call.n_voices, n_total = call.n_total;
    const size_t T = tracks->n_tracks;
    if (T < 1 || T > dusp::kScoreTrackMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": a call has 1 .. 8 tracks, not " + std::to_string(T));
    if (!tracks->h_track_of) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the tracks' h_track_of is NULL: every voice goes to a track or, with -1, straight to the mix");
    for (size_t k = 0; k < n_voices; k++)
        if (tracks->h_track_of[k] < -1 || tracks->h_track_of[k] >= (int64_t)T)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + " names track " + std::to_string(tracks->h_track_of[k]) + " of " + std::to_string(T) +
                                            ": track_of holds -1 (straight to the mix) or a track, 0 .. " + std::to_string(T - 1));
    for (size_t g = 0; tracks->h_faders && g < T; g++)
        if (!std::isfinite(tracks->h_faders[g])) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the fader of track " + std::to_string(g) + " is not finite");
    if (tracks->h_track_sends && !buses) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": track_sends without buses: a level is what a track gives to a bus");
    if (buses && !tracks->h_track_sends)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": buses without track_sends: with tracks every bus needs a level a track (track_sends of shape (buses, tracks))");
    if (buses && buses->h_sends)
        CTX_FAIL(ctx, DUSP_ERR_UNSUPPORTED, w + ": sends and tracks do not go together: with tracks the buses are fed by track_sends, a level a track");
    for (size_t b = 0; buses && b < buses->n_buses; b++)
        for (size_t g = 0; g < T; g++)
            if (!std::isfinite(tracks->h_track_sends[b * T + g]))
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the level of track " + std::to_string(g) + " into bus " + std::to_string(b) + " is not finite");
    if (tracks->n_programs > T) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + std::to_string(tracks->n_programs) + " track programs for " + std::to_string(T) + " tracks: a program serves at least one track");
    if (tracks->n_programs && !tracks->programs) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the tracks' programs are NULL");
    slot_of.assign(T, T);
    size_t slot = 0;
    for (size_t p = 0; p < tracks->n_programs; p++) {
        const dusp_score_track_program &tp = tracks->programs[p];
        const std::string the = "track program " + std::to_string(p);
        const dusp_score_master as_master{tp.prog, tp.h_params};
        if (int rc = score_master_check(call, &as_master, n_ch, ScoreNoun{the, "a track program", "track "})) return rc;
        if (master && master->prog == tp.prog) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also the master: its buffers would be used twice; build it on its own");
        for (size_t b = 0; buses && b < buses->n_buses; b++)
            if (buses->buses[b].prog == tp.prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " is also bus " + std::to_string(b) + ": its buffers would be used twice; build it on its own");
        for (size_t q = 0; q < p; q++)
            if (tracks->programs[q].prog == tp.prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": track programs " + std::to_string(q) + " and " + std::to_string(p) + " are the same program: its buffers would be used twice; build it twice");
        if (tp.n_tracks < 1 || !tp.h_tracks) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " lists no tracks: a track program serves at least one");
        for (size_t j = 0; j < tp.n_tracks; j++) {
            const size_t g = tp.h_tracks[j];
            if (g >= T) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " lists track " + std::to_string(g) + " of " + std::to_string(T));
            if (slot_of[g] != T) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " lists track " + std::to_string(g) + ", which has a circuit already: a track goes through one");
            slot_of[g] = slot++;
        }
        if (tp.n_tracks * n_ch * n_total > dusp::kScoreRowMax)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + the + " renders (tracks x channels) x timeline samples, which must not exceed 2^31: give tracks of one circuit programs of their own, or render such a piece in windows of the timeline");
    }
    for (size_t g = 0; g < T; g++)
        if (slot_of[g] == T) slot_of[g] = slot++;
    return DUSP_OK;
}

// What a host render with tracks does between its last tile and its buses: every track program rendered ONCE over the adjacent RAW
// timelines of its tracks (d_mix_tracks: instance j * n_ch + c hears channel c of its j-th track) from its initial state into its own
// d_host_out, as a master is (`|| 0` at its own copy-out); then ONE launch of the mix kernel: the direct timeline in d_mix and every
// track's output — its program's, or its raw timeline where it has no circuit — times its fader, left-deep into d_mix in place, and
// times its levels into the buses' feeds (d_mix_sends, from +0).  raw: buses or a master follow, which read the sums as they stand.
// With stems (d_stems given): the same mix into d_out (nullptr: d_mix in place), direct || 0 kept in slot 0 of d_stems and every track's
// term || 0 in slot 1 + g, a slot the timeline's floats.
static int score_tracks_mix(const PieceCall &call, const std::vector<size_t> &slot_of, size_t n_ch, int raw, PieceBatches &rendered, float *d_out, float *d_stems) {
    dusp_program *prog = call.prog0();
    dusp_ctx *ctx = prog->ctx;
    const dusp_score_tracks *tracks = call.tracks;
    const dusp_score_buses *buses = call.buses;
    const size_t n_total = call.n_total;
    const size_t row = n_ch * n_total;
    const float *y[dusp::kScoreTrackMax] = {};
    float *slots[dusp::kScoreTrackMax] = {};
    for (size_t g = 0; g < tracks->n_tracks; g++) {
        y[g] = prog->d_mix_tracks.p + slot_of[g] * row;
        if (d_stems) slots[g] = d_stems + (1 + g) * row;
    }
    for (size_t p = 0; p < tracks->n_programs; p++) {
        const dusp_score_track_program &tp = tracks->programs[p];
        const size_t n_inst = tp.n_tracks * n_ch;
        rendered.emplace_back(new TiledBatch(tp.prog, n_inst, tp.h_params, nullptr, n_inst));  // (one tile: every track and channel)
        if (int rc = rendered.back()->render_tile(0, n_inst, n_total, prog->d_mix_tracks.p + slot_of[tp.h_tracks[0]] * row)) return rc;
        for (size_t j = 0; j < tp.n_tracks; j++) y[tp.h_tracks[j]] = tp.prog->d_host_out.p + j * row;
    }
    HIP_TRY(ctx, dusp::launch_score_tracks(prog->d_mix.p, y, tracks->h_faders, tracks->h_track_sends, (uint32_t)tracks->n_tracks, buses ? (uint32_t)buses->n_buses : 0u,
                                           d_out ? d_out : prog->d_mix.p, nullptr, buses ? prog->d_mix_sends.p : nullptr, d_stems, d_stems ? slots : nullptr, (uint64_t)row, raw,
                                           ctx->stream));
    return DUSP_OK;
}

// ---- the stages of a host render ----

// check, the parts: each a program of the call's context that fits the placement, none twice.  -> their channels, and how many
// instances they list together
static int piece_check_parts(const PieceCall &call, size_t n_ch, PieceFacts &F, size_t &n_listed) {
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who);
    const dusp_score_part *parts = call.parts;
    const bool stereo = call.place.kind == ScoreKind::stereo, panned = call.place.kind == ScoreKind::pan, taps = call.place.kind == ScoreKind::space;
    std::vector<size_t> &part_ch = F.part_ch;
    part_ch.assign(call.n_parts, n_ch);
    for (size_t p = 0; p < call.n_parts; p++) {
        if (!parts[p].prog) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the program of part " + std::to_string(p) + " is NULL");
        if (parts[p].prog->ctx != ctx) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " was built on another context: all parts of a piece share one");
        part_ch[p] = parts[p].prog->P.out_bufs.size();
        if (stereo && part_ch[p] != 1 && part_ch[p] != 2)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(part_ch[p]) + " output channels: a voice of a stereo piece has one or two");
        if ((panned || taps) && part_ch[p] != 1)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(part_ch[p]) + " output channels: a " + (panned ? "panned" : "placed") + " voice is mono");
        if (!stereo && part_ch[p] != n_ch)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": part " + std::to_string(p) + " has " + std::to_string(part_ch[p]) + " output channels, part 0 has " + std::to_string(n_ch) +
                                            ": all parts of a piece have the same number");
        for (size_t q = 0; q < p; q++)
            if (parts[q].prog == parts[p].prog)
                CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": parts " + std::to_string(q) + " and " + std::to_string(p) + " are the same program: its tile buffer would be used twice; make them one part or build it twice");
        n_listed += parts[p].n_instances;
    }
    return DUSP_OK;
}

// check, what the call delivers: the signals of a call with stems, and what a call with meters sized its arrays for
static int piece_check_delivery(const PieceCall &call, PieceFacts &F) {
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who);
    const dusp_score_stems *stems = call.stems;
    const dusp_score_meters *meters = call.meters;
    const size_t n_signals = F.n_signals = 1 + call.n_tracks() + call.n_buses() + 1;
    if (stems && stems->n_signals != n_signals)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the stems' n_signals is " + std::to_string(stems->n_signals) + ", the call delivers " + std::to_string(n_signals) + ": the direct mix, " +
                                        std::to_string(call.n_tracks()) + " tracks, " + std::to_string(call.n_buses()) + " buses and the mix");
    if (stems && !call.h_out) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_out is NULL: a call with stems delivers its " + std::to_string(n_signals) + " signals there");
    const uint32_t rate = F.sample_rate = (uint32_t)call.prog0()->P.g.sample_rate;
    if (meters) {
        const size_t n_metered = stems ? n_signals : 1, n_blocks = dusp::meter_blocks(call.n_total, rate);
        if (rate < dusp::kMeterRateMin)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": meters need a sample rate of at least 8000 Hz, not " + std::to_string(rate) + ": the K-weighting's shelf lies at 1682 Hz");
        if (meters->n_signals != n_metered)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' n_signals is " + std::to_string(meters->n_signals) + ", the call delivers " + std::to_string(n_metered) +
                                            (stems ? ": its stems and the mix" : ": the mix"));
        if (meters->n_blocks != n_blocks)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' n_blocks is " + std::to_string(meters->n_blocks) + ", a timeline of " + std::to_string(call.n_total) + " samples at " +
                                            std::to_string(rate) + " Hz has " + std::to_string(n_blocks) + " blocks (dusp_meter_blocks)");
        if (!meters->h_rms) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' h_rms is NULL: every signal's RMS a channel goes there");
        if (!meters->h_lufs) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the meters' h_lufs is NULL: every signal's loudness goes there");
    }
    return DUSP_OK;
}

// check: every refusal of a call, before anything renders, in this order — which refusal a call with several faults gets is behaviour
// (tests/test_gpu_piece_precedence.py) — and what the later stages need to know.  The call's placement gets what travels with it: the
// per-voice levels of buses without tracks, and the voices' channels of a stereo piece
static int piece_check(PieceCall &call, PieceFacts &F) {
    dusp_ctx *ctx = call.ctx();
    const char *who = call.who;
    const std::string w(who);
    const dusp_score_part *parts = call.parts;
    const size_t n_parts = call.n_parts, n_voices = call.n_voices, n_total_samples = call.n_total;
    const uint32_t *h_part_of = call.h_part_of;
    ScorePlacement &place = call.place;
    const size_t n_ch = call.prog0()->P.out_bufs.size();  // (a voice's)
    if (call.buses && !call.tracks) {  // (the levels travel with the placement: a tile's are its voices'; with tracks the levels are the tracks')
        place.n_buses = call.buses->n_buses;
        place.sends_stride = n_voices;
        place.h_sends = call.buses->h_sends;
    }
    if (!h_part_of || !call.h_onsets) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_part_of or h_onsets is NULL");
    if (n_voices < 1 || n_voices > (1u << 24)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": need 1..2^24 voices");
    if (int rc = place.check_taps(ctx, who, n_voices, n_total_samples)) return rc;
    const size_t n_out_ch = F.n_out_ch = place.timeline_channels(n_ch);
    F.timeline = n_out_ch * n_total_samples;
    size_t n_listed = 0;
    if (int rc = piece_check_parts(call, n_ch, F, n_listed)) return rc;
    if (call.master)
        if (int rc = score_master_check(call, call.master, n_out_ch, ScoreNoun{"the master", "a master", ""})) return rc;
    if (call.buses)
        if (int rc = score_buses_check(call, n_out_ch)) return rc;
    if (call.tracks)
        if (int rc = score_tracks_check(call, n_out_ch, F.slot_of)) return rc;
    if (int rc = piece_check_delivery(call, F)) return rc;
    if (!samples_in_range(n_total_samples) || n_out_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the timeline must have 1..2^31 samples and channels x timeline samples must not exceed 2^31: render such a piece in windows of the timeline");
    if (call.stems && F.n_signals * n_out_ch * n_total_samples > dusp::kScoreRowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": signals x channels x timeline samples must not exceed 2^31 with stems (" + std::to_string(F.n_signals) + " signals): render such a piece in windows of the timeline");
    if (int rc = place.check_values(ctx, who, n_voices)) return rc;
    // voice k of the chain: the next unused instance of part h_part_of[k]
    std::vector<size_t> used(n_parts, 0);
    F.instance_of.resize(n_voices);
    for (size_t k = 0; k < n_voices; k++) {
        if (h_part_of[k] >= n_parts) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": voice " + std::to_string(k) + " names part " + std::to_string(h_part_of[k]) + " of " + std::to_string(n_parts));
        F.instance_of[k] = used[h_part_of[k]]++;
    }
    if (place.kind == ScoreKind::stereo) {
        F.row_channels.resize(n_voices);
        for (size_t k = 0; k < n_voices; k++) F.row_channels[k] = (uint32_t)F.part_ch[h_part_of[k]];
        place.h_row_channels = F.row_channels.data();
    }
    if (int rc = place.check_kinds(ctx, who, n_voices)) return rc;
    for (size_t p = 0; p < n_parts; p++)
        if (used[p] != parts[p].n_instances || n_listed != n_voices)
            CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": h_part_of names part " + std::to_string(p) + " " + std::to_string(used[p]) + " times, the part has " +
                                            std::to_string(parts[p].n_instances) + " instances: every instance is one voice of the chain");
    for (size_t p = 0; p < n_parts; p++) {  // (the sizes the tiles are made from; tiled_batch_prepare refuses the rest, in front of any render)
        if (int rc = check_batch(ctx, who, parts[p].n_instances, parts[p].n_voice_samples)) return rc;
        if (F.part_ch[p] * parts[p].n_voice_samples > kMixRowMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": channels x voice samples must not exceed 2^31");
    }
    return DUSP_OK;
}

// check, behind every other refusal of the call (the tiles' included: a format or normalise that is none): what a call with a
// loudness record is held to
static int piece_check_loudness(const PieceCall &call, const PieceFacts &F) {
    const dusp_score_loudness *loud = call.loud;
    if (!loud) return DUSP_OK;
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who);
    if (!loud->h_true_peak) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the loudness record's h_true_peak is NULL: the true peak of every signal and channel goes there");
    if (loud->deliver && !call.meters) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": deliver at a loudness target needs meters: the gain comes from the loudness of the mix");
    if (loud->deliver && !call.format)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": deliver at a loudness target needs a PCM format, not 0: frames of DUSP_PCM_F32 are the f32 delivery at a target");
    if (loud->deliver && call.normalise != 0)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": deliver at a loudness target does not go with normalise " + std::to_string(call.normalise) + ": the target decides the gain, normalise must be 0");
    if (loud->deliver && !std::isfinite(loud->target_lufs)) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the loudness target must be a finite number of LUFS, not " + std::to_string(loud->target_lufs));
    if (loud->deliver && !(std::isfinite(loud->ceiling_dbtp) && loud->ceiling_dbtp <= 0.0))
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": the true-peak ceiling must be a finite number of dBTP at most 0, not " + std::to_string(loud->ceiling_dbtp));
    if (F.sample_rate < dusp::kMeterRateMin)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": meters need a sample rate of at least 8000 Hz, not " + std::to_string(F.sample_rate) + ": the K-weighting's shelf lies at 1682 Hz");
    return DUSP_OK;
}

// check, behind the loudness record's: what a call with a limiter is held to
static int piece_check_limiter(const PieceCall &call) {
    const dusp_score_limiter *limiter = call.limiter;
    if (!limiter) return DUSP_OK;
    dusp_ctx *ctx = call.ctx();
    const std::string w(call.who);
    if (!call.loud || !call.loud->deliver) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + dusp::kLimiterNeedsDeliver);
    if (limiter->window_samples < 1 || limiter->window_samples > dusp::kLimiterWindowMax)
        CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + dusp::kLimiterWindowRange + std::to_string(limiter->window_samples));
    if (call.release > dusp::kLimiterReleaseMax) CTX_FAIL(ctx, DUSP_ERR_ARG, w + ": " + dusp::kLimiterReleaseRange + std::to_string(call.release));
    return DUSP_OK;
}

// The tiles of a call: runs of the chain's voices whose rows together fit tile_bytes.  A part's share of tile i is its instances
// [share[p][i], share[p][i + 1]), one contiguous range since its instances enter the chain in their own order; its tile buffer holds the
// largest share
struct PieceTiles {
    std::vector<size_t> starts;  // tile i: the voices [starts[i], starts[i + 1])
    size_t n_tiles = 0;
    std::vector<std::vector<size_t>> share;
    std::vector<uint32_t> row_samples;  // a voice's samples a channel
};

// tiles: the tiles cut, the parts' shares of them, and every part's tile buffer made ready (which refuses what is left to refuse)
static int piece_tiles(const PieceCall &call, const PieceFacts &F, PieceTiles &T) {
    dusp_ctx *ctx = call.ctx();
    const dusp_score_part *parts = call.parts;
    const size_t n_parts = call.n_parts, n_voices = call.n_voices;
    const uint32_t *h_part_of = call.h_part_of;
    std::vector<uint64_t> row_bytes(n_voices);
    T.row_samples.resize(n_voices);
    size_t staged = 0, free_bytes = 0, total_bytes = 0;
    for (size_t k = 0; k < n_voices; k++) {
        T.row_samples[k] = (uint32_t)parts[h_part_of[k]].n_voice_samples;  // (at most 2^31 / channels: tiled_batch_prepare)
        row_bytes[k] = (uint64_t)F.part_ch[h_part_of[k]] * T.row_samples[k] * sizeof(float);
    }
    for (size_t p = 0; p < n_parts; p++) staged += parts[p].prog->d_host_out.cap * sizeof(float);
    if (call.tile_bytes == 0 && ctx->knobs.mix_tile_mb <= 0) HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    T.starts = dusp::piece_tile_starts(row_bytes.data(), n_voices, call.tile_bytes, ctx->knobs.mix_tile_mb, free_bytes, staged, ctx->n_cus);
    const size_t n_tiles = T.n_tiles = T.starts.size() - 1;
    T.share.assign(n_parts, std::vector<size_t>(n_tiles + 1, 0));
    std::vector<size_t> seen(n_parts, 0);
    for (size_t i = 0; i < n_tiles; i++) {
        for (size_t k = T.starts[i]; k < T.starts[i + 1]; k++) seen[h_part_of[k]]++;
        for (size_t p = 0; p < n_parts; p++) T.share[p][i + 1] = seen[p];
    }
    for (size_t p = 0; p < n_parts; p++) {
        size_t most = 1, unused = 0;
        for (size_t i = 0; i < n_tiles; i++) most = std::max(most, T.share[p][i + 1] - T.share[p][i]);
        if (int rc = tiled_batch_prepare(parts[p].prog, call.who, parts[p].n_instances, parts[p].n_voice_samples, parts[p].h_params, nullptr, most, call.format, call.normalise, call.h_out,
                                         &unused))
            return rc;
    }
    return DUSP_OK;
}

// The launches of a call.  Without tracks a tile is one launch, over its voices as they stand in the call's arrays.  With tracks a tile
// has one launch a DESTINATION that has voices in it — the direct timeline (0) and every track's (1 + g) — over that destination's
// voices alone, gathered; tiles ascend, so every destination's chain is in index order
struct TileLaunch {
    ScoreLaunch L;
    size_t dest, gains_at;  // which timeline; where its voices' gains begin in d_mix_gains
};
struct PiecePlans {
    std::vector<TileLaunch> launches;
    std::vector<size_t> first_launch;                 // tile i's launches: first_launch[i] .. first_launch[i + 1]
    std::vector<std::vector<unsigned char>> renders;  // does part p render in tile i?
    std::vector<float> ordered_gains;                 // (with tracks: the gains in launch order, uploaded once)
};

// plans: every launch's plan, over its union window, made up front under the call's one budget — shared out over the tiles, and a
// tile's share over its launches by their voices — into one image: the rows' addresses are known, since the tile buffers stand
static int piece_plans(const PieceCall &call, const PieceFacts &F, const PieceTiles &T, PiecePlans &P) {
    dusp_ctx *ctx = call.ctx();
    const dusp_score_part *parts = call.parts;
    const uint32_t *h_part_of = call.h_part_of;
    const size_t n_dests = call.tracks ? 1 + call.tracks->n_tracks : 1;
    P.first_launch.assign(T.n_tiles + 1, 0);
    P.renders.assign(T.n_tiles, std::vector<unsigned char>(call.n_parts, 0));
    const size_t tile_budget = score_plan_budget(ctx) / T.n_tiles;
    if (int rc = score_image_begin(ctx)) return rc;
    const auto t_plan = std::chrono::steady_clock::now();
    std::vector<uint64_t> rows;
    std::vector<unsigned char> listed;
    std::vector<size_t> which;  // (with tracks: the voices of a launch, by their numbers in the call, and their arrays gathered)
    std::vector<int64_t> onsets, lengths;
    std::vector<uint32_t> samples;
    ScoreGathered gathered;
    for (size_t i = 0; i < T.n_tiles; i++) {
        const size_t lo = T.starts[i], tile_voices = T.starts[i + 1] - lo;
        for (size_t dest = 0; dest < n_dests; dest++) {
            which.clear();
            for (size_t k = lo; call.tracks && k < T.starts[i + 1]; k++)
                if ((size_t)(call.tracks->h_track_of[k] + 1) == dest) which.push_back(k);
            if (call.tracks && which.empty()) continue;
            const size_t n = call.tracks ? which.size() : tile_voices;
            auto voice = [&](size_t k) { return call.tracks ? which[k] : lo + k; };
            P.launches.push_back(TileLaunch{ScoreLaunch(call.place.kind), dest, call.tracks ? P.ordered_gains.size() : lo});
            rows.resize(n);
            for (size_t k = 0; k < n; k++) {  // voice k of the launch, in its part's tile buffer
                const size_t v = voice(k), p = h_part_of[v];
                rows[k] = (uint64_t)(uintptr_t)(parts[p].prog->d_host_out.p + (F.instance_of[v] - T.share[p][i]) * F.part_ch[p] * parts[p].n_voice_samples);
            }
            // (without tracks the launch's arrays are the call's from `lo` on: nothing is copied)
            const int64_t *h_onsets = call.h_onsets + lo, *h_lengths = call.h_lengths ? call.h_lengths + lo : nullptr;
            const uint32_t *row_samples = T.row_samples.data() + lo;
            if (call.tracks) {
                onsets.resize(n), lengths.resize(n), samples.resize(n);
                for (size_t k = 0; k < n; k++) {
                    onsets[k] = call.h_onsets[which[k]];
                    if (call.h_lengths) lengths[k] = call.h_lengths[which[k]];
                    samples[k] = T.row_samples[which[k]];
                    if (call.h_gains) P.ordered_gains.push_back(call.h_gains[which[k]]);
                }
                h_onsets = onsets.data(), h_lengths = call.h_lengths ? lengths.data() : nullptr, row_samples = samples.data();
            }
            if (int rc = score_rows_add(ctx, call.who, h_onsets, h_lengths, row_samples, rows.data(), n, call.tracks ? 0 : lo, call.n_total, /*whole_timeline=*/false,
                                        tile_budget * n / tile_voices, call.tracks ? call.place.gather(which.data(), n, gathered) : call.place.tile(lo), P.launches.back().L, &listed,
                                        call.tracks ? which.data() : nullptr))
                return rc;
            for (size_t k = 0; k < n; k++)
                if (listed[k]) P.renders[i][h_part_of[voice(k)]] = 1;
        }
        P.first_launch[i + 1] = P.launches.size();
    }
    if (ctx->knobs.jit_log >= 2)  // (DUSP_JIT_LOG=2: what the plans cost the host)
        fprintf(stderr, "[dusp host piece] %zu plans over %zu voices of %zu parts in %.0f us on the host: %zu bytes\n", P.launches.size(), call.n_voices, call.n_parts,
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_plan).count(), ctx->h_score_plan.size());
    return DUSP_OK;
}

// what a circuit over `n_inst` channels of the timeline renders into, and its columns (a master, a bus: the timeline's channels; a track
// program: its tracks' times those)
static int piece_circuit_buffers(dusp_ctx *ctx, dusp_program *circuit, size_t n_inst, size_t n_total) {
    HIP_TRY(ctx, circuit->d_host_out.ensure(n_inst * n_total));
    if (circuit->P.g.n_params) HIP_TRY(ctx, circuit->d_host_par.ensure((size_t)circuit->P.g.n_params * n_inst));
    return DUSP_OK;
}

// buffers: the timeline's running sums and, as the call has them, what the master, the buses and the track programs make of theirs
// (one more [channels][n_total] each, a track program one a track), the send and track timelines and every signal of a delivery with
// stems; the gains and the image to the device; the sums from +0
static int piece_buffers(const PieceCall &call, const PieceFacts &F, const PiecePlans &P) {
    dusp_ctx *ctx = call.ctx();
    dusp_program *prog0 = call.prog0();
    const size_t timeline = F.timeline;
    HIP_TRY(ctx, prog0->d_mix.ensure(timeline));
    if (call.master)
        if (int rc = piece_circuit_buffers(ctx, call.master->prog, F.n_out_ch, call.n_total)) return rc;
    if (call.buses) {
        HIP_TRY(ctx, prog0->d_mix_sends.ensure(call.buses->n_buses * timeline));
        for (size_t b = 0; b < call.buses->n_buses; b++)
            if (int rc = piece_circuit_buffers(ctx, call.buses->buses[b].prog, F.n_out_ch, call.n_total)) return rc;
    }
    if (call.tracks) {
        HIP_TRY(ctx, prog0->d_mix_tracks.ensure(call.tracks->n_tracks * timeline));
        for (size_t p = 0; p < call.tracks->n_programs; p++)
            if (int rc = piece_circuit_buffers(ctx, call.tracks->programs[p].prog, call.tracks->programs[p].n_tracks * F.n_out_ch, call.n_total)) return rc;
    }
    if (call.stems) HIP_TRY(ctx, prog0->d_stems.ensure(F.n_signals * timeline));
    if (call.h_gains) {  // (4 bytes a voice, where the plans take 32 and more: the whole piece's at once; with tracks in launch order)
        HIP_TRY(ctx, prog0->d_mix_gains.ensure(call.n_voices));
        HIP_TRY(ctx, hipMemcpyAsync(prog0->d_mix_gains.p, call.tracks ? P.ordered_gains.data() : call.h_gains, call.n_voices * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = score_image_upload(ctx, ctx->stream)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(prog0->d_mix.p, 0, timeline * sizeof(float), ctx->stream));
    if (call.place.n_buses) HIP_TRY(ctx, hipMemsetAsync(prog0->d_mix_sends.p, 0, call.place.n_buses * timeline * sizeof(float), ctx->stream));  // (per-voice levels)
    if (call.tracks) HIP_TRY(ctx, hipMemsetAsync(prog0->d_mix_tracks.p, 0, call.tracks->n_tracks * timeline * sizeof(float), ctx->stream));
    return DUSP_OK;
}

// render: tile by tile, the parts that have a voice reaching a timeline, then the tile's launches, each in place and raw into its
// destination's running sums
static int piece_render(const PieceCall &call, const PieceFacts &F, const PieceTiles &T, const PiecePlans &P, PieceBatches &batches) {
    dusp_ctx *ctx = call.ctx();
    dusp_program *prog0 = call.prog0();
    const dusp_score_part *parts = call.parts;
    float *d_sends = call.place.n_buses ? prog0->d_mix_sends.p : nullptr;  // (per-voice levels; with tracks the mix kernel writes the buses' feeds, from +0)
    for (size_t p = 0; p < call.n_parts; p++) batches.emplace_back(new TiledBatch(parts[p].prog, parts[p].n_instances, parts[p].h_params, T.share[p]));
    for (size_t i = 0; i < T.n_tiles; i++) {
        for (size_t p = 0; p < call.n_parts; p++)  // (no voice of the tile reaches a timeline: nothing to render)
            if (P.renders[i][p])
                if (int rc = batches[p]->render_tile(T.share[p][i], T.share[p][i + 1] - T.share[p][i], parts[p].n_voice_samples)) return rc;
        for (size_t j = P.first_launch[i]; j < P.first_launch[i + 1]; j++) {
            const TileLaunch &launch = P.launches[j];
            if (launch.L.w_hi <= launch.L.w_lo) continue;
            const float *d_gains = call.h_gains ? prog0->d_mix_gains.p + launch.gains_at : nullptr;
            float *d_into = launch.dest ? prog0->d_mix_tracks.p + F.slot_of[launch.dest - 1] * F.timeline : prog0->d_mix.p;
            if (int rc = score_launch(ctx, launch.L, F.n_out_ch, call.n_total, d_gains, d_into, /*raw=*/1, d_into, ctx->stream, nullptr, 0, d_sends, d_sends)) return rc;
        }
    }
    return DUSP_OK;
}

// deliver_host of a block that no kernel writes any more, [n_signals][n_ch][n_total] — metered on the way where the call has meters: the
// meter kernels run on the context's stream in front of the peak and encode kernels, over the f32 signals in front of the PCM gain, and
// what they leave is gated once the delivery has waited for the stream
//
// With a loudness record the true-peak kernel runs behind the meter kernels and in front of the peak kernel.  Without
// deliver its words come down where the meters' sums do, behind a delivery that is the call's without the record.  With deliver the
// peak kernel follows, then the ONE wait for the stream: the gates, the largest true peak of any signal and channel and the loudness of
// the MIX — the last signal — give the level (truepeak_plan.hpp true_peak_loudness_gain, f64 on the host), which the encoders read as
// every signal's peak word under DUSP_NORMALISE_FULL: one gain for all, the encode kernels unchanged
//
// With a limiter the host then decides, in f64, whether it is engaged.  Not engaged: nothing more is launched.  Engaged:
// the limiter's kernels over the block IN PLACE — nothing reads the block behind the delivery — then the same measurement again over the
// limited block with a second wait, and the gain comes from that second measurement
//
// words, smallest: where the true peaks' words and the limiter's smallest sum come down, asynchronously — the CALLER's (deliver_metered),
// who waits for the stream before they go out of scope where a step in between has failed
static int deliver_metered_steps(dusp_program *prog, const char *who, const dusp_score_meters *meters, const dusp_score_loudness *loud, const dusp_score_limiter *limiter,
                                 uint32_t release, uint32_t sample_rate, float *d_block, size_t n_signals, size_t n_ch, size_t n_total, int format, int normalise, float *h_peaks, void *h_out,
                                 bool common_peak, std::vector<uint64_t> &words, uint64_t &smallest) {
    dusp_ctx *ctx = prog->ctx;
    const bool at_target = loud && loud->deliver;
    if (at_target) {
        double largest = 0.0, gain = 1.0, threshold = 0.0, reduction = 1.0;
        float level = 1.0f;
        // one measurement of the block as it stands: the meter kernels, the true-peak kernel, the peak kernel, the ONE wait -> the gain
        auto measure = [&]() -> int {
            if (int rc = meter_launch(ctx, d_block, n_signals, n_ch, n_total, sample_rate, ctx->stream)) return rc;
            if (int rc = true_peak_launch(ctx, d_block, n_signals, n_ch, n_total, sample_rate, ctx->stream)) return rc;
            if (h_peaks)
                if (int rc = deliver_peaks(prog, d_block, n_signals, n_ch, n_total, h_peaks)) return rc;
            if (int rc = true_peak_download(ctx, n_signals * n_ch, words, ctx->stream)) return rc;
            if (int rc = meter_finish(ctx, who, n_signals, n_ch, n_total, sample_rate, ctx->stream, meters->h_rms, meters->h_lufs, meters->h_momentary)) return rc;  // (waits)
            if (int rc = true_peak_values(ctx, who, words, loud->h_true_peak, &largest)) return rc;
            dusp::true_peak_loudness_gain(meters->h_lufs[n_signals - 1], largest, loud->target_lufs, loud->ceiling_dbtp, gain, level);
            return DUSP_OK;
        };
        if (int rc = measure()) return rc;
        const double lufs_in = meters->h_lufs[n_signals - 1], true_peak_in = largest;
        bool engaged = false;
        if (limiter) {  // (engaged where the gain is not unity and some true peak lies above the ceiling seen from the target)
            threshold = dusp::limiter_threshold(lufs_in, loud->target_lufs, loud->ceiling_dbtp);
            engaged = level != 1.0f && threshold > 0.0 && std::isfinite(threshold) && largest > threshold;
        }
        if (engaged) {
            const uint32_t L = (uint32_t)limiter->window_samples;
            if (int rc = limit_launch(ctx, d_block, n_signals, n_ch, n_total, sample_rate, threshold, L, ctx->stream, release)) return rc;  // (with a release of its own)
            if (int rc = limit_download(ctx, &smallest, ctx->stream)) return rc;
            if (int rc = measure()) return rc;  // (the limited block; its wait is the download's too)
            if (int rc = limit_reduction(ctx, who, smallest, L, &reduction)) return rc;
        }
        if (limiter) {
            if (limiter->h_engaged) *limiter->h_engaged = engaged;
            if (limiter->h_threshold) *limiter->h_threshold = threshold;
            if (limiter->h_reduction) *limiter->h_reduction = reduction;
            if (limiter->h_lufs_in) *limiter->h_lufs_in = lufs_in;
            if (limiter->h_true_peak_in) *limiter->h_true_peak_in = true_peak_in;
        }
        if (loud->h_gain) *loud->h_gain = gain;
        if (loud->h_level) *loud->h_level = level;
        return deliver_at_level(prog, d_block, n_signals, n_ch, n_total, format, level, h_out);
    }
    if (meters)
        if (int rc = meter_launch(ctx, d_block, n_signals, n_ch, n_total, sample_rate, ctx->stream)) return rc;
    if (loud)
        if (int rc = true_peak_launch(ctx, d_block, n_signals, n_ch, n_total, sample_rate, ctx->stream)) return rc;
    if (int rc = deliver_host(prog, d_block, nullptr, n_signals, n_ch, n_total, format, normalise, h_peaks, h_out, common_peak)) return rc;
    if (loud)
        if (int rc = true_peak_download(ctx, n_signals * n_ch, words, ctx->stream)) return rc;
    if (meters) {  // (waits for the stream)
        if (int rc = meter_finish(ctx, who, n_signals, n_ch, n_total, sample_rate, ctx->stream, meters->h_rms, meters->h_lufs, meters->h_momentary)) return rc;
    } else if (loud) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (!loud) return DUSP_OK;
    if (int rc = true_peak_values(ctx, who, words, loud->h_true_peak, nullptr)) return rc;
    if (loud->h_gain) *loud->h_gain = 1.0;
    if (loud->h_level) *loud->h_level = 1.0f;
    return DUSP_OK;
}

static int deliver_metered(dusp_program *prog, const char *who, const dusp_score_meters *meters, const dusp_score_loudness *loud, const dusp_score_limiter *limiter, uint32_t release,
                           uint32_t sample_rate,
                           float *d_block, size_t n_signals, size_t n_ch, size_t n_total, int format, int normalise, float *h_peaks, void *h_out, bool common_peak) {
    std::vector<uint64_t> words;
    uint64_t smallest = 0;
    const int rc = deliver_metered_steps(prog, who, meters, loud, limiter, release, sample_rate, d_block, n_signals, n_ch, n_total, format, normalise, h_peaks, h_out, common_peak, words, smallest);
    if (rc) (void)hipStreamSynchronize(prog->ctx->stream);  // (a copy into `words` or `smallest` may still be on its way)
    return rc;
}

// The one delivery: n_signals signals from d_block, under one gain where common_peak says so; it waits for the stream.  With a master
// the RAW sums in d_mix — no `|| 0`: a unit behind a Sum hears the Sum's own values — are first its input block as they stand, channel c
// the one input stream of instance c: its render from its initial state, deciding as a tile of a mix decides (it waits for its compiled
// kernel), applies `|| 0` at its own copy-out into its d_host_out — which the caller delivers from or, with stems, has copied device to
// device into the last slot of the block
static int piece_deliver(const PieceCall &call, const PieceFacts &F, float *d_block, size_t n_signals, bool common_peak, PieceBatches &batches) {
    dusp_ctx *ctx = call.ctx();
    dusp_program *prog0 = call.prog0();
    if (call.master) {
        batches.emplace_back(new TiledBatch(call.master->prog, F.n_out_ch, call.master->h_params, nullptr, F.n_out_ch));  // (one tile: all channels)
        if (int rc = batches.back()->render_tile(0, F.n_out_ch, call.n_total, prog0->d_mix.p)) return rc;
        if (call.stems)
            HIP_TRY(ctx, hipMemcpyAsync(prog0->d_stems.p + (n_signals - 1) * F.timeline, call.master->prog->d_host_out.p, F.timeline * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return deliver_metered(prog0, call.who, call.meters, call.loud, call.limiter, (uint32_t)call.release, F.sample_rate, d_block, n_signals, F.n_out_ch, call.n_total, call.format, call.normalise, call.h_peak, call.h_out, common_peak);
}

// guards, behind the delivery: the buffers of the piece that the call used, then every auxiliary program's own
static int piece_guards(const PieceCall &call) {
    dusp_ctx *ctx = call.ctx();
    dusp_program *prog0 = call.prog0();
    if (int rc = score_guards(ctx, call.who, {&prog0->d_mix, &prog0->d_mix_gains, call.buses ? &prog0->d_mix_sends : nullptr, call.tracks ? &prog0->d_mix_tracks : nullptr,
                                              call.stems ? &prog0->d_stems : nullptr, call.stems ? &prog0->d_host_peak_common : nullptr}))
        return rc;
    if (call.master)
        if (int rc = check_guards(call.master->prog, ctx->stream)) return rc;
    for (size_t b = 0; b < call.n_buses(); b++)
        if (int rc = check_guards(call.buses->buses[b].prog, ctx->stream)) return rc;
    for (size_t p = 0; call.tracks && p < call.tracks->n_programs; p++)
        if (int rc = check_guards(call.tracks->programs[p].prog, ctx->stream)) return rc;
    return DUSP_OK;
}

// finish: the tracks' mix, the buses' return, the stem of a bare timeline, then the delivery and the guards.  The kernel that makes the
// mix LAST applies the delivery's `|| 0` — unless a master follows, whose copy-out has it and which reads the sums raw — and, with
// stems, keeps the stems on the way (slot s: d_stems + s timelines) and writes the mix into the last slot itself; with a master the raw
// mix stays in d_mix for it.  A call with none of these has the rows kernel's `|| 0` over the timeline's channels, a launch without voices
static int piece_finish(const PieceCall &call, const PieceFacts &F, PieceBatches &batches) {
    dusp_ctx *ctx = call.ctx();
    dusp_program *prog0 = call.prog0();
    const bool stems = call.stems != nullptr, master = call.master != nullptr, buses = call.buses != nullptr, tracks = call.tracks != nullptr;
    const size_t timeline = F.timeline;
    float *d_slots = stems ? prog0->d_stems.p : nullptr, *d_last = stems && !master ? d_slots + (F.n_signals - 1) * timeline : nullptr;
    if (tracks)
        if (int rc = score_tracks_mix(call, F.slot_of, F.n_out_ch, /*raw=*/buses || master, batches, buses ? nullptr : d_last, d_slots)) return rc;
    if (buses)  // (per-note sends: the dry timeline gets its slot here)
        if (int rc = score_buses_return(prog0, call.buses, F.n_out_ch, call.n_total, /*raw=*/master, batches, d_last, stems && !tracks ? d_slots : nullptr,
                                        stems ? d_slots + (1 + call.n_tracks()) * timeline : nullptr))
            return rc;
    if (stems && !tracks && !buses)  // (one timeline: its stem and the mix; raw and in place in front of a master)
        HIP_TRY(ctx, dusp::launch_score_tracks(prog0->d_mix.p, nullptr, nullptr, nullptr, 0, 0, d_last ? d_last : prog0->d_mix.p, nullptr, nullptr, d_slots, nullptr, (uint64_t)timeline,
                                               /*raw=*/master, ctx->stream));
    if (!stems && !master && !buses && !tracks)
        if (int rc = score_launch(ctx, ScoreLaunch(ScoreKind::rows, call.n_total), F.n_out_ch, call.n_total, nullptr, prog0->d_mix.p, /*raw=*/0, prog0->d_mix.p, ctx->stream, nullptr, 0))
            return rc;
    float *d_block = stems ? d_slots : master ? call.master->prog->d_host_out.p : prog0->d_mix.p;
    if (int rc = piece_deliver(call, F, d_block, stems ? F.n_signals : 1, /*common_peak=*/stems, batches)) return rc;
    for (auto &batch : batches) batch->staged = false;  // (the delivery has waited for the stream)
    return piece_guards(call);
}

// every entry of this file: the parts' voices placed as call.place says into a timeline of place.timeline_channels(a voice's)
static int render_host_score_parts(PieceCall call) {
    if (!call.parts || !call.n_parts || !call.parts[0].prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = call.ctx();
    return guarded(ctx->err, call.who, [&]() -> int {
        PieceFacts facts;
        PieceTiles tiles;  // (the stages' results, each read by the stages behind it)
        PiecePlans plans;
        if (int rc = piece_check(call, facts)) return rc;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        if (int rc = piece_tiles(call, facts, tiles)) return rc;
        if (int rc = piece_check_loudness(call, facts)) return rc;
        if (int rc = piece_check_limiter(call)) return rc;
        if (int rc = piece_plans(call, facts, tiles, plans)) return rc;
        if (int rc = piece_buffers(call, facts, plans)) return rc;
        PieceBatches batches;  // (behind the plans and tiles: a batch whose vectors are still on their way waits for the stream as it goes)
        if (int rc = piece_render(call, facts, tiles, plans, batches)) return rc;
        return piece_finish(call, facts, batches);
    });
}

// ---- the entries ----

// the call of an entry but its placement (plain rows) and its features
static PieceCall piece_call(const char *who, const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                            const float *h_gains, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    return PieceCall{who, parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, ScorePlacement(ScoreKind::rows), n_total_samples, tile_bytes, format, normalise, h_out, h_peak};
}

// the entries that take the placement as a record (dusp_score_placement; NULL: plain rows): call, with its features, gets the placement
static int render_host_score_piece(PieceCall call, const dusp_score_placement *placement) {
    if (!call.parts || !call.n_parts || !call.parts[0].prog) return DUSP_ERR_ARG;
    dusp_ctx *ctx = call.ctx();
    const char *who = call.who;
    const dusp_score_placement plain{DUSP_PLACE_ROWS, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
    const dusp_score_placement &by = placement ? *placement : plain;
    switch (by.kind) {
    case DUSP_PLACE_ROWS:
        call.place = ScorePlacement(ScoreKind::rows, by.h_fracs, nullptr, nullptr);
        break;
    case DUSP_PLACE_PAN:
    case DUSP_PLACE_STEREO:
        if (!by.h_pans) CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": h_pans is NULL");
        call.place = ScorePlacement(by.kind == DUSP_PLACE_PAN ? ScoreKind::pan : ScoreKind::stereo, by.h_fracs, by.h_pans, by.h_comp);
        break;
    case DUSP_PLACE_SPACE:
        call.place = ScorePlacement(by.n_speakers, by.h_delays, by.h_tap_gains);
        break;
    default:
        CTX_FAIL(ctx, DUSP_ERR_ARG, std::string(who) + ": the placement's kind must be DUSP_PLACE_ROWS (0), DUSP_PLACE_PAN (1), DUSP_PLACE_SPACE (2) or DUSP_PLACE_STEREO (3)");
    }
    return render_host_score_parts(call);
}

}  // namespace

extern "C" {

int dusp_render_host_score_parts(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                 const int64_t *h_lengths, const float *h_gains, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out,
                                 float *h_peak) {
    return render_host_score_parts(piece_call("dusp_render_host_score_parts", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format,
                                              normalise, h_out, h_peak));
}

int dusp_render_host_score_parts_pan(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                     const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                     int format, int normalise, void *h_out, float *h_peak) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    if (!h_pans) CTX_FAIL(parts[0].prog->ctx, DUSP_ERR_ARG, "dusp_render_host_score_parts_pan: h_pans is NULL");
    PieceCall call = piece_call("dusp_render_host_score_parts_pan", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise, h_out,
                                h_peak);
    call.place = ScorePlacement(ScoreKind::pan, nullptr, h_pans, h_comp);
    return render_host_score_parts(call);
}

int dusp_render_host_score_parts_frac(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const double *h_fracs,
                                      const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp, size_t n_total_samples, size_t tile_bytes,
                                      int format, int normalise, void *h_out, float *h_peak) {
    PieceCall call = piece_call("dusp_render_host_score_parts_frac", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise, h_out,
                                h_peak);
    call.place = ScorePlacement(h_pans ? ScoreKind::pan : ScoreKind::rows, h_fracs, h_pans, h_comp);
    return render_host_score_parts(call);
}

int dusp_render_host_score_parts_space(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                       const int64_t *h_lengths, const float *h_gains, size_t n_speakers, const double *h_delays, const double *h_tap_gains,
                                       size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    PieceCall call = piece_call("dusp_render_host_score_parts_space", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise,
                                h_out, h_peak);
    call.place = ScorePlacement(n_speakers, h_delays, h_tap_gains);
    return render_host_score_parts(call);
}

int dusp_render_host_score_parts_stereo(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                        const double *h_fracs, const int64_t *h_lengths, const float *h_gains, const float *h_pans, const double *h_comp,
                                        size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    if (!parts || !n_parts || !parts[0].prog) return DUSP_ERR_ARG;
    if (!h_pans) CTX_FAIL(parts[0].prog->ctx, DUSP_ERR_ARG, "dusp_render_host_score_parts_stereo: h_pans is NULL");
    PieceCall call = piece_call("dusp_render_host_score_parts_stereo", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise,
                                h_out, h_peak);
    call.place = ScorePlacement(ScoreKind::stereo, h_fracs, h_pans, h_comp);
    return render_host_score_parts(call);
}

int dusp_render_host_score_piece(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                 const float *h_gains, const dusp_score_placement *placement, const dusp_score_master *master, size_t n_total_samples, size_t tile_bytes,
                                 int format, int normalise, void *h_out, float *h_peak) {
    PieceCall call = piece_call("dusp_render_host_score_piece", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise, h_out, h_peak);
    call.master = master;
    return render_host_score_piece(call, placement);
}

// ... and with effect sends (buses NULL: dusp_render_host_score_piece under this entry's name)
int dusp_render_host_score_piece_buses(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                       const float *h_gains, const dusp_score_placement *placement, const dusp_score_buses *buses, const dusp_score_master *master,
                                       size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    PieceCall call = piece_call("dusp_render_host_score_piece_buses", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise,
                                h_out, h_peak);
    call.master = master, call.buses = buses;
    return render_host_score_piece(call, placement);
}

// ... and with tracks (tracks NULL: dusp_render_host_score_piece_buses under this entry's name)
int dusp_render_host_score_piece_tracks(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                        const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                        const dusp_score_master *master, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peak) {
    PieceCall call = piece_call("dusp_render_host_score_piece_tracks", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise,
                                h_out, h_peak);
    call.master = master, call.buses = buses, call.tracks = tracks;
    return render_host_score_piece(call, placement);
}

// ... and with stems (stems NULL: dusp_render_host_score_piece_tracks under this entry's name)
int dusp_render_host_score_piece_stems(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                       const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                       const dusp_score_master *master, const dusp_score_stems *stems, size_t n_total_samples, size_t tile_bytes, int format, int normalise,
                                       void *h_out, float *h_peaks) {
    PieceCall call = piece_call("dusp_render_host_score_piece_stems", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise,
                                h_out, h_peaks);
    call.master = master, call.buses = buses, call.tracks = tracks, call.stems = stems;
    return render_host_score_piece(call, placement);
}

// ... and with meters: the RMS and the loudness of every signal the call delivers (meters NULL: dusp_render_host_score_piece_stems under
// this entry's name)
int dusp_render_host_score_piece_meters(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                        const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                        const dusp_score_master *master, const dusp_score_stems *stems, const dusp_score_meters *meters, size_t n_total_samples, size_t tile_bytes,
                                        int format, int normalise, void *h_out, float *h_peaks) {
    PieceCall call = piece_call("dusp_render_host_score_piece_meters", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise,
                                h_out, h_peaks);
    call.master = master, call.buses = buses, call.tracks = tracks, call.stems = stems, call.meters = meters;
    return render_host_score_piece(call, placement);
}

// ... and with a loudness record: the true peak of every signal and channel the call delivers and, with deliver, PCM frames at a loudness
// target under a true-peak ceiling (loudness NULL: dusp_render_host_score_piece_meters under this entry's name); with a limiter the
// delivered signals are limited to the ceiling in front of the gain.  One body for the two entries, each under its own name
static int render_host_score_piece_limiter(const char *who, const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                           const int64_t *h_lengths, const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                           const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems, const dusp_score_meters *meters,
                                           const dusp_score_loudness *loudness, const dusp_score_limiter *limiter, size_t n_total_samples, size_t tile_bytes, int format, int normalise,
                                           void *h_out, float *h_peaks, size_t release = 0) {
    PieceCall call = piece_call(who, parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, n_total_samples, tile_bytes, format, normalise, h_out, h_peaks);
    call.master = master, call.buses = buses, call.tracks = tracks, call.stems = stems, call.meters = meters, call.loud = loudness, call.limiter = limiter, call.release = release;
    return render_host_score_piece(call, placement);
}

int dusp_render_host_score_piece_loudness(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                          const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                          const dusp_score_master *master, const dusp_score_stems *stems, const dusp_score_meters *meters, const dusp_score_loudness *loudness,
                                          size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peaks) {
    return render_host_score_piece_limiter("dusp_render_host_score_piece_loudness", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, tracks, buses, master, stems,
                                           meters, loudness, nullptr, n_total_samples, tile_bytes, format, normalise, h_out, h_peaks);
}

int dusp_render_host_score_piece_limiter(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets, const int64_t *h_lengths,
                                         const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks, const dusp_score_buses *buses,
                                         const dusp_score_master *master, const dusp_score_stems *stems, const dusp_score_meters *meters, const dusp_score_loudness *loudness,
                                         const dusp_score_limiter *limiter, size_t n_total_samples, size_t tile_bytes, int format, int normalise, void *h_out, float *h_peaks) {
    return render_host_score_piece_limiter("dusp_render_host_score_piece_limiter", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, tracks, buses, master, stems,
                                           meters, loudness, limiter, n_total_samples, tile_bytes, format, normalise, h_out, h_peaks);
}

// ... and with a release of the limiter's own (release_samples = 0, or limiter NULL: the entry above under this entry's name)
int dusp_render_host_score_piece_limiter_release(const dusp_score_part *parts, size_t n_parts, size_t n_voices, const uint32_t *h_part_of, const int64_t *h_onsets,
                                                 const int64_t *h_lengths, const float *h_gains, const dusp_score_placement *placement, const dusp_score_tracks *tracks,
                                                 const dusp_score_buses *buses, const dusp_score_master *master, const dusp_score_stems *stems, const dusp_score_meters *meters,
                                                 const dusp_score_loudness *loudness, const dusp_score_limiter_release *limiter, size_t n_total_samples, size_t tile_bytes, int format,
                                                 int normalise, void *h_out, float *h_peaks) {
    return render_host_score_piece_limiter("dusp_render_host_score_piece_limiter_release", parts, n_parts, n_voices, h_part_of, h_onsets, h_lengths, h_gains, placement, tracks, buses, master,
                                           stems, meters, loudness, limiter ? &limiter->limiter : nullptr, n_total_samples, tile_bytes, format, normalise, h_out, h_peaks,
                                           limiter ? limiter->release_samples : 0);
}

}  // extern "C"
