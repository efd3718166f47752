// dusp_amd/csrc/abi_internal.hpp on the CPU: the registry of a program's device workspaces (dusp_workspaces::for_each_workspace) is what the
// destructor and the guard check (DUSP_GUARD=1) walk.  Built against tests/native/hip_mem_stub — "device" memory is host memory — under
// AddressSanitizer:
//   * the registry visits every DevBuf member once (kCount of them, which a static_assert in the header ties to the struct's size);
//   * with a guard length set, every workspace grown, the registry-driven check passes;
//   * one byte flipped in the guard region of each workspace in turn: the check names THAT workspace; restored, it passes again;
//   * the program's destructor gives everything back (the sanitizer's leak check at exit);
//   * the shared argument checks (check_batch / check_channels / check_pcm_format / check_normalise) give each entry point's own text.
// Prints one JSON line.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../dusp_amd/csrc/abi_internal.hpp"

thread_local std::string g_error;  // (abi_context.hip's, for the header's declaration)

int main() {
    long bad = 0, flips = 0;
    g_guard_bytes = 4096;
    {
        dusp_program prog;
        struct Entry { const char *name; unsigned char *guard; void *buffer; };
        std::vector<Entry> entries;
        size_t n = 3;
        prog.for_each_workspace([&](const char *name, auto &buf) {
            if (buf.ensure(n) != hipSuccess || buf.cap != n) bad++, std::printf("FAIL: %s does not grow\n", name);
            entries.push_back({name, (unsigned char *)buf.p + buf.cap * sizeof(*buf.p), (void *)&buf});
            n += 5;  // (every workspace its own size: a guard looked for at another's offset is not found)
        });
        std::set<void *> distinct;
        for (const Entry &e : entries) distinct.insert(e.buffer);
        if (entries.size() != dusp_workspaces::kCount || distinct.size() != dusp_workspaces::kCount)
            bad++, std::printf("FAIL: the registry visits %zu workspaces (%zu distinct), the program owns %zu\n", entries.size(), distinct.size(), dusp_workspaces::kCount);
        for (const Entry &e : entries)
            if ((unsigned char *)e.buffer < (unsigned char *)static_cast<dusp_workspaces *>(&prog) || (unsigned char *)e.buffer >= (unsigned char *)static_cast<dusp_workspaces *>(&prog) + sizeof(dusp_workspaces))
                bad++, std::printf("FAIL: %s is not a member of dusp_workspaces\n", e.name);
        if (const char *hit = prog.first_overwritten()) bad++, std::printf("FAIL: untouched guards, but the check names %s\n", hit);
        const size_t offsets[] = {0, 1, 4095};
        for (const Entry &e : entries)
            for (size_t at : offsets) {
                const unsigned char was = e.guard[at];
                e.guard[at] ^= 0x40;
                const char *hit = prog.first_overwritten();
                flips++;
                if (!hit || std::strcmp(hit, e.name) != 0) bad++, std::printf("FAIL: guard byte %zu of %s overwritten, the check names %s\n", at, e.name, hit ? hit : "nothing");
                e.guard[at] = was;
                if (prog.first_overwritten()) bad++, std::printf("FAIL: %s restored, the check still fails\n", e.name);
            }
        // (without a guard length nothing is looked at: what a library with one copy of g_guard_bytes per file would do everywhere)
        entries[0].guard[0] ^= 0x40;
        g_guard_bytes = 0;
        if (prog.first_overwritten()) bad++, std::printf("FAIL: a check without guards\n");
        g_guard_bytes = 4096;
        if (!prog.first_overwritten()) bad++, std::printf("FAIL: the overwritten byte is not seen again\n");
        entries[0].guard[0] ^= 0x40;
        // swap: the two rings change places, guards and all
        float *rings = prog.d_rings.p;
        const size_t cap = prog.d_rings.cap;
        prog.d_rings.swap(prog.d_rings_wave);
        if (prog.d_rings_wave.p != rings || prog.d_rings_wave.cap != cap || prog.d_rings.p == rings || prog.first_overwritten()) bad++, std::printf("FAIL: swap\n");
    }
    // the shared argument checks: status and text as the entry points have always given them (the hosts match on these)
    long texts = 0;
    {
        dusp_ctx ctx;
        auto expect = [&](int rc, int want_rc, const char *want_text) {
            texts++;
            if (rc != want_rc || (want_rc != DUSP_OK && ctx.err != want_text)) bad++, std::printf("FAIL: rc %d \"%s\", expected %d \"%s\"\n", rc, ctx.err.c_str(), want_rc, want_text);
        };
        expect(check_batch(&ctx, "render", 0, 256), DUSP_ERR_ARG, "render: n_instances must be in [1, 2^24] and n_samples in [1, 2^31]");
        expect(check_batch(&ctx, "dusp_render_host_mix", ((size_t)1 << 24) + 1, 256), DUSP_ERR_ARG, "dusp_render_host_mix: n_instances must be in [1, 2^24] and n_samples in [1, 2^31]");
        expect(check_batch(&ctx, "render", 1, 0), DUSP_ERR_ARG, "render: n_instances must be in [1, 2^24] and n_samples in [1, 2^31]");
        expect(check_batch(&ctx, "render", 1, ((size_t)1 << 31) + 1), DUSP_ERR_ARG, "render: n_instances must be in [1, 2^24] and n_samples in [1, 2^31]");
        expect(check_batch(&ctx, "render", (size_t)1 << 24, (size_t)1 << 31), DUSP_OK, "");
        expect(check_channels(&ctx, "dusp_render_host_pcm", 65), DUSP_ERR_UNSUPPORTED, "dusp_render_host_pcm: the outlet must have 1..64 channels");
        expect(check_channels(&ctx, "dusp_render_host_mix", 0), DUSP_ERR_UNSUPPORTED, "dusp_render_host_mix: the outlet must have 1..64 channels");
        expect(check_channels(&ctx, "dusp_render_host_mix", 64), DUSP_OK, "");
        expect(check_pcm_format(&ctx, "dusp_encode_device", 4, false), DUSP_ERR_ARG, "dusp_encode_device: format must be DUSP_PCM_S16 (1), DUSP_PCM_S24 (2) or DUSP_PCM_F32 (3)");
        expect(check_pcm_format(&ctx, "dusp_render_host_pcm", 0, false), DUSP_ERR_ARG, "dusp_render_host_pcm: format must be DUSP_PCM_S16 (1), DUSP_PCM_S24 (2) or DUSP_PCM_F32 (3)");
        expect(check_pcm_format(&ctx, "dusp_render_host_mix", 4, true), DUSP_ERR_ARG,
               "dusp_render_host_mix: format must be 0 (planar f32), DUSP_PCM_S16 (1), DUSP_PCM_S24 (2) or DUSP_PCM_F32 (3)");
        expect(check_pcm_format(&ctx, "dusp_render_host_mix", 0, true), DUSP_OK, "");
        for (int f : {DUSP_PCM_S16, DUSP_PCM_S24, DUSP_PCM_F32}) expect(check_pcm_format(&ctx, "dusp_encode_device", f, false), DUSP_OK, "");
        expect(check_normalise(&ctx, "dusp_encode_device", 3), DUSP_ERR_ARG, "dusp_encode_device: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)");
        expect(check_normalise(&ctx, "dusp_render_host_mix", -1), DUSP_ERR_ARG, "dusp_render_host_mix: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)");
        for (int n : {0, 1, 2}) expect(check_normalise(&ctx, "dusp_render_host_pcm", n), DUSP_OK, "");
    }
    std::printf("{\"workspaces\": %zu, \"flips\": %ld, \"texts\": %ld, \"bad\": %ld}\n", dusp_workspaces::kCount, flips, texts, bad);
    return bad ? 1 : 0;
}
