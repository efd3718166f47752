// mix_kernel_check.cpp — the text of dusp_amd/csrc/mix_engine.hip compiled for the HOST (hip_host_stub/: lanes one after the other) and held to
// a plain loop over the contract — acc = init ? init : term(0); acc = f32(acc + term(i)) — on bit patterns, for every launcher choice (one /
// four floats a lane, 8 / 32 rows in flight, workgroups of 64 / 256), with and without gains, init (a second buffer, in place), raw, and
// outputs / inputs off the 16-byte boundaries, between sentinels.  Built with -fsanitize=address,undefined by tests/test_mix_host.py: an index
// past a buffer is an error here, not a fault on a shared GPU.  Prints {"cases": n, "bad": m}.
#include "../../dusp_amd/csrc/mix_engine.hip"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <random>
static float or0(float a) { return (a != a || a == 0.0f) ? 0.0f : a; }
int main() {
    std::mt19937 rng(7);
    std::normal_distribution<float> nd;
    int shapes[][3] = {{1,1,1},{2,1,255},{3,2,257},{9,1,1001},{17,3,513},{5,33,300},{70,1,1031},{64,2,512},{5,2,1028},{33,1,64},{40,1,8}};
    long checked = 0, bad = 0;
    for (auto &sh : shapes) {
        const size_t I = sh[0], row = (size_t)sh[1] * sh[2];
        for (int width : {0, 1, 4}) for (int depth : {0, 8, 32}) for (int gains : {0, 1}) for (int init : {0, 1, 2}) for (int raw : {0, 1})
        for (int off : {0, 1, 3}) for (int inoff : {0, 2}) {
            if ((off || inoff) && (depth == 8 || init == 1)) continue;  // keep it quick
            // 16-byte aligned bases + offsets
            std::vector<float> in_s(I * row + 8), out_s(row + 136), init_s(row + 8), g(I);
            float *in = (float *)(((uintptr_t)in_s.data() + 15) & ~(uintptr_t)15) + inoff;
            float *outb = (float *)(((uintptr_t)out_s.data() + 15) & ~(uintptr_t)15);
            float *ini = (float *)(((uintptr_t)init_s.data() + 15) & ~(uintptr_t)15);
            for (size_t k = 0; k < I * row; k++) in[k] = nd(rng) * std::pow(10.f, (float)(k / row % 7) - 3);
            for (size_t k = 0; k < row; k += 37) in[(k * 31 % I) * row + k] = (k & 1) ? -0.0f : INFINITY;
            if (row > 2) for (size_t i = 0; i < I; i++) in[i * row + 2] = -0.0f;
            if (row > 5) in[(I / 2) * row + 5] = NAN;
            for (auto &x : g) x = 0.05f + 1.9f * (rng() % 1000) / 1000.f;
            for (size_t k = 0; k < row; k++) ini[k] = 30 * nd(rng);
            const float S = -12345.678f;
            for (size_t k = 0; k < 64 + off + row + 64; k++) outb[k] = S;
            float *out = outb + 64 + off;
            const float *pinit = nullptr;
            if (init == 1) pinit = ini;
            if (init == 2) { memcpy(out, ini, row * 4); pinit = out; }
            // reference
            std::vector<float> want(row);
            for (size_t p = 0; p < row; p++) {
                volatile float acc; size_t i = 0;
                if (init) acc = ini[p]; else { acc = gains ? in[p] * g[0] : in[p]; i = 1; }
                for (; i < I; i++) { volatile float t = gains ? in[i * row + p] * g[i] : in[i * row + p]; acc = acc + t; }
                want[p] = raw ? (float)acc : or0(acc);
            }
            dusp::launch_mix(in, gains ? g.data() : nullptr, pinit, out, row, (uint32_t)I, raw, /* n_cus: small, so that these row lengths lie on both sides of the launcher's thresholds */ 2, width, depth, nullptr);
            bool ok = true;
            for (size_t k = 0; k < 64 + (size_t)off; k++) ok &= memcmp(&outb[k], &S, 4) == 0;
            for (size_t k = 0; k < 64; k++) ok &= memcmp(&out[row + k], &S, 4) == 0;
            for (size_t p = 0; p < row; p++) {
                if (want[p] != want[p]) ok &= out[p] != out[p];
                else ok &= memcmp(&out[p], &want[p], 4) == 0;
            }
            checked++;
            if (!ok) { bad++; printf("MISMATCH shape %d %d %d width %d depth %d gains %d init %d raw %d off %d inoff %d (threads %d grid %u)\n", sh[0], sh[1], sh[2], width, depth, gains, init, raw, off, inoff, g_last_threads, g_last_grid); }
        }
    }
    printf("{\"cases\": %ld, \"bad\": %ld}\n", checked, bad);
    return bad != 0;
}
