// abi_context.hip — the C ABI (include/dusp_hip.h): library version and errors, contexts and their knobs, wave tables, pinned host memory.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "abi_internal.hpp"
#include "device_util.hpp"
#include "jit_engine.hpp"
#include "table_checks.hpp"

thread_local std::string g_error;

static dusp::Knobs read_knobs() {
    dusp::Knobs k;
    auto num = [](const char *name, int fallback) {
        const char *e = getenv(name);
        return e && *e ? atoi(e) : fallback;
    };
    if (const char *t = getenv("DUSP_FUSED_TABLE")) k.fused_table_global = t[0] == 'g';
    k.fused_R = num("DUSP_FUSED_R", k.fused_R);
    k.fused_items = num("DUSP_FUSED_ITEMS", k.fused_items);
    k.fused_fx32 = num("DUSP_FUSED_FX32", k.fused_fx32);
    k.fused_segmajor = num("DUSP_FUSED_SEGMAJOR", k.fused_segmajor);
    k.wave_segments = num("DUSP_WAVE_SEGMENTS", k.wave_segments);
    k.wave_max_waves = num("DUSP_WAVE_MAX_WAVES", k.wave_max_waves);
    k.wave_jit = num("DUSP_WAVE_JIT", k.wave_jit);
    k.wave_per_wave = num("DUSP_WAVE_PER_WAVE", k.wave_per_wave);
    k.jit_profile = num("DUSP_JIT_PROFILE", k.jit_profile);
    k.filter_fma = num("DUSP_FILTER_FMA", k.filter_fma);
    k.jit_spill_bytes = num("DUSP_JIT_SPILL", k.jit_spill_bytes);
    k.jit_lds_table = num("DUSP_JIT_LDS_TABLE", k.jit_lds_table);
    k.jit_lean = num("DUSP_JIT_LEAN", k.jit_lean);
    k.jit_log = num("DUSP_JIT_LOG", k.jit_log);
    k.ring_window = num("DUSP_RING_WINDOW", k.ring_window);
    k.filter_scan = num("DUSP_FILTER_SCAN", k.filter_scan);
    k.filter_warm = num("DUSP_FILTER_WARM", k.filter_warm);
    k.jit_nt = num("DUSP_JIT_NT", k.jit_nt);
    k.delay_line = num("DUSP_DELAY_LINE", k.delay_line);
    k.jit_rotate = num("DUSP_JIT_ROTATE", k.jit_rotate);
    k.ring_poison = num("DUSP_RING_POISON", k.ring_poison);
    k.mix_width = num("DUSP_MIX_WIDTH", k.mix_width);
    k.mix_depth = num("DUSP_MIX_DEPTH", k.mix_depth);
    k.mix_tile_mb = num("DUSP_MIX_TILE_MB", k.mix_tile_mb);
    k.score_plan_kb = num("DUSP_SCORE_PLAN_KB", k.score_plan_kb);
    if (const char *f = getenv("DUSP_JIT_FORCE")) {
        int w = 0, r = 0;
        if (std::sscanf(f, "%dx%d", &w, &r) == 2 && w >= 1 && w <= 16 && r >= 1 && r <= 4) k.jit_force_waves = w, k.jit_force_per_wave = r;
    }
    return k;
}

extern "C" {

const char *dusp_version(void) { return "dusp-hip 0.1.0 (gfx950)"; }
int dusp_abi_version(void) { return DUSP_ABI_VERSION; }

int dusp_device_count(void) {
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) {
        try {
            g_error = std::string("no usable HIP device: ") + hipGetErrorString(e) + " (this library has no CPU fallback)";
        } catch (...) {
        }
        return DUSP_ERR_HIP;
    }
    return count;
}

const char *dusp_last_error(const dusp_ctx *ctx) { return ctx ? ctx->err.c_str() : g_error.c_str(); }

int dusp_ctx_create(int device, dusp_ctx **out) {
    return guarded(g_error, "dusp_ctx_create", [&]() -> int {
    if (!out) {
        g_error = "dusp_ctx_create: out is NULL";
        return DUSP_ERR_ARG;
    }
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count < 1) {
        g_error = std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
                  " (this library has no CPU fallback)";
        return DUSP_ERR_HIP;
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= count) {
        g_error = "device index out of range";
        return DUSP_ERR_ARG;
    }
    std::unique_ptr<dusp_ctx> ctx(new (std::nothrow) dusp_ctx);
    if (!ctx) {
        g_error = "out of memory";
        return DUSP_ERR_ARG;
    }
    ctx->device = device;
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreate(&ctx->stream)) != hipSuccess) {
        g_error = std::string("HIP error: ") + hipGetErrorString(e);
        return DUSP_ERR_HIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->n_cus = prop.multiProcessorCount;
    ctx->knobs = read_knobs();
    if (const char *g = getenv("DUSP_GUARD"))  // (process-wide, set by the first context: allocations made before keep their size)
        if (atoi(g) > 0 && !g_guard_bytes) g_guard_bytes = 4096;
    dusp::jit_configure();  // (the code-object cache directory: read once per process)
    *out = ctx.release();
    return DUSP_OK;
    });
}

void dusp_ctx_destroy(dusp_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
    }
    if (ctx->d_tables) (void)hipFree(ctx->d_tables);
    if (ctx->d_score_plan) (void)hipFree(ctx->d_score_plan);
    if (ctx->d_meter) (void)hipFree(ctx->d_meter);
    if (ctx->d_true_peak) (void)hipFree(ctx->d_true_peak);
    if (ctx->d_limit) (void)hipFree(ctx->d_limit);
    if (ctx->d_limit_release) (void)hipFree(ctx->d_limit_release);
    for (hipEvent_t ev : ctx->meter_marks)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->limit_marks)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : ctx->limit_release_marks)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->score_uploaded) (void)hipEventDestroy(ctx->score_uploaded);
    if (ctx->score_done) (void)hipEventDestroy(ctx->score_done);
    for (hipEvent_t ev : {ctx->score_up0, ctx->score_t0, ctx->score_t1})
        if (ev) (void)hipEventDestroy(ev);
    for (auto &b : ctx->host_pool) (void)hipHostFree(b.p);
    delete ctx;
}

int dusp_table_upload(dusp_ctx *ctx, int table_id, const float *table, size_t n) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, "dusp_table_upload", [&]() -> int {
    if (table_id < 0 || table_id >= dusp::kNumTables || !table || n < 9 || n > (1u << 22) + 1)
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_table_upload: bad table id, pointer or length");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_tables) {
        ctx->table_len = (uint32_t)n;
        ctx->table_stride = (uint32_t)((n + 1 + 3) & ~(size_t)3);  // >= n+1 entries (one pad for idx+1), 16-byte rows
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_tables, sizeof(float) * dusp::kNumTables * ctx->table_stride + g_guard_bytes));
        HIP_TRY(ctx, hipMemset(ctx->d_tables, 0, sizeof(float) * dusp::kNumTables * ctx->table_stride));
        if (g_guard_bytes) HIP_TRY(ctx, hipMemset((char *)ctx->d_tables + sizeof(float) * dusp::kNumTables * ctx->table_stride, kGuardPattern, g_guard_bytes));
        ctx->tables_guarded = g_guard_bytes != 0;
    } else if (n != ctx->table_len) {
        CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_table_upload: all tables of a context must have the same length");
    }
    std::vector<float> row(ctx->table_stride, 0.f);
    std::memcpy(row.data(), table, n * sizeof(float));
    for (size_t k = n; k < row.size(); k++) row[k] = table[n - 1];  // pad: keeps an idx+1 read finite and in range
    HIP_TRY(ctx, hipMemcpy(ctx->d_tables + (size_t)table_id * ctx->table_stride, row.data(),
                           row.size() * sizeof(float), hipMemcpyHostToDevice));
    // T[N-t] == -T[t] for t = 1..N-1 lets a fused kernel keep half the table in LDS
    bool antisym = (n % 2) == 1;
    for (size_t t = 1; antisym && t < n; t++) antisym = table[n - t] == -table[t];
    ctx->table_antisym[table_id] = antisym;
    bool finite = true;
    for (size_t t = 0; finite && t < n; t++) finite = std::isfinite(table[t]);
    ctx->table_finite[table_id] = finite;
    bool big = finite;
    for (size_t t = 0; big && t < n; t++) big = table[t] == 0.f || std::fabs(table[t]) >= 9.5367431640625e-07f;
    ctx->table_fx32_ok[table_id] = big;
    ctx->table_delta[table_id] = dusp::table_delta_class(table, n);
    {
        float top = 0.f;
        for (size_t t = 0; t < n; t++) top = std::max(top, std::fabs(table[t]));
        ctx->table_bound[table_id] = !finite ? 1000 : top == 0.f ? 0 : std::ilogb(top) + 1;
    }
    ctx->table_set[table_id] = true;
    ctx->table_generation++;
    // closed forms (device_util.hpp): every entry has to match, sign of zero included
    auto same_bits = [](float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; };
    const uint32_t sr = (uint32_t)n - 1;
    ctx->table_form[table_id] = dusp::TABLE_FORM_DATA;
    if (table_id >= 1 && table_id <= 3 && n <= 131073) {
        const int forms[3] = {dusp::TABLE_FORM_SAW, dusp::TABLE_FORM_SQUARE, dusp::TABLE_FORM_TRIANGLE};
        const dusp::TableForm F = dusp::make_table_form(forms[table_id - 1], sr);
        bool ok = F.form != dusp::TABLE_FORM_TRIANGLE || sr % 4 == 0;
        for (uint32_t i = 0; ok && i <= sr; i++) ok = same_bits(dusp::closed_table_entry(F, i), table[i]);
        if (ok) ctx->table_form[table_id] = F.form;
    }
    if (table_id == 0 || table_id == 4) {
        ctx->h_tables[table_id ? 1 : 0].assign(table, table + n);
        ctx->table_form[4] = dusp::TABLE_FORM_DATA;
        const std::vector<float> &sine = ctx->h_tables[0], &bit8 = ctx->h_tables[1];
        if (sine.size() == n && bit8.size() == n && ctx->table_antisym[0] && sr % 2 == 0) {
            // as the kernels see the sine table: the half image in LDS, mirrored with a sign above the middle
            bool ok = true;
            for (uint32_t i = 0; ok && i <= sr; i++) ok = same_bits(dusp::eightbit_of_sine(i > sr / 2 ? -sine[n - i] : sine[i]), bit8[i]);
            if (ok) ctx->table_form[4] = dusp::TABLE_FORM_8BIT;
        }
    }
    return DUSP_OK;
    });
}

int dusp_host_alloc(dusp_ctx *ctx, size_t n_bytes, void **out) {
    if (!ctx) return DUSP_ERR_ARG;
    return guarded(ctx->err, "dusp_host_alloc", [&]() -> int {
    if (!out) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_host_alloc: out is NULL");
    *out = nullptr;
    if (n_bytes < 1 || n_bytes > ((size_t)1 << 40)) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_host_alloc: size out of range");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> pool_lock(ctx->host_pool_mutex);
    // smallest free buffer that fits and is not wastefully large; pinning fresh pages is the slow part, so buffers are kept
    dusp_ctx::HostBuf *best = nullptr;
    for (auto &b : ctx->host_pool)
        if (!b.in_use && b.bytes >= n_bytes && b.bytes <= n_bytes + n_bytes / 4 + 65536 && (!best || b.bytes < best->bytes)) best = &b;
    if (best) {
        best->in_use = true;
        *out = best->p;
        return DUSP_OK;
    }
    size_t idle = 0;  // keep the pool's idle part bounded: free idle buffers first when the new one would push it past 4 GiB
    for (auto &b : ctx->host_pool) idle += b.in_use ? 0 : b.bytes;
    for (size_t k = ctx->host_pool.size(); k-- > 0 && idle + n_bytes > ((size_t)4 << 30);)
        if (!ctx->host_pool[k].in_use) {
            idle -= ctx->host_pool[k].bytes;
            (void)hipHostFree(ctx->host_pool[k].p);
            ctx->host_pool.erase(ctx->host_pool.begin() + (long)k);
        }
    ctx->host_pool.reserve(ctx->host_pool.size() + 1);
    void *p = nullptr;
    HIP_TRY(ctx, hipHostMalloc(&p, n_bytes, hipHostMallocDefault));
    ctx->host_pool.push_back({p, n_bytes, true});
    *out = p;
    return DUSP_OK;
    });
}

int dusp_host_free(dusp_ctx *ctx, void *p) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!p) return DUSP_OK;
    {
        std::lock_guard<std::mutex> pool_lock(ctx->host_pool_mutex);  // (nothing else of the context is touched on this path: a finalizer thread may call it)
        for (auto &b : ctx->host_pool)
            if (b.p == p && b.in_use) {
                b.in_use = false;  // stays pinned for the next render of that size (dusp_ctx_destroy releases the pool)
                return DUSP_OK;
            }
    }
    CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_host_free: not a live buffer of this context");
}

const char *dusp_jit_cache_dir(void) { return dusp::jit_cache_directory(); }

int dusp_fill_device(dusp_ctx *ctx, float *d_out, size_t n_floats, float value, void *stream_) {
    if (!ctx) return DUSP_ERR_ARG;
    if (!d_out || (n_floats & 3) || ((uintptr_t)d_out & 15)) CTX_FAIL(ctx, DUSP_ERR_ARG, "dusp_fill_device: need a 16-byte aligned buffer of 4k floats");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, dusp::launch_fill(d_out, n_floats, value, stream_of(ctx, stream_)));
    return DUSP_OK;
}

}  // extern "C"

