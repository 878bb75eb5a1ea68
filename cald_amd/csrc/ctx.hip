// ctx.hip -- error state, the context (stream, arena, scratch), the cald_internal_* accessors of train_*.hip (train_host.h) / jpeg.hip / comm.hip, the event
// profile (cald_profile_*) and the one conv launch every layer goes through (run_conv).
#include "host.h"

static thread_local char g_err[512] = "";
int cald_host::fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return code;
}

// shared with jpeg.hip (internal, not part of the C ABI)
int cald_internal_fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return code;
}
void cald_internal_train_release(cald_ctx* c);   // train_geom.hip: per-context geometry cache and staging ring

extern "C" const char* cald_last_error(void) { return g_err; }
extern "C" int cald_version(void) { return 100; }

// =============================================================================================
// context
// =============================================================================================
hipStream_t cald_internal_stream(cald_ctx* c) { return c->stream; }
int cald_internal_device(cald_ctx* c) { return c->device; }
const float* cald_internal_zeros(cald_ctx* c) { return c->d_zeros; }
// grow-only scratch shared by the calls of one context; every user is ordered on the context stream
int cald_internal_scratch(cald_ctx* c, size_t bytes, void** out) {
    if (bytes > c->train_scratch_cap) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->train_scratch) HIPCHK(hipFree(c->train_scratch));
        c->train_scratch = nullptr; c->train_scratch_cap = 0;
        const size_t want = bytes + (bytes >> 2);
        HIPCHK(hipMalloc((void**)&c->train_scratch, want));
        c->train_scratch_cap = want;
    }
    *out = c->train_scratch;
    return 0;
}

int cald_host::arena_reserve(cald_ctx* c, size_t bytes) {
    if (bytes <= c->arena_cap) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->arena) HIPCHK(hipFree(c->arena));
    c->arena = nullptr; c->arena_cap = 0;
    size_t want = bytes + (bytes >> 3);
    HIPCHK(hipMalloc((void**)&c->arena, want));
    c->arena_cap = want;
    return 0;
}

extern "C" int cald_ctx_create(int device, void* stream, cald_ctx** out) {
    if (!out) return fail(CALD_ERR_INVALID, "out is null");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(CALD_ERR_INVALID, "device %d out of range (%d devices)", device, ndev);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CALD_ERR_INVALID, "libcaldhip is built for gfx950 (MI355X); device %d is %s", device, prop.gcnArchName);
    cald_ctx* c = new cald_ctx();
    c->device = device;
    if (stream) c->stream = (hipStream_t)stream;
    else { HIPCHK(hipStreamCreate(&c->stream)); c->own_stream = true; }
    HIPCHK(hipMalloc((void**)&c->d_plan, sizeof(BatchPlan)));
    HIPCHK(hipMalloc((void**)&c->d_views, sizeof(ViewDesc) * CALD_MAX_VIEWS));
    HIPCHK(hipMalloc((void**)&c->d_zeros, 256));
    HIPCHK(hipMemset(c->d_zeros, 0, 256));
    HIPCHK(hipMalloc((void**)&c->d_roi_rows, 8));
    HIPCHK(hipMemset(c->d_roi_rows, 0, 8));
    HIPCHK(hipMalloc((void**)&c->d_prune_stat, 32));
    HIPCHK(hipMalloc((void**)&c->d_prune_log, (size_t)CALD_PRUNE_LOG * 32));
    HIPCHK(hipMemset(c->d_prune_log, 0, (size_t)CALD_PRUNE_LOG * 32));
    HIPCHK(hipMemset(c->d_prune_stat, 0, 32));
    HIPCHK(hipMalloc((void**)&c->d_prune_check, 8));
    HIPCHK(hipMemset(c->d_prune_check, 0, 8));
    for (int i = 0; i < cald_ctx::NSTAGE; i++) {
        HIPCHK(hipHostMalloc((void**)&c->h_stage[i], sizeof(BatchPlan) + sizeof(ViewDesc) * CALD_MAX_VIEWS));
        HIPCHK(hipEventCreateWithFlags(&c->stage_ev[i], hipEventDisableTiming));
    }
    *out = c;
    return 0;
}
extern "C" int cald_ctx_sync(cald_ctx* c) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int cald_ctx_destroy(cald_ctx* c) {
    if (!c) return 0;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    for (auto& kv : c->pil) { hipFree(kv.second.d_bounds); hipFree(kv.second.d_kk); }
    for (auto& t : c->prof_launches) { hipEventDestroy(t.e0); hipEventDestroy(t.e1); }
    if (c->tot0) hipEventDestroy(c->tot0);
    if (c->tot1) hipEventDestroy(c->tot1);
    if (c->arena) hipFree(c->arena);
    if (c->train_scratch) hipFree(c->train_scratch);
    cald_internal_train_release(c);
    for (int i = 0; i < cald_ctx::NSTAGE; i++) { if (c->h_stage[i]) hipHostFree(c->h_stage[i]); if (c->stage_ev[i]) hipEventDestroy(c->stage_ev[i]); }
    hipFree(c->d_plan); hipFree(c->d_views); hipFree(c->d_zeros); hipFree(c->d_roi_rows); hipFree(c->d_prune_stat); hipFree(c->d_prune_log); hipFree(c->d_prune_check);
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

extern "C" int cald_profile_enable(cald_ctx* c, int on) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof = on != 0;
    for (auto& t : c->prof_launches) { hipEventDestroy(t.e0); hipEventDestroy(t.e1); }
    c->prof_launches.clear(); c->prof_flops = 0.0; c->prof_extra_launches = 0; c->tot_ms = 0.0; c->tot_open = false;
    c->prof_prune_flops_cap[0] = c->prof_prune_flops_cap[1] = 0.0;
    c->prof_roi_rows_cap = 0.0; c->prof_roi_flops_cap = 0.0; c->prof_roi_views = 0;
    HIPCHK(hipMemsetAsync(c->d_roi_rows, 0, 8, c->stream));
    HIPCHK(hipMemsetAsync(c->d_prune_stat, 0, 32, c->stream));
    HIPCHK(hipMemsetAsync(c->d_prune_log, 0, (size_t)CALD_PRUNE_LOG * 32, c->stream));
    c->prune_log_n = 0; c->prof_gather.clear();
    if (on && !c->tot0) { HIPCHK(hipEventCreate(&c->tot0)); HIPCHK(hipEventCreate(&c->tot1)); }
    return 0;
}
extern "C" int cald_profile_read(cald_ctx* c, double* gemm_ms, double* gemm_flops, int64_t* launches, double* total_ms) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    HIPCHK(hipStreamSynchronize(c->stream));
    double ms = 0.0, look_fl = 0.0; int64_t look_n = 0;
    for (const ProfLaunch& L : c->prof_launches) {
        if (L.tag) { look_fl += L.flops; look_n++; continue; }       // the fp16 look-ahead of rpn_prune.hip: cald_profile_prune()
        float t = 0.f; HIPCHK(hipEventElapsedTime(&t, L.e0, L.e1)); ms += t;
    }
    if (gemm_ms) *gemm_ms = ms;
    // RoI-head layers were booked at the row capacity (CALD_ROI_CAP per view); rescale them to the measured rows
    unsigned long long rows = 0;
    HIPCHK(hipMemcpy(&rows, c->d_roi_rows, 8, hipMemcpyDeviceToHost));
    double fl = c->prof_flops - look_fl;
    if (c->prof_roi_rows_cap > 0.0) fl -= c->prof_roi_flops_cap * (1.0 - (double)rows / c->prof_roi_rows_cap);
    unsigned long long st[4] = {0, 0, 0, 0};     // the gathered RPN launches were booked on every pixel of P2 / P3: rescale to the selected rows
    HIPCHK(hipMemcpy(st, c->d_prune_stat, 32, hipMemcpyDeviceToHost));
    // booked: one dense head per selection stage (two); executed: the selected rows of both stages together
    for (int l = 0; l < 2; l++) if (st[2 * l + 1]) fl -= c->prof_prune_flops_cap[l] * (1.0 - (double)st[2 * l] / (2.0 * (double)st[2 * l + 1]));
    if (gemm_flops) *gemm_flops = fl;
    if (launches) *launches = (int64_t)c->prof_launches.size() - look_n + c->prof_extra_launches;   // a timed region can hold several kernel launches
    if (total_ms) *total_ms = c->tot_ms;
    return 0;
}

extern "C" int cald_profile_prune(cald_ctx* c, double* look_ms, double* look_flops, double* selected_frac2, double* worst_bound_ratio, double* pruned_flops) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    HIPCHK(hipStreamSynchronize(c->stream));
    double ms = 0.0, fl = 0.0;
    for (const ProfLaunch& L : c->prof_launches)
        if (L.tag) { float t = 0.f; HIPCHK(hipEventElapsedTime(&t, L.e0, L.e1)); ms += t; fl += L.flops; }
    unsigned long long st[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(st, c->d_prune_stat, 32, hipMemcpyDeviceToHost));
    if (look_ms) *look_ms = ms;
    if (look_flops) *look_flops = fl;
    if (selected_frac2) for (int l = 0; l < 2; l++) selected_frac2[l] = st[2 * l + 1] ? (double)st[2 * l] / (double)st[2 * l + 1] : 0.0;
    if (worst_bound_ratio) *worst_bound_ratio = (double)c->prune_worst;
    if (pruned_flops) {      // exact FLOPs of the dense head that the gathered launches did NOT execute (cald_profile_read leaves them out)
        double fl2 = 0.0;
        for (int l = 0; l < 2; l++) if (st[2 * l + 1]) fl2 += c->prof_prune_flops_cap[l] / 2.0 * (1.0 - (double)st[2 * l] / (double)st[2 * l + 1]);
        *pruned_flops = fl2;
    }
    return 0;
}

extern "C" int cald_profile_roi_rows(cald_ctx* c, double* mean_rows_per_view, int64_t* views) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    HIPCHK(hipStreamSynchronize(c->stream));
    unsigned long long rows = 0;
    HIPCHK(hipMemcpy(&rows, c->d_roi_rows, 8, hipMemcpyDeviceToHost));
    if (views) *views = c->prof_roi_views;
    if (mean_rows_per_view) *mean_rows_per_view = c->prof_roi_views ? (double)rows / (double)c->prof_roi_views : 0.0;
    return 0;
}

extern "C" int cald_profile_cutout(cald_ctx* c, double* rows3, double* dense_rows3, int64_t* batches, int64_t* fallbacks) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    for (int i = 0; i < 3; i++) { if (rows3) rows3[i] = c->cut_rows[i]; if (dense_rows3) dense_rows3[i] = c->cut_dense[i]; }
    if (batches) *batches = c->cut_batches;
    if (fallbacks) *fallbacks = c->cut_fallbacks;
    return 0;
}

extern "C" int cald_profile_cutout_stages(cald_ctx* c, double* rows6, double* dense_rows6, double* tiles6, double* dense_tiles6, int64_t* kept3) {
    if (!c) return fail(CALD_ERR_INVALID, "ctx is null");
    for (int i = 0; i < 6; i++) {
        if (rows6) rows6[i] = c->cut_st_rows[i];
        if (dense_rows6) dense_rows6[i] = c->cut_st_dense[i];
        if (tiles6) tiles6[i] = c->cut_st_tiles[i];
        if (dense_tiles6) dense_tiles6[i] = c->cut_st_dense_tiles[i];
    }
    if (kept3) for (int i = 0; i < 3; i++) kept3[i] = c->cut_kept[i];
    return 0;
}

extern "C" int cald_profile_dump(cald_ctx* c, const char* path) {
    if (!c || !path) return fail(CALD_ERR_INVALID, "null argument");
    HIPCHK(hipStreamSynchronize(c->stream));
    FILE* f = fopen(path, "w");
    if (!f) return fail(CALD_ERR_INVALID, "cannot open %s", path);
    fprintf(f, "launch,desc,gflop,ms,tflops\n");
    std::vector<unsigned long long> lg((size_t)CALD_PRUNE_LOG * 4, 0ull);
    if (!c->prof_gather.empty()) HIPCHK(hipMemcpy(lg.data(), c->d_prune_log, lg.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < c->prof_launches.size(); i++) {
        const ProfLaunch& L = c->prof_launches[i];
        float t = 0.f; hipEventElapsedTime(&t, L.e0, L.e1);
        double fl = L.flops;
        const char* extra = L.tag ? ",f16x3-lookahead" : "";
        auto g = c->prof_gather.find(i);
        if (g != c->prof_gather.end()) {       // a gathered launch of the certified pruning: FLOPs of the rows it computed, not of every pixel
            for (int l = 0; l < 2; l++) {
                const unsigned long long sel = lg[(size_t)g->second.log * 4 + 2 * l], tot = lg[(size_t)g->second.log * 4 + 2 * l + 1];
                if (tot) fl -= g->second.cap[l] * (1.0 - (double)sel / (double)tot);
            }
            extra = ",gathered-rows";
        }
        fprintf(f, "%zu,\"%s%s\",%.3f,%.4f,%.2f\n", i, L.desc.c_str(), extra, fl / 1e9, t, fl / (t * 1e-3) / 1e12);
    }
    fclose(f);
    return 0;
}
extern "C" int cald_profile_prune_fallbacks(cald_ctx* c, int64_t* n) {
    if (!c || !n) return fail(CALD_ERR_INVALID, "null argument");
    *n = (int64_t)c->prune_fallbacks;
    return 0;
}

// One timed launch of the profile: prof_begin before it, prof_end after it (books the launch under `tag` with `flops` and the formatted
// description).  Both do nothing while the profile is off.
int cald_host::prof_begin(cald_ctx* c, ProfLaunch& t) {
    if (!c->prof) return 0;
    HIPCHK(hipEventCreate(&t.e0)); HIPCHK(hipEventCreate(&t.e1));
    HIPCHK(hipEventRecord(t.e0, c->stream));
    return 0;
}
int cald_host::prof_end(cald_ctx* c, ProfLaunch& t, double flops, int tag, const char* fmt, ...) {
    if (!c->prof) return 0;
    HIPCHK(hipEventRecord(t.e1, c->stream));
    char d[160];
    va_list ap; va_start(ap, fmt); vsnprintf(d, sizeof(d), fmt, ap); va_end(ap);
    t.flops = flops; t.tag = tag; t.desc = d;
    c->prof_launches.push_back(t); c->prof_flops += flops;
    return 0;
}

// conv launch with optional event bracketing.  A launch no kernel takes is an error.
int cald_host::conv_refused(const ConvArgs& a) {
    return fail(CALD_ERR_UNSUPPORTED, "no conv kernel implements this launch (Cin=%d Cout=%d k=%dx%d residual=%d up=%d mask=%d gather=%d energy4=%d out16=%d)",
                a.Cin, a.Cout, a.KH, a.KW, a.residual != nullptr, a.up != nullptr, a.mask != nullptr, a.gather != nullptr, a.energy4 != nullptr,
                a.out16 != nullptr);
}
int cald_host::run_conv(cald_ctx* c, const ConvArgs& a, double flops) {
    ProfLaunch t; int rc;
    if ((rc = prof_begin(c, t))) return rc;
    const char* k = launch_conv(a, c->stream);
    if ((rc = prof_end(c, t, flops, c->prof_tag_now, "mt=%d,Cin=%d,Cout=%d,k=%dx%d,s=%d", a.total_mtiles, a.Cin, a.Cout, a.KH, a.KW, a.stride))) return rc;
    if (!k) return conv_refused(a);
    return 0;
}
