// forward.hip -- one forward of the detector over a ragged batch of views: the level plan, the arena layout, the conv launches of every
// layer (single, fused pair, group, gathered rows of the cut_out reuse), forward_model, cald_forward and cald_debug_tensor.
#include "host.h"

// =============================================================================================
// forward
// =============================================================================================
// Rows of the RoI-head GEMMs are grouped 32 views to a segment: 32 000 rows = exactly 250 tiles of 128, and the segment's fc6 operand
// (32 000 x 12 544 floats = 1.6 GB) stays inside the 2 GB a buffer resource / a 32-bit byte offset can address.
#define ROI_DENSE_VIEWS 32
void cald_host::build_plan(BatchPlan& P, int V, const ViewDesc* views, const int (*hp)[2], bool retina) {
    memset(&P, 0, sizeof(P));
    for (int l = 0; l < CALD_MAX_LEVELS; l++) {
        long long off = 0; int tile = 0;
        for (int v = 0; v <= V; v++) {
            LevelSeg& s = P.seg[l][v];
            s.pix_off = off; s.tile_start = tile;
            if (v == V) break;
            int H, W;
            if (l == 7 && retina) { int h6 = (hp[v][0] / 32 - 1) / 2 + 1, w6 = (hp[v][1] / 32 - 1) / 2 + 1; H = (h6 - 1) / 2 + 1; W = (w6 - 1) / 2 + 1; }
            else if (l == 7) { H = 1; W = CALD_ROI_CAP; }
            else if (l == 8) {   // the RoI-head GEMMs' view of level 7: dense rows, in segments of ROI_DENSE_VIEWS views (see forward_model)
                const int first = v * ROI_DENSE_VIEWS, cnt = first < V ? (V - first < ROI_DENSE_VIEWS ? V - first : ROI_DENSE_VIEWS) : 0;
                H = cnt ? 1 : 0; W = cnt * CALD_ROI_CAP;
            }
            else if (l == 6) { H = (hp[v][0] / 32 - 1) / 2 + 1; W = (hp[v][1] / 32 - 1) / 2 + 1; }
            else { H = hp[v][0] >> l; W = hp[v][1] >> l; }
            s.H = H; s.W = W;
            off += (long long)H * W;
            tile += (H * W + 127) / 128;
        }
    }
}
static int level_tiles(const BatchPlan& P, int l, int V) { return P.seg[l][V].tile_start; }

struct FwdBufs {
    float *in0, *c1, *p1, *X[2], *T1, *T2, *D, *Cf[4], *inner[4], *Pf[5], *rpn_h[5];
    unsigned long long* cand_key; float *cand_box, *sorted_box, *sorted_raw; int* sorted_count;
    float* proposals; int* prop_count; int* roi_order;
    float *roi, *f6, *f7, *pr, *prob, *pmax; unsigned long long* keys; float* cbox; int* key_count;
    // RetinaNet
    float *ret_t[2][2][5], *cls_h[5], *reg_h[5], *rcand_box, *kept_box; unsigned long long* rcand_key;   // ret_t[tower][ping-pong][level]
    float* rpn_tl[5];
    int *cand_count, *kept_anchor, *kept_count; int cand_cap; int max_anchors; unsigned char* cand_skip;
    unsigned* Pf16[5];   // CALD_PRECISION_F16X3: split twins of the tensors that stay fp32 as well
    // decision-margin audit (audit.hip): what the RPN / post-processing kernels leave behind for it
    unsigned long long *next_key, *trunc_key, *kept_key; float* post_maxc;
    // certified RPN pruning (rpn_prune.hip), levels P2 / P3
    float *prune_energy[2], *prune_pn[2], *prune_rows[2][2]; int *prune_map[2][2], *prune_nsel[2]; unsigned* prune_p16[2]; unsigned* prune_tau;      // [stage][level] row lists of the two selection stages
    float* prune_look[2];        // capture mode only: the look-ahead's head map before select / scatter overwrite it
};

// conv_stem.hip wants every view's output to be an exact grid of 8 x 16 pixel blocks (padded sizes are multiples of 32); seg: host copy,
// V + 1 entries
bool cald_host::stem_grid_exact(const LevelSeg* seg, int V) {
    for (int v = 0; v < V; v++) {
        const LevelSeg& s = seg[v];
        if (!(s.H % 8 == 0 && s.W % 16 == 0 && seg[v + 1].tile_start - s.tile_start == (s.H / 8) * (s.W / 16))) return false;
    }
    return true;
}
static double fill_conv_args(cald_model* m, ConvArgs& a, const ConvLayer& L, const float* in, float* out, int lin, int lout, int V, bool relu,
                             const float* residual = nullptr, const float* up = nullptr, int lup = 0, const int* dyn = nullptr,
                             bool in_relu = false) {
    const BatchPlan* dp = m->ctx->d_plan;
    a.in = in; a.out = out; a.w = L.w; a.w4 = L.w4; a.w16 = L.w16; a.w16_unscale = L.w16_unscale; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    a.residual = residual; a.up = up;
    a.seg_in = dp->seg[lin]; a.seg_out = dp->seg[lout]; a.seg_up = dp->seg[lup];
    a.dyn_rows = dyn; a.row_map = nullptr; a.gather = nullptr; a.V = V;
    a.Cin = L.Cin; a.Cout = L.Cout; a.CoutPad = L.CoutPad; a.Kpad = L.Kpad;
    a.KH = L.KH; a.KW = L.KW; a.stride = L.stride; a.pad = L.pad; a.relu = relu ? 1 : 0;
    a.total_mtiles = level_tiles(m->plan, lout, V);
    a.out_ld = L.Cout; a.in_relu = in_relu ? 1 : 0; a.zeros = m->ctx->d_zeros;
    a.mask = nullptr;
    // the kernels address a view's tensor through a buffer resource / 32-bit byte offsets: a view (or a dense RoI-row segment) must stay
    // below 2 GB per operand -- refuse loudly instead of reading zeros past the end (as a 64-view fc6 operand in one segment once did)
    for (int v = 0; v < V; v++) {
        const long long pin = (long long)m->plan.seg[lin][v].H * m->plan.seg[lin][v].W, pout = (long long)m->plan.seg[lout][v].H * m->plan.seg[lout][v].W;
        if (pin * L.Cin * 4 > 0x7FFE0000LL || pout * L.Cout * 4 > 0x7FFE0000LL) {
            return (double)fail(CALD_ERR_UNSUPPORTED, "a view's activation tensor exceeds 2 GB (level %d -> %d, %lld x %d / %lld x %d elements)", lin, lout, pin, L.Cin, pout, L.Cout);
        }
    }
    a.in16 = nullptr; a.out16 = nullptr; a.ex16 = 0; a.energy4 = nullptr; a.trace = nullptr;
    if (!m->split.empty()) {
        const float* ex = residual ? residual : up;
        if (ex) {
            auto fe = m->split.find(ex);
            if (fe != m->split.end() && fe->second.fp32_dead) {
                if (!a.w16) return (double)fail(CALD_ERR_STATE, "a layer outside conv_h3 / conv_h4 adds a tensor kept in split form only");
                a.ex16 = 1;          // same buffer, split form: the epilogue reads it through h16.h
            }
        }
        auto fi = m->split.find(in);
        if (fi != m->split.end()) {
            if (a.w16 && !in_relu) a.in16 = fi->second.s16;
            else if (fi->second.fp32_dead) return (double)fail(CALD_ERR_STATE, "a layer outside conv_h3 reads a tensor kept in split form only");
        }
        auto fo = m->split.find(out);
        if (fo != m->split.end()) {
            if (!a.w16) return (double)fail(CALD_ERR_STATE, "a layer outside conv_h3 writes a tensor with a split twin");
            a.out16 = fo->second.s16;
            if (fo->second.fp32_dead) a.out = nullptr;
        }
    }
    a.wstem = L.wstem && stem_grid_exact(m->plan.seg[lout], V) ? L.wstem : nullptr;
    return 2.0 * (double)level_pix(m->plan, lout, V) * (double)L.Cout * (double)(L.KH * L.KW * L.CinTrue);
}
static int conv_on(cald_model* m, const ConvLayer& L, const float* in, float* out, int lin, int lout, int V, bool relu,
                   const float* residual = nullptr, const float* up = nullptr, int lup = 0, const int* dyn = nullptr,
                   bool in_relu = false) {
    ConvArgs a;
    const double flops = fill_conv_args(m, a, L, in, out, lin, lout, V, relu, residual, up, lup, dyn, in_relu);
    if (flops < 0.0) return (int)flops;            // fill_conv_args failed: the (negative) status code
    return run_conv(m->ctx, a, flops);
}
// Bottleneck conv2 (3 x 3) + conv3 (1 x 1 expand, + residual) of one block: ONE launch when conv_p4.hip's fused kernel covers the
// shapes (the 64-channel blocks of layer 1, exact fp32 mode) -- the 64-channel tensor `mid` is then never written -- else two launches.
static int conv_pair_on(cald_model* m, const ConvLayer& L2, const ConvLayer& L3, const float* in, float* mid, float* out, int lin, int lout,
                        int V, const float* residual) {
    cald_ctx* c = m->ctx;
    if (m->cfg.precision == CALD_PRECISION_FP32 && L2.stride == 1 && lin == lout) {
        ConvArgs a2, a3;
            const double f2 = fill_conv_args(m, a2, L2, in, mid, lin, lout, V, true);
        const double f3 = fill_conv_args(m, a3, L3, mid, out, lout, lout, V, true, residual);
        if (f2 < 0.0 || f3 < 0.0) return (int)(f2 < 0.0 ? f2 : f3);
        ProfLaunch t; int rc;
        if ((rc = prof_begin(c, t))) return rc;
        if (launch_conv_p4_fused(a2, a3, c->stream) != nullptr)
            return prof_end(c, t, f2 + f3, 0, "mt=%d,Cin=%d,Cout=%d,k=3x3+1x1,s=1,fused->%d", a2.total_mtiles, a2.Cin, a2.Cout, a3.Cout);
        if (c->prof) { hipEventDestroy(t.e0); hipEventDestroy(t.e1); }      // the fused kernel declined: the two launches below time themselves
    }
    int rc = conv_on(m, L2, in, mid, lin, lout, V, true);
    if (rc) return rc;
    return conv_on(m, L3, mid, out, lout, lout, V, true, residual);
}
// independent convolutions (ConvSpec) issued as ONE launch when they fit the same tiled kernel
static int conv_group_on(cald_model* m, const ConvSpec* sp, int n, int V) {
    ConvArgs a[CALD_MAX_GROUP];
    double flops = 0.0; int tiles = 0;
    for (int i = 0; i < n; i++) {
        const double f = fill_conv_args(m, a[i], *sp[i].L, sp[i].in, sp[i].out, sp[i].level, sp[i].level, V, sp[i].relu, nullptr, nullptr, 0, sp[i].dyn);
        if (f < 0.0) return (int)f;
        a[i].row_map = sp[i].row_map;
        if (sp[i].in16) a[i].in16 = sp[i].in16;       // the input also exists in split form (rpn_prune.hip's look-ahead)
        if (sp[i].out16) a[i].out16 = sp[i].out16;
        a[i].energy4 = sp[i].energy4;
        flops += f; tiles += a[i].total_mtiles;
    }
    cald_ctx* c = m->ctx;
    const char* names[CALD_MAX_GROUP];
    ProfLaunch t; int rc;
    if ((rc = prof_begin(c, t))) return rc;
    const int launches = launch_conv_group(a, n, c->stream, names);
    if (c->prof) c->prof_extra_launches += launches - 1;
    if ((rc = prof_end(c, t, flops, c->prof_tag_now, "mt=%d,Cin=%d,Cout=%d,k=%dx%d,s=%d,group=%d", tiles, a[0].Cin, a[0].Cout, a[0].KH, a[0].KW, a[0].stride, n))) return rc;
    for (int i = 0; i < n; i++) if (!names[i]) return conv_refused(a[i]);
    return 0;
}

// one conv of a reused block on the rows of gather set `kind` (conv_p4.hip's gathered-rows mode: every row stored at its own pixel)
static int gconv_on(cald_model* m, const ConvLayer& L, const float* in, float* out, int lin, int lout, int V, bool relu, const float* residual,
                    const FwdReuse& ru, int b, int kind) {
    if (!ru.tiles[b][kind]) return 0;
    ConvArgs a;
    const double f = fill_conv_args(m, a, L, in, out, lin, lout, V, relu, residual);
    if (f < 0.0) return (int)f;
    const char* base = ru.d_gp + (size_t)(2 * b + kind) * cut_plan_set_bytes(V);
    a.seg_out = reinterpret_cast<const LevelSeg*>(base);
    a.gather = reinterpret_cast<const GatherSet*>(base + (size_t)(V + 1) * sizeof(LevelSeg));
    a.total_mtiles = ru.tiles[b][kind];
    return run_conv(m->ctx, a, 2.0 * ru.rows[b][kind] * (double)L.Cout * (double)(L.KH * L.KW * L.CinTrue));
}

// feat_only: the features-only forward (FwdFeatures) -- nothing behind the pyramid is laid out
static void fwd_layout(cald_model* m, Bump& B, FwdBufs& F, int V, bool feat_only = false) {
    const BatchPlan& P = m->plan;
    const long long px[8] = {level_pix(P, 0, V), level_pix(P, 1, V), level_pix(P, 2, V), level_pix(P, 3, V),
                             level_pix(P, 4, V), level_pix(P, 5, V), level_pix(P, 6, V), level_pix(P, 7, V)};
    m->split.clear();
    static const bool split_on = !(getenv("CALD_H3_S16") && atoi(getenv("CALD_H3_S16")) == 0);
    const bool sp16 = m->cfg.precision == CALD_PRECISION_F16X3 && split_on;
    auto both = [&](float* t, unsigned*& twin, size_t n) { if (sp16) { twin = B.get<unsigned>(n); m->split[t] = {twin, false}; } };
    auto only = [&](float* t) { if (sp16) m->split[t] = {reinterpret_cast<unsigned*>(t), true}; };
    F.in0 = B.get<float>(px[0] * 4);
    F.c1 = B.get<float>(px[1] * 64);
    F.p1 = B.get<float>(px[2] * 64);
    F.X[0] = B.get<float>(px[2] * 256); F.X[1] = B.get<float>(px[2] * 256);
    F.T1 = B.get<float>(px[2] * 128); F.T2 = B.get<float>(px[2] * 64); F.D = B.get<float>(px[2] * 256);
    const int cch[4] = {256, 512, 1024, 2048};
    for (int i = 0; i < 4; i++) F.Cf[i] = B.get<float>(px[2 + i] * cch[i]);
    // split forms (F16X3, h16.h): every tensor whose readers are conv_h3 / conv_h4 layers lives in split form ONLY, in the buffer the fp32
    // tensor would have used (same 4 bytes per element): the pooled stem output, the inner tensors of a bottleneck, the block outputs
    // (read as a GEMM operand by the next block's conv1 / downsample conv / the FPN lateral, and as the residual by conv3's epilogue,
    // which joins hi + lo again), the downsample branch, the laterals (operand of the 3 x 3 output conv, top-down term of the next
    // lateral's epilogue).  22 significant bits instead of 24 on those tensors -- the precision every GEMM operand of this mode has.
    only(F.p1); only(F.T1); only(F.T2); only(F.X[0]); only(F.X[1]); only(F.D);
    for (int i = 0; i < 4; i++) only(F.Cf[i]);
    if (m->cfg.arch == CALD_ARCH_RETINANET) {
        const int K = m->cfg.num_classes, per = m->cfg.detections_per_img;
        for (int i = 0; i < 3; i++) F.inner[i] = B.get<float>(px[3 + i] * 256);
        for (int i = 0; i < 5; i++) F.Pf[i] = B.get<float>(px[3 + i] * 256);
        if (!feat_only) for (int h = 0; h < 2; h++) for (int q = 0; q < 2; q++) for (int i = 0; i < 5; i++) F.ret_t[h][q][i] = B.get<float>(px[3 + i] * 256);
        // RetinaNet: laterals, P3..P5 and P7 feed conv_h3 / conv_h4 layers only; P6 is also read through a ReLU by p7 (fp32 input path of
        // conv_h3); the tower tensors go from matrix-pipe layer to matrix-pipe layer.
        for (int i = 0; i < 3; i++) only(F.inner[i]);
        only(F.Pf[0]); only(F.Pf[1]); only(F.Pf[2]); both(F.Pf[3], F.Pf16[3], px[6] * 256); only(F.Pf[4]);
        if (feat_only) return;
        for (int h = 0; h < 2; h++) for (int q = 0; q < 2; q++) for (int i = 0; i < 5; i++) only(F.ret_t[h][q][i]);
        for (int i = 0; i < 5; i++) { F.cls_h[i] = B.get<float>(px[3 + i] * m->cls_out.Cout); F.reg_h[i] = B.get<float>(px[3 + i] * 36); }
        int maxa = 0;
        for (int v = 0; v < V; v++) { int t = 0; for (int l = 3; l < 8; l++) t += P.seg[l][v].H * P.seg[l][v].W * 9; if (t > maxa) maxa = t; }
        int cap = 1024; while (cap < maxa) cap <<= 1;
        F.max_anchors = maxa; F.cand_cap = cap;
        F.cand_count = B.get<int>((size_t)V * K);
        F.rcand_key = B.get<unsigned long long>((size_t)V * K * cap);
        F.rcand_box = B.get<float>((size_t)V * K * cap * 4);
        F.cand_skip = B.get<unsigned char>((size_t)V * K * cap);
        F.kept_anchor = B.get<int>((size_t)V * K * per);
        F.kept_box = B.get<float>((size_t)V * K * per * 4);
        F.kept_count = B.get<int>((size_t)V * K);
        return;
    }
    for (int i = 0; i < 4; i++) F.inner[i] = B.get<float>(px[2 + i] * 256);
    for (int i = 0; i < 5; i++) F.Pf[i] = B.get<float>(px[2 + i] * 256);
    if (!feat_only) for (int i = 0; i < 5; i++) F.rpn_tl[i] = B.get<float>(px[2 + i] * 256);
    // Faster R-CNN: P2..P5 -> RPN conv (split form) + RoIAlign (fp32): both forms, written by the MFMA-bound 3 x 3 output convs.  P6 is a
    // strided pixel copy of P5 -- a pixel's 1 KB is copied whole, so the copy of the split twin IS the split form of P6 (only the RPN
    // conv reads it).  Laterals: split form only.
    for (int i = 0; i < 4; i++) only(F.inner[i]);
    for (int i = 0; i < 4; i++) both(F.Pf[i], F.Pf16[i], px[2 + i] * 256);
    only(F.Pf[4]);
    if (feat_only) return;
    for (int i = 0; i < 5; i++) F.rpn_h[i] = B.get<float>(px[2 + i] * 15);
    const int pre = m->cfg.rpn_pre_nms_top_n;
    F.cand_key = B.get<unsigned long long>((size_t)V * 5 * pre);
    F.cand_box = B.get<float>((size_t)V * 5 * pre * 4);
    F.sorted_box = B.get<float>((size_t)V * 5 * pre * 4);
    F.sorted_raw = B.get<float>((size_t)V * 5 * pre * 4);
    F.sorted_count = B.get<int>(V);
    F.proposals = B.get<float>((size_t)V * CALD_ROI_CAP * 4);
    F.prop_count = B.get<int>(V);
    F.roi_order = B.get<int>((size_t)V * 1024);
    F.roi = B.get<float>((size_t)V * CALD_ROI_CAP * 12544);
    F.f6 = B.get<float>((size_t)V * CALD_ROI_CAP * 1024);
    F.f7 = B.get<float>((size_t)V * CALD_ROI_CAP * 1024);
    only(F.roi); only(F.f6); only(F.f7);           // RoIAlign -> fc6 -> fc7 -> predictor: conv_h3 layers all the way
    F.pr = B.get<float>((size_t)V * CALD_ROI_CAP * m->pred.Cout);
    F.prob = B.get<float>((size_t)V * CALD_ROI_CAP * m->cfg.num_classes);
    F.pmax = B.get<float>((size_t)V * CALD_ROI_CAP);
    F.keys = B.get<unsigned long long>((size_t)V * m->key_cap);
    F.cbox = B.get<float>((size_t)V * 2 * m->key_cap * 4);
    F.key_count = B.get<int>(V);
    for (int i = 0; i < 2; i++) {
        F.prune_energy[i] = F.prune_pn[i] = F.prune_look[i] = nullptr; F.prune_p16[i] = nullptr;
        for (int s2 = 0; s2 < 2; s2++) { F.prune_rows[s2][i] = nullptr; F.prune_map[s2][i] = nullptr; }
        if (!m->prune) continue;           // RetinaNet never gets here; f16x3 / pruning-off models do not pay for the scratch
        F.prune_energy[i] = B.get<float>(px[2 + i] * 4); F.prune_pn[i] = B.get<float>(px[2 + i]); F.prune_p16[i] = B.get<unsigned>(px[2 + i] * 256);
        for (int s2 = 0; s2 < 2; s2++) { F.prune_rows[s2][i] = B.get<float>(px[2 + i] * 15); F.prune_map[s2][i] = B.get<int>(px[2 + i]); }
        if (m->prune_capture) F.prune_look[i] = B.get<float>(px[2 + i] * 15);
    }
    for (int s2 = 0; s2 < 2; s2++) F.prune_nsel[s2] = m->prune ? B.get<int>((size_t)2 * V) : nullptr;
    F.prune_tau = m->prune ? B.get<unsigned>((size_t)2 * V) : nullptr;
    F.next_key = B.get<unsigned long long>((size_t)V * 10); F.trunc_key = B.get<unsigned long long>((size_t)V * 2);
    F.kept_key = B.get<unsigned long long>((size_t)V * m->det_cap()); F.post_maxc = B.get<float>(V);
}

__global__ void accumulate_rows_kernel(const int* __restrict__ counts, int V, unsigned long long* acc) {
    unsigned long long s = 0;
    for (int v = threadIdx.x; v < V; v += 64) s += (unsigned long long)counts[v];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (threadIdx.x == 0) atomicAdd(acc, s);
}

// views: host descriptors with src/H/W/flip/rects filled; Hr/Wr/Ho/Wo are filled here.  feat (host.h FwdFeatures): the forward stops after
// the FPN and hands out the pyramid; `det` is then not used, and pruning, cut_out reuse and the audit do not apply.
int cald_host::forward_model(cald_model* m, int V, ViewDesc* views, const DetBuffers& det, float* audit_out, bool prune_ok, const FwdReuse* ru,
                             FwdFeatures* feat) {
    cald_ctx* c = m->ctx;
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized (call cald_model_finalize)");
    if (V < 1 || V > CALD_MAX_VIEWS) return fail(CALD_ERR_INVALID, "n_views must be 1..%d", CALD_MAX_VIEWS);
    if (feat && (audit_out || prune_ok || ru)) return fail(CALD_ERR_INVALID, "a features-only forward takes no audit, pruning or cut_out reuse");
    if (!feat && det.cap < m->det_cap()) return fail(CALD_ERR_INVALID, "detection capacity %d < required %d", det.cap, m->det_cap());
    HIPCHK(hipSetDevice(c->device));
    int hp[CALD_MAX_VIEWS][2];
    int max_pix0 = 0, max_pix2 = 0, max_pix6 = 0;
    for (int v = 0; v < V; v++) {
        ViewDesc& d = views[v];
        if (!d.src || d.H <= 0 || d.W <= 0 || d.nrect < 0 || d.nrect > CALD_MAX_CUT) return fail(CALD_ERR_INVALID, "view %d is malformed", v);
        int Hp, Wp;
        transform_size(d.H, d.W, m->cfg.min_size, m->cfg.max_size, &d.Hr, &d.Wr, &Hp, &Wp);
        d.Ho = d.H; d.Wo = d.W;
        if (feat && feat->pad_to) {      // the loader batch's common size (torchvision's ImageList): Hr / Wr stay the view's own, the rest is zero
            const int Hq = feat->pad_to[v][0], Wq = feat->pad_to[v][1];
            if (Hq % 32 || Wq % 32 || Hq < Hp || Wq < Wp)
                return fail(CALD_ERR_INVALID, "view %d: pad_to %d x %d must be a multiple of 32 and at least the view's own %d x %d", v, Hq, Wq, Hp, Wp);
            Hp = Hq; Wp = Wq;
        }
        hp[v][0] = Hp; hp[v][1] = Wp;
        if (Hp * Wp > max_pix0) max_pix0 = Hp * Wp;
    }
    const bool retina = m->cfg.arch == CALD_ARCH_RETINANET;
    if (audit_out && (retina || m->cfg.rpn_pre_nms_top_n > 1024 || m->det_cap() > 512))
        return fail(CALD_ERR_UNSUPPORTED, "the decision-margin audit covers Faster R-CNN with rpn_pre_nms_top_n <= 1024 and <= 512 detections per image");
    build_plan(m->plan, V, views, hp, retina);
    m->last_V = V; m->last_views.assign(views, views + V);
    for (int v = 0; v < V; v++) {
        int p2 = m->plan.seg[2][v].H * m->plan.seg[2][v].W; if (p2 > max_pix2) max_pix2 = p2;
        int p6 = m->plan.seg[6][v].H * m->plan.seg[6][v].W; if (p6 > max_pix6) max_pix6 = p6;
    }
    FwdBufs F;
    { Bump dry(nullptr, true); fwd_layout(m, dry, F, V, feat != nullptr); int rc = arena_reserve(c, dry.off); if (rc) return rc; }
    { Bump real(c->arena, false); fwd_layout(m, real, F, V, feat != nullptr); }
    {
        const int si = c->stage_i; c->stage_i = (si + 1) % cald_ctx::NSTAGE;
        HIPCHK(hipEventSynchronize(c->stage_ev[si]));
        memcpy(c->h_stage[si], &m->plan, sizeof(BatchPlan));
        memcpy(c->h_stage[si] + sizeof(BatchPlan), views, sizeof(ViewDesc) * V);
        HIPCHK(hipMemcpyAsync(c->d_plan, c->h_stage[si], sizeof(BatchPlan), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_views, c->h_stage[si] + sizeof(BatchPlan), sizeof(ViewDesc) * V, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->stage_ev[si], c->stream));
    }
    const BatchPlan* dp = c->d_plan;
    hipStream_t st = c->stream;
    int rc;
    m->dbg.clear();

    // ---- transform + ResNet body (rows A14, A15) ----
    launch_preprocess(c->d_views, dp->seg[0], F.in0, V, max_pix0, st);
    m->dbg["input"] = {F.in0, 0, 4, 0};
    if ((rc = conv_on(m, m->conv1, F.in0, F.c1, 0, 1, V, true))) return rc;
    m->dbg["conv1"] = {F.c1, 1, 64, 0};
    launch_maxpool(F.c1, F.p1, dp->seg[1], dp->seg[2], 64, V, max_pix2, st, m->split.count(F.p1) != 0);
    m->dbg["pool1"] = {F.p1, 2, 64, 0};
    const float* cur = F.p1; int lvl = 2, layer = 0, xi = 0;
    for (size_t b = 0; b < m->blocks.size(); b++) {
        const Bottleneck& B = m->blocks[b];
        const int lout = lvl + (B.c2.stride == 2 ? 1 : 0);
        const bool kept = ru && (int)b < ru->nblk;          // cut_out reuse: this block's output is the retained tensor
        float* dst = kept ? ru->out[b] : (B.layer_end ? F.Cf[layer] : F.X[xi]);
        const float* idn = cur;
        if (kept && ru->mode == 2 && ru->gather[layer]) {
            // the dirty pixels only: T1 on what conv2's windows read, the rest on the dirty set of the output, written over the retained tensor
            if (B.has_down) { if ((rc = gconv_on(m, B.down, cur, F.D, lvl, lout, V, false, nullptr, *ru, (int)b, 0))) return rc; idn = F.D; }
            if ((rc = gconv_on(m, B.c1, cur, F.T1, lvl, lvl, V, true, nullptr, *ru, (int)b, 1))) return rc;
            if ((rc = gconv_on(m, B.c2, F.T1, F.T2, lvl, lout, V, true, nullptr, *ru, (int)b, 0))) return rc;
            if ((rc = gconv_on(m, B.c3, F.T2, dst, lout, lout, V, true, idn, *ru, (int)b, 0))) return rc;
        } else {
            if (B.has_down) { if ((rc = conv_on(m, B.down, cur, F.D, lvl, lout, V, false))) return rc; idn = F.D; }
            if ((rc = conv_on(m, B.c1, cur, F.T1, lvl, lvl, V, true))) return rc;
            if ((rc = conv_pair_on(m, B.c2, B.c3, F.T1, F.T2, dst, lvl, lout, V, idn))) return rc;
        }
        if (B.layer_end) F.Cf[layer] = dst;
        cur = dst; lvl = lout;
        if (B.layer_end) layer++; else xi ^= 1;
    }
    const char* cn[4] = {"C2", "C3", "C4", "C5"};
    const int cch[4] = {256, 512, 1024, 2048};
    for (int i = 0; i < 4; i++) m->dbg[cn[i]] = {F.Cf[i], 2 + i, cch[i], 0};
    if (retina) {
        // ---- FPN on C3..C5 + LastLevelP6P7 (retinanet_cal.py:618-619) ----
        if ((rc = conv_on(m, m->fpn_inner[2], F.Cf[3], F.inner[2], 5, 5, V, false))) return rc;
        for (int i = 1; i >= 0; i--)
            if ((rc = conv_on(m, m->fpn_inner[i], F.Cf[1 + i], F.inner[i], 3 + i, 3 + i, V, false, nullptr, F.inner[i + 1], 4 + i))) return rc;
        {
            ConvSpec sp[3];
            for (int i = 0; i < 3; i++) sp[i] = {&m->fpn_layer[i], F.inner[i], F.Pf[i], 3 + i, false};
            if ((rc = conv_group_on(m, sp, 3, V))) return rc;
        }
        if ((rc = conv_on(m, m->p6, F.Pf[2], F.Pf[3], 5, 6, V, false))) return rc;
        const char* pn[5] = {"P3", "P4", "P5", "P6", "P7"};
        if (feat) {                  // P3..P6, and P7 where the caller pools it
            const int np = feat->p7 ? 5 : 4;
            if (feat->p7 && (rc = conv_on(m, m->p7, F.Pf[3], F.Pf[4], 6, 7, V, false, nullptr, nullptr, 0, nullptr, true))) return rc;
            for (int i = 0; i < np; i++) {
                m->dbg[pn[i]] = {F.Pf[i], 3 + i, 256, 0};
                auto sp = m->split.find(F.Pf[i]);
                feat->P[i] = F.Pf[i]; feat->split_only[i] = sp != m->split.end() && sp->second.fp32_dead; feat->plan_level[i] = 3 + i;
            }
            HIPCHK(hipGetLastError());
            return 0;
        }
        if ((rc = conv_on(m, m->p7, F.Pf[3], F.Pf[4], 6, 7, V, false, nullptr, nullptr, 0, nullptr, true))) return rc;
        const char* cnm[5] = {"cls0", "cls1", "cls2", "cls3", "cls4"};
        const char* rnm[5] = {"reg0", "reg1", "reg2", "reg3", "reg4"};
        for (int i = 0; i < 5; i++) m->dbg[pn[i]] = {F.Pf[i], 3 + i, 256, 0};
        // ---- heads (retinanet_cal.py:36-241): 4 x (3x3 conv + ReLU) + 3x3 output conv, per level ----
        // both towers x five levels share one launch per tower depth (10 independent problems, weights shared across levels)
        for (int t = 0; t < 4; t++) {
            ConvSpec sp[10];
            for (int hsel = 0; hsel < 2; hsel++)
                for (int i = 0; i < 5; i++)
                    sp[hsel * 5 + i] = {&(hsel == 0 ? m->cls_tower : m->reg_tower)[t], t == 0 ? F.Pf[i] : F.ret_t[hsel][(t - 1) & 1][i],
                                        F.ret_t[hsel][t & 1][i], 3 + i, true};
            if ((rc = conv_group_on(m, sp, 10, V))) return rc;
        }
        for (int hsel = 0; hsel < 2; hsel++) {
            ConvSpec sp[5];
            for (int i = 0; i < 5; i++) sp[i] = {hsel == 0 ? &m->cls_out : &m->reg_out, F.ret_t[hsel][1][i], hsel == 0 ? F.cls_h[i] : F.reg_h[i], 3 + i, false};
            if ((rc = conv_group_on(m, sp, 5, V))) return rc;
        }
        for (int i = 0; i < 5; i++) {
            m->dbg[cnm[i]] = {F.cls_h[i], 3 + i, m->cls_out.Cout, 0};
            m->dbg[rnm[i]] = {F.reg_h[i], 3 + i, 36, 0};
        }
        RetinaArgs ra;
        for (int i = 0; i < 5; i++) { ra.cls[i] = F.cls_h[i]; ra.reg[i] = F.reg_h[i]; ra.seg[i] = dp->seg[3 + i]; }
        ra.seg0 = dp->seg[0]; ra.views = c->d_views; ra.base_anchors = m->d_anchors;
        ra.cls_ld = m->cls_out.Cout; ra.reg_ld = 36; ra.A = 9; ra.K = m->cfg.num_classes; ra.V = V;
        ra.score_thr = m->cfg.box_score_thresh; ra.nms_thr = m->cfg.box_nms_thresh; ra.min_box = 1e-2f;
        ra.per_class = m->cfg.detections_per_img; ra.cand_cap = F.cand_cap;
        ra.cand_count = F.cand_count; ra.cand_key = F.rcand_key; ra.cand_box = F.rcand_box; ra.cand_skip = F.cand_skip;
        ra.kept_anchor = F.kept_anchor; ra.kept_box = F.kept_box; ra.kept_count = F.kept_count; ra.det = det;
        launch_retina_postprocess(ra, F.max_anchors, st);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // ---- FPN (row A16) ----
    const bool prune = m->prune && prune_ok;
    if ((rc = conv_on(m, m->fpn_inner[3], F.Cf[3], F.inner[3], 5, 5, V, false))) return rc;
    for (int i = 2; i >= 0; i--)
        if ((rc = conv_on(m, m->fpn_inner[i], F.Cf[i], F.inner[i], 2 + i, 2 + i, V, false, nullptr, F.inner[i + 1], 3 + i))) return rc;
    {
        ConvSpec sp[4];
        for (int i = 0; i < 4; i++) sp[i] = {&m->fpn_layer[i], F.inner[i], F.Pf[i], 2 + i, false};
        if (prune)                // the pruning's per-pixel energy and the look-ahead's split-fp16 operand come out of these convs' epilogues (conv_p4.hip)
            for (int i = 0; i < 2; i++) { sp[i].out16 = F.prune_p16[i]; sp[i].energy4 = F.prune_energy[i]; }
        if ((rc = conv_group_on(m, sp, 4, V))) return rc;
    }
    if (feat) {                      // P2..P5: neither LastLevelMaxPool nor the RPN runs
        const char* fn[4] = {"P2", "P3", "P4", "P5"};
        for (int i = 0; i < 4; i++) {
            m->dbg[fn[i]] = {F.Pf[i], 2 + i, 256, 0};
            auto sp = m->split.find(F.Pf[i]);
            feat->P[i] = F.Pf[i]; feat->split_only[i] = sp != m->split.end() && sp->second.fp32_dead; feat->plan_level[i] = 2 + i;
        }
        HIPCHK(hipGetLastError());
        return 0;
    }
    {   // LastLevelMaxPool: max_pool2d(P5, 1, 2) = every other pixel of every other row; in F16X3 the copy runs on P5's split twin
        auto tw = m->split.find(F.Pf[3]);
        const bool p6_split = m->split.count(F.Pf[4]) != 0 && tw != m->split.end();
        launch_subsample2(p6_split ? reinterpret_cast<const float*>(tw->second.s16) : F.Pf[3], F.Pf[4], dp->seg[5], dp->seg[6], 256, V, max_pix6, st);
    }
    const char* pn[5] = {"P2", "P3", "P4", "P5", "P6"};
    for (int i = 0; i < 5; i++) m->dbg[pn[i]] = {F.Pf[i], 2 + i, 256, 0};
    // ---- RPN (row A17) ----
    const char* rn[5] = {"rpn0", "rpn1", "rpn2", "rpn3", "rpn4"};
    if (prune) {
        // certified pruning (rpn_prune.hip): P2 / P3 first on the fp16 matrix pipe, then exactly at the pixels that can hold one of the
        // level's pre_nms_top_n anchors; P4..P6 dense as ever.  Same bits at every anchor the top-k can select.
        ConvSpec sp[5];
        RpnPruneArgs pr;
        for (int i = 0; i < 2; i++) {
            pr.seg[i] = dp->seg[2 + i]; pr.energy[i] = F.prune_energy[i]; pr.pnorm[i] = F.prune_pn[i]; pr.head[i] = F.rpn_h[i]; pr.head_out[i] = F.rpn_h[i];
            for (int s2 = 0; s2 < 2; s2++) { pr.head_rows[s2][i] = F.prune_rows[s2][i]; pr.row_map[s2][i] = F.prune_map[s2][i]; }
        }
        int log_slot[2];
        for (int s2 = 0; s2 < 2; s2++) {
            log_slot[s2] = (c->prof && c->prune_log_n < CALD_PRUNE_LOG) ? c->prune_log_n++ : -1;
            pr.nsel[s2] = F.prune_nsel[s2]; pr.log[s2] = log_slot[s2] >= 0 ? c->d_prune_log + (size_t)log_slot[s2] * 4 : nullptr;
        }
        pr.tau_key = F.prune_tau; pr.stat = c->prof ? c->d_prune_stat : nullptr; pr.check = c->d_prune_check;
        for (int q = 0; q < 3; q++) { pr.c1[q] = m->prune_c1[q]; pr.c0[q] = m->prune_c0[q]; }
        pr.head_ld = 15; pr.pre_n = m->cfg.rpn_pre_nms_top_n; pr.V = V;
        c->prof_tag_now = 1;
        for (int i = 0; i < 2; i++) { sp[i] = {&m->rpn_conv16, F.Pf[i], F.rpn_tl[i], 2 + i, true}; sp[i].in16 = F.prune_p16[i]; }
        rc = conv_group_on(m, sp, 2, V);
        for (int i = 0; i < 2; i++) sp[i] = {&m->rpn_head, F.rpn_tl[i], F.rpn_h[i], 2 + i, false};
        if (!rc) rc = conv_group_on(m, sp, 2, V);
        c->prof_tag_now = 0;
        if (rc) return rc;
        // FLOPs the gathered launches are booked with when they cover every pixel (each stage's launches are: cald_profile_read / _dump rescale them)
        const double cap_conv[2] = {2.0 * (double)level_pix(m->plan, 2, V) * 2304.0 * 256.0, 2.0 * (double)level_pix(m->plan, 3, V) * 2304.0 * 256.0};
        const double cap_head[2] = {2.0 * (double)level_pix(m->plan, 2, V) * 256.0 * 15.0, 2.0 * (double)level_pix(m->plan, 3, V) * 256.0 * 15.0};
        if (m->prune_capture)
            for (int i = 0; i < 2; i++) {
                HIPCHK(hipMemcpyAsync(F.prune_look[i], F.rpn_h[i], (size_t)level_pix(m->plan, 2 + i, V) * 15 * sizeof(float), hipMemcpyDeviceToDevice, st));
                const char* ln[2] = {"rpn_look0", "rpn_look1"}; const char* bn[2] = {"rpn_pnorm0", "rpn_pnorm1"};
                m->dbg[ln[i]] = {F.prune_look[i], 2 + i, 15, 0}; m->dbg[bn[i]] = {F.prune_pn[i], 2 + i, 1, 0};
            }
        // stage 0 recomputes P2 / P3 rows only; stage 1's launches also carry the dense levels P4..P6
        for (int s2 = 0; s2 < 2; s2++) {
            const int np = s2 == 1 ? 5 : 2;
            launch_rpn_prune_select(pr, max_pix2, s2, st);
            for (int i = 0; i < np; i++) sp[i] = {&m->rpn_conv, F.Pf[i], F.rpn_tl[i], 2 + i, true};
            for (int i = 0; i < 2; i++) { sp[i].dyn = F.prune_nsel[s2] + i * V; sp[i].row_map = F.prune_map[s2][i]; }      // gathered rows, compact output
            if ((rc = conv_group_on(m, sp, np, V))) return rc;
            if (c->prof) {
                for (int i = 0; i < 2; i++) c->prof_prune_flops_cap[i] += cap_conv[i];
                if (log_slot[s2] >= 0) c->prof_gather[c->prof_launches.size() - 1] = {log_slot[s2], {cap_conv[0], cap_conv[1]}};
            }
            for (int i = 0; i < np; i++) sp[i] = {&m->rpn_head, F.rpn_tl[i], i < 2 ? F.prune_rows[s2][i] : F.rpn_h[i], 2 + i, false};
            for (int i = 0; i < 2; i++) sp[i].dyn = F.prune_nsel[s2] + i * V;
            if ((rc = conv_group_on(m, sp, np, V))) return rc;
            if (c->prof) {
                for (int i = 0; i < 2; i++) c->prof_prune_flops_cap[i] += cap_head[i];
                if (log_slot[s2] >= 0) c->prof_gather[c->prof_launches.size() - 1] = {log_slot[s2], {cap_head[0], cap_head[1]}};
            }
        }
        launch_rpn_prune_scatter(pr, st);
        for (int i = m->prune_capture ? 0 : 2; i < 5; i++) m->dbg[rn[i]] = {F.rpn_h[i], 2 + i, 15, 0};      // (P2 / P3 head maps are exact only where selected, -FLT_MAX elsewhere: a debug view in capture mode only)
    } else {   // the shared-weight RPN head over the five levels: one launch for the 3x3 conv, one for the fused 1x1 heads
        ConvSpec sp[5];
        for (int i = 0; i < 5; i++) sp[i] = {&m->rpn_conv, F.Pf[i], F.rpn_tl[i], 2 + i, true};
        if ((rc = conv_group_on(m, sp, 5, V))) return rc;
        for (int i = 0; i < 5; i++) sp[i] = {&m->rpn_head, F.rpn_tl[i], F.rpn_h[i], 2 + i, false};
        if ((rc = conv_group_on(m, sp, 5, V))) return rc;
        for (int i = 0; i < 5; i++) m->dbg[rn[i]] = {F.rpn_h[i], 2 + i, 15, 0};
    }
    RpnArgs ra;
    for (int i = 0; i < 5; i++) { ra.head[i] = F.rpn_h[i]; ra.seg[i] = dp->seg[2 + i]; }
    ra.seg0 = dp->seg[0]; ra.views = c->d_views; ra.base_anchors = m->d_anchors;
    ra.head_ld = 15; ra.A = 3; ra.V = V; ra.pre_n = m->cfg.rpn_pre_nms_top_n; ra.post_n = m->cfg.rpn_post_nms_top_n;
    ra.nms_thr = m->cfg.rpn_nms_thresh; ra.min_size = 1e-3f;
    ra.cand_key = F.cand_key; ra.cand_box = F.cand_box; ra.sorted_box = F.sorted_box; ra.sorted_raw = F.sorted_raw;
    ra.sorted_count = F.sorted_count; ra.proposals = F.proposals; ra.prop_stride = CALD_ROI_CAP; ra.prop_count = F.prop_count;
    ra.next_key = audit_out ? F.next_key : nullptr; ra.trunc_key = audit_out ? F.trunc_key : nullptr;
    launch_rpn(ra, st);
    m->dbg["proposals"] = {F.proposals, 7, 4, 1};
    // ---- box head (rows A18, A19, A20) ----
    RoiArgs ro;
    for (int i = 0; i < 4; i++) { ro.feat[i] = F.Pf[i]; ro.seg[i] = dp->seg[2 + i]; }
    ro.C = 256; ro.V = V; ro.proposals = F.proposals; ro.prop_count = F.prop_count; ro.out = F.roi; ro.order = F.roi_order;
    ro.out16 = m->split.count(F.roi) ? 1 : 0;
    launch_roi_align(ro, st);
    m->dbg["roi"] = {F.roi, 7, 12544, 1};
    const double fl_before_roi = c->prof_flops;
    // The RoI buffers are dense [V][1000][C]; as per-view problems every view pads its 1 000 rows to eight 128-row tiles (2.4 % idle
    // rows in fc6).  Rows of a GEMM are independent, so the three layers run as ONE problem of V * 1000 rows (level 8: 500 tiles for
    // 64 views, a tile may straddle two views; segments of 32 views keep byte offsets inside 31 bits).  Rows beyond a view's proposal count hold stale finite-or-not data and are never
    // read downstream (post-processing walks r < count); the profile counts FLOPs on the measured rows as before.
    const int Vr = (V + ROI_DENSE_VIEWS - 1) / ROI_DENSE_VIEWS;
    if ((rc = conv_on(m, m->fc6, F.roi, F.f6, 8, 8, Vr, true))) return rc;
    if ((rc = conv_on(m, m->fc7, F.f6, F.f7, 8, 8, Vr, true))) return rc;
    if ((rc = conv_on(m, m->pred, F.f7, F.pr, 8, 8, Vr, false))) return rc;
    if (c->prof) {
        hipLaunchKernelGGL(accumulate_rows_kernel, dim3(1), dim3(64), 0, st, F.prop_count, V, c->d_roi_rows);
        c->prof_roi_rows_cap += (double)V * CALD_ROI_CAP; c->prof_roi_flops_cap += c->prof_flops - fl_before_roi; c->prof_roi_views += V;
    }
    m->dbg["fc6"] = {F.f6, 7, 1024, 1}; m->dbg["fc7"] = {F.f7, 7, 1024, 1}; m->dbg["pred"] = {F.pr, 7, m->pred.Cout, 1};
    PostArgs pa;
    pa.pred = F.pr; pa.pred_ld = m->pred.Cout; pa.C = m->cfg.num_classes; pa.V = V;
    pa.proposals = F.proposals; pa.prop_count = F.prop_count; pa.views = c->d_views;
    pa.score_thr = m->cfg.box_score_thresh; pa.nms_thr = m->cfg.box_nms_thresh;
    pa.prob = F.prob; pa.pmax = F.pmax; pa.keys = F.keys; pa.cbox = F.cbox; pa.key_count = F.key_count; pa.key_cap = m->key_cap;
    pa.det = det;
    pa.kept_key = audit_out ? F.kept_key : nullptr; pa.post_maxc = audit_out ? F.post_maxc : nullptr;
    launch_frcnn_postprocess(pa, st);
    if (audit_out) {
        AuditArgs au;
        au.cand_key = F.cand_key; au.cand_box = F.cand_box; au.sorted_box = F.sorted_box; au.flags = reinterpret_cast<const unsigned char*>(F.sorted_raw);
        au.next_key = F.next_key; au.trunc_key = F.trunc_key; au.pre_n = ra.pre_n; au.post_n = ra.post_n; au.rpn_nms_thr = ra.nms_thr; au.min_size = ra.min_size;
        au.proposals = F.proposals; au.prop_count = F.prop_count;
        for (int i = 0; i < 4; i++) au.seg[i] = dp->seg[2 + i];
        au.prob = F.prob; au.pred = F.pr; au.pred_ld = m->pred.Cout; au.C = m->cfg.num_classes; au.views = c->d_views;
        au.keys = F.keys; au.key_count = F.key_count; au.key_cap = m->key_cap; au.kept_key = F.kept_key; au.post_maxc = F.post_maxc;
        au.det_count = det.count; au.cap = det.cap; au.score_thr = pa.score_thr; au.post_nms_thr = pa.nms_thr;
        au.V = V; au.delta = 1e-2f; au.out = audit_out;
        launch_audit(au, st);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int fill_view(ViewDesc& d, const cald_view& v) {
    memset(&d, 0, sizeof(d));
    d.src = v.image_dev; d.H = v.H; d.W = v.W; d.flip = v.flip ? 1 : 0; d.nrect = v.nrect; d.noise = v.noise_dev;
    if (v.nrect < 0 || v.nrect > CALD_MAX_CUT) return fail(CALD_ERR_INVALID, "nrect must be 0..%d", CALD_MAX_CUT);
    for (int i = 0; i < 4 * v.nrect; i++) d.rects[i] = v.rects[i];
    return 0;
}

extern "C" int cald_forward(cald_model* m, int n_views, const cald_view* views, const cald_dets* out) {
    if (!m || !views || !out) return fail(CALD_ERR_INVALID, "null argument");
    if (n_views < 1 || n_views > CALD_MAX_VIEWS) return fail(CALD_ERR_INVALID, "n_views must be 1..%d", CALD_MAX_VIEWS);
    std::vector<ViewDesc> vd(n_views);
    for (int i = 0; i < n_views; i++) { int rc = fill_view(vd[i], views[i]); if (rc) return rc; }
    DetBuffers det;
    det.boxes = out->boxes_dev; det.scores = out->scores_dev; det.labels = (long long*)out->labels_dev; det.props = out->props_dev;
    det.prob_max = out->prob_max_dev; det.scores_cls = out->scores_cls_dev; det.count = out->count_dev;
    det.cap = out->cap; det.C = m->cfg.num_classes;
    if (!det.boxes || !det.scores || !det.labels || !det.props || !det.prob_max || !det.scores_cls || !det.count)
        return fail(CALD_ERR_INVALID, "output buffers must all be provided");
    return forward_model(m, n_views, vd.data(), det, nullptr, m->prune_capture);
}

extern "C" int cald_debug_tensor(cald_model* m, const char* name, int view, float* host_out, int64_t capacity, int64_t* shape3) {
    if (!m || !name || !host_out || !shape3) return fail(CALD_ERR_INVALID, "null argument");
    auto it = m->dbg.find(name);
    if (it == m->dbg.end()) return fail(CALD_ERR_INVALID, "no intermediate tensor named '%s'", name);
    if (view < 0 || view >= m->last_V) return fail(CALD_ERR_INVALID, "view out of range");
    const DebugEntry& e = it->second;
    const LevelSeg& s = m->plan.seg[e.level][view];
    int64_t n = (int64_t)s.H * s.W * e.C;
    shape3[0] = s.H; shape3[1] = s.W; shape3[2] = e.C;
    if (n > capacity) return fail(CALD_ERR_INVALID, "buffer too small: need %lld floats", (long long)n);
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    HIPCHK(hipMemcpy(host_out, e.ptr + s.pix_off * e.C, n * sizeof(float), hipMemcpyDeviceToHost));
    auto sp = m->split.find(e.ptr);
    if (sp != m->split.end() && sp->second.fp32_dead) {
        // CALD_PRECISION_F16X3: the tensor exists in split form only (h16.h: per 16-channel chunk [16 fp16 hi | 16 fp16 lo] of 16 x, in
        // the buffer the fp32 tensor would have used) -- hand out the values, not the raw words
        if (e.C % 16) return fail(CALD_ERR_STATE, "split-form tensor '%s' with %d channels", name, e.C);
        std::vector<float> dec((size_t)n);
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(host_out);
        for (int64_t p = 0; p < n / e.C; p++)
            for (int c = 0; c < e.C; c++) {
                const unsigned char* b = raw + ((size_t)p * e.C + (c & ~15)) * 4 + (c & 15) * 2;
                _Float16 hi, lo; memcpy(&hi, b, 2); memcpy(&lo, b + 32, 2);
                dec[(size_t)p * e.C + c] = ((float)hi + (float)lo) * 0.0625f;
            }
        memcpy(host_out, dec.data(), (size_t)n * sizeof(float));
    }
    return 0;
}
