// forward.hip -- one forward of the detector over a ragged batch of views: the level plan, each stage's arena layout, the conv launches of every layer
// (single, fused pair, group, gathered rows of the cut_out reuse), forward_model as a run of named stages (ForwardRun) up to the tail its FwdRequest names, cald_forward, cald_debug_tensor.
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

// ---- arena scratch, one struct per stage of ForwardRun; a stage that does not run is not laid out.  Bump::get rounds every buffer to 256
// bytes on its own, so the arena's total does not depend on the order of the calls ----
// split forms (F16X3, h16.h): every tensor whose readers are conv_h3 / conv_h4 layers lives in split form ONLY, in the buffer the fp32
// tensor would have used (same 4 bytes per element): the pooled stem output, the inner tensors of a bottleneck, the block outputs
// (read as a GEMM operand by the next block's conv1 / downsample conv / the FPN lateral, and as the residual by conv3's epilogue,
// which joins hi + lo again), the downsample branch, the laterals (operand of the 3 x 3 output conv, top-down term of the next
// lateral's epilogue).  22 significant bits instead of 24 on those tensors -- the precision every GEMM operand of this mode has.
struct SplitReg {
    cald_model* m; Bump& B; bool on;
    void only(float* t) { if (on) m->split[t] = {reinterpret_cast<unsigned*>(t), true}; }
    void both(float* t, unsigned*& twin, size_t n) { if (on) { twin = B.get<unsigned>(n); m->split[t] = {twin, false}; } }      // fp32 and a split twin
};
static const int CCH[4] = {256, 512, 1024, 2048};      // channels of C2..C5
struct BodyBufs {
    float *in0, *c1, *p1, *X[2], *T1, *T2, *D, *Cf[4];
    void layout(Bump& B, SplitReg& S, const long long* px) {
        in0 = B.get<float>(px[0] * 4); c1 = B.get<float>(px[1] * 64); p1 = B.get<float>(px[2] * 64);
        X[0] = B.get<float>(px[2] * 256); X[1] = B.get<float>(px[2] * 256);
        T1 = B.get<float>(px[2] * 128); T2 = B.get<float>(px[2] * 64); D = B.get<float>(px[2] * 256);
        for (int i = 0; i < 4; i++) { Cf[i] = B.get<float>(px[2 + i] * CCH[i]); S.only(Cf[i]); }
        S.only(p1); S.only(T1); S.only(T2); S.only(X[0]); S.only(X[1]); S.only(D);
    }
};
// Faster R-CNN: four laterals and P2..P6 from level 2.  P2..P5 -> RPN conv (split form) + RoIAlign (fp32): both forms, written by the
// MFMA-bound 3 x 3 output convs.  P6 is a strided pixel copy of P5 -- a pixel's 1 KB is copied whole, so the copy of the split twin IS the
// split form of P6 (only the RPN conv reads it).  RetinaNet: three laterals and P3..P7 from level 3.  P3..P5 and P7 feed conv_h3 / conv_h4
// layers only; P6 is also read through a ReLU by p7 (fp32 input path of conv_h3).  Laterals: split form only.
struct PyramidBufs {
    float *inner[4], *Pf[5]; unsigned* Pf16[5];   // CALD_PRECISION_F16X3: split twins of the tensors that stay fp32 as well
    void layout(Bump& B, SplitReg& S, const long long* px, bool retina) {
        const int first = retina ? 3 : 2, nl = retina ? 3 : 4;
        for (int i = 0; i < nl; i++) { inner[i] = B.get<float>(px[first + i] * 256); S.only(inner[i]); }
        for (int i = 0; i < 5; i++) {
            Pf[i] = B.get<float>(px[first + i] * 256);
            if (i == 4 || (retina && i < 3)) S.only(Pf[i]); else S.both(Pf[i], Pf16[i], px[first + i] * 256);
        }
    }
};
void cald_host::RetinaTailBufs::layout(Bump& B, int V, int K, int per_class, int maxa) {
    max_anchors = maxa;
    cand_cap = 1024; while (cand_cap < maxa) cand_cap <<= 1;       // a power of two at least the anchor count
    cand_count = B.get<int>((size_t)V * K); cand_key = B.get<unsigned long long>((size_t)V * K * cand_cap);
    cand_box = B.get<float>((size_t)V * K * cand_cap * 4); cand_skip = B.get<unsigned char>((size_t)V * K * cand_cap);
    kept_anchor = B.get<int>((size_t)V * K * per_class); kept_box = B.get<float>((size_t)V * K * per_class * 4); kept_count = B.get<int>((size_t)V * K);
}
void cald_host::RetinaSsmBufs::layout(Bump& B, int V, int K, int per_class, int maxa) {
    cand_cap = maxa > 0 ? maxa : 1; nblk = (cand_cap + 255) / 256;
    const size_t VK = (size_t)V * K, rows = VK * per_class;
    cand_count = B.get<int>(VK); blk_off = B.get<int>(VK * nblk); list = B.get<int>(VK * cand_cap); vmax = B.get<unsigned>(V); al = B.get<int>(V);
    picks = B.get<int>(VK * CALD_SSM_RETINA_TAKE); n_picks = B.get<int>(VK);
    kept_anchor = B.get<int>(rows); kept_box = B.get<float>(rows * 4); kept_count = B.get<int>(VK);
    row_off = B.get<int>(VK); count = B.get<int>(V); total = B.get<int>(1);
    boxes = B.get<float>(rows * 4); scores = B.get<float>(rows); labels = B.get<signed char>(rows * (K - 1));
}
struct RetinaBufs {
    float *ret_t[2][2][5], *cls_h[5], *reg_h[5]; RetinaTailBufs tail;   // ret_t[tower][ping-pong][level]: from matrix-pipe layer to matrix-pipe layer
    void layout(Bump& B, SplitReg& S, const long long* px, int V, int cls_ld, int K, int per_class, int max_anchors, RetinaSsmBufs* ssm_tail) {
        for (int h = 0; h < 2; h++) for (int q = 0; q < 2; q++) for (int i = 0; i < 5; i++) { ret_t[h][q][i] = B.get<float>(px[3 + i] * 256); S.only(ret_t[h][q][i]); }
        for (int i = 0; i < 5; i++) { cls_h[i] = B.get<float>(px[3 + i] * cls_ld); reg_h[i] = B.get<float>(px[3 + i] * 36); }
        if (ssm_tail) ssm_tail->layout(B, V, K, per_class, max_anchors); else tail.layout(B, V, K, per_class, max_anchors);
    }
};
void cald_host::ProposalBufs::layout(Bump& B, int V) { proposals = B.get<float>((size_t)V * CALD_ROI_CAP * 4); prop_count = B.get<int>(V); }
struct RpnBufs {
    float *rpn_tl[5], *rpn_h[5], *cand_box, *sorted_box, *sorted_raw; unsigned long long* cand_key; int* sorted_count; ProposalBufs prop;
    void layout(Bump& B, const long long* px, int V, int pre) {
        for (int i = 0; i < 5; i++) { rpn_tl[i] = B.get<float>(px[2 + i] * 256); rpn_h[i] = B.get<float>(px[2 + i] * 15); }
        cand_key = B.get<unsigned long long>((size_t)V * 5 * pre); cand_box = B.get<float>((size_t)V * 5 * pre * 4);
        sorted_box = B.get<float>((size_t)V * 5 * pre * 4); sorted_raw = B.get<float>((size_t)V * 5 * pre * 4); sorted_count = B.get<int>(V);
        prop.layout(B, V);
    }
};
// certified RPN pruning (rpn_prune.hip), levels P2 / P3: f16x3 / pruning-off models do not pay for the scratch
struct PruneBufs {
    float *energy[2] = {}, *pn[2] = {}, *rows[2][2] = {}; int *map[2][2] = {}, *nsel[2] = {}; unsigned* p16[2] = {}; unsigned* tau = nullptr;   // [stage][level] row lists of the two selection stages
    float* look[2] = {};         // capture mode only: the look-ahead's head map before select / scatter overwrite it
    void layout(Bump& B, const long long* px, int V, bool capture) {
        for (int i = 0; i < 2; i++) {
            energy[i] = B.get<float>(px[2 + i] * 4); pn[i] = B.get<float>(px[2 + i]); p16[i] = B.get<unsigned>(px[2 + i] * 256);
            for (int s2 = 0; s2 < 2; s2++) { rows[s2][i] = B.get<float>(px[2 + i] * 15); map[s2][i] = B.get<int>(px[2 + i]); }
            if (capture) look[i] = B.get<float>(px[2 + i] * 15);
        }
        for (int s2 = 0; s2 < 2; s2++) nsel[s2] = B.get<int>((size_t)2 * V);
        tau = B.get<unsigned>((size_t)2 * V);
    }
};
void cald_host::RoiBufs::layout(Bump& B, int V, int C) { order = B.get<int>((size_t)V * 1024); roi = B.get<float>((size_t)V * CALD_ROI_CAP * 49 * C); }
void cald_host::PostBufs::layout(Bump& B, int V, int C, int cap) {
    key_cap = cap;
    prob = B.get<float>((size_t)V * CALD_ROI_CAP * C); pmax = B.get<float>((size_t)V * CALD_ROI_CAP);
    keys = B.get<unsigned long long>((size_t)V * key_cap); cbox = B.get<float>((size_t)V * 2 * key_cap * 4); key_count = B.get<int>(V);
    skip = B.get<unsigned char>((size_t)V * key_cap);
}
void cald_host::SsmBufs::layout(Bump& B, int V, int C, int cap) {
    const size_t K = (size_t)(C - 1), rows = (size_t)V * K * cap;
    prob = B.get<float>((size_t)V * CALD_ROI_CAP * C); vmax = B.get<unsigned>(V);
    kept_prop = B.get<int>(rows); kept_box = B.get<float>(rows * 4); cls_count = B.get<int>((size_t)V * K); row_off = B.get<int>((size_t)V * K);
    al = B.get<int>(V); count = B.get<int>(V); total = B.get<int>(1);
    boxes = B.get<float>(rows * 4); scores = B.get<float>(rows * K); labels = B.get<signed char>(rows * K);
}
struct BoxBufs {
    RoiBufs roi; float *f6, *f7, *pr; PostBufs post;
    void layout(Bump& B, SplitReg& S, int V, int pred_ld, int C, int key_cap) {
        roi.layout(B, V, 256);
        f6 = B.get<float>((size_t)V * CALD_ROI_CAP * 1024); f7 = B.get<float>((size_t)V * CALD_ROI_CAP * 1024);
        S.only(roi.roi); S.only(f6); S.only(f7);           // RoIAlign -> fc6 -> fc7 -> predictor: conv_h3 layers all the way
        pr = B.get<float>((size_t)V * CALD_ROI_CAP * pred_ld);
        post.layout(B, V, C, key_cap);
    }
};
// decision-margin audit (audit.hip): what the RPN / post-processing kernels leave behind for it
struct AuditBufs {
    unsigned long long *next_key, *trunc_key, *kept_key; float* post_maxc;
    void layout(Bump& B, int V, int det_cap) {
        next_key = B.get<unsigned long long>((size_t)V * 10); trunc_key = B.get<unsigned long long>((size_t)V * 2);
        kept_key = B.get<unsigned long long>((size_t)V * det_cap); post_maxc = B.get<float>(V);
    }
};

RoiArgs cald_host::roi_args(const RoiBufs& S, const float* const* feat, const BatchPlan* plan, int C, int V, const ProposalBufs& P, bool out16) {
    RoiArgs ro{};
    for (int i = 0; i < 4; i++) { ro.feat[i] = feat[i]; ro.seg[i] = plan->seg[2 + i]; }
    ro.C = C; ro.V = V; ro.proposals = P.proposals; ro.prop_count = P.prop_count; ro.out = S.roi; ro.order = S.order; ro.out16 = out16 ? 1 : 0;
    return ro;
}
PostArgs cald_host::post_args(const PostBufs& S, const float* pred, int pred_ld, int C, int V, const ProposalBufs& P, const ViewDesc* views,
                              float score_thr, float nms_thr, const DetBuffers& det) {
    PostArgs pa{};
    pa.pred = pred; pa.pred_ld = pred_ld; pa.C = C; pa.V = V; pa.proposals = P.proposals; pa.prop_count = P.prop_count; pa.views = views; pa.score_thr = score_thr; pa.nms_thr = nms_thr;
    pa.prob = S.prob; pa.pmax = S.pmax; pa.keys = S.keys; pa.cbox = S.cbox; pa.key_count = S.key_count; pa.key_cap = S.key_cap; pa.det = det;
    pa.skip = S.skip;
    return pa;
}
SsmArgs cald_host::ssm_args(const SsmBufs& S, const float* pred, int pred_ld, int C, int V, const ProposalBufs& P, const ViewDesc* views, float score_thr, int cap) {
    SsmArgs sa{};
    sa.pred = pred; sa.pred_ld = pred_ld; sa.C = C; sa.V = V; sa.proposals = P.proposals; sa.prop_count = P.prop_count; sa.views = views;
    sa.score_thr = score_thr; sa.nms_thr = SSM_NMS_THR; sa.conf_thr = SSM_CONF_THR; sa.cap = cap;
    sa.prob = S.prob; sa.vmax = S.vmax; sa.kept_prop = S.kept_prop; sa.kept_box = S.kept_box; sa.cls_count = S.cls_count; sa.row_off = S.row_off;
    sa.al = S.al; sa.count = S.count; sa.total = S.total; sa.boxes = S.boxes; sa.scores = S.scores; sa.labels = S.labels;
    return sa;
}
RetinaArgs cald_host::retina_args(const RetinaTailBufs& S, const float* const* cls, const float* const* reg, const BatchPlan* plan, const ViewDesc* views,
                                  const float* base_anchors, int A, int K, int V, float score_thr, float nms_thr, int per_class, const DetBuffers& det) {
    RetinaArgs ra{};
    for (int i = 0; i < 5; i++) { ra.cls[i] = cls[i]; ra.reg[i] = reg[i]; ra.seg[i] = plan->seg[3 + i]; }
    ra.seg0 = plan->seg[0]; ra.views = views; ra.base_anchors = base_anchors;
    ra.cls_ld = A * K; ra.reg_ld = A * 4; ra.A = A; ra.K = K; ra.V = V; ra.score_thr = score_thr; ra.nms_thr = nms_thr; ra.min_box = 1e-2f;
    ra.per_class = per_class; ra.cand_cap = S.cand_cap;
    ra.cand_count = S.cand_count; ra.cand_key = S.cand_key; ra.cand_box = S.cand_box; ra.cand_skip = S.cand_skip;
    ra.kept_anchor = S.kept_anchor; ra.kept_box = S.kept_box; ra.kept_count = S.kept_count; ra.det = det;
    return ra;
}

RetinaSsmArgs cald_host::retina_ssm_args(const RetinaSsmBufs& S, const float* const* cls, const float* const* reg, const BatchPlan* plan, const ViewDesc* views,
                                         const float* base_anchors, int A, int K, int V, float score_thr, float nms_thr, int per_class) {
    RetinaTailBufs T; T.cand_cap = S.cand_cap; T.cand_count = S.cand_count; T.kept_anchor = S.kept_anchor; T.kept_box = S.kept_box; T.kept_count = S.kept_count;
    RetinaSsmArgs sa{};
    sa.r = retina_args(T, cls, reg, plan, views, base_anchors, A, K, V, score_thr, nms_thr, per_class, DetBuffers{});
    sa.conf_thr = SSM_CONF_THR; sa.nblk = S.nblk; sa.blk_off = S.blk_off; sa.list = S.list; sa.vmax = S.vmax; sa.al = S.al; sa.picks = S.picks; sa.n_picks = S.n_picks;
    sa.row_off = S.row_off; sa.count = S.count; sa.total = S.total; sa.boxes = S.boxes; sa.scores = S.scores; sa.labels = S.labels;
    return sa;
}
int cald_host::retina_ssm_pick_stop(cald_ctx* c, const RetinaSsmBufs& S, int V, int K, cald_ssm_pick_fn pick, void* user, int image0, int* h_counts) {
    const int T = CALD_SSM_RETINA_TAKE;
    std::vector<int> al((size_t)V), counts((size_t)V * K), picks((size_t)V * K * T, 0), np((size_t)V * K, 0);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(al.data(), S.al, (size_t)V * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(counts.data(), S.cand_count, (size_t)V * K * 4, hipMemcpyDeviceToHost));
    for (int v = 0; v < V; v++) {
        const int* cn = &counts[(size_t)v * K]; int* pk = &picks[(size_t)v * K * T]; int* n = &np[(size_t)v * K];
        for (int k = 0; k < K; k++)
            if (cn[k] < 0 || cn[k] > S.cand_cap) return fail(CALD_ERR_HIP, "retina ssm: image %d class %d has %d candidates (at most %d anchors)", image0 + v, k, cn[k], S.cand_cap);
        if (al[(size_t)v]) continue;
        const int rc = pick(user, image0 + v, K, cn, pk, n);
        if (rc) return fail(CALD_ERR_INVALID, "retina ssm: the pick callback returned %d for image %d", rc, image0 + v);
        for (int k = 0; k < K; k++) {
            if (n[k] < 0 || n[k] > cn[k] || n[k] > T)
                return fail(CALD_ERR_INVALID, "retina ssm: image %d class %d: %d picks of %d candidates (at most %d)", image0 + v, k, n[k], cn[k], T);
            for (int j = 0; j < n[k]; j++)
                if (pk[(size_t)k * T + j] < 0 || pk[(size_t)k * T + j] >= cn[k])
                    return fail(CALD_ERR_INVALID, "retina ssm: image %d class %d: pick %d is %d, outside 0..%d", image0 + v, k, j, pk[(size_t)k * T + j], cn[k] - 1);
        }
    }
    HIPCHK(hipMemcpy(S.picks, picks.data(), picks.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(S.n_picks, np.data(), np.size() * 4, hipMemcpyHostToDevice));
    if (h_counts) memcpy(h_counts, counts.data(), counts.size() * 4);
    return 0;
}

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
    a.total_mtiles = level_tiles(m->plan, lout, V); a.packed_rows = 0;
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
    a.in16 = nullptr; a.out16 = nullptr; a.ex16 = 0; a.in_scale = 0.0f; a.energy4 = nullptr; a.trace = nullptr;
    a.head_w = nullptr; a.head_out = nullptr; a.head_ld = 0; a.head_b[0] = a.head_b[1] = a.head_b[2] = 0.0f;
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
// Packed row tiles ("packed row tiles"): a dense launch -- host-planned rows, every pixel of the level -- offers conv_p4
// the level's row count; the tile count a launch is booked and classed with stays the per-view one.  Not offered: launches whose row
// counts live on the device (dyn_rows / row_map), the gathered launches of the cut_out reuse, the fused layer-1 pair.
bool cald_host::conv_pack_default() {
    static const bool on = !(getenv("CALD_CONV_PACK") && atoi(getenv("CALD_CONV_PACK")) == 0);
    return on;
}
static void offer_packing(cald_model* m, ConvArgs& a, int lin, int lout, int lup, int V) {
    if (!(m->row_packing < 0 ? conv_pack_default() : m->row_packing != 0) || a.dyn_rows || a.row_map || a.gather || a.mask) return;
    a.packed_rows = conv_pack_rows(m->plan.seg[lin], m->plan.seg[lout], a.up ? m->plan.seg[lup] : nullptr, V, a.Cin, a.out_ld);
}
static int conv_on(cald_model* m, const ConvLayer& L, const float* in, float* out, int lin, int lout, int V, bool relu,
                   const float* residual = nullptr, const float* up = nullptr, int lup = 0, const int* dyn = nullptr,
                   bool in_relu = false) {
    ConvArgs a;
    const double flops = fill_conv_args(m, a, L, in, out, lin, lout, V, relu, residual, up, lup, dyn, in_relu);
    if (flops < 0.0) return (int)flops;            // fill_conv_args failed: the (negative) status code
    offer_packing(m, a, lin, lout, lup, V);
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
        offer_packing(m, a[i], sp[i].level, sp[i].level, 0, V);
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

// the FPN output convs of the cut_out forward on their output dirty sets (gather sets 2 nblk + i of the plan), as ONE grouped launch: every
// problem carries its own GatherSet -- and P2 / P3 the pruning's extras, patched at the same pixels.  No launch where no view has a rectangle.
static int gconv_group_on(cald_model* m, const ConvSpec* sp, int n, int V, const FwdReuse& ru) {
    ConvArgs a[CALD_MAX_GROUP];
    double flops = 0.0; int tiles = 0;
    for (int i = 0; i < n; i++) {
        const double f = fill_conv_args(m, a[i], *sp[i].L, sp[i].in, sp[i].out, sp[i].level, sp[i].level, V, sp[i].relu);
        if (f < 0.0) return (int)f;
        const char* base = ru.d_gp + (size_t)(2 * ru.nblk + i) * cut_plan_set_bytes(V);
        a[i].seg_out = reinterpret_cast<const LevelSeg*>(base);
        a[i].gather = reinterpret_cast<const GatherSet*>(base + (size_t)(V + 1) * sizeof(LevelSeg));
        a[i].total_mtiles = ru.fpn_tiles[i];
        a[i].out16 = sp[i].out16; a[i].energy4 = sp[i].energy4;
        flops += 2.0 * ru.fpn_rows[i] * (double)sp[i].L->Cout * (double)(sp[i].L->KH * sp[i].L->KW * sp[i].L->CinTrue); tiles += ru.fpn_tiles[i];
    }
    if (!tiles) return 0;
    cald_ctx* c = m->ctx;
    ProfLaunch t; int rc;
    if ((rc = prof_begin(c, t))) return rc;
    const char* k = launch_conv_p4_group(a, n, c->stream);
    if ((rc = prof_end(c, t, flops, c->prof_tag_now, "mt=%d,Cin=%d,Cout=%d,k=%dx%d,s=%d,group=%d,gathered-rows", tiles, a[0].Cin, a[0].Cout, a[0].KH, a[0].KW, a[0].stride, n))) return rc;
    return k ? 0 : conv_refused(a[0]);
}

__global__ void accumulate_rows_kernel(const int* __restrict__ counts, int V, unsigned long long* acc) {
    unsigned long long s = 0;
    for (int v = threadIdx.x; v < V; v += 64) s += (unsigned long long)counts[v];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (threadIdx.x == 0) atomicAdd(acc, s);
}

static const float RPN_MIN_SIZE = 1e-3f;
// One forward as a run of named stages (run() chains them).  views: host descriptors with src/H/W/flip/rects filled; Hr/Wr/Ho/Wo are filled
// by prepare().  rq (host.h FwdRequest) names the tail: STOCK ends in the detections; FEATURES stops after the FPN and hands out the pyramid;
// SSM / RETINA_SSM run that tail in place of the stock one.  Pruning, cut_out reuse and the audit belong to the stock tail alone.
struct ForwardRun {
    cald_model* m; int V; ViewDesc* views; const FwdRequest& rq;
    // ---- filled by prepare() ----
    cald_ctx* c = nullptr; hipStream_t st = nullptr; const BatchPlan* dp = nullptr;
    const FwdReuse* ru = nullptr; float* audit_out = nullptr;      // the stock tail's (null for every other)
    bool retina = false, prune = false;
    bool is(FwdRequest::Tail t) const { return rq.tail == t; }
    int hp[CALD_MAX_VIEWS][2], max_pix0 = 0, max_pix2 = 0, max_pix6 = 0;
    BodyBufs Fb; PyramidBufs Fp; RetinaBufs Fr; RpnBufs Fn; PruneBufs Fq; BoxBufs Fx; AuditBufs Fa;
    // the scratch of the stages this forward will run, in their order
    void layout(Bump& B) {
        const BatchPlan& P = m->plan; long long px[8];
        for (int l = 0; l < 8; l++) px[l] = level_pix(P, l, V);
        m->split.clear();
        static const bool split_on = !(getenv("CALD_H3_S16") && atoi(getenv("CALD_H3_S16")) == 0);
        SplitReg S{m, B, m->cfg.precision == CALD_PRECISION_F16X3 && split_on};
        Fb.layout(B, S, px);
        Fp.layout(B, S, px, retina);
        if (is(FwdRequest::FEATURES)) return;
        if (retina) {
            int maxa = 0;
            for (int v = 0; v < V; v++) { int t = 0; for (int l = 3; l < 8; l++) t += P.seg[l][v].H * P.seg[l][v].W * 9; if (t > maxa) maxa = t; }
            Fr.layout(B, S, px, V, m->cls_out.Cout, m->cfg.num_classes, m->cfg.detections_per_img, maxa, is(FwdRequest::RETINA_SSM) ? &rq.rssm->out : nullptr);
            return;
        }
        Fn.layout(B, px, V, m->cfg.rpn_pre_nms_top_n);
        if (m->prune) Fq.layout(B, px, V, m->prune_capture);
        Fx.layout(B, S, V, m->pred.Cout, m->cfg.num_classes, m->key_cap);
        Fa.layout(B, V, m->det_cap());
        if (is(FwdRequest::SSM)) rq.ssm->out.layout(B, V, m->cfg.num_classes, m->cfg.detections_per_img);
    }
    // argument checks, the level plan, the arena, the staging-ring copy of plan and views
    int prepare() {
        c = m->ctx;
        if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized (call cald_model_finalize)");
        if (V < 1 || V > CALD_MAX_VIEWS) return fail(CALD_ERR_INVALID, "n_views must be 1..%d", CALD_MAX_VIEWS);
        switch (rq.tail) {      // what the tail needs of the model and of its own arguments
        case FwdRequest::STOCK:
            if (rq.stock.det.cap < m->det_cap()) return fail(CALD_ERR_INVALID, "detection capacity %d < required %d", rq.stock.det.cap, m->det_cap());
            ru = rq.stock.ru; audit_out = rq.stock.audit_out; prune = m->prune && rq.stock.prune_ok;
            break;
        case FwdRequest::FEATURES: break;
        case FwdRequest::SSM:
            if (m->cfg.arch != CALD_ARCH_FRCNN) return fail(CALD_ERR_INVALID, "the SSM forward is a plain Faster R-CNN forward");
            break;
        case FwdRequest::RETINA_SSM:
            if (!rq.rssm->pick || m->cfg.arch != CALD_ARCH_RETINANET || m->cfg.num_classes < 2)
                return fail(CALD_ERR_INVALID, "the RetinaNet SSM forward is a plain RetinaNet forward with a pick callback and at least two classes");
        }
        HIPCHK(hipSetDevice(c->device));
        for (int v = 0; v < V; v++) {
            ViewDesc& d = views[v];
            if (!d.src || d.H <= 0 || d.W <= 0 || d.nrect < 0 || d.nrect > CALD_MAX_CUT) return fail(CALD_ERR_INVALID, "view %d is malformed", v);
            int Hp, Wp;
            transform_size(d.H, d.W, m->cfg.min_size, m->cfg.max_size, &d.Hr, &d.Wr, &Hp, &Wp);
            d.Ho = d.H; d.Wo = d.W;
            if (is(FwdRequest::FEATURES) && rq.feat->pad_to) {      // the loader batch's common size (torchvision's ImageList): Hr / Wr stay the view's own, the rest is zero
                const int Hq = rq.feat->pad_to[v][0], Wq = rq.feat->pad_to[v][1];
                if (Hq % 32 || Wq % 32 || Hq < Hp || Wq < Wp)
                    return fail(CALD_ERR_INVALID, "view %d: pad_to %d x %d must be a multiple of 32 and at least the view's own %d x %d", v, Hq, Wq, Hp, Wp);
                Hp = Hq; Wp = Wq;
            }
            hp[v][0] = Hp; hp[v][1] = Wp;
            if (Hp * Wp > max_pix0) max_pix0 = Hp * Wp;
        }
        retina = m->cfg.arch == CALD_ARCH_RETINANET;
        if (audit_out && m->box_min_size > 0.0f) return fail(CALD_ERR_UNSUPPORTED, "the decision-margin audit does not cover small-box removal (box_min_size > 0)");
        if (audit_out && retina && m->cfg.detections_per_img > AUDIT_MAX_DET)
            return fail(CALD_ERR_UNSUPPORTED, "the decision-margin audit holds a class's detections in LDS: RetinaNet with detections_per_img <= %d (AUDIT_MAX_DET)", AUDIT_MAX_DET);
        if (audit_out && !retina && (m->cfg.rpn_pre_nms_top_n > 1024 || m->det_cap() > AUDIT_MAX_DET))
            return fail(CALD_ERR_UNSUPPORTED, "the decision-margin audit covers Faster R-CNN with rpn_pre_nms_top_n <= 1024 and <= %d detections per image", AUDIT_MAX_DET);
        build_plan(m->plan, V, views, hp, retina);
        m->last_V = V; m->last_views.assign(views, views + V);
        for (int v = 0; v < V; v++) {
            int p2 = m->plan.seg[2][v].H * m->plan.seg[2][v].W; if (p2 > max_pix2) max_pix2 = p2;
            int p6 = m->plan.seg[6][v].H * m->plan.seg[6][v].W; if (p6 > max_pix6) max_pix6 = p6;
        }
        { Bump dry(nullptr, true); layout(dry); int rc = arena_reserve(c, dry.off); if (rc) return rc; }
        { Bump real(c->arena, false); layout(real); }
        const int si = c->stage_i; c->stage_i = (si + 1) % cald_ctx::NSTAGE;
        HIPCHK(hipEventSynchronize(c->stage_ev[si]));
        memcpy(c->h_stage[si], &m->plan, sizeof(BatchPlan));
        memcpy(c->h_stage[si] + sizeof(BatchPlan), views, sizeof(ViewDesc) * V);
        HIPCHK(hipMemcpyAsync(c->d_plan, c->h_stage[si], sizeof(BatchPlan), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d_views, c->h_stage[si] + sizeof(BatchPlan), sizeof(ViewDesc) * V, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->stage_ev[si], c->stream));
        dp = c->d_plan; st = c->stream;
        m->dbg.clear();
        return 0;
    }
    int dense_block(const Bottleneck& B, const float* cur, float* dst, int lvl, int lout) {
        int rc; const float* idn = cur;
        if (B.has_down) { if ((rc = conv_on(m, B.down, cur, Fb.D, lvl, lout, V, false))) return rc; idn = Fb.D; }
        if ((rc = conv_on(m, B.c1, cur, Fb.T1, lvl, lvl, V, true))) return rc;
        return conv_pair_on(m, B.c2, B.c3, Fb.T1, Fb.T2, dst, lvl, lout, V, idn);
    }
    // cut_out reuse, the dirty pixels only: T1 on what conv2's windows read, the rest on the dirty set of the output, written over the retained tensor
    int gathered_block(const Bottleneck& B, int b, const float* cur, float* dst, int lvl, int lout) {
        int rc; const float* idn = cur;
        if (B.has_down) { if ((rc = gconv_on(m, B.down, cur, Fb.D, lvl, lout, V, false, nullptr, *ru, b, 0))) return rc; idn = Fb.D; }
        if ((rc = gconv_on(m, B.c1, cur, Fb.T1, lvl, lvl, V, true, nullptr, *ru, b, 1))) return rc;
        if ((rc = gconv_on(m, B.c2, Fb.T1, Fb.T2, lvl, lout, V, true, nullptr, *ru, b, 0))) return rc;
        return gconv_on(m, B.c3, Fb.T2, dst, lout, lout, V, true, idn, *ru, b, 0);
    }
    // transform + ResNet body (rows A14, A15)
    int body() {
        int rc;
        launch_preprocess(c->d_views, dp->seg[0], Fb.in0, V, max_pix0, st);
        m->dbg["input"] = {Fb.in0, 0, 4, 0};
        if ((rc = conv_on(m, m->conv1, Fb.in0, Fb.c1, 0, 1, V, true))) return rc;
        m->dbg["conv1"] = {Fb.c1, 1, 64, 0};
        launch_maxpool(Fb.c1, Fb.p1, dp->seg[1], dp->seg[2], 64, V, max_pix2, st, m->split.count(Fb.p1) != 0);
        m->dbg["pool1"] = {Fb.p1, 2, 64, 0};
        const float* cur = Fb.p1; int lvl = 2, layer = 0, xi = 0;
        for (size_t b = 0; b < m->blocks.size(); b++) {
            const Bottleneck& B = m->blocks[b];
            const int lout = lvl + (B.c2.stride == 2 ? 1 : 0);
            const bool kept = ru && (int)b < ru->nblk;          // cut_out reuse: this block's output is the retained tensor
            float* dst = kept ? ru->out[b] : (B.layer_end ? Fb.Cf[layer] : Fb.X[xi]);
            if ((rc = kept && ru->mode == 2 && ru->gather[layer] ? gathered_block(B, (int)b, cur, dst, lvl, lout) : dense_block(B, cur, dst, lvl, lout))) return rc;
            if (B.layer_end) Fb.Cf[layer] = dst;
            cur = dst; lvl = lout;
            if (B.layer_end) layer++; else xi ^= 1;
        }
        const char* cn[4] = {"C2", "C3", "C4", "C5"};
        for (int i = 0; i < 4; i++) m->dbg[cn[i]] = {Fb.Cf[i], 2 + i, CCH[i], 0};
        return 0;
    }
    void name_pyramid(int first, int n) { for (int i = 0; i < n; i++) m->dbg["P" + std::to_string(first + i)] = {Fp.Pf[i], first + i, 256, 0}; }
    // FPN (row A16) on C2..C5, or on C3..C5 + LastLevelP6P7 (retinanet_cal.py:618-619; a features-only forward runs p7 only where the caller pools it)
    int fpn() {
        const int first = retina ? 3 : 2, nl = retina ? 3 : 4, c0 = 4 - nl;      // RetinaNet: Cf[1..3] = C3..C5 -> P3..P5; Faster R-CNN: Cf[0..3] = C2..C5 -> P2..P5
        int rc; ConvSpec sp[4];
        // cut_out reuse: P2..P5 (and the pruning's extras of P2 / P3) are the retained tensors -- the reference forward writes them, the cut_out
        // forward patches them below; the RPN, the look-ahead, RoIAlign, p6_subsample and the debug views read them through Fp / Fq
        const bool kept = ru && ru->fpn && !retina;
        if (kept) {
            for (int i = 0; i < 4; i++) Fp.Pf[i] = ru->pf[i];
            if (prune) for (int i = 0; i < 2; i++) { Fq.p16[i] = ru->p16[i]; Fq.energy[i] = ru->energy[i]; }
        }
        if ((rc = conv_on(m, m->fpn_inner[nl - 1], Fb.Cf[3], Fp.inner[nl - 1], 5, 5, V, false))) return rc;
        for (int i = nl - 2; i >= 0; i--)
            if ((rc = conv_on(m, m->fpn_inner[i], Fb.Cf[c0 + i], Fp.inner[i], first + i, first + i, V, false, nullptr, Fp.inner[i + 1], first + 1 + i))) return rc;
        for (int i = 0; i < nl; i++) m->dbg["inner" + std::to_string(first + i)] = {Fp.inner[i], first + i, 256, 0};
        for (int i = 0; i < nl; i++) sp[i] = {&m->fpn_layer[i], Fp.inner[i], Fp.Pf[i], first + i, false};
        if (prune)                // (Faster R-CNN only) the pruning's per-pixel energy and the look-ahead's split-fp16 operand come out of these convs' epilogues (conv_p4.hip)
            for (int i = 0; i < 2; i++) { sp[i].out16 = Fq.p16[i]; sp[i].energy4 = Fq.energy[i]; }
        if ((rc = kept && ru->mode == 2 && ru->gather_fpn ? gconv_group_on(m, sp, nl, V, *ru) : conv_group_on(m, sp, nl, V))) return rc;
        if (!retina) return 0;
        if ((rc = conv_on(m, m->p6, Fp.Pf[2], Fp.Pf[3], 5, 6, V, false))) return rc;
        if (is(FwdRequest::FEATURES) && !rq.feat->p7) return 0;
        return conv_on(m, m->p7, Fp.Pf[3], Fp.Pf[4], 6, 7, V, false, nullptr, nullptr, 0, nullptr, true);
    }
    // the features-only forward's result: `n` pyramid tensors from plan level `first` (neither LastLevelMaxPool nor a head runs)
    void hand_out(int first, int n) {
        name_pyramid(first, n);
        for (int i = 0; i < n; i++) {
            auto sp = m->split.find(Fp.Pf[i]);
            rq.feat->P[i] = Fp.Pf[i]; rq.feat->split_only[i] = sp != m->split.end() && sp->second.fp32_dead; rq.feat->plan_level[i] = first + i;
        }
    }
    // heads (retinanet_cal.py:36-241): 4 x (3x3 conv + ReLU) + 3x3 output conv, per level; then the tail
    int retina_head_and_tail() {
        int rc;
        // both towers x five levels share one launch per tower depth (10 independent problems, weights shared across levels)
        for (int t = 0; t < 4; t++) {
            ConvSpec sp[10];
            for (int hsel = 0; hsel < 2; hsel++)
                for (int i = 0; i < 5; i++)
                    sp[hsel * 5 + i] = {&(hsel == 0 ? m->cls_tower : m->reg_tower)[t], t == 0 ? Fp.Pf[i] : Fr.ret_t[hsel][(t - 1) & 1][i],
                                        Fr.ret_t[hsel][t & 1][i], 3 + i, true};
            if ((rc = conv_group_on(m, sp, 10, V))) return rc;
        }
        for (int hsel = 0; hsel < 2; hsel++) {
            ConvSpec sp[5];
            for (int i = 0; i < 5; i++) sp[i] = {hsel == 0 ? &m->cls_out : &m->reg_out, Fr.ret_t[hsel][1][i], hsel == 0 ? Fr.cls_h[i] : Fr.reg_h[i], 3 + i, false};
            if ((rc = conv_group_on(m, sp, 5, V))) return rc;
        }
        for (int i = 0; i < 5; i++) {
            m->dbg["cls" + std::to_string(i)] = {Fr.cls_h[i], 3 + i, m->cls_out.Cout, 0};
            m->dbg["reg" + std::to_string(i)] = {Fr.reg_h[i], 3 + i, 36, 0};
        }
        if (is(FwdRequest::RETINA_SSM)) return retina_ssm_tail();
        const RetinaArgs ra = retina_args(Fr.tail, Fr.cls_h, Fr.reg_h, dp, c->d_views, m->d_anchors, 9, m->cfg.num_classes, V, m->cfg.box_score_thresh,
                                          m->cfg.box_nms_thresh, m->cfg.detections_per_img, rq.stock.det);
        launch_retina_postprocess(ra, Fr.tail.max_anchors, st);
        if (audit_out) launch_audit_retina(ra, audit_out, st);
        return 0;
    }
    // the SSM tail (retina_ssm.hip) on the same head tensors: phase A, the host stop for the picks, phase B
    int retina_ssm_tail() {
        const RetinaSsmArgs sa = retina_ssm_args(rq.rssm->out, Fr.cls_h, Fr.reg_h, dp, c->d_views, m->d_anchors, 9, m->cfg.num_classes, V, m->cfg.box_score_thresh,
                                                 m->cfg.box_nms_thresh, m->cfg.detections_per_img);
        launch_retina_ssm_phase_a(sa, st);
        HIPCHK(hipGetLastError());
        if (int rc = retina_ssm_pick_stop(c, rq.rssm->out, V, m->cfg.num_classes, rq.rssm->pick, rq.rssm->user, rq.rssm->image0, nullptr)) return rc;
        launch_retina_ssm_phase_b(sa, st);
        return 0;
    }
    // LastLevelMaxPool: max_pool2d(P5, 1, 2) = every other pixel of every other row; in F16X3 the copy runs on P5's split twin
    void p6_subsample() {
        auto tw = m->split.find(Fp.Pf[3]);
        const bool p6_split = m->split.count(Fp.Pf[4]) != 0 && tw != m->split.end();
        launch_subsample2(p6_split ? reinterpret_cast<const float*>(tw->second.s16) : Fp.Pf[3], Fp.Pf[4], dp->seg[5], dp->seg[6], 256, V, max_pix6, st);
        name_pyramid(2, 5);
    }
    void name_rpn(int first) { for (int i = first; i < 5; i++) m->dbg["rpn" + std::to_string(i)] = {Fn.rpn_h[i], 2 + i, 15, 0}; }
    // RPN (row A17): the shared-weight head over the five levels, one launch for the 3x3 conv, one for the fused 1x1 heads
    int rpn_dense() {
        int rc; ConvSpec sp[5];
        for (int i = 0; i < 5; i++) sp[i] = {&m->rpn_conv, Fp.Pf[i], Fn.rpn_tl[i], 2 + i, true};
        if ((rc = conv_group_on(m, sp, 5, V))) return rc;
        for (int i = 0; i < 5; i++) sp[i] = {&m->rpn_head, Fn.rpn_tl[i], Fn.rpn_h[i], 2 + i, false};
        if ((rc = conv_group_on(m, sp, 5, V))) return rc;
        name_rpn(0);
        return 0;
    }
    // the look-ahead of P2 / P3 as ONE conv_h4 launch with the 1 x 1 head's objectness logits in its epilogue (ConvArgs::head_out); *fused stays
    // false, and nothing was launched, where conv_h4 does not take the launch.  Booked with the FLOPs it executes: the 3 x 3 conv + 3 head channels
    int look_fused_on(const ConvSpec* sp, bool* fused) {
        ConvArgs a[2]; double flops = 0.0; int tiles = 0;
        for (int i = 0; i < 2; i++) {
            const double f = fill_conv_args(m, a[i], *sp[i].L, sp[i].in, nullptr, sp[i].level, sp[i].level, V, sp[i].relu);
            if (f < 0.0) return (int)f;
            a[i].in16 = sp[i].in16;
            a[i].head_w = m->look_head_w; a[i].head_out = Fn.rpn_h[i]; a[i].head_ld = 15;
            for (int q = 0; q < 3; q++) a[i].head_b[q] = m->look_head_b[q];
            flops += f + 2.0 * (double)level_pix(m->plan, sp[i].level, V) * 256.0 * 3.0; tiles += a[i].total_mtiles;
        }
        if (!m->look_head_w || !conv_h4_group_takes(a, 2, m->look_fuse == 2)) return 0;       // nothing prepared, nothing launched: the two launches follow
        if (m->prune_capture)       // the debug view "rpn_look0/1" shows zeros in the channels the fused look-ahead does not evaluate
            for (int i = 0; i < 2; i++) HIPCHK(hipMemsetAsync(Fn.rpn_h[i], 0, (size_t)level_pix(m->plan, 2 + i, V) * 15 * sizeof(float), st));
        ProfLaunch t; int rc;
        if ((rc = prof_begin(c, t))) return rc;
        const char* k = launch_conv_h4_group(a, 2, st, m->look_fuse == 2);
        *fused = true;
        if (!k) { prof_end(c, t, 0.0, c->prof_tag_now, "refused"); return conv_refused(a[0]); }
        return prof_end(c, t, flops, c->prof_tag_now, "mt=%d,Cin=%d,Cout=%d,k=%dx%d,s=%d,group=2,head=3", tiles, a[0].Cin, a[0].Cout, a[0].KH, a[0].KW, a[0].stride);
    }
    // certified pruning (rpn_prune.hip): P2 / P3 first on the fp16 matrix pipe, then exactly at the pixels that can hold one of the
    // level's pre_nms_top_n anchors; P4..P6 dense as ever.  Same bits at every anchor the top-k can select.
    int rpn_pruned() {
        int rc; ConvSpec sp[5];
        RpnPruneArgs pr;
        for (int i = 0; i < 2; i++) {
            pr.seg[i] = dp->seg[2 + i]; pr.energy[i] = Fq.energy[i]; pr.pnorm[i] = Fq.pn[i]; pr.head[i] = Fn.rpn_h[i]; pr.head_out[i] = Fn.rpn_h[i];
            for (int s2 = 0; s2 < 2; s2++) { pr.head_rows[s2][i] = Fq.rows[s2][i]; pr.row_map[s2][i] = Fq.map[s2][i]; }
        }
        int log_slot[2];
        for (int s2 = 0; s2 < 2; s2++) {
            log_slot[s2] = (c->prof && c->prune_log_n < CALD_PRUNE_LOG) ? c->prune_log_n++ : -1;
            pr.nsel[s2] = Fq.nsel[s2]; pr.log[s2] = log_slot[s2] >= 0 ? c->d_prune_log + (size_t)log_slot[s2] * 4 : nullptr;
        }
        pr.tau_key = Fq.tau; pr.stat = c->prof ? c->d_prune_stat : nullptr; pr.check = c->d_prune_check;
        for (int q = 0; q < 3; q++) { pr.c1[q] = m->prune_c1[q]; pr.c0[q] = m->prune_c0[q]; }
        pr.head_ld = 15; pr.pre_n = m->cfg.rpn_pre_nms_top_n; pr.V = V;
        c->prof_tag_now = 1;
        for (int i = 0; i < 2; i++) { sp[i] = {&m->rpn_conv16, Fp.Pf[i], Fn.rpn_tl[i], 2 + i, true}; sp[i].in16 = Fq.p16[i]; }
        // one launch where conv_h4 takes it (cald_model_set_look_fuse): the objectness logits come out of its epilogue; else the hidden tensor
        // is written and the exact 1 x 1 head reads it, as on small inputs (conv_h3)
        bool fused = false;
        rc = m->look_fuse ? look_fused_on(sp, &fused) : 0;
        if (!rc && !fused) {
            rc = conv_group_on(m, sp, 2, V);
            for (int i = 0; i < 2; i++) sp[i] = {&m->rpn_head, Fn.rpn_tl[i], Fn.rpn_h[i], 2 + i, false};
            if (!rc) rc = conv_group_on(m, sp, 2, V);
        }
        c->prof_tag_now = 0;
        if (rc) return rc;
        // FLOPs the gathered launches are booked with when they cover every pixel (each stage's launches are: cald_profile_read / _dump rescale them)
        const double cap_conv[2] = {2.0 * (double)level_pix(m->plan, 2, V) * 2304.0 * 256.0, 2.0 * (double)level_pix(m->plan, 3, V) * 2304.0 * 256.0};
        const double cap_head[2] = {2.0 * (double)level_pix(m->plan, 2, V) * 256.0 * 15.0, 2.0 * (double)level_pix(m->plan, 3, V) * 256.0 * 15.0};
        if (m->prune_capture)
            for (int i = 0; i < 2; i++) {
                HIPCHK(hipMemcpyAsync(Fq.look[i], Fn.rpn_h[i], (size_t)level_pix(m->plan, 2 + i, V) * 15 * sizeof(float), hipMemcpyDeviceToDevice, st));
                const char* ln[2] = {"rpn_look0", "rpn_look1"}; const char* bn[2] = {"rpn_pnorm0", "rpn_pnorm1"};
                m->dbg[ln[i]] = {Fq.look[i], 2 + i, 15, 0}; m->dbg[bn[i]] = {Fq.pn[i], 2 + i, 1, 0};
            }
        // stage 0 recomputes P2 / P3 rows only; stage 1's launches also carry the dense levels P4..P6
        for (int s2 = 0; s2 < 2; s2++) {
            const int np = s2 == 1 ? 5 : 2;
            launch_rpn_prune_select(pr, max_pix2, s2, st);
            for (int i = 0; i < np; i++) sp[i] = {&m->rpn_conv, Fp.Pf[i], Fn.rpn_tl[i], 2 + i, true};
            for (int i = 0; i < 2; i++) { sp[i].dyn = Fq.nsel[s2] + i * V; sp[i].row_map = Fq.map[s2][i]; }      // gathered rows, compact output
            if ((rc = conv_group_on(m, sp, np, V))) return rc;
            if (c->prof) {
                for (int i = 0; i < 2; i++) c->prof_prune_flops_cap[i] += cap_conv[i];
                if (log_slot[s2] >= 0) c->prof_gather[c->prof_launches.size() - 1] = {log_slot[s2], {cap_conv[0], cap_conv[1]}};
            }
            for (int i = 0; i < np; i++) sp[i] = {&m->rpn_head, Fn.rpn_tl[i], i < 2 ? Fq.rows[s2][i] : Fn.rpn_h[i], 2 + i, false};
            for (int i = 0; i < 2; i++) sp[i].dyn = Fq.nsel[s2] + i * V;
            if ((rc = conv_group_on(m, sp, np, V))) return rc;
            if (c->prof) {
                for (int i = 0; i < 2; i++) c->prof_prune_flops_cap[i] += cap_head[i];
                if (log_slot[s2] >= 0) c->prof_gather[c->prof_launches.size() - 1] = {log_slot[s2], {cap_head[0], cap_head[1]}};
            }
        }
        launch_rpn_prune_scatter(pr, max_pix2, st);
        name_rpn(m->prune_capture ? 0 : 2);      // (P2 / P3 head maps are exact only where selected, -FLT_MAX elsewhere: a debug view in capture mode only)
        return 0;
    }
    void proposals() {
        RpnArgs ra;
        for (int i = 0; i < 5; i++) { ra.head[i] = Fn.rpn_h[i]; ra.seg[i] = dp->seg[2 + i]; }
        ra.seg0 = dp->seg[0]; ra.views = c->d_views; ra.base_anchors = m->d_anchors;
        ra.head_ld = 15; ra.A = 3; ra.V = V; ra.pre_n = m->cfg.rpn_pre_nms_top_n; ra.post_n = m->cfg.rpn_post_nms_top_n;
        ra.nms_thr = m->cfg.rpn_nms_thresh; ra.min_size = RPN_MIN_SIZE;
        ra.cand_key = Fn.cand_key; ra.cand_box = Fn.cand_box; ra.sorted_box = Fn.sorted_box; ra.sorted_raw = Fn.sorted_raw;
        ra.sorted_count = Fn.sorted_count; ra.proposals = Fn.prop.proposals; ra.prop_stride = CALD_ROI_CAP; ra.prop_count = Fn.prop.prop_count;
        ra.next_key = audit_out ? Fa.next_key : nullptr; ra.trunc_key = audit_out ? Fa.trunc_key : nullptr;
        launch_rpn(ra, st);
        m->dbg["proposals"] = {Fn.prop.proposals, 7, 4, 1};
    }
    // box head (rows A18, A19, A20)
    int box_head() {
        int rc;
        launch_roi_align(roi_args(Fx.roi, Fp.Pf, dp, 256, V, Fn.prop, m->split.count(Fx.roi.roi) != 0), st);
        m->dbg["roi"] = {Fx.roi.roi, 7, 12544, 1};
        const double fl_before_roi = c->prof_flops;
        // The RoI buffers are dense [V][1000][C]; as per-view problems every view pads its 1 000 rows to eight 128-row tiles (2.4 % idle
        // rows in fc6).  Rows of a GEMM are independent, so the three layers run as ONE problem of V * 1000 rows (level 8: 500 tiles for
        // 64 views, a tile may straddle two views; segments of 32 views keep byte offsets inside 31 bits).  Rows beyond a view's proposal count hold stale finite-or-not data and are never
        // read downstream (post-processing walks r < count); the profile counts FLOPs on the measured rows as before.
        const int Vr = (V + ROI_DENSE_VIEWS - 1) / ROI_DENSE_VIEWS;
        if ((rc = conv_on(m, m->fc6, Fx.roi.roi, Fx.f6, 8, 8, Vr, true))) return rc;
        if ((rc = conv_on(m, m->fc7, Fx.f6, Fx.f7, 8, 8, Vr, true))) return rc;
        if ((rc = conv_on(m, m->pred, Fx.f7, Fx.pr, 8, 8, Vr, false))) return rc;
        if (c->prof) {
            hipLaunchKernelGGL(accumulate_rows_kernel, dim3(1), dim3(64), 0, st, Fn.prop.prop_count, V, c->d_roi_rows);
            c->prof_roi_rows_cap += (double)V * CALD_ROI_CAP; c->prof_roi_flops_cap += c->prof_flops - fl_before_roi; c->prof_roi_views += V;
        }
        m->dbg["fc6"] = {Fx.f6, 7, 1024, 1}; m->dbg["fc7"] = {Fx.f7, 7, 1024, 1}; m->dbg["pred"] = {Fx.pr, 7, m->pred.Cout, 1};
        return 0;
    }
    void postprocess() {
        PostArgs pa = post_args(Fx.post, Fx.pr, m->pred.Cout, m->cfg.num_classes, V, Fn.prop, c->d_views, m->cfg.box_score_thresh, m->cfg.box_nms_thresh, rq.stock.det);
        pa.kept_key = audit_out ? Fa.kept_key : nullptr; pa.post_maxc = audit_out ? Fa.post_maxc : nullptr;
        pa.min_box = m->box_min_size;
        launch_frcnn_postprocess(pa, st);
    }
    // the SSM tail (ssm.hip) on the same predictor rows and proposals
    void ssm_postprocess() {
        launch_ssm_postprocess(ssm_args(rq.ssm->out, Fx.pr, m->pred.Cout, m->cfg.num_classes, V, Fn.prop, c->d_views, m->cfg.box_score_thresh,
                                        m->cfg.detections_per_img), st);
    }
    void audit() {
        AuditArgs au;
        au.cand_key = Fn.cand_key; au.cand_box = Fn.cand_box; au.sorted_box = Fn.sorted_box; au.flags = reinterpret_cast<const unsigned char*>(Fn.sorted_raw);
        au.next_key = Fa.next_key; au.trunc_key = Fa.trunc_key; au.pre_n = m->cfg.rpn_pre_nms_top_n; au.post_n = m->cfg.rpn_post_nms_top_n;
        au.rpn_nms_thr = m->cfg.rpn_nms_thresh; au.min_size = RPN_MIN_SIZE;
        au.proposals = Fn.prop.proposals; au.prop_count = Fn.prop.prop_count;
        for (int i = 0; i < 4; i++) au.seg[i] = dp->seg[2 + i];
        au.prob = Fx.post.prob; au.pred = Fx.pr; au.pred_ld = m->pred.Cout; au.C = m->cfg.num_classes; au.views = c->d_views;
        au.keys = Fx.post.keys; au.key_count = Fx.post.key_count; au.key_cap = m->key_cap; au.kept_key = Fa.kept_key; au.post_maxc = Fa.post_maxc;
        au.det_count = rq.stock.det.count; au.cap = rq.stock.det.cap; au.score_thr = m->cfg.box_score_thresh; au.post_nms_thr = m->cfg.box_nms_thresh;
        au.V = V; au.delta = 1e-2f; au.out = audit_out;
        launch_audit(au, st);
    }
    int run() {
        int rc;
        if ((rc = prepare()) || (rc = body()) || (rc = fpn())) return rc;
        if (is(FwdRequest::FEATURES)) hand_out(retina ? 3 : 2, retina && rq.feat->p7 ? 5 : 4);
        else if (retina) { name_pyramid(3, 5); if ((rc = retina_head_and_tail())) return rc; }
        else {
            p6_subsample();
            if ((rc = prune ? rpn_pruned() : rpn_dense())) return rc;
            proposals();
            if ((rc = box_head())) return rc;
            if (is(FwdRequest::SSM)) ssm_postprocess(); else postprocess();
            if (audit_out) audit();
        }
        HIPCHK(hipGetLastError());
        return 0;
    }
};

int cald_host::forward_model(cald_model* m, int V, ViewDesc* views, const FwdRequest& rq) { return ForwardRun{m, V, views, rq}.run(); }

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
    if (int rc = dets_from_abi(out, m->cfg.num_classes, &det)) return rc;
    return forward_model(m, n_views, vd.data(), FwdRequest::detect(det, m->prune_capture));
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
