// cutout_reuse.hip -- the cut_out reuse planner (host.h CutPlanner) and its test hook cald_debug_cutout_forward.  A reference forward keeps the
// block outputs of its first three stages (on Faster R-CNN also the FPN output convs' results) in a retention slot; the cut_out forward of the
// same images recomputes over them only the pixels its rectangles reach (host_logic.h cut_geometry, conv_p4.hip's gathered rows).  The planner
// lays out the slot, builds the gather plan and gates each stage between gathered and dense launches; forward.hip runs the FwdReuse it fills.
#include "host.h"

#define CUT_GATHER_MAX_COST 0.7    // a stage runs gathered while its tiles cost at most this fraction of the dense stage
// The FPN output convs are one more gated stage under the same rule.  A value of its own is not needed: on the bench pool the grouped
// gathered launch runs at 141.5 TF/s on the rows it computes against the dense group's 144.9 (profiles/cutout_fpn_launches_new.csv), 0.98 of
// it, so it pays up to about 0.97 of the dense tiles, and every cut_out forward of that pool is far below either value (tile fraction
// 0.64).  (The parent's table could not price it: its gathered 3 x 3 256 -> 256 launches, layer3's, are 280 - 540 tiles, under one round of
// the 768 workgroup slots, so their TF/s shows the round's quantisation and not the gathered rows' cost.)
#define CUT_FPN_MAX_COST CUT_GATHER_MAX_COST

static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// On by default in the exact sweeps; CALD_CUTOUT_REUSE=0 turns it off for the process (A/B, escape hatch), cald_model_set_cutout_reuse for a
// model.  Exact fp32 only (conv_p4.hip's gathered rows), and a backbone whose first three stages fit the block table
void CutPlanner::enable(bool has_cutout, bool audit) {
    static const bool env_on = !(getenv("CALD_CUTOUT_REUSE") && atoi(getenv("CALD_CUTOUT_REUSE")) == 0);
    on = (m->cr.mode < 0 ? env_on : m->cr.mode != 0) && has_cutout && !audit && m->cfg.precision == CALD_PRECISION_FP32 && nblk < CUT_MAX_BLOCKS;
}

// the blocks the cut_out reuse retains and gathers (the first three stages), and the whole backbone for its geometry
CutPlanner::CutPlanner(cald_model* m_, bool prune_ok_) : m(m_), prune_ok(prune_ok_) {
    retina = m->cfg.arch == CALD_ARCH_RETINANET;
    for (int b = 0, layer = 0, l = 2; b < (int)m->blocks.size() && layer < 3 && nblk < CUT_MAX_BLOCKS; b++) {
        const Bottleneck& Bk = m->blocks[b];
        blk_stride[nblk] = Bk.c2.stride; blk_lin[nblk] = l; l += Bk.c2.stride == 2 ? 1 : 0; blk_lout[nblk] = l; blk_stage[nblk] = layer;
        nblk++;
        if (Bk.layer_end) layer++;
    }
    {
        int layer = 0; bool fits = true;
        for (size_t b = 0; b < m->blocks.size(); b++) {
            if (ngeo == CUT_MAX_BLOCKS || layer > 3) { fits = false; break; }
            geo_stride[ngeo] = m->blocks[b].c2.stride;
            if (m->blocks[b].layer_end) c_blk[layer++] = ngeo;
            ngeo++;
        }
        fpn_ok = fits && layer == 4 && !retina && ngeo >= nblk;
        if (!fpn_ok) { ngeo = nblk; for (int b = 0; b < nblk; b++) geo_stride[b] = blk_stride[b]; }
    }
}

void CutPlanner::plan_of(int nv, const ViewDesc* vs) {
    int hp[CALD_MAX_VIEWS][2];
    for (int v = 0; v < nv; v++) { int Hr, Wr; transform_size(vs[v].H, vs[v].W, m->cfg.min_size, m->cfg.max_size, &Hr, &Wr, &hp[v][0], &hp[v][1]); }
    build_plan(rplan, nv, vs, hp, retina);
}
// The slot's size, and `ru` (may be null) over it at `base`: the retained block outputs of rplan, back to back.  fpn, the extended slot: then
// P2..P5 of the FPN output convs and, where this run prunes, the split copy and the energy of P2 / P3 (forward.hip PruneBufs) -- a slot laid
// out this way serves the three-stage retention unchanged
size_t CutPlanner::retain_layout(int nv, bool fpn, char* base, FwdReuse* ru) const {
    const BatchPlan& P = rplan;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += al(bytes); return p; };
    for (int b = 0; b < nblk; b++) { char* p = take((size_t)level_pix(P, blk_lout[b], nv) * (size_t)m->blocks[b].c3.Cout * 4); if (ru) ru->out[b] = reinterpret_cast<float*>(p); }
    if (!fpn) return off;
    for (int i = 0; i < 4; i++) { char* p = take((size_t)level_pix(P, 2 + i, nv) * 256 * 4); if (ru) ru->pf[i] = reinterpret_cast<float*>(p); }
    if (m->prune && prune_ok)
        for (int i = 0; i < 2; i++) {
            char* p = take((size_t)level_pix(P, 2 + i, nv) * 256 * 4); char* e = take((size_t)level_pix(P, 2 + i, nv) * 4 * 4);
            if (ru) { ru->p16[i] = reinterpret_cast<unsigned*>(p); ru->energy[i] = reinterpret_cast<float*>(e); }
        }
    if (ru) ru->fpn = true;
    return off;
}

int CutPlanner::retain(int q, int nb, const ViewDesc* views, FwdReuse& ru) {
    if (!on) return CUT_KEPT_NONE;
    cald_ctx* c = m->ctx;
    plan_of(nb, views);
    cald_model::CutReuse& R = m->cr;
    // graded: the extended slot (+ the FPN outputs); where that is refused -- by the allocator, once and for the model's life, or by the
    // test hook's cap -- the three stages only; where that fails too, nothing (the batch's cut_out views run dense)
    const size_t need3 = retain_layout(nb, false, nullptr, nullptr), needx = fpn_ok ? retain_layout(nb, true, nullptr, nullptr) : 0;
    bool ext = fpn_ok && !R.ext_refused && !(R.ext_cap && needx > R.ext_cap);
    for (int attempt = 0; attempt < 2; attempt++) {
        const size_t need = ext ? needx : need3;
        if (need <= R.cap[q]) break;
        // grown on demand; the slot's last reader (the cut_out forward two batches back) is in the stream ahead
        HIPCHK(hipStreamSynchronize(c->stream));
        if (R.slot[q]) hipFree(R.slot[q]);
        R.slot[q] = nullptr; R.cap[q] = 0;
        if (hipMalloc((void**)&R.slot[q], need + (need >> 3)) == hipSuccess) { R.cap[q] = need + (need >> 3); break; }
        (void)hipGetLastError(); R.slot[q] = nullptr;
        if (!ext) break;
        ext = false; R.ext_refused = true;
    }
    int kept = CUT_KEPT_NONE;
    if (R.slot[q]) {
        ru.mode = 1; ru.nblk = nblk; kept = ext ? CUT_KEPT_FPN : CUT_KEPT_STAGES;
        retain_layout(nb, ext, R.slot[q], &ru);
    } else c->cut_fallbacks++;       // no room on a shared GPU: this batch's cut_out views run dense
    c->cut_kept[kept]++;
    return kept;
}

int CutPlanner::cut_plan(int parity, bool fpn, int V, const ViewDesc* vs, FwdReuse& ru) {
    cald_ctx* c = m->ctx;
    cald_model::CutReuse& R = m->cr;
    const size_t per = cut_plan_set_bytes(V), total = per * (2 * (size_t)nblk + (fpn ? 4 : 0));
    if (!R.d_gp) {
        const size_t cap = cut_plan_set_bytes(CALD_MAX_VIEWS) * (2 * CUT_MAX_BLOCKS + 4);
        HIPCHK(hipMalloc((void**)&R.d_gp, cap));
        HIPCHK(hipHostMalloc((void**)&R.h_gp[0], cap)); HIPCHK(hipHostMalloc((void**)&R.h_gp[1], cap));
    }
    plan_of(V, vs);
    const BatchPlan& P = rplan;
    char* const h = R.h_gp[parity];
    std::vector<CutSet> g_out((size_t)V * ngeo), g_t1((size_t)V * ngeo), g_fpn((size_t)V * 4);
    for (int v = 0; v < V; v++) {
        int Hr, Wr, Hp, Wp; CutSet pool1;
        transform_size(vs[v].H, vs[v].W, m->cfg.min_size, m->cfg.max_size, &Hr, &Wr, &Hp, &Wp);
        cut_geometry(vs[v].H, vs[v].W, Hr, Wr, Hp, Wp, vs[v].nrect, vs[v].rects, ngeo, geo_stride, &pool1, &g_out[(size_t)v * ngeo], &g_t1[(size_t)v * ngeo]);
        if (fpn) {
            CutSet cs[4], inner[4];
            for (int i = 0; i < 4; i++) cs[i] = g_out[(size_t)v * ngeo + c_blk[i]];
            cut_fpn_geometry(Hp, Wp, cs, inner, &g_fpn[(size_t)v * 4]);
        }
    }
    // one gather set of the plan: per view the level's geometry with tile_start counting the set's tiles, then the set as disjoint rectangles
    auto put_set = [&](size_t index, int lvl, const CutSet* sets, size_t stride_v, int* tiles_out, double* rows_out) {
        LevelSeg* sg = reinterpret_cast<LevelSeg*>(h + index * per);
        GatherSet* gs = reinterpret_cast<GatherSet*>(reinterpret_cast<char*>(sg) + (size_t)(V + 1) * sizeof(LevelSeg));
        int tiles = 0; double rows = 0.0;
        for (int v = 0; v < V; v++) {
            LevelSeg L = P.seg[lvl][v]; L.tile_start = tiles; sg[v] = L;
            CutRect rr[CALD_GATHER_RECTS];
            int n = cut_disjoint(sets[(size_t)v * stride_v], rr, CALD_GATHER_RECTS);
            if (n < 0) { n = 1; rr[0] = {0, 0, L.W - 1, L.H - 1}; }       // too fragmented: the whole view
            GatherSet& G = gs[v]; memset(&G, 0, sizeof(G));
            G.nr = n;
            for (int q = 0; q < n; q++) {
                G.x0[q] = rr[q].x0; G.y0[q] = rr[q].y0; G.w[q] = rr[q].x1 - rr[q].x0 + 1;
                G.cum[q + 1] = G.cum[q] + G.w[q] * (rr[q].y1 - rr[q].y0 + 1);
            }
            tiles += (G.cum[n] + 127) / 128; rows += (double)G.cum[n];
        }
        sg[V] = P.seg[lvl][V]; sg[V].tile_start = tiles;
        *tiles_out = tiles; *rows_out = rows;
    };
    auto kf = [](const ConvLayer& L) { return (double)L.Cout * (double)(L.KH * L.KW * L.CinTrue); };
    double cost_g[3] = {0, 0, 0}, cost_d[3] = {0, 0, 0}, rows_g[3] = {0, 0, 0}, rows_d[3] = {0, 0, 0}, tiles_g[3] = {0, 0, 0}, tiles_d[3] = {0, 0, 0};
    for (int b = 0; b < nblk; b++)
        for (int kind = 0; kind < 2; kind++) {
            const int lvl = kind ? blk_lin[b] : blk_lout[b];
            int tiles; double rows;
            put_set((size_t)(2 * b + kind), lvl, (kind ? g_t1.data() : g_out.data()) + b, (size_t)ngeo, &tiles, &rows);
            ru.tiles[b][kind] = tiles; ru.rows[b][kind] = rows;
            const Bottleneck& Bk = m->blocks[b];
            const double w = kind ? kf(Bk.c1) : kf(Bk.c2) + kf(Bk.c3) + (Bk.has_down ? kf(Bk.down) : 0.0);
            const double nconv = kind ? 1.0 : (Bk.has_down ? 3.0 : 2.0), dense = (double)level_pix(P, lvl, V);
            const int st = blk_stage[b];
            cost_g[st] += 128.0 * tiles * w; cost_d[st] += dense * w;
            rows_g[st] += rows * nconv; rows_d[st] += dense * nconv;
            tiles_g[st] += tiles * nconv; tiles_d[st] += (double)P.seg[lvl][V].tile_start * nconv;
        }
    // a stage runs gathered while its tiles cost at most CUT_GATHER_MAX_COST of the dense stage (the rest pays the halo, the per-view
    // tile tails and the unfused layer-1 pair); otherwise dense, over the retained tensors all the same
    for (int st = 0; st < 3; st++) {
        ru.gather[st] = m->cr.mode != 2 && cost_g[st] <= CUT_GATHER_MAX_COST * cost_d[st];
        c->cut_rows[st] += ru.gather[st] ? rows_g[st] : rows_d[st]; c->cut_dense[st] += rows_d[st];
        c->cut_st_rows[st] += ru.gather[st] ? rows_g[st] : rows_d[st]; c->cut_st_dense[st] += rows_d[st];
        c->cut_st_tiles[st] += ru.gather[st] ? tiles_g[st] : tiles_d[st]; c->cut_st_dense_tiles[st] += tiles_d[st];
    }
    // layer4 and the laterals run dense (their rows are booked as such); the FPN output convs are one more gated stage, all four levels
    // in one grouped gathered launch -- every level has the same weight per row, so its cost is its tiles
    {
        double r4 = 0.0, t4 = 0.0, rl = 0.0, tl = 0.0;
        int lvl = 2;
        for (size_t b = 0; b < m->blocks.size(); b++) {
            const Bottleneck& Bk = m->blocks[b];
            const int lo = lvl + (Bk.c2.stride == 2 ? 1 : 0);
            if ((int)b >= nblk) {
                const double n_in = 1.0, n_out = Bk.has_down ? 3.0 : 2.0;
                r4 += n_in * (double)level_pix(P, lvl, V) + n_out * (double)level_pix(P, lo, V);
                t4 += n_in * (double)P.seg[lvl][V].tile_start + n_out * (double)P.seg[lo][V].tile_start;
            }
            lvl = lo;
        }
        if (!retina) for (int i = 0; i < 4; i++) { rl += (double)level_pix(P, 2 + i, V); tl += (double)P.seg[2 + i][V].tile_start; }
        c->cut_st_rows[3] += r4; c->cut_st_dense[3] += r4; c->cut_st_tiles[3] += t4; c->cut_st_dense_tiles[3] += t4;
        c->cut_st_rows[CUT_STAGE_LATERAL] += rl; c->cut_st_dense[CUT_STAGE_LATERAL] += rl;
        c->cut_st_tiles[CUT_STAGE_LATERAL] += tl; c->cut_st_dense_tiles[CUT_STAGE_LATERAL] += tl;
        double fg = 0.0, fd = 0.0, frg = 0.0, frd = 0.0;
        if (fpn)
            for (int i = 0; i < 4; i++) {
                put_set(2 * (size_t)nblk + i, 2 + i, g_fpn.data() + i, 4, &ru.fpn_tiles[i], &ru.fpn_rows[i]);
                fg += ru.fpn_tiles[i]; frg += ru.fpn_rows[i];
            }
        if (!retina) for (int i = 0; i < 4; i++) { fd += (double)P.seg[2 + i][V].tile_start; frd += (double)level_pix(P, 2 + i, V); }
        ru.gather_fpn = fpn && m->cr.mode != 2 && 128.0 * fg <= CUT_FPN_MAX_COST * frd;
        c->cut_st_rows[CUT_STAGE_OUTPUT] += ru.gather_fpn ? frg : frd; c->cut_st_dense[CUT_STAGE_OUTPUT] += frd;
        c->cut_st_tiles[CUT_STAGE_OUTPUT] += ru.gather_fpn ? fg : fd; c->cut_st_dense_tiles[CUT_STAGE_OUTPUT] += fd;
    }
    if (hipMemcpyAsync(R.d_gp, h, total, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(CALD_ERR_HIP, "H2D of the cut_out gather plan failed");
    ru.mode = 2; ru.nblk = nblk; ru.d_gp = R.d_gp;
    retain_layout(V, fpn, R.slot[parity], &ru);
    c->cut_batches++;
    return 0;
}

// Test hook: the cut_out forward of a sweep batch on its own.  The views without their rectangles run as the reference forward (retaining
// what the model's reuse mode retains), then the views as given run as the cut_out forward over it -- mode 0: a plain dense forward -- and
// leave their detections in `out` and their tensors to cald_debug_tensor.  prune != 0: both forwards take the certified pruning's path.
extern "C" int cald_debug_cutout_forward(cald_model* m, int n_views, const cald_view* views, const cald_dets* out, int prune) {
    if (!m || !views || !out || n_views < 1 || n_views > CALD_MAX_VIEWS) return fail(CALD_ERR_INVALID, "bad argument");
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
    std::vector<ViewDesc> cut(n_views), ref(n_views);
    for (int i = 0; i < n_views; i++) {
        const cald_view& v = views[i];
        if (v.nrect < 0 || v.nrect > CALD_MAX_CUT || v.flip || v.noise_dev) return fail(CALD_ERR_INVALID, "view %d is no cut_out view", i);
        cut[i] = plain_view(v.image_dev, v.H, v.W); ref[i] = cut[i];
        cut[i].nrect = v.nrect;
        for (int q = 0; q < 4 * v.nrect; q++) cut[i].rects[q] = v.rects[q];
    }
    DetBuffers det;
    if (int rc = dets_from_abi(out, m->cfg.num_classes, &det)) return rc;
    cald_ctx* c = m->ctx;
    HIPCHK(hipSetDevice(c->device));
    CutPlanner planner(m, prune != 0);
    planner.enable(true, false);
    if (m->prune && prune) HIPCHK(hipMemsetAsync(c->d_prune_check, 0, 8, c->stream));
    FwdReuse ru_ref, ru_cut;
    const int kept = planner.retain(0, n_views, ref.data(), ru_ref);
    if (kept < 0) return kept;
    const bool reuse = kept != CUT_KEPT_NONE;
    int rc = forward_model(m, n_views, ref.data(), FwdRequest::detect(det, prune != 0, reuse ? &ru_ref : nullptr));
    if (!rc && reuse) rc = planner.cut_plan(0, kept == CUT_KEPT_FPN, n_views, cut.data(), ru_cut);
    if (!rc) rc = forward_model(m, n_views, cut.data(), FwdRequest::detect(det, prune != 0, reuse ? &ru_cut : nullptr));
    if (!rc) HIPCHK(hipStreamSynchronize(c->stream));
    return rc;
}
