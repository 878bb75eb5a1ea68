// sweep.hip -- the sweeps of the C ABI on the detector forward: cald_sweep / cald_sweep_audit as a pipeline of named stages (SweepRun; what its
// forwards retain and gather is cutout_reuse.hip's), the baselines cald_sweep_ltc / _lsc, the SSM sweeps cald_sweep_ssm / _ssm_retina.  Host-side
// restatements used here (host_logic.h): Python `random` (MT19937) + cutout rectangle selection (cald/cald_helper.py:88-132), np.linspace
// sub-sampling (cald_train.py:110-113), the float64 means of cald_train.py:225-228.
#include "host.h"

// helper: device detection buffers
void cald_host::free_det(DetBuffers& d) {
    hipFree(d.boxes); hipFree(d.scores); hipFree(d.labels); hipFree(d.props); hipFree(d.prob_max); hipFree(d.scores_cls); hipFree(d.count);
    memset(&d, 0, sizeof(d));
}
// all-or-nothing: on any failed hipMalloc everything already allocated is released and `d` is left zeroed
int cald_host::alloc_det(DetBuffers& d, int V, int cap, int C) {
    memset(&d, 0, sizeof(d));
    d.cap = cap; d.C = C;
    hipError_t e = hipMalloc((void**)&d.boxes, (size_t)V * cap * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&d.scores, (size_t)V * cap * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d.labels, (size_t)V * cap * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&d.props, (size_t)V * cap * 16);
    if (e == hipSuccess) e = hipMalloc((void**)&d.prob_max, (size_t)V * cap * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d.scores_cls, (size_t)V * cap * C * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d.count, (size_t)V * 4);
    if (e != hipSuccess) {
        free_det(d);
        return fail(CALD_ERR_HIP, "hipMalloc of detection buffers (%d views x %d rows x %d classes) failed: %s", V, cap, C, hipGetErrorString(e));
    }
    return 0;
}
// one of the model's batch-level detection-buffer sets (`views`: how many views it holds) holds at least VT views; after a failed growth
// the model owns none
static int ensure_det(cald_model* m, DetBuffers& set, int& views, int VT) {
    if (views >= VT) return 0;
    if (views) {
        HIPCHK(hipStreamSynchronize(m->ctx->stream));
        free_det(set);
        views = 0;
    }
    int rc = alloc_det(set, VT, m->det_cap(), m->cfg.num_classes);
    if (rc) return rc;
    views = VT;
    return 0;
}
// the buffers of D from view `o` on
static DetBuffers det_at(const DetBuffers& D, size_t o) {
    DetBuffers d2 = D;
    const int cap = D.cap, C = D.C;
    d2.boxes += o * cap * 4; d2.scores += o * cap; d2.labels += o * cap; d2.props += o * cap * 4;
    d2.prob_max += o * cap; d2.scores_cls += o * cap * C; d2.count += o;
    return d2;
}
// views per augmented forward: 96 fills whole rounds of the 768 workgroup slots in the mid-size layers and fc6 (CALD_FWD_VIEWS overrides)
static int sweep_fwd_views() {
    static const int env = getenv("CALD_FWD_VIEWS") ? atoi(getenv("CALD_FWD_VIEWS")) : 96;
    return env < 1 ? 1 : (env > CALD_MAX_VIEWS ? CALD_MAX_VIEWS : env);
}
// n augmented views run in forwards of <= sweep_fwd_views() views, evenly sized (159 views run as 80 + 79, not 96 + 63: a short last forward
// leaves most of its launches under-filled; results do not depend on the split).  96 views per forward: the mid-size layers and fc6 then
// fill whole rounds of the 768 workgroup slots (measured +1.0 % on the sweep).  Forward f of the fwd_count(n) takes views [a0, a0 + nv).
static int fwd_count(int n) { return (n + sweep_fwd_views() - 1) / sweep_fwd_views(); }
static void fwd_span(int n, int f, int* a0, int* nv) {
    const int n_fw = fwd_count(n);
    *a0 = (int)(((long long)n * f) / n_fw); *nv = (int)(((long long)n * (f + 1)) / n_fw) - *a0;
}

namespace {
// =============================================================================================
// the sweep (get_uncertainty, cald_train.py:91-231)
// =============================================================================================
// Host state of one batch from its reference forward to its float64 means.  Two live at a time: while the host builds the augmented
// views of batch k (cutout needs the reference boxes on the host) the GPU already runs the reference forward of batch k + 1, and the
// scores of batch k come back while batch k + 1 is being built -- the stream never waits for the host (round 3 stopped twice per batch).
struct SweepBatch {
    int i0 = 0, nb = 0, P = 0, VV = 0; bool live = false;
    int* h_count; float* h_boxes; int* h_ints; float* h_par; NoiseJob* h_jobs; float* h_cons; float* h_clsc; float* h_vm; float* h_pm;   // pinned
    std::vector<int> ref_n, pair_img, view_img, pair_aug, view_aug;   // pair_img: the pair's image slot = the view index of its reference view
    std::vector<char> view_inert;     // cut_out reuse: a stand-in view of an image without detections (its results are not used)
    std::vector<float> cut_margin;
    int kept = CUT_KEPT_NONE;         // what the reference forward retained in slot k & 1 (CutPlanner::retain)
    // what build_aug_views hands to enqueue_aug_forwards and enqueue_scoring
    std::vector<int> ref_sel, pair_kind, view_isref;
    std::vector<float> pair_par;
    std::vector<ViewDesc> aviews;
};

// One pass of cald_sweep[_audit] over the images.  force_dense: the RPN head runs dense even where the model prunes it (the repeat after a
// pruning tripwire fired)
struct SweepRun {
    cald_model* m; int n_images; const uint8_t* const* images_dev; const int* H; const int* W; const int64_t* pool_pos;
    const cald_sweep_cfg* cfg; double* consistency_out; double* cls_corr_out; float* margins_out; bool force_dense;
    // ---- filled by setup() ----
    cald_ctx* c = nullptr;
    bool audit = false, prune_ok = false;
    int C = 0, cap = 0, A = 0, B = 0, VT = 0, NB = 0, P_MAX = 0, cut_a = -1;
    PairLayout lay{0, 0, 0}; size_t n_ints = 0;
    DetBuffers* DS[2] = {nullptr, nullptr};
    int* d_ints = nullptr; float *d_par = nullptr, *d_cons = nullptr, *d_clsc = nullptr; NoiseJob* d_jobs = nullptr; unsigned long long* d_lsum = nullptr;
    float *d_vm[2] = {nullptr, nullptr}, *d_pm = nullptr;     // decision-margin audit: per-view records of the two detection-buffer sets, per-pair records
    SweepBatch bt[2];
    CutPlanner planner;      // cut_out reuse

    static size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

    // argument checks, detection buffers, the model-owned scratch and how this run carves it
    int setup() {
        if (!m || !images_dev || !H || !W || !pool_pos || !cfg || !consistency_out || !cls_corr_out) return fail(CALD_ERR_INVALID, "null argument");
        audit = margins_out != nullptr;
        prune_ok = !audit && !force_dense;      // the audit wants every anchor's own logit: dense RPN head
        if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
        c = m->ctx;
        HIPCHK(hipSetDevice(c->device));
        C = m->cfg.num_classes; cap = m->det_cap();
        A = cfg->n_augs;
        if (A < 0 || A > CALD_MAX_AUGS) return fail(CALD_ERR_INVALID, "n_augs %d outside [0, %d]", A, CALD_MAX_AUGS);
        int n_noise = 0; bool any_gauss = false;
        for (int a = 0; a < A; a++) {
            const int k = cfg->augs[a].kind;
            if (k < CALD_AUG_FLIP || k > CALD_AUG_ROTATE) return fail(CALD_ERR_INVALID, "augmentation %d: unknown kind %d", a, k);
            if (k == CALD_AUG_CUTOUT && (cfg->augs[a].param < 1.0 || cfg->augs[a].param > (double)CALD_MAX_CUT))
                return fail(CALD_ERR_INVALID, "cutout: cut_num must be in [1, %d]", CALD_MAX_CUT);
            if (k == CALD_AUG_RESIZE && !(cfg->augs[a].param > 0.0)) return fail(CALD_ERR_INVALID, "resize: ratio must be positive");
            n_noise += (k == CALD_AUG_GAUSS || k == CALD_AUG_SALT_PEPPER);
            any_gauss |= k == CALD_AUG_GAUSS;
        }
        if (n_noise > CALD_MAX_NOISE_SEG) return fail(CALD_ERR_INVALID, "at most %d GaussianNoise / SaltPepperNoise views per image", CALD_MAX_NOISE_SEG);
        if (any_gauss)
            for (int i = 0; i < n_images; i++)
                if (randn_unsupported(H[i], W[i]))
                    return fail(CALD_ERR_UNSUPPORTED, "GaussianNoise on image %d (%dx%d): torch.randn of fewer than 16 elements takes torch's scalar path, which is not implemented", i, H[i], W[i]);
        B = sweep_batch(cfg->batch_images, 64);
        VT = B * (1 + A);
        NB = (n_images + B - 1) / B;
        // the second set of detection buffers exists only when two batches are really in flight (a one-batch shard would pay VT x cap x C
        // floats of HBM for nothing)
        const bool two_sets = NB > 1;
        { int rc0 = ensure_det(m, m->sweep_det, m->sweep_det_views, VT); if (rc0) return rc0; }
        if (two_sets) { int rc0 = ensure_det(m, m->sweep_det2, m->sweep_det2_views, VT); if (rc0) return rc0; }
        DS[0] = &m->sweep_det; DS[1] = two_sets ? &m->sweep_det2 : &m->sweep_det;
        P_MAX = B * (A > 0 ? A : 1);
        lay = PairLayout{P_MAX, B, VT}; n_ints = lay.n_ints();
        // ---- persistent scratch (model-owned): device buffers of the scoring stage, pinned host staging in two sets (batch parity) ----
        cald_model::SweepScratch& S = m->ss;
        const size_t dev_need = al(n_ints * 4) + al((size_t)P_MAX * 12 * 4) + al((size_t)P_MAX * 4) + al((size_t)VT * (C - 1) * 4) + al(sizeof(NoiseJob) * B) +
                                al(sizeof(unsigned long long) * P_MAX) + 2 * al((size_t)VT * CALD_VM * 4) + al((size_t)P_MAX * 2 * 4);
        const size_t pin_set = al((size_t)VT * 4) + al((size_t)B * cap * 16) + al(n_ints * 4) + al((size_t)P_MAX * 12 * 4) + al(sizeof(NoiseJob) * B) +
                               al((size_t)P_MAX * 4) + al((size_t)VT * (C - 1) * 4) + al((size_t)VT * CALD_VM * 4) + al((size_t)P_MAX * 2 * 4);
        if (dev_need > S.dev_bytes || 2 * pin_set > S.pin_bytes) {
            HIPCHK(hipStreamSynchronize(c->stream));
            if (S.dev) { hipFree(S.dev); S.dev = nullptr; S.dev_bytes = 0; }
            if (S.pin) { hipHostFree(S.pin); S.pin = nullptr; S.pin_bytes = 0; }
            HIPCHK(hipMalloc((void**)&S.dev, dev_need)); S.dev_bytes = dev_need;
            HIPCHK(hipHostMalloc((void**)&S.pin, 2 * pin_set)); S.pin_bytes = 2 * pin_set;
        }
        for (int i = 0; i < 2; i++) {
            if (!S.ev_ref[i]) HIPCHK(hipEventCreateWithFlags(&S.ev_ref[i], hipEventDisableTiming));
            if (!S.ev_score[i]) HIPCHK(hipEventCreateWithFlags(&S.ev_score[i], hipEventDisableTiming));
        }
        { Bump b(S.dev, false); d_ints = b.get<int>(n_ints); d_par = b.get<float>((size_t)P_MAX * 12); d_cons = b.get<float>(P_MAX);
          d_clsc = b.get<float>((size_t)VT * (C - 1)); d_jobs = b.get<NoiseJob>(B); d_lsum = b.get<unsigned long long>(P_MAX);
          d_vm[0] = b.get<float>((size_t)VT * CALD_VM); d_vm[1] = b.get<float>((size_t)VT * CALD_VM); d_pm = b.get<float>((size_t)P_MAX * 2); }
        for (int q = 0; q < 2; q++) {
            Bump b(S.pin + (size_t)q * pin_set, false);
            bt[q].h_count = b.get<int>(VT); bt[q].h_boxes = b.get<float>((size_t)B * cap * 4); bt[q].h_ints = b.get<int>(n_ints);
            bt[q].h_par = b.get<float>((size_t)P_MAX * 12); bt[q].h_jobs = b.get<NoiseJob>(B); bt[q].h_cons = b.get<float>(P_MAX);
            bt[q].h_clsc = b.get<float>((size_t)VT * (C - 1));
            bt[q].h_vm = b.get<float>((size_t)VT * CALD_VM); bt[q].h_pm = b.get<float>((size_t)P_MAX * 2);
        }
        if (m->prune && prune_ok) HIPCHK(hipMemsetAsync(c->d_prune_check, 0, 8, c->stream));
        // ---- cut_out reuse (exact fp32, conv_p4.hip's gathered rows): the reference forward keeps the block outputs of the first three stages,
        // and the batch's first cut_out augmentation recomputes only its dirty pixels over them ----
        for (int a = 0; a < A && cut_a < 0; a++) if (cfg->augs[a].kind == CALD_AUG_CUTOUT) cut_a = a;
        planner = CutPlanner(m, prune_ok);
        planner.enable(cut_a >= 0, audit);
        return 0;
    }
    // reference views of batch k -> detections into set k & 1, counts + boxes to the pinned host set, event
    int enqueue_ref(int k) {
        SweepBatch& b = bt[k & 1];
        b.i0 = k * B; b.nb = (n_images - b.i0 < B) ? n_images - b.i0 : B; b.live = true; b.P = 0; b.VV = b.nb;
        std::vector<ViewDesc> views = ref_views(images_dev, H, W, b.i0, b.nb);
        const DetBuffers& D = *DS[k & 1];
        FwdReuse ru;
        const int kept = planner.retain(k & 1, b.nb, views.data(), ru);
        if (kept < 0) return kept;
        b.kept = kept;
        const FwdRequest rq = FwdRequest::detect(D, prune_ok, kept != CUT_KEPT_NONE ? &ru : nullptr).audited(audit ? d_vm[k & 1] : nullptr);
        if (int r = forward_model(m, b.nb, views.data(), rq)) return r;
        if (hipMemcpyAsync(b.h_count, D.count, (size_t)b.nb * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(b.h_boxes, D.boxes, (size_t)b.nb * cap * 16, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(m->ss.ev_ref[k & 1], c->stream) != hipSuccess) return fail(CALD_ERR_HIP, "D2H of reference detections failed");
        return 0;
    }
    // augmented views of batch k, built on the host in the reference's order (cald_train.py:124-183; needs the batch's reference detections
    // on the host), with the augmentation launches they need
    int build_aug_views(int k) {
        SweepBatch& b = bt[k & 1];
        cald_model::SweepScratch& S = m->ss;
        const int nb = b.nb, i0 = b.i0;
        if (hipEventSynchronize(S.ev_ref[k & 1]) != hipSuccess) return fail(CALD_ERR_HIP, "reference forward failed: %s", hipGetErrorString(hipGetLastError()));
        const int* h_count = b.h_count; const float* h_boxes = b.h_boxes;
        b.ref_sel.assign((size_t)B * 50, 0); b.pair_aug.clear(); b.pair_kind.clear(); b.view_isref.assign(VT, 0);
        b.ref_n.assign(B, 0); b.pair_img.clear(); b.view_img.assign(VT, 0); b.cut_margin.assign(B, INFINITY);
        b.view_aug.assign(VT, 0); b.view_inert.assign(VT, 0);
        b.pair_par.clear(); b.aviews.clear();
        int njobs = 0;
        size_t need = 0;
        for (int i = 0; i < nb; i++) {
            if (h_count[i] == 0) continue;
            const int Hi = H[i0 + i], Wi = W[i0 + i];
            for (int a = 0; a < A; a++) {
                const int kd = cfg->augs[a].kind; const double prm = cfg->augs[a].param;
                if (kd == CALD_AUG_SALT_PEPPER) need += al((size_t)Hi * Wi * 3);
                else if (kd == CALD_AUG_GAUSS) need += al((size_t)Hi * Wi * 3 * sizeof(float));
                else if (kd == CALD_AUG_COLOR_ADJUST) need += 2 * al((size_t)Hi * Wi * 3);
                else if (kd == CALD_AUG_RESIZE) {
                    const int ow = (int)((double)Wi * prm), oh = (int)((double)Hi * prm);
                    if (ow < 1 || oh < 1) return fail(CALD_ERR_INVALID, "resize ratio %g empties a %dx%d image", prm, Hi, Wi);
                    need += al((size_t)oh * ow * 3) + al((size_t)Hi * ow * 3);
                } else if (kd == CALD_AUG_ROTATE) {
                    int fx[6], nh, nw; pil_rotate_setup(Hi, Wi, prm, fx, &nh, &nw);
                    need += al((size_t)nh * nw * 3) + al((size_t)nh * Wi * 3) + al((size_t)Hi * Wi * 3);
                }
            }
        }
        if (need > S.aug_cap) {      // the arena of augmented images is reused batch after batch in stream order; growing it drains the stream
            HIPCHK(hipStreamSynchronize(c->stream));
            if (S.d_aug) hipFree(S.d_aug);
            S.d_aug = nullptr; S.aug_cap = 0;
            if (hipMalloc((void**)&S.d_aug, need + (need >> 2)) != hipSuccess) return fail(CALD_ERR_HIP, "hipMalloc of the augmentation arena failed");
            S.aug_cap = need + (need >> 2);
        }
        size_t aug_off = 0;
        auto take = [&](size_t bytes) { uint8_t* p = S.d_aug + aug_off; aug_off += al(bytes); return p; };
        int r = 0;
        for (int i = 0; i < nb; i++) {
            b.view_img[i] = i; b.view_isref[i] = 1;
            const int n = h_count[i];
            b.ref_n[i] = subsample_indices(n, &b.ref_sel[(size_t)i * 50]);
            if (n == 0) continue;
            const int Hi = H[i0 + i], Wi = W[i0 + i];
            const uint64_t seed = (uint64_t)cfg->base_seed * 1000003ull + (uint64_t)pool_pos[i0 + i];
            float sub[50 * 4];
            for (int q = 0; q < b.ref_n[i]; q++) memcpy(sub + 4 * q, &h_boxes[((size_t)i * cap + b.ref_sel[(size_t)i * 50 + q]) * 4], 16);
            int cur_a = 0;
            auto add_view = [&](const ViewDesc& vd, int kind, const float* par) {
                const int vidx = nb + (int)b.aviews.size();
                b.aviews.push_back(vd); b.view_img[vidx] = i; b.view_isref[vidx] = 0; b.view_aug[vidx] = cur_a;
                b.pair_img.push_back(i); b.pair_aug.push_back(vidx); b.pair_kind.push_back(kind);
                for (int q = 0; q < 12; q++) b.pair_par.push_back(par ? par[q] : 0.0f);
            };
            const ViewDesc base = plain_view(images_dev[i0 + i], Hi, Wi);
            PyRandom pyrng; pyrng.seed(seed);          // ColorSwap's randint and every cutout of this image, in call order
            NoiseJob nj; memset(&nj, 0, sizeof(nj)); nj.seed = seed; nj.src = images_dev[i0 + i]; nj.H = Hi; nj.W = Wi;
            for (int a = 0; a < A && !r; a++) {
                const int kd = cfg->augs[a].kind; const double prm = cfg->augs[a].param;
                float par[12] = {0};
                cur_a = a;
                if (kd == CALD_AUG_FLIP) { ViewDesc v = base; v.flip = 1; pair_params(1, Hi, Wi, prm, par); add_view(v, 1, par); }
                else if (kd == CALD_AUG_GAUSS) {            // image + torch.randn(size) * std / 255.0
                    NoiseSeg& sg = nj.seg[nj.nseg++]; sg.kind = 0; sg.p0 = (float)prm; sg.p1 = 0.0f;
                    sg.dst = take((size_t)Hi * Wi * 3 * sizeof(float));
                    ViewDesc v = base; v.noise = reinterpret_cast<const float*>(sg.dst); add_view(v, 0, nullptr);
                } else if (kd == CALD_AUG_SALT_PEPPER) {    // noise = torch.rand(size); < prob/2 -> max, > 1 - prob/2 -> min
                    NoiseSeg& sg = nj.seg[nj.nseg++]; sg.kind = 1; sg.p0 = (float)(prm / 2.0); sg.p1 = (float)(1.0 - prm / 2.0);
                    sg.dst = take((size_t)Hi * Wi * 3);
                    ViewDesc v = base; v.src = reinterpret_cast<const uint8_t*>(sg.dst); add_view(v, 0, nullptr);
                } else if (kd == CALD_AUG_COLOR_ADJUST) {
                    uint8_t* tmp = take((size_t)Hi * Wi * 3); uint8_t* dst = take((size_t)Hi * Wi * 3);
                    launch_color_adjust(images_dev[i0 + i], Hi, Wi, (float)prm, tmp, d_lsum + b.pair_img.size(), dst, c->stream);
                    ViewDesc v = base; v.src = dst; add_view(v, 0, nullptr);
                } else if (kd == CALD_AUG_COLOR_SWAP) {
                    ViewDesc v = base; v.swap = pyrng.randbelow(6); add_view(v, 0, nullptr);
                } else if (kd == CALD_AUG_CUTOUT) {
                    ViewDesc v = base;
                    float cm = INFINITY;
                    v.nrect = cutout_rects(pyrng, Hi, Wi, b.ref_n[i], sub, (int)prm, v.rects, &cm);
                    if (cm < b.cut_margin[i]) b.cut_margin[i] = cm;
                    add_view(v, 0, nullptr);
                } else if (kd == CALD_AUG_RESIZE) {
                    const int ow = (int)((double)Wi * prm), oh = (int)((double)Hi * prm);
                    uint8_t* dst = take((size_t)oh * ow * 3); uint8_t* tmp = take((size_t)Hi * ow * 3);
                    if ((r = pil_resize(c, images_dev[i0 + i], Hi, Wi, dst, oh, ow, tmp, 0))) break;
                    pair_params(2, Hi, Wi, prm, par); add_view(plain_view(dst, oh, ow), 2, par);
                } else if (kd == CALD_AUG_ROTATE) {
                    int fx[6], nh, nw; pil_rotate_setup(Hi, Wi, prm, fx, &nh, &nw);
                    uint8_t* rot = take((size_t)nh * nw * 3); uint8_t* tmp = take((size_t)nh * Wi * 3); uint8_t* dst = take((size_t)Hi * Wi * 3);
                    launch_affine_nearest(images_dev[i0 + i], Hi, Wi, rot, nh, nw, fx, c->stream);
                    if ((r = pil_resize(c, rot, nh, nw, dst, Hi, Wi, tmp, 1))) break;      // new_image.resize((w, h)): BICUBIC default
                    ViewDesc v = base; v.src = dst;
                    pair_params(3, Hi, Wi, prm, par);
                    add_view(v, 3, par);
                }
            }
            if (r) return r;
            if (nj.nseg) b.h_jobs[njobs++] = nj;
        }
        if (njobs) {
            if (hipMemcpyAsync(d_jobs, b.h_jobs, sizeof(NoiseJob) * njobs, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(CALD_ERR_HIP, "H2D of noise jobs failed");
            launch_noise_stream(d_jobs, njobs, c->stream);
        }
        return 0;
    }

    // forwards of batch k's augmented views: with the cut_out reuse its cut_out views first, as one forward in the reference forward's
    // image order; the others in evenly sized forwards (fwd_span)
    int enqueue_aug_forwards(int k) {
        SweepBatch& b = bt[k & 1];
        const DetBuffers& D = *DS[k & 1];
        const int nb = b.nb, na = (int)b.aviews.size();
        int r, n_rest = na, rest_slot = nb;
        ViewDesc* rest_views = b.aviews.data();
        std::vector<ViewDesc> rest;
        int n_cut = 0;
        for (int j = 0; j < na; j++) n_cut += b.view_aug[nb + j] == cut_a;
        b.VV = nb + na;
        if (b.kept != CUT_KEPT_NONE && n_cut > 0 && 2 * nb + (na - n_cut) <= VT) {
            // cut_out reuse: image i's cut_out view takes slot nb + i (a stand-in copy of the reference view, no rectangle, for an image
            // without detections: same plan as the reference forward), the other augmented views slots 2 nb + ... in their order
            std::vector<ViewDesc> cutv(nb);
            std::vector<int> slot(na), nimg(VT, 0), naug(VT, 0);
            std::vector<char> has(nb, 0), ninert(VT, 0);
            for (int i = 0; i < nb; i++) nimg[i] = i;
            int nr2 = 0;
            for (int j = 0; j < na; j++) {
                const int img = b.view_img[nb + j];
                if (b.view_aug[nb + j] == cut_a) { slot[j] = nb + img; cutv[img] = b.aviews[j]; has[img] = 1; }
                else { slot[j] = 2 * nb + nr2++; rest.push_back(b.aviews[j]); }
                nimg[slot[j]] = img; naug[slot[j]] = b.view_aug[nb + j];
            }
            for (int i = 0; i < nb; i++)
                if (!has[i]) {
                    cutv[i] = plain_view(images_dev[b.i0 + i], H[b.i0 + i], W[b.i0 + i]);
                    nimg[nb + i] = i; naug[nb + i] = cut_a; ninert[nb + i] = 1;
                }
            for (size_t p = 0; p < b.pair_aug.size(); p++) b.pair_aug[p] = slot[b.pair_aug[p] - nb];
            b.view_img = nimg; b.view_aug = naug; b.view_inert = ninert;
            FwdReuse ru;
            if ((r = planner.cut_plan(k & 1, b.kept == CUT_KEPT_FPN, nb, cutv.data(), ru))) return r;
            if ((r = forward_model(m, nb, cutv.data(), FwdRequest::detect(det_at(D, (size_t)nb), prune_ok, &ru)))) return r;
            b.VV = 2 * nb + nr2; n_rest = nr2; rest_slot = 2 * nb; rest_views = rest.data();
        } else if (b.kept != CUT_KEPT_NONE) {
            c->cut_fallbacks++;
        }
        for (int f = 0; f < fwd_count(n_rest); f++) {
            int a0, nv; fwd_span(n_rest, f, &a0, &nv);
            const size_t o = (size_t)(rest_slot + a0);
            const FwdRequest rq = FwdRequest::detect(det_at(D, o), prune_ok).audited(audit ? d_vm[k & 1] + o * CALD_VM : nullptr);
            if ((r = forward_model(m, nv, rest_views + a0, rq))) return r;
        }
        return 0;
    }

    // scoring stage of batch k: the pair / view tables to the device, consistency + cls_corr (+ the pair audit), scores to the host, event
    int enqueue_scoring(int k) {
        SweepBatch& b = bt[k & 1];
        const DetBuffers& D = *DS[k & 1];
        const int P = (int)b.pair_img.size(), VV = b.VV;
        b.P = P;
        memset(b.h_ints, 0, n_ints * 4);
        const PairLayout::Ptrs hp = lay.at(b.h_ints), dp = lay.at(d_ints);
        for (int p = 0; p < P; p++) { hp.ref_view[p] = hp.pair_img[p] = b.pair_img[p]; hp.aug_view[p] = b.pair_aug[p]; hp.aug_kind[p] = b.pair_kind[p]; }
        memcpy(hp.ref_sel, b.ref_sel.data(), (size_t)B * 50 * 4); memcpy(hp.ref_n, b.ref_n.data(), (size_t)B * 4);
        memcpy(hp.view_img, b.view_img.data(), (size_t)VT * 4); memcpy(hp.view_isref, b.view_isref.data(), (size_t)VT * 4);
        if (P) memcpy(b.h_par, b.pair_par.data(), (size_t)P * 12 * 4);
        if (hipMemcpyAsync(d_ints, b.h_ints, n_ints * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            (P && hipMemcpyAsync(d_par, b.h_par, (size_t)P * 12 * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)) return fail(CALD_ERR_HIP, "H2D failed");
        const ScoreArgs sa = lay.score_args(d_ints, D, d_par, P, cfg->bp, d_cons);
        launch_consistency(sa, c->stream);
        launch_cls_corr(D, dp.ref_sel, dp.ref_n, dp.view_img, dp.view_isref, VV, d_clsc, c->stream);
        if (audit) {
            // RetinaNet rows carry no proposal: "another proposal" reads "another box" -- the detections of one anchor (one per class above
            // the threshold) share box, scores_cls and prob_max, as those of one proposal do
            ScoreArgs pa = sa;
            if (m->cfg.arch == CALD_ARCH_RETINANET) pa.det.props = pa.det.boxes;
            launch_pair_audit(pa, d_pm, c->stream);
            if (hipMemcpyAsync(b.h_vm, d_vm[k & 1], (size_t)VV * CALD_VM * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                (P && hipMemcpyAsync(b.h_pm, d_pm, (size_t)P * 2 * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)) return fail(CALD_ERR_HIP, "D2H of the audit records failed");
        }
        if ((P && hipMemcpyAsync(b.h_cons, d_cons, (size_t)P * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipMemcpyAsync(b.h_clsc, d_clsc, (size_t)VV * (C - 1) * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(m->ss.ev_score[k & 1], c->stream) != hipSuccess) return fail(CALD_ERR_HIP, "scoring stage failed: %s", hipGetErrorString(hipGetLastError()));
        return 0;
    }

    // float64 means of a scored batch (cald_train.py:225-228); waits for its scores
    int finish(int k) {
        SweepBatch& b = bt[k & 1];
        if (!b.live) return 0;
        if (hipEventSynchronize(m->ss.ev_score[k & 1]) != hipSuccess) return fail(CALD_ERR_HIP, "scoring stage failed: %s", hipGetErrorString(hipGetLastError()));
        const int nb = b.nb, P = b.P, VV = b.VV;
        std::vector<std::vector<int>> img_pairs(nb), img_views(nb);
        for (int p = 0; p < P; p++) img_pairs[b.pair_img[p]].push_back(p);
        for (int v = nb; v < VV; v++) if (!b.view_inert[v]) img_views[b.view_img[v]].push_back(v);
        // float64 sums in augmentation order (the cut_out reuse stores a batch's cut_out views ahead of the others)
        for (int i = 0; i < nb; i++)
            std::stable_sort(img_views[i].begin(), img_views[i].end(), [&](int x, int y) { return b.view_aug[x] < b.view_aug[y]; });
        for (int i = 0; i < nb; i++) {
            double* cc = cls_corr_out + (size_t)(b.i0 + i) * (C - 1);
            const int nvw = 1 + (int)img_views[i].size();
            for (int k2 = 0; k2 < C - 1; k2++) {
                double sm = (double)b.h_clsc[(size_t)i * (C - 1) + k2];
                for (int v : img_views[i]) sm += (double)b.h_clsc[(size_t)v * (C - 1) + k2];
                cc[k2] = sm / (double)nvw;
            }
            if (b.h_count[i] == 0 || img_pairs[i].empty()) { consistency_out[b.i0 + i] = 0.0; continue; }
            std::vector<double> cs;
            for (int p : img_pairs[i]) cs.push_back((double)b.h_cons[p]);
            consistency_out[b.i0 + i] = np_sum(cs.data(), (int)cs.size()) / (double)cs.size();
        }
        if (audit) {
            // per image: the smallest margin of each decision kind over its views / pairs (include/cald_hip.h CALD_MARGIN_*)
            for (int i = 0; i < nb; i++) {
                float* mg = margins_out + (size_t)(b.i0 + i) * CALD_N_MARGINS;
                for (int q = 0; q < CALD_N_MARGINS; q++) mg[q] = INFINITY;
                auto take_view = [&](int v) {
                    for (int q = 0; q <= VM_POST_CAP; q++) { const float t = b.h_vm[(size_t)v * CALD_VM + q]; if (t < mg[q]) mg[q] = t; }
                    const float t = b.h_vm[(size_t)v * CALD_VM + VM_POST_SMALL];        // RetinaNet's remove_small_boxes; +inf on a Faster R-CNN view
                    if (t < mg[CALD_MARGIN_POST_SMALL]) mg[CALD_MARGIN_POST_SMALL] = t;
                };
                take_view(i);
                for (int v : img_views[i]) take_view(v);
                mg[CALD_MARGIN_REF_SUBSAMPLE] = b.h_vm[(size_t)i * CALD_VM + VM_POST_SUBORDER];
                for (int p : img_pairs[i]) {
                    if (b.h_pm[2 * p] < mg[CALD_MARGIN_ARGMAX]) mg[CALD_MARGIN_ARGMAX] = b.h_pm[2 * p];
                    if (b.h_pm[2 * p + 1] != 0.0f) {
                        const float t = b.h_vm[(size_t)b.pair_aug[p] * CALD_VM + VM_POST_TOP2];
                        if (t < mg[CALD_MARGIN_ZERO_ROW]) mg[CALD_MARGIN_ZERO_ROW] = t;
                    }
                }
                mg[CALD_MARGIN_CUTOUT] = b.cut_margin[i];
            }
        }
        b.live = false;
        return 0;
    }

    int run() {
        int rc = setup();
        if (rc) return rc;
        // stream order: ref(0), ref(1), aug(0), score(0), ref(2), aug(1), score(1), ... -- the host builds batch k's views while the GPU runs
        // the reference forward of batch k + 1, and reads batch k's scores while batch k + 1 is on the GPU
        if (NB > 0) rc = enqueue_ref(0);
        for (int k = 0; k < NB && !rc; k++) {
            if (k + 1 < NB) {
                if ((rc = finish(k - 1))) break;              // set (k + 1) & 1 is batch k - 1's: its means first (its scores are long back)
                if ((rc = enqueue_ref(k + 1))) break;
            }
            if ((rc = build_aug_views(k)) || (rc = enqueue_aug_forwards(k)) || (rc = enqueue_scoring(k))) break;
        }
        for (int k = (NB >= 2 ? NB - 2 : 0); k < NB && !rc; k++) rc = finish(k);
        if (rc) hipStreamSynchronize(c->stream);
        return rc;
    }
};
}  // namespace

static int sweep_checked(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                         const int64_t* pool_pos, const cald_sweep_cfg* cfg, double* consistency_out, double* cls_corr_out, float* margins_out) {
    SweepRun first{m, n_images, images_dev, H, W, pool_pos, cfg, consistency_out, cls_corr_out, margins_out, false};
    int rc = first.run();
    if (rc || !(m->prune && first.prune_ok && first.NB > 0)) return rc;
    // the certified pruning's two tripwires: the bound, checked on every anchor that was evaluated both ways (15 - 60 % of P2 / P3), and the
    // range of the split (an activation of |x| >= 4094 or a non-finite one).  Either one voids the certificate on this data: the results
    // just computed are discarded and the same sweep is run again with the dense head, which needs neither (it used to fail)
    cald_ctx* c = m->ctx;
    float chk[2] = {0.0f, 0.0f};
    HIPCHK(hipMemcpy(chk, c->d_prune_check, 8, hipMemcpyDeviceToHost));
    const bool range = chk[1] != 0.0f;
    if (chk[0] == chk[0] && !range && !m->prune_bound_voided) c->prune_worst = chk[0] > c->prune_worst ? chk[0] : c->prune_worst;
    if (!(chk[0] <= 1.0f) || range) {
        c->prune_fallbacks++;
        SweepRun dense{m, n_images, images_dev, H, W, pool_pos, cfg, consistency_out, cls_corr_out, margins_out, true};
        rc = dense.run();
    }
    return rc;
}
extern "C" int cald_sweep(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                          const int64_t* pool_pos, const cald_sweep_cfg* cfg, double* consistency_out, double* cls_corr_out) {
    return sweep_checked(m, n_images, images_dev, H, W, pool_pos, cfg, consistency_out, cls_corr_out, nullptr);
}
extern "C" int cald_sweep_audit(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                                const int64_t* pool_pos, const cald_sweep_cfg* cfg, double* consistency_out, double* cls_corr_out,
                                float* margins_out) {
    if (!margins_out) return fail(CALD_ERR_INVALID, "null argument");
    return sweep_checked(m, n_images, images_dev, H, W, pool_pos, cfg, consistency_out, cls_corr_out, margins_out);
}


// =============================================================================================
// baseline sweeps on the same detector forward
// =============================================================================================
// lt_c_train.py:105-121 get_uncertainty: one forward per image, min over detections of |IoU(box, prop) + prob_max - 1|
extern "C" int cald_sweep_ltc(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                              int batch_images, double* uncertainty_out) {
    if (!m || !images_dev || !H || !W || !uncertainty_out) return fail(CALD_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
    if (m->cfg.arch != CALD_ARCH_FRCNN) return fail(CALD_ERR_INVALID, "lt_c needs the Faster R-CNN outputs (props)");
    cald_ctx* c = m->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int B = sweep_batch(batch_images, 64);
    { int rc0 = ensure_det(m, m->sweep_det, m->sweep_det_views, B); if (rc0) return rc0; }
    ScopedDev scratch(c->stream); float* d_out = nullptr;
    if (int rc0 = scratch.alloc(&d_out, (size_t)B * 4)) return rc0;
    std::vector<float> h(B);
    int rc = 0;
    for (int i0 = 0; i0 < n_images && !rc; i0 += B) {
        const int nb = (n_images - i0 < B) ? n_images - i0 : B;
        std::vector<ViewDesc> views = ref_views(images_dev, H, W, i0, nb);
        if ((rc = forward_model(m, nb, views.data(), FwdRequest::detect(m->sweep_det)))) break;
        launch_lt_uncertainty(m->sweep_det, nb, d_out, c->stream);
        if (hipMemcpyAsync(h.data(), d_out, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(CALD_ERR_HIP, "lt_c scoring failed: %s", hipGetErrorString(hipGetLastError())); break; }
        for (int i = 0; i < nb; i++) uncertainty_out[i0 + i] = (double)h[i];
    }
    return rc;
}

int cald_host::ssm_collect_rows(hipStream_t st, const char* hook, int image0, const SsmRows& R, int V, size_t score_cols, size_t label_cols, int64_t view_rows,
                                int64_t row0, int64_t rows_cap, int* al_out, int* count_out, float* boxes_out, float* scores_out, int8_t* labels_out, int* total_out) {
    int total = 0;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(al_out, R.al, (size_t)V * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(count_out, R.count, (size_t)V * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&total, R.total, 4, hipMemcpyDeviceToHost));
    int64_t sum = 0;
    for (int i = 0; i < V; i++) {
        const int n = count_out[i];
        if (n < 0 || n > view_rows || (al_out[i] && n) || (hook && n != total))
            return hook ? fail(CALD_ERR_HIP, "%s postprocess returned %d rows (al %d, total %d, cap %d)", hook, n, al_out[i], total, (int)view_rows)
                        : fail(CALD_ERR_HIP, "ssm postprocess returned %d rows for image %d (cap %lld)", n, image0 + i, (long long)view_rows);
        sum += n;
    }
    if (sum != total) return fail(CALD_ERR_HIP, "ssm postprocess: the batch's rows (%d) are not the sum of its images' (%lld)", total, (long long)sum);
    if (total && row0 + total <= rows_cap) {
        HIPCHK(hipMemcpy(boxes_out + row0 * 4, R.boxes, (size_t)total * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(scores_out + row0 * score_cols, R.scores, (size_t)total * score_cols * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(labels_out + row0 * label_cols, R.labels, (size_t)total * label_cols, hipMemcpyDeviceToHost));
    }
    *total_out = total;
    return 0;
}

// ssm/ssm_helper.py:9-33 get_uncertainty, the body of both SSM sweeps: one forward per image with the tail `tail` names in place of the
// ordinary one -- Faster R-CNN's (ssm.hip), or RetinaNet's (retina_ssm.hip), whose host stop (the picks of the batch's images, in order) sits
// inside forward_model, between the tail's two phases.  Per batch the flags and counts come back first, then exactly the batch's rows,
// appended to the caller's arrays.  The entry points have checked the arguments and the architecture.
static int ssm_sweep(cald_model* m, FwdRequest::Tail tail, cald_ssm_pick_fn pick, void* user, const char* name, int n_images, const uint8_t* const* images_dev,
                     const int* H, const int* W, int batch_images, int64_t rows_cap, int* al_out, int* count_out, float* boxes_out, float* scores_out,
                     int8_t* labels_out, int64_t* rows_needed_out) {
    if (n_images < 0 || rows_cap < 0) return fail(CALD_ERR_INVALID, "n_images and rows_cap must be >= 0");
    cald_ctx* c = m->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int B = sweep_batch(batch_images, 64);
    const bool retina = tail == FwdRequest::RETINA_SSM;
    // Faster R-CNN: C - 1 foreground classes, a score and a label per class and row; RetinaNet: C classes, one score and C - 1 labels per row
    const size_t C = (size_t)m->cfg.num_classes, score_cols = retina ? 1 : C - 1, label_cols = C - 1;
    const int64_t view_rows = (int64_t)(retina ? C : C - 1) * m->cfg.detections_per_img;
    int64_t rows = 0;
    for (int i0 = 0; i0 < n_images; i0 += B) {
        const int nb = (n_images - i0 < B) ? n_images - i0 : B;
        std::vector<ViewDesc> views = ref_views(images_dev, H, W, i0, nb);
        FwdSsm fs; FwdRetinaSsm fr; fr.pick = pick; fr.user = user; fr.image0 = i0;
        int rc, total = 0;
        if ((rc = forward_model(m, nb, views.data(), retina ? FwdRequest::retina_ssm_tail(&fr) : FwdRequest::ssm_tail(&fs)))) return rc;
        if ((rc = ssm_collect_rows(c->stream, nullptr, i0, retina ? fr.out.rows() : fs.out.rows(), nb, score_cols, label_cols, view_rows, rows, rows_cap,
                                   al_out + i0, count_out + i0, boxes_out, scores_out, labels_out, &total))) return rc;
        rows += total;
    }
    *rows_needed_out = rows;
    if (rows > rows_cap) return fail(CALD_ERR_INVALID, "%s: rows_cap %lld is too small, the sweep needs %lld rows", name, (long long)rows_cap, (long long)rows);
    return 0;
}
extern "C" int cald_sweep_ssm(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W, int batch_images,
                              int64_t rows_cap, int* al_out, int* count_out, float* boxes_out, float* scores_out, int8_t* labels_out,
                              int64_t* rows_needed_out) {
    if (!m || !images_dev || !H || !W || !al_out || !count_out || !boxes_out || !scores_out || !labels_out || !rows_needed_out)
        return fail(CALD_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
    if (m->cfg.arch != CALD_ARCH_FRCNN) return fail(CALD_ERR_INVALID, "the SSM sweep covers Faster R-CNN only");
    return ssm_sweep(m, FwdRequest::SSM, nullptr, nullptr, "cald_sweep_ssm", n_images, images_dev, H, W, batch_images, rows_cap, al_out, count_out, boxes_out,
                     scores_out, labels_out, rows_needed_out);
}
extern "C" int cald_sweep_ssm_retina(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W, int batch_images,
                                     cald_ssm_pick_fn pick, void* user, int64_t rows_cap, int* al_out, int* count_out, float* boxes_out,
                                     float* scores_out, int8_t* labels_out, int64_t* rows_needed_out) {
    if (!m || !images_dev || !H || !W || !pick || !al_out || !count_out || !boxes_out || !scores_out || !labels_out || !rows_needed_out)
        return fail(CALD_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
    if (m->cfg.arch != CALD_ARCH_RETINANET) return fail(CALD_ERR_INVALID, "cald_sweep_ssm_retina covers RetinaNet only (Faster R-CNN: cald_sweep_ssm)");
    if (m->cfg.num_classes < 2) return fail(CALD_ERR_INVALID, "the RetinaNet SSM tail needs at least two classes (labels have K - 1 columns)");
    return ssm_sweep(m, FwdRequest::RETINA_SSM, pick, user, "cald_sweep_ssm_retina", n_images, images_dev, H, W, batch_images, rows_cap, al_out, count_out,
                     boxes_out, scores_out, labels_out, rows_needed_out);
}

// ls_c_train.py:108-155 get_uncertainty: reference view + GaussianNoise(image, 8 i), i = 1..6 (six consecutive torch.randn
// draws on the per-image re-seeded generator), top-30 reference boxes by prob_max, IoU stability weighted by prob_max, minus
// U = max(1 - prob_max).
extern "C" int cald_sweep_lsc(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                              const int64_t* pool_pos, uint64_t base_seed, int batch_images, double* stability_out) {
    if (!m || !images_dev || !H || !W || !pool_pos || !stability_out) return fail(CALD_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
    for (int i = 0; i < n_images; i++)
        if (randn_unsupported(H[i], W[i]))
            return fail(CALD_ERR_UNSUPPORTED, "GaussianNoise on image %d (%dx%d): torch.randn of fewer than 16 elements takes torch's scalar path, which is not implemented", i, H[i], W[i]);
    cald_ctx* c = m->ctx;
    HIPCHK(hipSetDevice(c->device));
    const int A = 6;
    const int B = sweep_batch(batch_images, 32);
    const int cap = m->det_cap(), VT = B * (1 + A), P_MAX = B * A;
    { int rc0 = ensure_det(m, m->sweep_det, m->sweep_det_views, VT); if (rc0) return rc0; }
    DetBuffers& D = m->sweep_det;
    int* d_ints = nullptr; float *d_par = nullptr, *d_rows = nullptr; NoiseJob* d_gjobs = nullptr; float* d_noise = nullptr; size_t noise_cap = 0;
    const PairLayout L{P_MAX, B, 0};
    const size_t n_ints = L.n_ints();
    ScopedDev scratch(c->stream);
    {
        int rc0;
        if ((rc0 = scratch.alloc(&d_ints, n_ints * 4)) || (rc0 = scratch.alloc(&d_par, (size_t)P_MAX * 12 * 4)) ||
            (rc0 = scratch.alloc(&d_rows, (size_t)P_MAX * 50 * 4)) || (rc0 = scratch.alloc(&d_gjobs, sizeof(NoiseJob) * B))) return rc0;
    }
    HIPCHK(hipMemset(d_par, 0, (size_t)P_MAX * 12 * 4));
    std::vector<int> h_count(VT); std::vector<float> h_pm((size_t)B * cap), h_rows((size_t)P_MAX * 50);
    int rc = 0;
    for (int i0 = 0; i0 < n_images && !rc; i0 += B) {
        const int nb = (n_images - i0 < B) ? n_images - i0 : B;
        std::vector<ViewDesc> views = ref_views(images_dev, H, W, i0, nb);
        if ((rc = forward_model(m, nb, views.data(), FwdRequest::detect(D)))) break;
        if (hipMemcpyAsync(h_count.data(), D.count, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipMemcpyAsync(h_pm.data(), D.prob_max, (size_t)nb * cap * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(CALD_ERR_HIP, "D2H of reference detections failed"); break; }
        // host: the scored reference boxes (host_logic.h ls_select), noise jobs, views
        std::vector<int> ref_sel((size_t)B * 50, 0), ref_n(B, 0), pair_aug, pair_img;
        std::vector<ViewDesc> aviews; std::vector<NoiseJob> gjobs;
        size_t need = 0;
        for (int i = 0; i < nb; i++) if (h_count[i] > 0) need += ((size_t)H[i0 + i] * W[i0 + i] * 3 * A * 4 + 255) & ~(size_t)255;
        if (need > noise_cap) { if (d_noise) hipFree(d_noise); d_noise = nullptr; noise_cap = 0;
            if (hipMalloc((void**)&d_noise, need + (need >> 2)) != hipSuccess) { rc = fail(CALD_ERR_HIP, "hipMalloc of the noise arena failed"); break; } noise_cap = need + (need >> 2); }
        size_t noff = 0;
        for (int i = 0; i < nb; i++) {
            const int n = h_count[i];
            if (n == 0) continue;
            ref_n[i] = ls_select(n, &h_pm[(size_t)i * cap], &ref_sel[(size_t)i * 50]);
            const int Hi = H[i0 + i], Wi = W[i0 + i], ne = Hi * Wi * 3;
            float* nbase = reinterpret_cast<float*>(reinterpret_cast<char*>(d_noise) + noff); noff += ((size_t)ne * A * 4 + 255) & ~(size_t)255;
            NoiseJob gj; memset(&gj, 0, sizeof(gj));
            gj.src = images_dev[i0 + i]; gj.H = Hi; gj.W = Wi; gj.nseg = A; gj.seed = (uint64_t)base_seed * 1000003ull + (uint64_t)pool_pos[i0 + i];
            for (int k = 0; k < A; k++) { gj.seg[k].kind = 0; gj.seg[k].p0 = 8.0f * (float)(k + 1); gj.seg[k].dst = nbase + (size_t)k * ne; }
            gjobs.push_back(gj);
            for (int k = 0; k < A; k++) {
                ViewDesc v = plain_view(images_dev[i0 + i], Hi, Wi); v.noise = nbase + (size_t)k * ne;
                pair_img.push_back(i); pair_aug.push_back(nb + (int)aviews.size());
                aviews.push_back(v);
            }
        }
        if (!gjobs.empty()) {
            if (hipMemcpyAsync(d_gjobs, gjobs.data(), sizeof(NoiseJob) * gjobs.size(), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(CALD_ERR_HIP, "H2D of gaussian-noise jobs failed"); break; }
            launch_noise_stream(d_gjobs, (int)gjobs.size(), c->stream);
        }
        const int na = (int)aviews.size();
        // evenly sized forwards, as cald_sweep issues them (192 views run 96 + 96, not 128 + 64; CALD_MAX_VIEWS is the hard cap)
        for (int f = 0; f < fwd_count(na) && !rc; f++) {
            int a0, nv; fwd_span(na, f, &a0, &nv);
            rc = forward_model(m, nv, aviews.data() + a0, FwdRequest::detect(det_at(D, (size_t)(nb + a0))));
        }
        if (rc) break;
        const int P = (int)pair_img.size();
        std::vector<int> ints(n_ints, 0);
        const PairLayout::Ptrs hp = L.at(ints.data());
        for (int p = 0; p < P; p++) { hp.ref_view[p] = hp.pair_img[p] = pair_img[p]; hp.aug_view[p] = pair_aug[p]; hp.aug_kind[p] = 0; }
        memcpy(hp.ref_sel, ref_sel.data(), (size_t)B * 50 * 4); memcpy(hp.ref_n, ref_n.data(), (size_t)B * 4);
        if (hipMemcpyAsync(d_ints, ints.data(), n_ints * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(CALD_ERR_HIP, "H2D failed"); break; }
        launch_max_iou(L.score_args(d_ints, D, d_par, P, 0.f, nullptr), d_rows, c->stream);
        if ((P && hipMemcpyAsync(h_rows.data(), d_rows, (size_t)P * 50 * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(CALD_ERR_HIP, "ls_c scoring failed: %s", hipGetErrorString(hipGetLastError())); break; }
        // host: float64 / float32 numpy arithmetic of ls_c_train.py:151-153 (host_logic.h ls_tail)
        std::vector<std::vector<int>> img_pairs(nb);
        for (int p = 0; p < P; p++) img_pairs[pair_img[p]].push_back(p);
        for (int i = 0; i < nb; i++) {
            if (h_count[i] == 0) { stability_out[i0 + i] = 0.0; continue; }
            const int N = ref_n[i];
            std::vector<float> pm(N); std::vector<const float*> rows;
            for (int k = 0; k < N; k++) pm[k] = h_pm[(size_t)i * cap + ref_sel[(size_t)i * 50 + k]];
            for (int p : img_pairs[i]) rows.push_back(&h_rows[(size_t)p * 50]);
            stability_out[i0 + i] = ls_tail(N, pm.data(), (int)rows.size(), rows.data());
        }
    }
    hipStreamSynchronize(c->stream);
    if (d_noise) hipFree(d_noise);          // the fixed scratch belongs to `scratch`
    return rc;
}
