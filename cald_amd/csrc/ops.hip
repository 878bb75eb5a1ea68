// ops.hip -- the stand-alone operators of the C ABI (cald_op_*): parity hooks of the tests and tools, outside any model.  Host-side
// restatements used here (host_logic.h, no device work): cutout rectangle selection (cald/cald_helper.py:88-132), Pillow's resampling
// coefficients (cald_helper.py:47-53), the detector-transform size rule (torchvision GeneralizedRCNNTransform).
#include "host.h"

// =============================================================================================
// host-side restatements
// =============================================================================================
extern "C" int cald_op_transform_size(int H, int W, int min_size, int max_size, int* Hr, int* Wr, int* Hp, int* Wp) {
    if (H <= 0 || W <= 0 || min_size <= 0 || max_size <= 0) return fail(CALD_ERR_INVALID, "bad sizes");
    transform_size(H, W, min_size, max_size, Hr, Wr, Hp, Wp);
    return 0;
}

extern "C" int cald_op_cutout_rects(uint64_t seed, int H, int W, int N, const float* boxes, int cut_num, int* rects_out, int* n_out) {
    if (cut_num < 0 || cut_num > CALD_MAX_CUT) return fail(CALD_ERR_INVALID, "cut_num must be 0..%d", CALD_MAX_CUT);
    *n_out = cutout_rects(seed, H, W, N, boxes, cut_num, rects_out);
    return 0;
}

extern "C" int cald_op_cutout_geometry(int H, int W, int min_size, int max_size, int nrect, const int* rects, int nblk, const int* strides, int* out) {
    if (H < 1 || W < 1 || nrect < 0 || nrect > CALD_MAX_CUT || (nrect && !rects) || nblk < 0 || nblk > 64 || (nblk && !strides) || !out)
        return fail(CALD_ERR_INVALID, "bad argument");
    int Hr, Wr, Hp, Wp;
    transform_size(H, W, min_size, max_size, &Hr, &Wr, &Hp, &Wp);
    std::vector<CutSet> o(nblk + 1), t(nblk + 1);
    cut_geometry(H, W, Hr, Wr, Hp, Wp, nrect, rects, nblk, strides, &o[0], o.data() + 1, t.data() + 1);
    t[0].n = 0;
    for (int e = 0; e <= nblk; e++)
        for (int k = 0; k < 2; k++) {
            const CutSet& sset = k ? t[e] : o[e];
            int* q = out + (size_t)(2 * e + k) * (1 + 4 * CUT_SET_MAX);
            memset(q, 0, sizeof(int) * (1 + 4 * CUT_SET_MAX));
            q[0] = sset.n;
            for (int i = 0; i < sset.n; i++) { q[1 + 4 * i] = sset.r[i].x0; q[2 + 4 * i] = sset.r[i].y0; q[3 + 4 * i] = sset.r[i].x1; q[4 + 4 * i] = sset.r[i].y1; }
        }
    return 0;
}
// The FPN sets of the cut_out reuse (host_logic.h cut_fpn_geometry) over a whole backbone: `strides` are conv2's strides of all nblk blocks;
// a stage ends before the next stride-2 block and with the last block, and there must be four of them (C2..C5).  out: eight sets in
// cald_op_cutout_geometry's form ([n, then x0 y0 x1 y1 per rectangle], 1 + 4 CUT_SET_MAX ints each): inner P2..P5, then output P2..P5.
extern "C" int cald_op_cutout_fpn_geometry(int H, int W, int min_size, int max_size, int nrect, const int* rects, int nblk, const int* strides, int* out) {
    if (H < 1 || W < 1 || nrect < 0 || nrect > CALD_MAX_CUT || (nrect && !rects) || nblk < 4 || nblk > 64 || !strides || !out)
        return fail(CALD_ERR_INVALID, "bad argument");
    int ends[4], ne = 0;
    for (int b = 0; b < nblk; b++)
        if (b == nblk - 1 || strides[b + 1] == 2) { if (ne == 4) return fail(CALD_ERR_INVALID, "more than four stages"); ends[ne++] = b; }
    if (ne != 4) return fail(CALD_ERR_INVALID, "the strides describe %d stages, not four", ne);
    int Hr, Wr, Hp, Wp;
    transform_size(H, W, min_size, max_size, &Hr, &Wr, &Hp, &Wp);
    std::vector<CutSet> o(nblk), t(nblk);
    CutSet pool1, cs[4], sets[8];
    cut_geometry(H, W, Hr, Wr, Hp, Wp, nrect, rects, nblk, strides, &pool1, o.data(), t.data());
    for (int i = 0; i < 4; i++) cs[i] = o[ends[i]];
    cut_fpn_geometry(Hp, Wp, cs, sets, sets + 4);
    for (int e = 0; e < 8; e++) {
        int* q = out + (size_t)e * (1 + 4 * CUT_SET_MAX);
        memset(q, 0, sizeof(int) * (1 + 4 * CUT_SET_MAX));
        q[0] = sets[e].n;
        for (int i = 0; i < sets[e].n; i++) { q[1 + 4 * i] = sets[e].r[i].x0; q[2 + 4 * i] = sets[e].r[i].y0; q[3 + 4 * i] = sets[e].r[i].x1; q[4 + 4 * i] = sets[e].r[i].y1; }
    }
    return 0;
}
static int get_pil(cald_ctx* c, int inSize, int outSize, int fid, PilCoef* out) {
    PilKey key{inSize, outSize, fid};
    auto it = c->pil.find(key);
    if (it == c->pil.end()) {
        std::vector<int> b, k;
        PilCoef pc; pc.ksize = pil_coeffs(inSize, outSize, fid, b, k);
        ScopedDev sd(c->stream); int rc;
        if ((rc = sd.upload(&pc.d_bounds, b.data(), b.size() * sizeof(int))) || (rc = sd.upload(&pc.d_kk, k.data(), k.size() * sizeof(int)))) return rc;
        sd.release();           // both tables exist: the context's cache owns them from here on
        it = c->pil.insert(std::make_pair(key, pc)).first;
    }
    *out = it->second;
    return 0;
}
// dst [oh][ow][3]; tmp must hold H*ow*3 bytes
int cald_host::pil_resize(cald_ctx* c, const uint8_t* src, int H, int W, uint8_t* dst, int oh, int ow, uint8_t* tmp, int fid) {
    const uint8_t* cur = src;
    if (ow != W) {
        PilCoef pc; int rc = get_pil(c, W, ow, fid, &pc); if (rc) return rc;
        uint8_t* hdst = (oh != H) ? tmp : dst;
        launch_pil_horizontal(src, H, W, hdst, ow, pc.d_bounds, pc.d_kk, pc.ksize, c->stream);
        cur = hdst;
    }
    if (oh != H) {
        PilCoef pc; int rc = get_pil(c, H, oh, fid, &pc); if (rc) return rc;
        launch_pil_vertical(cur, H, ow, dst, oh, pc.d_bounds, pc.d_kk, pc.ksize, c->stream);
    } else if (ow == W) {
        HIPCHK(hipMemcpyAsync(dst, src, (size_t)H * W * 3, hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}
extern "C" int cald_op_pil_resize(cald_ctx* c, const uint8_t* src_dev, int H, int W, uint8_t* dst_dev, int oh, int ow) {
    if (!c || !src_dev || !dst_dev || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) return fail(CALD_ERR_INVALID, "bad arguments");
    ScopedDev sd(c->stream);
    uint8_t* tmp; int rc;
    if ((rc = sd.alloc(&tmp, (size_t)H * ow * 3))) return rc;
    return pil_resize(c, src_dev, H, W, dst_dev, oh, ow, tmp);
}

// One NoiseJob of up to CALD_MAX_NOISE_SEG views drawn in order from one generator, one launch of noise_stream_kernel: what the sweep
// issues per image, without a model.  kinds[g] = CALD_AUG_GAUSS (params[g] = std, dsts[g] = float [3][H][W]) or CALD_AUG_SALT_PEPPER
// (params[g] = prob, dsts[g] = uint8 [H][W][3]).
extern "C" int cald_op_noise_stream(cald_ctx* c, uint64_t seed, const uint8_t* src_dev, int H, int W, int nseg, const int* kinds,
                                    const double* params, void* const* dsts) {
    if (!c || !src_dev || H <= 0 || W <= 0 || !kinds || !params || !dsts) return fail(CALD_ERR_INVALID, "cald_op_noise_stream: bad arguments");
    if (nseg < 1 || nseg > CALD_MAX_NOISE_SEG) return fail(CALD_ERR_INVALID, "cald_op_noise_stream: 1..%d segments", CALD_MAX_NOISE_SEG);
    NoiseJob nj; memset(&nj, 0, sizeof(nj));
    nj.seed = seed; nj.src = src_dev; nj.H = H; nj.W = W; nj.nseg = nseg;
    for (int g = 0; g < nseg; g++) {
        NoiseSeg& sg = nj.seg[g];
        if (!dsts[g]) return fail(CALD_ERR_INVALID, "cald_op_noise_stream: segment %d has no destination", g);
        sg.dst = dsts[g];
        if (kinds[g] == CALD_AUG_GAUSS) {
            if (randn_unsupported(H, W))
                return fail(CALD_ERR_UNSUPPORTED, "GaussianNoise on a %dx%d image: torch.randn of fewer than 16 elements takes torch's scalar path, which is not implemented", H, W);
            sg.kind = 0; sg.p0 = (float)params[g]; sg.p1 = 0.0f;
        } else if (kinds[g] == CALD_AUG_SALT_PEPPER) {
            sg.kind = 1; sg.p0 = (float)(params[g] / 2.0); sg.p1 = (float)(1.0 - params[g] / 2.0);
        } else return fail(CALD_ERR_INVALID, "cald_op_noise_stream: segment %d: kind %d is neither GAUSS nor SALT_PEPPER", g, kinds[g]);
    }
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    NoiseJob* d; int rc;
    if ((rc = sd.upload(&d, &nj, sizeof(nj)))) return rc;
    launch_noise_stream(d, 1, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(CALD_ERR_HIP, "noise stream failed: %s", hipGetErrorString(e));
    return CALD_OK;
}

// One augmented view of one image, outside the sweep (the helper API of cald/cald_helper.py and the parity tests).
// A fresh generator is seeded with `seed` (torch's for GAUSS / SALT_PEPPER, Python's for COLOR_SWAP).
extern "C" int cald_op_augment(cald_ctx* c, int kind, double param, uint64_t seed, const uint8_t* src_dev, int H, int W,
                               int n_boxes, const float* boxes, void* dst_dev, float* boxes_out, int* aux_out) {
    if (!c || H <= 0 || W <= 0) return fail(CALD_ERR_INVALID, "bad arguments");
    if (kind == CALD_AUG_COLOR_SWAP) {
        if (!aux_out) return fail(CALD_ERR_INVALID, "color_swap: aux_out is null");
        PyRandom r; r.seed(seed);
        aux_out[0] = r.randbelow(6);
        return CALD_OK;
    }
    if (!src_dev || !dst_dev) return fail(CALD_ERR_INVALID, "null image pointer");
    HIPCHK(hipSetDevice(c->device));
    const size_t nbytes = (size_t)H * W * 3;
    ScopedDev sd(c->stream); int rc;
    if (kind == CALD_AUG_GAUSS || kind == CALD_AUG_SALT_PEPPER) {
        void* dsts[1] = {dst_dev};
        return cald_op_noise_stream(c, seed, src_dev, H, W, 1, &kind, &param, dsts);
    }
    if (kind == CALD_AUG_COLOR_ADJUST) {
        uint8_t* tmp;
        if ((rc = sd.alloc(&tmp, nbytes + 256))) return rc;
        unsigned long long* lsum = reinterpret_cast<unsigned long long*>(tmp + ((nbytes + 7) & ~(size_t)7));
        launch_color_adjust(src_dev, H, W, (float)param, tmp, lsum, reinterpret_cast<uint8_t*>(dst_dev), c->stream);
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(CALD_ERR_HIP, "color adjust failed: %s", hipGetErrorString(e));
        return CALD_OK;
    }
    if (kind == CALD_AUG_ROTATE) {
        if (n_boxes < 0 || (n_boxes && (!boxes || !boxes_out))) return fail(CALD_ERR_INVALID, "rotate: null boxes");
        int fx[6], nh, nw; pil_rotate_setup(H, W, param, fx, &nh, &nw);
        uint8_t* ws;
        const size_t a = ((size_t)nh * nw * 3 + 255) & ~(size_t)255;
        if ((rc = sd.alloc(&ws, a + (size_t)nh * W * 3))) return rc;
        launch_affine_nearest(src_dev, H, W, ws, nh, nw, fx, c->stream);
        if ((rc = pil_resize(c, ws, nh, nw, reinterpret_cast<uint8_t*>(dst_dev), H, W, ws + a, 1))) return rc;
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(CALD_ERR_HIP, "rotate failed: %s", hipGetErrorString(e));
        float par[12]; rotate_box_params(H, W, param, nw, nh, par);
        rotate_boxes_host(par, boxes, n_boxes, boxes_out);
        return CALD_OK;
    }
    return fail(CALD_ERR_INVALID, "cald_op_augment: kind %d has its own entry point or needs no device work", kind);
}

// =============================================================================================
// operator-level entry points
// =============================================================================================
// device copies, owned by `sd`, of a layer's packings -- those the caller leaves in `pk`: they decide the kernel launch_conv picks -- and of its
// epilogue vectors (the first n entries of each, padded with zeros to CoutPad; null: no such term), into the weight and epilogue fields of `a`
static int upload_layer(ScopedDev& sd, const ConvPack& pk, const float* bias, const float* scale, const float* shift, int n, ConvArgs& a) {
    int rc;
    const float* src[3] = {bias, scale, shift}; const float** dst[3] = {&a.bias, &a.scale, &a.shift};
    for (int i = 0; i < 3; i++) {
        std::vector<float> v(pk.CoutPad, 0.0f);
        if (src[i]) std::copy(src[i], src[i] + n, v.begin());
        if ((rc = sd.upload(dst[i], src[i] ? v.data() : nullptr, v.size() * 4))) return rc;
    }
    if ((rc = sd.upload(&a.w, pk.w.data(), pk.w.size() * 4)) || (rc = sd.upload(&a.w4, pk.w4.empty() ? nullptr : pk.w4.data(), pk.w4.size() * 4)) ||
        (rc = sd.upload(&a.w16, pk.w16.empty() ? nullptr : pk.w16.data(), pk.w16.size() * 2)) ||
        (rc = sd.upload(&a.wstem, pk.wstem.empty() ? nullptr : pk.wstem.data(), pk.wstem.size() * 4))) return rc;
    a.w16_unscale = pk.w16_unscale; a.CoutPad = pk.CoutPad; a.Kpad = pk.Kpad;
    return 0;
}
static int op_conv2d(cald_ctx* c, int precision, const float* in, int H, int W, int Cin, const float* weight, int Cout, int KH, int KW,
                     int stride, int pad, const float* bias, const float* bn_scale, const float* bn_shift,
                     const float* residual, int relu, float* out) {
    if (!c || !in || !weight || !out) return fail(CALD_ERR_INVALID, "null argument");
    if (Cin % 4) return fail(CALD_ERR_INVALID, "Cin must be a multiple of 4");
    HIPCHK(hipSetDevice(c->device));
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    ConvPack pk;
    pack_conv({weight}, {Cout}, Cin, Cin, KH, KW, stride, pad, precision == CALD_PRECISION_F16X3, &pk);
    pk.wstem.clear();       // this entry point never runs conv_stem.hip
    BatchPlan P; memset(&P, 0, sizeof(P));
    P.seg[0][0].H = H; P.seg[0][0].W = W; P.seg[0][1].pix_off = (long long)H * W; P.seg[0][1].tile_start = (H * W + 127) / 128;
    P.seg[1][0].H = Ho; P.seg[1][0].W = Wo; P.seg[1][1].pix_off = (long long)Ho * Wo; P.seg[1][1].tile_start = (Ho * Wo + 127) / 128;
    ScopedDev sd(c->stream);
    ConvArgs a; memset(&a, 0, sizeof(a));
    BatchPlan* d_p; int rc;
    if ((rc = upload_layer(sd, pk, bias, bn_scale, bn_scale ? bn_shift : nullptr, Cout, a)) || (rc = sd.upload(&a.in, in, (size_t)H * W * Cin * 4)) ||
        (rc = sd.alloc(&a.out, (size_t)Ho * Wo * Cout * 4)) || (rc = sd.upload(&a.residual, residual, (size_t)Ho * Wo * Cout * 4)) ||
        (rc = sd.upload(&d_p, &P, sizeof(P)))) return rc;
    a.seg_in = d_p->seg[0]; a.seg_out = d_p->seg[1]; a.seg_up = d_p->seg[1];
    a.V = 1; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
    a.relu = relu; a.total_mtiles = (Ho * Wo + 127) / 128; a.out_ld = Cout; a.zeros = c->d_zeros;
    const bool launched = launch_conv(a, c->stream) != nullptr;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, a.out, (size_t)Ho * Wo * Cout * 4, hipMemcpyDeviceToHost));
    return launched ? 0 : conv_refused(a);
}
extern "C" int cald_op_conv2d(cald_ctx* c, const float* in, int H, int W, int Cin, const float* weight, int Cout, int KH, int KW,
                              int stride, int pad, const float* bias, const float* bn_scale, const float* bn_shift,
                              const float* residual, int relu, float* out) {
    return op_conv2d(c, CALD_PRECISION_FP32, in, H, W, Cin, weight, Cout, KH, KW, stride, pad, bias, bn_scale, bn_shift, residual, relu, out);
}
// ---------------------------------------------------------------------------------------------
// test-only conv probe (tests/test_gpu_conv_variants.py): one launch of the product's launchers on a ragged batch the caller describes,
// under a forced kernel choice, with the product's own weight packing.  Output buffers are the caller's, copied whole to the device and
// back, so whatever the caller put beyond the rows / channels a kernel may write (its guard words) comes back for inspection.
// ---------------------------------------------------------------------------------------------
extern "C" int cald_op_conv_probe(cald_ctx* c, int precision, cald_conv_probe* pr, int n, int path, int tile, char* kernel, int kernel_cap) {
    if (!c || !pr || n < 1 || n > CALD_MAX_GROUP || !kernel || kernel_cap < 1) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: bad arguments");
    if (path < CONV_AUTO || path > CONV_H4_GROUP || tile < TILE_AUTO || tile > TILE_WIDE) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: bad path / tile");
    if (path == CONV_P4_FUSED && n != 2) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: the fused mode takes two problems (conv2, conv3)");
    HIPCHK(hipSetDevice(c->device));
    kernel[0] = 0;
    ScopedDev sd(c->stream);
    ConvArgs a[CALD_MAX_GROUP];
    struct Back { void* dev; void* host; size_t bytes; };
    std::vector<Back> back;
    int rc;
    for (int i = 0; i < n; i++) {
        const cald_conv_probe& p = pr[i];
        if (p.V < 1 || p.V > CALD_PROBE_MAX_VIEWS || p.Cin < 4 || p.Cin % 4 || p.Cout < 1 || p.KH < 1 || p.KW < 1 || p.stride < 1 || p.pad < 0 ||
            p.out_ld < p.Cout || !p.weight || !p.in)
            return fail(CALD_ERR_INVALID, "cald_op_conv_probe: problem %d: bad layer", i);
        // geometry: level 0 input, 1 output, 2 the coarser level of `up`
        std::vector<LevelSeg> seg(3 * (CALD_PROBE_MAX_VIEWS + 1));
        memset(seg.data(), 0, seg.size() * sizeof(LevelSeg));
        LevelSeg* si = &seg[0]; LevelSeg* so = &seg[CALD_PROBE_MAX_VIEWS + 1]; LevelSeg* su = &seg[2 * (CALD_PROBE_MAX_VIEWS + 1)];
        std::vector<GatherSet> gs(p.V);
        long long rows_out = 0;
        for (int v = 0; v < p.V; v++) {
            const int H = p.in_hw[v][0], W = p.in_hw[v][1];
            if (H < 0 || W < 0) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: negative view size");
            const int Ho = H && W ? (H + 2 * p.pad - p.KH) / p.stride + 1 : 0, Wo = H && W ? (W + 2 * p.pad - p.KW) / p.stride + 1 : 0;
            if (Ho < 0 || Wo < 0 || (H && W && (Ho < 1 || Wo < 1))) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: view %d smaller than the filter", v);
            si[v].H = H; si[v].W = W; so[v].H = Ho; so[v].W = Wo; su[v].H = p.up_hw[v][0]; su[v].W = p.up_hw[v][1];
            long long m = (long long)Ho * Wo;
            if (p.gather) {
                GatherSet& g = gs[v]; memset(&g, 0, sizeof(g));
                if (p.nrect[v] < 0 || p.nrect[v] > CALD_GATHER_RECTS) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: 0..%d rectangles", CALD_GATHER_RECTS);
                g.nr = p.nrect[v];
                for (int k = 0; k < g.nr; k++) {
                    const int* r = p.rect[v][k];
                    if (r[0] < 0 || r[1] < 0 || r[2] < 1 || r[3] < 1 || r[0] + r[2] > Wo || r[1] + r[3] > Ho)
                        return fail(CALD_ERR_INVALID, "cald_op_conv_probe: rectangle outside view %d", v);
                    g.x0[k] = r[0]; g.y0[k] = r[1]; g.w[k] = r[2]; g.cum[k + 1] = g.cum[k] + r[2] * r[3];
                }
                m = g.cum[g.nr];
            }
            si[v + 1].pix_off = si[v].pix_off + (long long)H * W;
            so[v + 1].pix_off = so[v].pix_off + (long long)Ho * Wo;
            su[v + 1].pix_off = su[v].pix_off + (long long)su[v].H * su[v].W;
            so[v + 1].tile_start = so[v].tile_start + (int)((m + 127) / 128);
            si[v + 1].tile_start = si[v].tile_start + (H * W + 127) / 128;
            rows_out = so[v + 1].pix_off;
        }
        const long long pix_in = si[p.V].pix_off, pix_up = su[p.V].pix_off;
        if ((p.out && p.out_n < rows_out * p.out_ld) || (p.out16 && p.out16_n < rows_out * p.out_ld) || (p.energy4 && p.energy4_n < rows_out * 4))
            return fail(CALD_ERR_INVALID, "cald_op_conv_probe: problem %d: an output buffer is smaller than the output", i);
        ConvPack pk;
        const int cin_true = p.cin_true > 0 ? p.cin_true : p.Cin;
        if (cin_true > p.Cin) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: cin_true > Cin");
        pack_conv({p.weight}, {p.Cout}, cin_true, p.Cin, p.KH, p.KW, p.stride, p.pad, precision == CALD_PRECISION_F16X3, &pk);
        if (!stem_grid_exact(so, p.V)) pk.wstem.clear();
        ConvArgs& A = a[i]; memset(&A, 0, sizeof(A));
        const LevelSeg* d_seg;
        const size_t out_b = (size_t)p.out_ld * 4;
        if ((rc = upload_layer(sd, pk, p.bias, p.bn_scale, p.bn_scale ? p.bn_shift : nullptr, p.Cout, A)) ||
            (rc = sd.upload(&A.in, p.in, (size_t)pix_in * p.Cin * 4)) || (rc = sd.upload(&A.in16, p.in16, (size_t)pix_in * p.Cin * 4)) ||
            (rc = sd.upload(&A.residual, p.residual, (size_t)rows_out * out_b)) || (rc = sd.upload(&A.up, p.up, (size_t)pix_up * out_b)) ||
            (rc = sd.upload(&A.mask, p.mask, (size_t)rows_out * out_b)) || (rc = sd.upload(&A.row_map, p.row_map, (size_t)rows_out * 4)) ||
            (rc = sd.upload(&A.dyn_rows, p.has_dyn ? p.dyn_rows : nullptr, (size_t)p.V * 4)) ||
            (rc = sd.upload(&A.gather, p.gather ? gs.data() : nullptr, gs.size() * sizeof(GatherSet))) ||
            (rc = sd.upload(&d_seg, seg.data(), seg.size() * sizeof(LevelSeg))) || (rc = sd.upload(&A.out, p.out, (size_t)p.out_n * 4)) ||
            (rc = sd.upload(&A.out16, p.out16, (size_t)p.out16_n * 4)) || (rc = sd.upload(&A.energy4, p.energy4, (size_t)p.energy4_n * 4))) return rc;
        if (p.head_out) {        // the look-ahead's head epilogue (conv_h4 grouped only: no other launcher knows the fields)
            if (path != CONV_H4_GROUP || !p.head_w || !p.head_b || p.head_ld < 3 || p.head_out_n < rows_out * p.head_ld)
                return fail(CALD_ERR_INVALID, "cald_op_conv_probe: problem %d: head fields need path 9, head_w, head_b, head_ld >= 3 and a buffer of the output's rows", i);
            if ((rc = sd.upload(&A.head_w, p.head_w, (size_t)3 * p.Cout * 4)) || (rc = sd.upload(&A.head_out, p.head_out, (size_t)p.head_out_n * 4))) return rc;
            for (int q = 0; q < 3; q++) A.head_b[q] = p.head_b[q];
            A.head_ld = p.head_ld;
            back.push_back({A.head_out, p.head_out, (size_t)p.head_out_n * 4});
        }
        A.seg_in = d_seg; A.seg_out = d_seg + CALD_PROBE_MAX_VIEWS + 1; A.seg_up = d_seg + 2 * (CALD_PROBE_MAX_VIEWS + 1);
        if (p.out) back.push_back({A.out, p.out, (size_t)p.out_n * 4});
        if (p.out16) back.push_back({A.out16, p.out16, (size_t)p.out16_n * 4});
        if (p.energy4) back.push_back({A.energy4, p.energy4, (size_t)p.energy4_n * 4});
        A.ex16 = p.ex16 ? 1 : 0;
        A.V = p.V; A.Cin = p.Cin; A.Cout = p.Cout;
        A.KH = p.KH; A.KW = p.KW; A.stride = p.stride; A.pad = p.pad; A.relu = p.relu ? 1 : 0; A.in_relu = p.in_relu ? 1 : 0;
        A.total_mtiles = so[p.V].tile_start; A.out_ld = p.out_ld; A.zeros = c->d_zeros;
        // row tiles (cald_conv_probe::row_packing): auto offers conv_p4 the packed row count under a forward's own rule
        if (p.row_packing < CALD_PROBE_PACK_AUTO || p.row_packing > CALD_PROBE_PACK_ON) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: problem %d: bad row_packing", i);
        const bool packable = !p.has_dyn && !p.row_map && !p.gather && !p.mask && p.Cin != 4 && path != CONV_P4_FUSED;
        if (packable && (p.row_packing == CALD_PROBE_PACK_ON || (p.row_packing == CALD_PROBE_PACK_AUTO && conv_pack_default())))
            A.packed_rows = conv_pack_rows(si, so, p.up ? su : nullptr, p.V, p.Cin, p.out_ld);
        if (p.row_packing == CALD_PROBE_PACK_ON && !A.packed_rows) return fail(CALD_ERR_INVALID, "cald_op_conv_probe: problem %d cannot run on packed row tiles", i);
    }
    if (path == CONV_P4_FUSED) a[1].in = a[0].out;       // conv3 reads conv2's output (which the fused kernel keeps on chip)
    const ConvForce f{path, tile};
    const char* names[CALD_MAX_GROUP] = {nullptr};
    if (path == CONV_P4_FUSED) names[0] = names[1] = launch_conv_p4_fused(a[0], a[1], c->stream);
    else if (n > 1 || path == CONV_P4_GROUP || path == CONV_H3_GROUP || path == CONV_H4_GROUP) launch_conv_group(a, n, c->stream, names, f);
    else names[0] = launch_conv(a[0], c->stream, f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    std::string all;
    for (int i = 0; i < n; i++) {
        if (!names[i]) return fail(CALD_ERR_UNSUPPORTED, "cald_op_conv_probe: problem %d refused under path %d tile %d", i, path, tile);
        if (all.find(names[i]) == std::string::npos) { if (!all.empty()) all += ";"; all += names[i]; }
    }
    for (const Back& b : back) HIPCHK(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    snprintf(kernel, (size_t)kernel_cap, "%s", all.c_str());
    return 0;
}
// host-only: the packed row tiles' lookup (common.h seg_find_row) and admission rule (conv_pack_rows) on a plan the caller describes
extern "C" int cald_op_row_pack_lookup(int V, const int* in_hw, const int* out_hw, int Cin, int out_ld, int64_t n, const int64_t* rows,
                                       int* view_out, int64_t* local_out, int64_t* packed_rows_out) {
    if (V < 1 || V > CALD_MAX_VIEWS || !in_hw || !out_hw || n < 0 || (n && (!rows || !view_out || !local_out)))
        return fail(CALD_ERR_INVALID, "cald_op_row_pack_lookup: bad arguments");
    std::vector<LevelSeg> si(V + 1), so(V + 1);
    memset(si.data(), 0, si.size() * sizeof(LevelSeg)); memset(so.data(), 0, so.size() * sizeof(LevelSeg));
    for (int v = 0; v < V; v++) {
        if (in_hw[2 * v] < 0 || in_hw[2 * v + 1] < 0 || out_hw[2 * v] < 0 || out_hw[2 * v + 1] < 0) return fail(CALD_ERR_INVALID, "cald_op_row_pack_lookup: negative size");
        si[v].H = in_hw[2 * v]; si[v].W = in_hw[2 * v + 1]; so[v].H = out_hw[2 * v]; so[v].W = out_hw[2 * v + 1];
        si[v + 1].pix_off = si[v].pix_off + (long long)si[v].H * si[v].W;
        so[v + 1].pix_off = so[v].pix_off + (long long)so[v].H * so[v].W;
    }
    for (int64_t i = 0; i < n; i++) {
        if (rows[i] < 0 || rows[i] >= so[V].pix_off) return fail(CALD_ERR_INVALID, "cald_op_row_pack_lookup: row %lld outside the level", (long long)rows[i]);
        const int v = seg_find_row(so.data(), V, rows[i]);
        view_out[i] = v; local_out[i] = rows[i] - so[v].pix_off;
    }
    if (packed_rows_out) *packed_rows_out = conv_pack_rows(si.data(), so.data(), nullptr, V, Cin, out_ld);
    return 0;
}
void launch_mfma_f16_probe(const unsigned short* A, const unsigned short* B, const unsigned* C, unsigned* D, long long n, hipStream_t stream);   // conv_h3.hip
extern "C" int cald_op_mfma_f16(cald_ctx* c, const uint16_t* A, const uint16_t* B, const uint32_t* C, uint32_t* D, int64_t n) {
    if (!c || !A || !B || !C || !D || n < 1) return fail(CALD_ERR_INVALID, "cald_op_mfma_f16: null argument or n < 1");
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    const unsigned short *dA, *dB; const unsigned* dC; unsigned* dD; int rc;
    if ((rc = sd.upload(&dA, A, (size_t)n * 32)) || (rc = sd.upload(&dB, B, (size_t)n * 32)) || (rc = sd.upload(&dC, C, (size_t)n * 4)) ||
        (rc = sd.alloc(&dD, (size_t)n * 4))) return rc;
    launch_mfma_f16_probe(dA, dB, dC, dD, (long long)n, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D, dD, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int cald_op_conv2d_f16x3(cald_ctx* c, const float* in, int H, int W, int Cin, const float* weight, int Cout, int KH, int KW,
                                    int stride, int pad, const float* bias, const float* bn_scale, const float* bn_shift,
                                    const float* residual, int relu, float* out) {
    return op_conv2d(c, CALD_PRECISION_F16X3, in, H, W, Cin, weight, Cout, KH, KW, stride, pad, bias, bn_scale, bn_shift, residual, relu, out);
}

// ---------------------------------------------------------------------------------------------
// kernel-tuning aid (tools/bench_conv.py): times ONE conv layer shape on a ragged batch of V equal views with
// pseudo-random data (MFMA power, hence the sustained clock, depends on the operand values: never bench on zeros)
// ---------------------------------------------------------------------------------------------
__global__ void fill_random_kernel(float* p, long long n, unsigned seed) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        unsigned x = (unsigned)i * 2654435761u ^ seed; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
        p[i] = ((float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f) * ((x & 7u) ? 1.0f : 0.0f);      // ~U(-1, 1), 1/8 zeros (post-ReLU-like)
    }
}
extern "C" int cald_op_conv_bench(cald_ctx* c, int V, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int residual,
                                  int relu, int iters, int group, double* ms_out, double* tflops_out) {
    if (!c || V < 1 || V > CALD_MAX_VIEWS || iters < 1 || !ms_out || group < 1 || group > CALD_MAX_GROUP) return fail(CALD_ERR_INVALID, "bad arguments");
    if (Cin % 4) return fail(CALD_ERR_INVALID, "Cin must be a multiple of 4");
    HIPCHK(hipSetDevice(c->device));
    const int KW = KH, Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    const int K = KH * KW * Cin;
    ConvPack pk; pk.CoutPad = cout_pad(Cout); pk.Kpad = round_up(K, 16);
    const int CoutPad = pk.CoutPad, Kpad = pk.Kpad;
    pk.w.assign((size_t)Kpad * CoutPad, 0.0f);
    const std::vector<float> b(CoutPad, 0.1f), sc(CoutPad, 1.0f), sh(CoutPad, 0.01f);
    unsigned r = 12345u;
    for (int k = 0; k < K; k++) for (int n = 0; n < Cout; n++) { r = r * 1664525u + 1013904223u; pk.w[(size_t)k * CoutPad + n] = ((float)(r >> 8) / 8388608.0f - 1.0f) * 0.05f; }
    if (CoutPad % 64 == 0 && ((Cin % 16 == 0 && KH * KW <= 32) || Cin == 4)) pk.w4 = pack_w4(pk.w, Kpad, CoutPad);
    BatchPlan P; memset(&P, 0, sizeof(P));
    for (int v = 0; v <= V; v++) {
        P.seg[0][v].pix_off = (long long)v * H * W; P.seg[0][v].tile_start = v * ((H * W + 127) / 128); P.seg[0][v].H = H; P.seg[0][v].W = W;
        P.seg[1][v].pix_off = (long long)v * Ho * Wo; P.seg[1][v].tile_start = v * ((Ho * Wo + 127) / 128); P.seg[1][v].H = Ho; P.seg[1][v].W = Wo;
    }
    ScopedDev sd(c->stream);
    float *d_in, *d_out, *d_res = nullptr; BatchPlan* d_p;
    const size_t n_in = (size_t)V * H * W * Cin, n_out = (size_t)V * Ho * Wo * Cout;
    ConvArgs a[CALD_MAX_GROUP]; memset(a, 0, sizeof(a));
    int rc;
    if ((rc = sd.alloc(&d_in, n_in * 4)) || (rc = sd.alloc(&d_out, n_out * 4 * group)) || (rc = upload_layer(sd, pk, b.data(), sc.data(), sh.data(), CoutPad, a[0])) ||
        (rc = sd.upload(&d_p, &P, sizeof(P)))) return rc;
    if (residual && (rc = sd.alloc(&d_res, n_out * 4))) return rc;
    hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, c->stream, d_in, (long long)n_in, 1u);
    if (d_res) hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, c->stream, d_res, (long long)n_out, 2u);
    a[0].in = d_in; a[0].residual = d_res; a[0].seg_in = d_p->seg[0]; a[0].seg_out = d_p->seg[1]; a[0].seg_up = d_p->seg[1]; a[0].V = V; a[0].Cin = Cin; a[0].Cout = Cout;
    a[0].KH = KH; a[0].KW = KW; a[0].stride = stride; a[0].pad = pad; a[0].relu = relu; a[0].total_mtiles = V * ((Ho * Wo + 127) / 128); a[0].out_ld = Cout; a[0].zeros = c->d_zeros;
    for (int gi = 0; gi < group; gi++) { a[gi] = a[0]; a[gi].out = d_out + (size_t)gi * n_out; }
    auto launch = [&]() { if (group > 1) launch_conv_group(a, group, c->stream); else launch_conv(a[0], c->stream); };
    launch(); launch();
    HIPCHK(hipGetLastError());
    hipEvent_t e0, e1; HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, c->stream));
    for (int i = 0; i < iters; i++) launch();
    HIPCHK(hipEventRecord(e1, c->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (const char* tp = getenv("CALD_CONV_TRACE")) {       // one more launch with the per-workgroup timeline recorded (conv_p4.hip), dumped raw
        const size_t nblk = 1u << 17;
        unsigned long long* d_tr;
        if ((rc = sd.alloc(&d_tr, nblk * 64))) return rc;
        HIPCHK(hipMemsetAsync(d_tr, 0, nblk * 64, c->stream));
        for (int gi = 0; gi < group; gi++) a[gi].trace = d_tr;
        launch();
        HIPCHK(hipStreamSynchronize(c->stream));
        std::vector<unsigned long long> h(nblk * 8);
        HIPCHK(hipMemcpy(h.data(), d_tr, nblk * 64, hipMemcpyDeviceToHost));
        size_t used = nblk; while (used > 0 && h[(used - 1) * 8] == 0) used--;
        if (FILE* f = fopen(tp, "wb")) { fwrite(h.data(), 64, used, f); fclose(f); }
        for (int gi = 0; gi < group; gi++) a[gi].trace = nullptr;
    }
    *ms_out = (double)ms / iters;
    if (tflops_out) *tflops_out = 2.0 * (double)V * Ho * Wo * Cout * (double)K * group / (*ms_out * 1e-3) / 1e12;
    return 0;
}

extern "C" int cald_op_consistency(cald_ctx* c, int N, const float* aug_box, const float* ref_scores_cls, const float* ref_pm,
                                   int M, const float* boxes, const float* scores_cls, const float* pm, int C, float bp,
                                   float* consistency_out) {
    if (!c || !consistency_out || N < 0 || M < 0 || C < 2 || C > 256) return fail(CALD_ERR_INVALID, "bad arguments");
    if (N > 50) return fail(CALD_ERR_INVALID, "at most 50 reference boxes (cald_train.py:110-113)");
    HIPCHK(hipSetDevice(c->device));
    const int cap = (N > M ? N : M) > 0 ? (N > M ? N : M) : 1;
    ScopedDev sd(c->stream); ScopedDet sdet;
    int rc = sdet.alloc(2, cap, C); if (rc) return rc;
    const DetBuffers& d = sdet.d;
    if (N) {
        HIPCHK(hipMemcpy(d.boxes, aug_box, (size_t)N * 16, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.scores_cls, ref_scores_cls, (size_t)N * C * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.prob_max, ref_pm, (size_t)N * 4, hipMemcpyHostToDevice));
    }
    if (M) {
        HIPCHK(hipMemcpy(d.boxes + (size_t)cap * 4, boxes, (size_t)M * 16, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.scores_cls + (size_t)cap * C, scores_cls, (size_t)M * C * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d.prob_max + cap, pm, (size_t)M * 4, hipMemcpyHostToDevice));
    }
    int counts[2] = {N, M};
    HIPCHK(hipMemcpy(d.count, counts, 8, hipMemcpyHostToDevice));
    int h[4 + 50 + 1] = {0};   // ref_view, aug_view, kind, pair_img | ref_sel[50] | ref_n
    h[0] = 0; h[1] = 1; h[2] = 0; h[3] = 0;
    for (int i = 0; i < 50; i++) h[4 + i] = i;
    h[54] = N;
    int* dh; float* dpar; float* dcons;
    if ((rc = sd.upload(&dh, h, sizeof(h))) || (rc = sd.alloc(&dpar, 48)) || (rc = sd.alloc(&dcons, 4))) return rc;
    HIPCHK(hipMemset(dpar, 0, 48));
    ScoreArgs a; a.det = d; a.ref_view = dh; a.aug_view = dh + 1; a.aug_kind = dh + 2; a.pair_img = dh + 3; a.ref_sel = dh + 4; a.ref_n = dh + 54;
    a.aug_param = dpar; a.P = 1; a.bp = bp; a.cons = dcons;
    launch_consistency(a, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(consistency_out, dcons, 4, hipMemcpyDeviceToHost));
    return 0;
}

// one ScopedDev allocation carved by `lay`: a dry Bump for the size, then the real one over it (the forward's arena, in small)
template <typename F> static int carve(ScopedDev& sd, F lay) {
    Bump dry(nullptr, true), real(nullptr, false); lay(dry);
    int rc = sd.alloc(&real.base, dry.off); if (rc) return rc;
    lay(real);
    return 0;
}
// one view's R proposals as the RPN leaves them: CALD_ROI_CAP rows, zero beyond the count
static int put_proposals(const ProposalBufs& P, const float* rois, int R) {
    HIPCHK(hipMemset(P.proposals, 0, (size_t)CALD_ROI_CAP * 16));
    if (R) HIPCHK(hipMemcpy(P.proposals, rois, (size_t)R * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(P.prop_count, &R, 4, hipMemcpyHostToDevice));
    return 0;
}
// the detections of view 0 to the host: the count, refused outside 0..cap (a kernel is wrong), then the arrays (props_out: Faster R-CNN only)
static int download_dets(cald_ctx* c, const DetBuffers& det, const char* what, float* boxes_out, float* scores_out, int64_t* labels_out, float* props_out,
                         float* prob_max_out, float* scores_cls_out, int* n_out) {
    HIPCHK(hipStreamSynchronize(c->stream));
    int n = 0;
    HIPCHK(hipMemcpy(&n, det.count, 4, hipMemcpyDeviceToHost));
    if (n < 0 || n > det.cap) return fail(CALD_ERR_HIP, "%s postprocess returned %d detections (cap %d)", what, n, det.cap);
    if (!n) { *n_out = 0; return 0; }
    HIPCHK(hipMemcpy(boxes_out, det.boxes, (size_t)n * 16, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(scores_out, det.scores, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(labels_out, det.labels, (size_t)n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(prob_max_out, det.prob_max, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(scores_cls_out, det.scores_cls, (size_t)n * det.C * 4, hipMemcpyDeviceToHost));
    if (props_out) HIPCHK(hipMemcpy(props_out, det.props, (size_t)n * 16, hipMemcpyDeviceToHost));
    *n_out = n;       // only once every array has arrived
    return 0;
}

// RoIHeads.postprocess_detections + transform.postprocess of ONE view on the kernels of the forward (roi.hip post_softmax_kernel /
// post_nms_kernel): host arrays in, host arrays out.  Parity hook for detection/frcnn_la.py:32-87, :292-315.
extern "C" int cald_op_frcnn_postprocess(cald_ctx* c, int R, int C, const float* logits, const float* deltas, const float* proposals,
                                         int Hr, int Wr, int Ho, int Wo, float score_thr, float nms_thr, int det_max,
                                         float* boxes_out, float* scores_out, int64_t* labels_out, float* props_out, float* prob_max_out,
                                         float* scores_cls_out, int* n_out) {
    return cald_op_frcnn_postprocess_min(c, R, C, logits, deltas, proposals, Hr, Wr, Ho, Wo, score_thr, nms_thr, det_max, 0.0f, boxes_out, scores_out,
                                         labels_out, props_out, prob_max_out, scores_cls_out, n_out);
}
// the same with the stock tail's remove_small_boxes (cald_model_set_box_min_size; 0 = off)
extern "C" int cald_op_frcnn_postprocess_min(cald_ctx* c, int R, int C, const float* logits, const float* deltas, const float* proposals,
                                             int Hr, int Wr, int Ho, int Wo, float score_thr, float nms_thr, int det_max, float box_min_size,
                                             float* boxes_out, float* scores_out, int64_t* labels_out, float* props_out, float* prob_max_out,
                                             float* scores_cls_out, int* n_out) {
    if (!(box_min_size >= 0.0f)) return fail(CALD_ERR_INVALID, "box_min_size must be >= 0");
    if (!c || !logits || !deltas || !proposals || !boxes_out || !scores_out || !labels_out || !props_out || !prob_max_out || !scores_cls_out || !n_out)
        return fail(CALD_ERR_INVALID, "null argument");
    if (R < 0 || R > CALD_ROI_CAP || C < 2 || C > 256 || det_max < 1 || det_max > 512) return fail(CALD_ERR_INVALID, "bad geometry (R <= %d, 2 <= C <= 256, det_max <= 512)", CALD_ROI_CAP);
    HIPCHK(hipSetDevice(c->device));
    const int ld = 5 * C;
    int key_cap = 1024; while (key_cap < R * (C - 1)) key_cap <<= 1;
    std::vector<float> pred((size_t)CALD_ROI_CAP * ld, 0.0f);
    for (int r = 0; r < R; r++) {
        memcpy(&pred[(size_t)r * ld], logits + (size_t)r * C, (size_t)C * 4);
        memcpy(&pred[(size_t)r * ld + C], deltas + (size_t)r * 4 * C, (size_t)4 * C * 4);
    }
    ViewDesc vd; memset(&vd, 0, sizeof(vd)); vd.Hr = Hr; vd.Wr = Wr; vd.Ho = Ho; vd.Wo = Wo;
    ScopedDev sd(c->stream); ScopedDet det;
    ProposalBufs pb; PostBufs S; float* d_pred; ViewDesc* d_vd; int rc;
    if ((rc = carve(sd, [&](Bump& B) { d_pred = B.get<float>(pred.size()); d_vd = B.get<ViewDesc>(1); pb.layout(B, 1); S.layout(B, 1, C, key_cap); })) ||
        (rc = det.alloc(1, det_max, C)) || (rc = put_proposals(pb, proposals, R))) return rc;
    HIPCHK(hipMemcpy(d_pred, pred.data(), pred.size() * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_vd, &vd, sizeof(vd), hipMemcpyHostToDevice));
    PostArgs pa = post_args(S, d_pred, ld, C, 1, pb, d_vd, score_thr, nms_thr, det.d);
    pa.min_box = box_min_size;
    launch_frcnn_postprocess(pa, c->stream);
    HIPCHK(hipGetLastError());
    return download_dets(c, det.d, "frcnn", boxes_out, scores_out, labels_out, props_out, prob_max_out, scores_cls_out, n_out);
}

// one view's predictor rows as the forward's box head leaves them: CALD_ROI_CAP rows of [C logits | 4 C deltas], zero beyond R
static std::vector<float> pack_pred(int R, int C, const float* logits, const float* deltas) {
    const int ld = 5 * C;
    std::vector<float> pred((size_t)CALD_ROI_CAP * ld, 0.0f);
    for (int r = 0; r < R; r++) {
        memcpy(&pred[(size_t)r * ld], logits + (size_t)r * C, (size_t)C * 4);
        memcpy(&pred[(size_t)r * ld + C], deltas + (size_t)r * 4 * C, (size_t)4 * C * 4);
    }
    return pred;
}
// RoIHeads.ssm_postprocess_detections + transform.postprocess of ONE view on the kernels of the SSM forward (ssm.hip), through the forward's
// own SsmBufs::layout and ssm_args: host arrays in, host arrays out.  Parity hook for detection/frcnn_ssm.py:44-102, :367, :400.
extern "C" int cald_op_ssm_postprocess(cald_ctx* c, int R, int C, const float* logits, const float* deltas, const float* proposals,
                                       int Hr, int Wr, int Ho, int Wo, float score_thr, int det_max,
                                       int* al_out, int* n_out, float* boxes_out, float* scores_out, int8_t* labels_out) {
    if (!c || !logits || !deltas || !proposals || !al_out || !n_out || !boxes_out || !scores_out || !labels_out) return fail(CALD_ERR_INVALID, "null argument");
    if (R < 0 || R > CALD_ROI_CAP || C < 2 || C > 256 || det_max < 1 || det_max > 512 || Hr < 1 || Wr < 1 || Ho < 1 || Wo < 1)
        return fail(CALD_ERR_INVALID, "bad geometry (R <= %d, 2 <= C <= 256, det_max <= 512, positive sizes)", CALD_ROI_CAP);
    HIPCHK(hipSetDevice(c->device));
    const std::vector<float> pred = pack_pred(R, C, logits, deltas);
    ViewDesc vd; memset(&vd, 0, sizeof(vd)); vd.Hr = Hr; vd.Wr = Wr; vd.Ho = Ho; vd.Wo = Wo;
    ScopedDev sd(c->stream);
    ProposalBufs pb; SsmBufs S; float* d_pred; ViewDesc* d_vd; int rc;
    if ((rc = carve(sd, [&](Bump& B) { d_pred = B.get<float>(pred.size()); d_vd = B.get<ViewDesc>(1); pb.layout(B, 1); S.layout(B, 1, C, det_max); })) ||
        (rc = put_proposals(pb, proposals, R))) return rc;
    HIPCHK(hipMemcpy(d_pred, pred.data(), pred.size() * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_vd, &vd, sizeof(vd), hipMemcpyHostToDevice));
    launch_ssm_postprocess(ssm_args(S, d_pred, 5 * C, C, 1, pb, d_vd, score_thr, det_max), c->stream);
    HIPCHK(hipGetLastError());
    int al = 0, n = 0, total = 0, cap = (C - 1) * det_max;
    if ((rc = ssm_collect_rows(c->stream, "ssm", 0, S.rows(), 1, (size_t)C - 1, (size_t)C - 1, cap, 0, cap, &al, &n, boxes_out, scores_out, labels_out, &total))) return rc;
    *al_out = al; *n_out = n;
    return 0;
}

// One view's RetinaNet heads for the two tail hooks below: the argument checks, the one-view plan (level 0: the padded input; levels 3..7:
// P3..P7), and the device copies of heads, plan, view and base anchors
struct RetinaHookIn {
    BatchPlan P; ViewDesc vd; size_t pix[5]; long long anchors = 0;
    BatchPlan* d_p = nullptr; ViewDesc* d_vd = nullptr; float *d_cls[5] = {}, *d_reg[5] = {}, *d_base = nullptr;
    int check(const float* const* cls, const float* const* reg, const int* level_hw, int A, int K, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo, int per_class) {
        if (A < 1 || A > 64 || K < 1 || K > 256 || per_class < 1 || per_class > 1024 || Hp < 1 || Wp < 1 || Hr < 1 || Wr < 1 || Ho < 1 || Wo < 1)
            return fail(CALD_ERR_INVALID, "bad geometry (1 <= A <= 64, 1 <= K <= 256, 1 <= per_class <= 1024, positive sizes)");
        memset(&P, 0, sizeof(P));
        P.seg[0][0].H = Hp; P.seg[0][0].W = Wp; P.seg[0][1].pix_off = (long long)Hp * Wp;
        for (int l = 0; l < 5; l++) {
            const int H = level_hw[2 * l], W = level_hw[2 * l + 1];
            if (H < 1 || W < 1 || H > Hp || W > Wp || !cls[l] || !reg[l]) return fail(CALD_ERR_INVALID, "level %d is malformed", l);
            P.seg[3 + l][0].H = H; P.seg[3 + l][0].W = W; P.seg[3 + l][1].pix_off = (long long)H * W; pix[l] = (size_t)H * W;
            anchors += (long long)H * W * A;
        }
        if (anchors > (1 << 20)) return fail(CALD_ERR_INVALID, "at most %d anchors", 1 << 20);
        memset(&vd, 0, sizeof(vd)); vd.Hr = Hr; vd.Wr = Wr; vd.Ho = Ho; vd.Wo = Wo;
        return 0;
    }
    void layout(Bump& B, int A, int K) {
        for (int l = 0; l < 5; l++) { d_cls[l] = B.get<float>(pix[l] * A * K); d_reg[l] = B.get<float>(pix[l] * A * 4); }
        d_p = B.get<BatchPlan>(1); d_vd = B.get<ViewDesc>(1); d_base = B.get<float>((size_t)5 * A * 4);
    }
    int upload(const float* const* cls, const float* const* reg, const float* base_anchors, int A, int K) {
        for (int l = 0; l < 5; l++) {
            HIPCHK(hipMemcpy(d_cls[l], cls[l], pix[l] * A * K * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_reg[l], reg[l], pix[l] * A * 16, hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemcpy(d_p, &P, sizeof(P), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_vd, &vd, sizeof(vd), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_base, base_anchors, (size_t)5 * A * 16, hipMemcpyHostToDevice));
        return 0;
    }
};

// RetinaNet.postprocess_detections + the stock transform.postprocess of ONE view on the kernels of the forward (retina.hip
// retina_cand_kernel / retina_class_nms_kernel / retina_emit_kernel): host arrays in, host arrays out, through the forward's own
// RetinaTailBufs::layout and retina_args (host.h); det cap K * per_class.  Parity hook for detection/retinanet_cal.py:402-490.
extern "C" int cald_op_retina_postprocess(cald_ctx* c, const float* const* cls, const float* const* reg, const int* level_hw, int A, int K,
                                          const float* base_anchors, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo,
                                          float score_thr, float nms_thr, int per_class,
                                          float* boxes_out, float* scores_out, int64_t* labels_out, float* prob_max_out,
                                          float* scores_cls_out, int* n_out) {
    if (!c || !cls || !reg || !level_hw || !base_anchors || !boxes_out || !scores_out || !labels_out || !prob_max_out || !scores_cls_out || !n_out)
        return fail(CALD_ERR_INVALID, "null argument");
    RetinaHookIn in; int rc;
    if ((rc = in.check(cls, reg, level_hw, A, K, Hp, Wp, Hr, Wr, Ho, Wo, per_class))) return rc;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream); ScopedDet det;
    RetinaTailBufs S;
    if ((rc = carve(sd, [&](Bump& B) { in.layout(B, A, K); S.layout(B, 1, K, per_class, (int)in.anchors); })) || (rc = det.alloc(1, K * per_class, K)) ||
        (rc = in.upload(cls, reg, base_anchors, A, K))) return rc;
    launch_retina_postprocess(retina_args(S, in.d_cls, in.d_reg, in.d_p, in.d_vd, in.d_base, A, K, 1, score_thr, nms_thr, per_class, det.d), S.max_anchors, c->stream);
    HIPCHK(hipGetLastError());
    return download_dets(c, det.d, "retina", boxes_out, scores_out, labels_out, nullptr, prob_max_out, scores_cls_out, n_out);
}

// The stock tail of ONE view as above, then the view's decision margins (audit.hip launch_audit_retina) in the public CALD_MARGIN_* numbering.
extern "C" int cald_op_retina_audit(cald_ctx* c, const float* const* cls, const float* const* reg, const int* level_hw, int A, int K,
                                    const float* base_anchors, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo,
                                    float score_thr, float nms_thr, int per_class, int* n_out, float* margins_out) {
    if (!c || !cls || !reg || !level_hw || !base_anchors || !n_out || !margins_out) return fail(CALD_ERR_INVALID, "null argument");
    RetinaHookIn in; int rc;
    if ((rc = in.check(cls, reg, level_hw, A, K, Hp, Wp, Hr, Wr, Ho, Wo, per_class))) return rc;
    if (per_class > AUDIT_MAX_DET) return fail(CALD_ERR_UNSUPPORTED, "the decision-margin audit holds a class's detections in LDS: per_class <= %d (AUDIT_MAX_DET)", AUDIT_MAX_DET);
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream); ScopedDet det;
    RetinaTailBufs S; float* d_vm = nullptr;
    if ((rc = carve(sd, [&](Bump& B) { in.layout(B, A, K); S.layout(B, 1, K, per_class, (int)in.anchors); d_vm = B.get<float>(CALD_VM); })) ||
        (rc = det.alloc(1, K * per_class, K)) || (rc = in.upload(cls, reg, base_anchors, A, K))) return rc;
    const RetinaArgs ra = retina_args(S, in.d_cls, in.d_reg, in.d_p, in.d_vd, in.d_base, A, K, 1, score_thr, nms_thr, per_class, det.d);
    launch_retina_postprocess(ra, S.max_anchors, c->stream);
    launch_audit_retina(ra, d_vm, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    float vm[CALD_VM];
    HIPCHK(hipMemcpy(vm, d_vm, sizeof(vm), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_out, det.d.count, sizeof(int), hipMemcpyDeviceToHost));
    for (int q = 0; q < CALD_N_MARGINS; q++) margins_out[q] = INFINITY;
    for (int q = VM_POST_THR; q <= VM_POST_CAP; q++) margins_out[q] = vm[q];
    margins_out[CALD_MARGIN_POST_SMALL] = vm[VM_POST_SMALL];
    margins_out[CALD_MARGIN_REF_SUBSAMPLE] = vm[VM_POST_SUBORDER];
    margins_out[CALD_MARGIN_ZERO_ROW] = vm[VM_POST_TOP2];
    return 0;
}

// RetinaNet.ssm_postprocess_detections + the stock transform.postprocess of ONE view on the kernels of the SSM forward (retina_ssm.hip), through
// the forward's own RetinaSsmBufs::layout, retina_ssm_args and host stop.  Parity hook for detection/retina_ssm.py:487-584.
extern "C" int cald_op_retina_ssm_postprocess(cald_ctx* c, const float* const* cls, const float* const* reg, const int* level_hw, int A, int K,
                                              const float* base_anchors, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo,
                                              float score_thr, float nms_thr, int per_class, cald_ssm_pick_fn pick, void* user,
                                              int* al_out, int* n_out, int* counts_out, float* boxes_out, float* scores_out, int8_t* labels_out) {
    if (!c || !cls || !reg || !level_hw || !base_anchors || !pick || !al_out || !n_out || !counts_out || !boxes_out || !scores_out || !labels_out)
        return fail(CALD_ERR_INVALID, "null argument");
    if (K < 2) return fail(CALD_ERR_INVALID, "the RetinaNet SSM tail needs K >= 2 (labels have K - 1 columns)");
    RetinaHookIn in; int rc;
    if ((rc = in.check(cls, reg, level_hw, A, K, Hp, Wp, Hr, Wr, Ho, Wo, per_class))) return rc;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    RetinaSsmBufs S;
    if ((rc = carve(sd, [&](Bump& B) { in.layout(B, A, K); S.layout(B, 1, K, per_class, (int)in.anchors); })) || (rc = in.upload(cls, reg, base_anchors, A, K))) return rc;
    const RetinaSsmArgs sa = retina_ssm_args(S, in.d_cls, in.d_reg, in.d_p, in.d_vd, in.d_base, A, K, 1, score_thr, nms_thr, per_class);
    launch_retina_ssm_phase_a(sa, c->stream);
    HIPCHK(hipGetLastError());
    if ((rc = retina_ssm_pick_stop(c, S, 1, K, pick, user, 0, counts_out))) return rc;
    launch_retina_ssm_phase_b(sa, c->stream);
    HIPCHK(hipGetLastError());
    int al = 0, n = 0, total = 0, cap = K * per_class;
    if ((rc = ssm_collect_rows(c->stream, "retina ssm", 0, S.rows(), 1, 1, (size_t)K - 1, cap, 0, cap, &al, &n, boxes_out, scores_out, labels_out, &total))) return rc;
    if (al) memset(counts_out, 0, (size_t)K * 4);
    *al_out = al; *n_out = n;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// test-only probe of the certified pruning (tests/test_gpu_rpn_prune_edges.py): one RpnPruneArgs and what ForwardRun::rpn_pruned runs with
// it, in its order -- select stage 0, select stage 1, scatter -- with the gathered exact convs between them PLAYED by the host: after each
// select, nsel / row_map come back, that stage's head_rows are gathered from the caller's dense exact map (compact per view at the view's
// pixel offset; NaN past nsel, so a row read beyond the count shows in check[0]) and go up again.  A count or a row index outside its view
// is refused before anything reads through it.  In / out arrays travel whole, guard words included (the header has the layout).
// ---------------------------------------------------------------------------------------------
extern "C" int cald_op_rpn_prune(cald_ctx* c, cald_rpn_prune_probe* p) {
    if (!c || !p) return fail(CALD_ERR_INVALID, "cald_op_rpn_prune: null argument");
    if (p->V < 1 || p->V > CALD_PRUNE_PROBE_MAX_VIEWS || p->guard < 0 || p->guard > 4096 || p->head_ld < 3 || p->head_ld > 64 || p->pre_n < 1)
        return fail(CALD_ERR_INVALID, "cald_op_rpn_prune: 1..%d views, guard 0..4096, head_ld 3..64, pre_n >= 1", CALD_PRUNE_PROBE_MAX_VIEWS);
    const int V = p->V, ld = p->head_ld; const size_t G = (size_t)p->guard;
    constexpr int SV = CALD_PRUNE_PROBE_MAX_VIEWS + 1;
    LevelSeg seg[2 * SV]; memset(seg, 0, sizeof(seg));
    size_t pix[2]; int max_pix = 0;                 // the select kernels' mask holds one bit per pixel of the largest view of EITHER level
    for (int l = 0; l < 2; l++) {
        for (int v = 0; v < V; v++) {
            const int H = p->hw[l][v][0], W = p->hw[l][v][1];
            if (H < 1 || W < 1 || (long long)H * W > (1 << 19)) return fail(CALD_ERR_INVALID, "cald_op_rpn_prune: level %d view %d: 1 <= H * W <= 2^19", l, v);
            seg[l * SV + v].H = H; seg[l * SV + v].W = W; seg[l * SV + v + 1].pix_off = seg[l * SV + v].pix_off + (long long)H * W;
            if (H * W > max_pix) max_pix = H * W;
        }
        pix[l] = (size_t)seg[l * SV + V].pix_off;
        if (!p->energy[l] || !p->exact[l] || !p->head[l] || !p->pnorm[l]) return fail(CALD_ERR_INVALID, "cald_op_rpn_prune: level %d: null array", l);
    }
    for (int s = 0; s < 2; s++) if (!p->nsel[s] || !p->row_map[s][0] || !p->row_map[s][1] || !p->tau_key) return fail(CALD_ERR_INVALID, "cald_op_rpn_prune: null output array");
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    RpnPruneArgs pr; memset(&pr, 0, sizeof(pr));
    const LevelSeg* d_seg; float* d_rows[2][2]; int rc;
    const size_t nw = (size_t)2 * V + G;
    if ((rc = sd.upload(&d_seg, seg, sizeof(seg))) || (rc = sd.upload(&pr.tau_key, p->tau_key, nw * 4)) || (rc = sd.upload(&pr.check, p->check, 8)) ||
        (rc = sd.alloc(&pr.stat, 32))) return rc;
    HIPCHK(hipMemset(pr.stat, 0, 32));
    for (int l = 0; l < 2; l++) {
        pr.seg[l] = d_seg + l * SV;
        if ((rc = sd.upload(&pr.energy[l], p->energy[l], pix[l] * 16)) || (rc = sd.upload(&pr.pnorm[l], p->pnorm[l], (pix[l] + G) * 4)) ||
            (rc = sd.upload(&pr.head_out[l], p->head[l], (pix[l] + G) * ld * 4))) return rc;
        pr.head[l] = pr.head_out[l];
        for (int s = 0; s < 2; s++) {
            if ((rc = sd.upload(&pr.row_map[s][l], p->row_map[s][l], (pix[l] + G) * 4)) || (rc = sd.alloc(&d_rows[s][l], pix[l] * ld * 4))) return rc;
            pr.head_rows[s][l] = d_rows[s][l];
        }
    }
    for (int s = 0; s < 2; s++) if ((rc = sd.upload(&pr.nsel[s], p->nsel[s], nw * 4))) return rc;
    for (int q = 0; q < 3; q++) { pr.c1[q] = p->c1[q]; pr.c0[q] = p->c0[q]; }
    pr.head_ld = ld; pr.pre_n = p->pre_n; pr.V = V;
    auto maps_back = [&](int s) {
        HIPCHK(hipMemcpy(p->nsel[s], pr.nsel[s], nw * 4, hipMemcpyDeviceToHost));
        for (int l = 0; l < 2; l++) HIPCHK(hipMemcpy(p->row_map[s][l], pr.row_map[s][l], (pix[l] + G) * 4, hipMemcpyDeviceToHost));
        return 0;
    };
    for (int s = 0; s < 2; s++) {
        launch_rpn_prune_select(pr, max_pix, s, c->stream);
        HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->stream));
        if ((rc = maps_back(s))) return rc;
        if (s == 0) HIPCHK(hipMemcpy(p->tau_key, pr.tau_key, nw * 4, hipMemcpyDeviceToHost));
        for (int l = 0; l < 2; l++) {       // the gathered exact conv + head of this stage
            std::vector<float> rows(pix[l] * ld, NAN);
            for (int v = 0; v < V; v++) {
                const LevelSeg& sg = seg[l * SV + v];
                const int npx = sg.H * sg.W, ns = p->nsel[s][l * V + v];
                if (ns < 0 || ns > npx) return fail(CALD_ERR_HIP, "cald_op_rpn_prune: stage %d level %d view %d selected %d of %d pixels", s, l, v, ns, npx);
                for (int r = 0; r < ns; r++) {
                    const int px = p->row_map[s][l][sg.pix_off + r];
                    if (px < 0 || px >= npx) return fail(CALD_ERR_HIP, "cald_op_rpn_prune: stage %d level %d view %d row %d maps to pixel %d of %d", s, l, v, r, px, npx);
                    memcpy(&rows[(size_t)(sg.pix_off + r) * ld], p->exact[l] + (size_t)(sg.pix_off + px) * ld, (size_t)ld * 4);
                }
            }
            HIPCHK(hipMemcpy(d_rows[s][l], rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        }
    }
    launch_rpn_prune_scatter(pr, max_pix, c->stream);
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->stream));
    for (int s = 0; s < 2; s++) if ((rc = maps_back(s))) return rc;          // once more, whole: neither a later select nor the scatter may have touched them
    for (int l = 0; l < 2; l++) {
        HIPCHK(hipMemcpy(p->head[l], pr.head_out[l], (pix[l] + G) * ld * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(p->pnorm[l], pr.pnorm[l], (pix[l] + G) * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(p->check, pr.check, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(p->stat, pr.stat, 32, hipMemcpyDeviceToHost));
    return 0;
}

// MultiScaleRoIAlign(7, sampling_ratio 2) of ONE view on the inference kernels (roi.hip): feats[l] = host [H_l][W_l][C] for the four
// levels P2..P5 (level_hw = {H0, W0, ..., H3, W3}), rois [R][4] in image coordinates, out [R][49][C] (host).  C == 256 runs the
// row-walk kernel, other C (multiple of 4) the gather kernel.  Parity hook for detection/frcnn_la.py:205-209.
extern "C" int cald_op_roi_align(cald_ctx* c, const float* const* feats, const int* level_hw, int C, int R, const float* rois, float* out) {
    if (!c || !feats || !level_hw || !rois || !out) return fail(CALD_ERR_INVALID, "null argument");
    if (R < 1 || R > CALD_ROI_CAP || C < 4 || C % 4) return fail(CALD_ERR_INVALID, "bad geometry (1 <= R <= %d, C a positive multiple of 4)", CALD_ROI_CAP);
    HIPCHK(hipSetDevice(c->device));
    BatchPlan P; memset(&P, 0, sizeof(P));
    size_t pix[4];
    for (int l = 0; l < 4; l++) {
        const int H = level_hw[2 * l], W = level_hw[2 * l + 1];
        if (H < 1 || W < 1 || !feats[l]) return fail(CALD_ERR_INVALID, "level %d is malformed", l);
        P.seg[2 + l][0].H = H; P.seg[2 + l][0].W = W; P.seg[2 + l][1].pix_off = (long long)H * W; pix[l] = (size_t)H * W;
    }
    ScopedDev sd(c->stream);
    ProposalBufs pb; RoiBufs S; float* d_f[4]; BatchPlan* d_p; int rc;
    if ((rc = carve(sd, [&](Bump& B) { for (int l = 0; l < 4; l++) d_f[l] = B.get<float>(pix[l] * C); d_p = B.get<BatchPlan>(1); pb.layout(B, 1); S.layout(B, 1, C); })) ||
        (rc = put_proposals(pb, rois, R))) return rc;
    for (int l = 0; l < 4; l++) HIPCHK(hipMemcpy(d_f[l], feats[l], pix[l] * C * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_p, &P, sizeof(P), hipMemcpyHostToDevice));
    launch_roi_align(roi_args(S, d_f, d_p, C, 1, pb, false), c->stream);
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, S.roi, (size_t)R * 49 * C * 4, hipMemcpyDeviceToHost));
    return 0;
}
// The same stage on V views at once, in the forward's own layout: the views' maps of a level share one buffer (BatchPlan::seg carries each
// view's size and pixel offset), proposals and output rows have CALD_ROI_CAP slots a view.  feats[4 v + l] = host [H][W][C] of view v's
// level l, level_hw [V][4][2], rois = the views' RoIs one after the other (counts[v] rows each).  out [V][rows_back][49][C] 32-bit words
// goes up into the first rows_back rows of each view's slot before the launch and comes back after it, so rows from counts[v] on show
// whether anything wrote them.  kernel 0: what the forward runs, 1: the gather kernel at any C.  order_out (optional) [V][1024].
extern "C" int cald_op_roi_align_views(cald_ctx* c, int V, const float* const* feats, const int* level_hw, const int* counts, const float* rois,
                                       int C, int out16, int kernel, int rows_back, uint32_t* out, int* order_out) {
    if (!c || !feats || !level_hw || !counts || !rois || !out) return fail(CALD_ERR_INVALID, "null argument");
    if (V < 1 || V > CALD_MAX_VIEWS || C < 4 || C > 1024 || C % 4 || (out16 && C % 16) || (out16 != 0 && out16 != 1) || (kernel != 0 && kernel != 1) ||
        rows_back < 1 || rows_back > CALD_ROI_CAP)
        return fail(CALD_ERR_INVALID, "bad geometry (1 <= V <= %d, C a multiple of 4 (16 in split form) up to 1024, out16 and kernel 0 or 1, 1 <= rows_back <= %d)",
                    CALD_MAX_VIEWS, CALD_ROI_CAP);
    BatchPlan P; memset(&P, 0, sizeof(P));
    size_t total = 0;
    for (int v = 0; v < V; v++) {
        if (counts[v] < 0 || counts[v] > CALD_ROI_CAP) return fail(CALD_ERR_INVALID, "view %d: count %d outside 0..%d", v, counts[v], CALD_ROI_CAP);
        total += (size_t)counts[v];
        for (int l = 0; l < 4; l++) {
            const int H = level_hw[(v * 4 + l) * 2], W = level_hw[(v * 4 + l) * 2 + 1];
            if (H < 1 || W < 1 || (long long)H * W > (1 << 22) || !feats[v * 4 + l]) return fail(CALD_ERR_INVALID, "view %d: level %d is malformed", v, l);
            P.seg[2 + l][v].H = H; P.seg[2 + l][v].W = W; P.seg[2 + l][v + 1].pix_off = P.seg[2 + l][v].pix_off + (long long)H * W;
        }
    }
    for (size_t i = 0; i < total * 4; i++) if (!std::isfinite(rois[i])) return fail(CALD_ERR_INVALID, "RoI %zu has a non-finite coordinate", i / 4);
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    ProposalBufs pb; RoiBufs S; float* d_f[4]; BatchPlan* d_p; int rc;
    if ((rc = carve(sd, [&](Bump& B) { for (int l = 0; l < 4; l++) d_f[l] = B.get<float>((size_t)level_pix(P, 2 + l, V) * C); d_p = B.get<BatchPlan>(1);
                                       pb.layout(B, V); S.layout(B, V, C); }))) return rc;
    HIPCHK(hipMemset(pb.proposals, 0, (size_t)V * CALD_ROI_CAP * 16));
    const size_t row = (size_t)49 * C;
    for (size_t v = 0, at = 0; v < (size_t)V; at += (size_t)counts[v], v++) {
        if (counts[v]) HIPCHK(hipMemcpy(pb.proposals + v * CALD_ROI_CAP * 4, rois + at * 4, (size_t)counts[v] * 16, hipMemcpyHostToDevice));
        for (int l = 0; l < 4; l++) {
            const LevelSeg& sg = P.seg[2 + l][v];
            HIPCHK(hipMemcpy(d_f[l] + (size_t)sg.pix_off * C, feats[v * 4 + l], (size_t)sg.H * sg.W * C * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemcpy(S.roi + v * CALD_ROI_CAP * row, out + v * rows_back * row, (size_t)rows_back * row * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(pb.prop_count, counts, (size_t)V * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_p, &P, sizeof(P), hipMemcpyHostToDevice));
    launch_roi_align(roi_args(S, d_f, d_p, C, V, pb, out16 != 0), c->stream, kernel);
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t v = 0; v < (size_t)V; v++)
        HIPCHK(hipMemcpy(out + v * rows_back * row, S.roi + v * CALD_ROI_CAP * row, (size_t)rows_back * row * 4, hipMemcpyDeviceToHost));
    if (order_out) HIPCHK(hipMemcpy(order_out, S.order, (size_t)V * 1024 * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int cald_op_cls_corr(cald_ctx* c, int n, const float* scores, const int64_t* labels, int C, float* out) {
    if (!c || !out || n < 0 || C < 2 || C > 256) return fail(CALD_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream); ScopedDet sdet;
    int rc = sdet.alloc(1, n > 0 ? n : 1, C); if (rc) return rc;
    const DetBuffers& d = sdet.d;
    if (n) { HIPCHK(hipMemcpy(d.scores, scores, (size_t)n * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d.labels, labels, (size_t)n * 8, hipMemcpyHostToDevice)); }
    HIPCHK(hipMemcpy(d.count, &n, 4, hipMemcpyHostToDevice));
    int h[2] = {0, 0}; int* dh; float* dout;
    if ((rc = sd.upload(&dh, h, 8)) || (rc = sd.alloc(&dout, (size_t)(C - 1) * 4))) return rc;
    launch_cls_corr(d, nullptr, nullptr, dh, dh + 1, 1, dout, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, dout, (size_t)(C - 1) * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The scoring stage of one sweep batch: the tables through PairLayout as the sweeps fill them, then score.hip's five launches.
extern "C" int cald_op_score_batch(cald_ctx* c, cald_score_probe* q) {
    if (!c || !q) return fail(CALD_ERR_INVALID, "null argument");
    const int V = q->V, cap = q->cap, C = q->C, B = q->n_img, P = q->P;
    if (!q->boxes || !q->props || !q->scores || !q->labels || !q->scores_cls || !q->prob_max || !q->count || !q->view_img || !q->view_isref ||
        !q->ref_sel || !q->ref_n || !q->ref_view || !q->aug_view || !q->pair_img || !q->aug_kind || !q->aug_param ||
        !q->cons || !q->cls_corr || !q->pair_audit || !q->max_iou || !q->lt) return fail(CALD_ERR_INVALID, "null argument");
    if (C < 2 || C > 256) return fail(CALD_ERR_INVALID, "C %d outside 2..256", C);
    if (V < 1 || V > CALD_MAX_VIEWS || cap < 1 || B < 1 || P < 0) return fail(CALD_ERR_INVALID, "bad geometry (1 <= V <= %d, cap >= 1, n_img >= 1, P >= 0)", CALD_MAX_VIEWS);
    for (int v = 0; v < V; v++) {
        if (q->count[v] < 0 || q->count[v] > cap) return fail(CALD_ERR_INVALID, "view %d: count %d outside 0..%d", v, q->count[v], cap);
        if (q->view_img[v] < 0 || q->view_img[v] >= B) return fail(CALD_ERR_INVALID, "view %d: image %d out of range", v, q->view_img[v]);
    }
    for (int i = 0; i < B; i++) {
        if (q->ref_n[i] < 0 || q->ref_n[i] > 50) return fail(CALD_ERR_INVALID, "image %d: ref_n %d outside 0..50 (cald_train.py:110-113)", i, q->ref_n[i]);
        for (int k = 0; k < q->ref_n[i]; k++)
            if (q->ref_sel[i * 50 + k] < 0 || q->ref_sel[i * 50 + k] >= cap) return fail(CALD_ERR_INVALID, "image %d: ref_sel[%d] = %d outside 0..%d", i, k, q->ref_sel[i * 50 + k], cap - 1);
    }
    for (int p = 0; p < P; p++) {
        if (q->ref_view[p] < 0 || q->ref_view[p] >= V || q->aug_view[p] < 0 || q->aug_view[p] >= V) return fail(CALD_ERR_INVALID, "pair %d: view out of range", p);
        if (q->pair_img[p] < 0 || q->pair_img[p] >= B) return fail(CALD_ERR_INVALID, "pair %d: image %d out of range", p, q->pair_img[p]);
        if (q->aug_kind[p] < 0 || q->aug_kind[p] > 3) return fail(CALD_ERR_INVALID, "pair %d: unknown aug_kind %d", p, q->aug_kind[p]);
    }
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream); ScopedDet sdet;
    int rc = sdet.alloc(V, cap, C); if (rc) return rc;
    const DetBuffers& D = sdet.d;
    const size_t rows = (size_t)V * cap;
    HIPCHK(hipMemcpy(D.boxes, q->boxes, rows * 16, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(D.props, q->props, rows * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.scores, q->scores, rows * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(D.labels, q->labels, rows * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.scores_cls, q->scores_cls, rows * C * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(D.prob_max, q->prob_max, rows * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.count, q->count, (size_t)V * 4, hipMemcpyHostToDevice));
    const PairLayout lay{P > 0 ? P : 1, B, V};
    std::vector<int> ints(lay.n_ints(), 0);
    const PairLayout::Ptrs hp = lay.at(ints.data());
    for (int p = 0; p < P; p++) { hp.ref_view[p] = q->ref_view[p]; hp.aug_view[p] = q->aug_view[p]; hp.aug_kind[p] = q->aug_kind[p]; hp.pair_img[p] = q->pair_img[p]; }
    memcpy(hp.ref_sel, q->ref_sel, (size_t)B * 50 * 4); memcpy(hp.ref_n, q->ref_n, (size_t)B * 4);
    memcpy(hp.view_img, q->view_img, (size_t)V * 4); memcpy(hp.view_isref, q->view_isref, (size_t)V * 4);
    int* d_ints; float *d_par, *d_cons, *d_clsc, *d_pm, *d_rows, *d_lt;
    if ((rc = sd.upload(&d_ints, ints.data(), ints.size() * 4)) || (rc = sd.alloc(&d_par, (size_t)P * 12 * 4)) || (rc = sd.alloc(&d_cons, (size_t)P * 4)) ||
        (rc = sd.alloc(&d_clsc, (size_t)V * (C - 1) * 4)) || (rc = sd.alloc(&d_pm, (size_t)P * 2 * 4)) || (rc = sd.alloc(&d_rows, (size_t)P * 50 * 4)) ||
        (rc = sd.alloc(&d_lt, (size_t)V * 4))) return rc;
    if (P) HIPCHK(hipMemcpy(d_par, q->aug_param, (size_t)P * 12 * 4, hipMemcpyHostToDevice));
    const PairLayout::Ptrs dp = lay.at(d_ints);
    const ScoreArgs sa = lay.score_args(d_ints, D, d_par, P, q->bp, d_cons);
    launch_consistency(sa, c->stream);
    launch_cls_corr(D, dp.ref_sel, dp.ref_n, dp.view_img, dp.view_isref, V, d_clsc, c->stream);
    launch_pair_audit(sa, d_pm, c->stream);
    launch_max_iou(sa, d_rows, c->stream);
    launch_lt_uncertainty(D, V, d_lt, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<float> h_rows((size_t)P * 50);
    if (P) {
        HIPCHK(hipMemcpy(q->cons, d_cons, (size_t)P * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(q->pair_audit, d_pm, (size_t)P * 2 * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_rows.data(), d_rows, (size_t)P * 50 * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(q->cls_corr, d_clsc, (size_t)V * (C - 1) * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(q->lt, d_lt, (size_t)V * 4, hipMemcpyDeviceToHost));
    for (int p = 0; p < P; p++) memcpy(q->max_iou + (size_t)p * 50, &h_rows[(size_t)p * 50], (size_t)q->ref_n[q->pair_img[p]] * 4);      // the kernel writes the live slots only
    return 0;
}

extern "C" int cald_op_pair_params(int kind, int H, int W, double param, float* par12_out) {
    if (!par12_out || kind < 0 || kind > 3 || H < 1 || W < 1) return fail(CALD_ERR_INVALID, "bad argument (kind 0..3, H, W >= 1)");
    pair_params(kind, H, W, param, par12_out);
    return 0;
}

extern "C" int cald_op_ls_tail(int n, const float* prob_max, int n_rows, const float* max_iou, int* sel_out, int* n_sel_out, double* score_out) {
    if (n < 0 || n_rows < 0 || (n && !prob_max) || !sel_out || !n_sel_out || (score_out && n && n_rows && !max_iou)) return fail(CALD_ERR_INVALID, "bad argument");
    const int N = ls_select(n, prob_max, sel_out);
    *n_sel_out = N;
    if (!score_out) return 0;
    std::vector<float> pm(N); std::vector<const float*> rows(n_rows);
    for (int k = 0; k < N; k++) pm[k] = prob_max[sel_out[k]];
    for (int r = 0; r < n_rows; r++) rows[r] = max_iou + (size_t)r * N;
    *score_out = ls_tail(N, pm.data(), n_rows, rows.data());
    return 0;
}
