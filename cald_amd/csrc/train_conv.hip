// train_conv.hip -- the inference kernels on a dense batch (task_model(images, targets) in train mode, cald_train.py:40-74): forward conv /
// linear layers (on conv_h3.hip / conv_h4.hip where the caller hands in the pack's split twin) and their data gradients (conv_p4.hip / conv_mfma.hip on the packs of train_pack.hip,
// or conv_h3.hip on a data-gradient pack's split twin with a per-tensor input scale -- cald_train_conv_dgrad_f16x3; a stride-2 layer's dY is first
// scattered onto the stride-1 grid, train_elementwise.hip), and the input side of the training forward: GeneralizedRCNNTransform
// (normalize, bilinear resize, zero-pad to the batch size), the stem's max-pool and LastLevelMaxPool on the kernels of elementwise.hip.
// Activations are dense NHWC batches [N][H][W][C].
#include "train_host.h"

// ConvArgs of one problem of a dense batch: the three parts of its packed buffer (g: the buffer's geometry; flags: which epilogue vectors the
// layer reads), the geometry tables of its input and output, no residual / up-sampled addend / mask.
static int conv_args(cald_ctx* c, ConvArgs& a, const PackGeom& g, const float* packed, int flags, int N, int H, int W, int Ho, int Wo, int kh, int kw,
                     int stride, int pad, const float* in, float* out, int out_ld) {
    const LevelSeg *si, *so;
    if (int rc = dense_seg(c, N, H, W, &si)) return rc;
    if (int rc = dense_seg(c, N, Ho, Wo, &so)) return rc;
    const long long n = (long long)g.Kpad * g.NPad;
    memset(&a, 0, sizeof(a));
    a.in = in; a.out = out; a.w = packed; a.w4 = packed + n;
    const float* vec = packed + 2 * n;
    a.bias = (flags & 1) ? vec : nullptr; a.scale = (flags & 2) ? vec + g.NPad : nullptr; a.shift = (flags & 2) ? vec + 2 * g.NPad : nullptr;
    a.seg_in = si; a.seg_out = so; a.seg_up = so;
    a.V = N; a.Cin = g.cin_conv; a.Cout = g.n_true; a.CoutPad = g.NPad; a.Kpad = g.Kpad; a.KH = kh; a.KW = kw; a.stride = stride; a.pad = pad;
    a.relu = (flags & 4) ? 1 : 0; a.total_mtiles = N * ((Ho * Wo + 127) / 128); a.out_ld = out_ld; a.zeros = cald_internal_zeros(c);
    return 0;
}
// in  [N][H][W][CinK];  out [N][Ho][Wo][out_ld] (channels >= Cout of a row are not written);  residual: same geometry as out
// with row stride Cout... (out_ld == Cout required when residual / up is given);  up: [N][Hup][Wup][Cout] nearest-upsampled and added.
// flags: bit 0 bias, bit 1 scale/shift (FrozenBatchNorm), bit 2 ReLU.  mode as in cald_train_pack_conv (the packed buffer's).
// The split twin of the pack (w16, or null) and of activations, checked against the shapes conv_h3.hip takes: a launch with w16 on another
// shape runs the exact kernels (the dispatcher's fall-through), which know no split activations.
// dgrad: w16 is a DATA-GRADIENT pack's twin (modes 1 / 3) and in_scale the power of two the fp32 gradient is staged at (conv_h3.hip; the mask
// rides in that kernel's epilogue); where conv_h3 does not take the shape the launch runs the exact kernels and never reads the twin.
struct Split16 { const void* w16; float unscale; const void* in16; int ex16; void* out16; bool dgrad; float in_scale; };
static bool pow2_scale(float s) { int e; return s > 0.0f && std::isfinite(s) && std::frexp(s, &e) == 0.5f; }
static int train_conv(cald_ctx* c, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                      int KH, int KW, int stride, int pad, int mode, int flags, const float* residual, const float* up,
                      int Hup, int Wup, const float* mask, float* out, int out_ld, const Split16& s16, const char** kernel) {
    if (kernel) *kernel = nullptr;
    if (!c || !in || !packed || !out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (N < 1 || H < 1 || W < 1 || stride < 1) TFAIL(CALD_ERR_INVALID, "bad geometry");
    THIP(hipSetDevice(cald_internal_device(c)));
    SEG_ENTRY();
    const PackGeom g = pack_geom(Cout, Cin, KH, KW, CinK, mode);
    const int kh = mode >= 2 ? 1 : KH, kw = mode >= 2 ? 1 : KW;
    const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
    if (Ho < 1 || Wo < 1) TFAIL(CALD_ERR_INVALID, "empty output");
    if ((residual || up) && out_ld != g.n_true) TFAIL(CALD_ERR_INVALID, "residual / upsample-add need out_ld == Cout");
    if (out_ld < g.n_true) TFAIL(CALD_ERR_INVALID, "out_ld < Cout");
    ConvArgs a;
    if (int rc = conv_args(c, a, g, packed, flags, N, H, W, Ho, Wo, kh, kw, stride, pad, in, out, out_ld)) return rc;
    a.residual = residual; a.up = up;
    if (up) { if (int rc = dense_seg(c, N, Hup, Wup, &a.seg_up)) return rc; }
    // mask (ReLU backward of the layer the result flows into): in the epilogue of the tiled kernel where it covers the shape, else a pass
    const bool fused = mask && p4_takes(g, kh * kw);
    if (mask && !fused && (out_ld != g.n_true || out_ld % 4)) TFAIL(CALD_ERR_INVALID, "mask on this shape needs a dense output with C %% 4 == 0");
    a.mask = fused ? mask : nullptr;
    if (s16.w16 && s16.dgrad) {
        if (mode != 1 && mode != 3) TFAIL(CALD_ERR_INVALID, "a data-gradient launch needs a data-gradient pack (mode 1 or 3)");
        if (up || !pow2_scale(s16.in_scale) || !pow2_scale(s16.unscale)) TFAIL(CALD_ERR_INVALID, "a data-gradient launch takes no up and needs in_scale and w16_unscale to be powers of two");
        if (h3_takes_grad(g, KH * KW, mode)) { a.w16 = s16.w16; a.w16_unscale = s16.unscale; a.in_scale = s16.in_scale; }
    } else if (s16.w16) {
        if ((mode != 0 && mode != 2) || mask) TFAIL(CALD_ERR_INVALID, "w16 belongs to a forward pack and takes no mask");
        if (h3_takes(g, KH * KW, mode)) { a.w16 = s16.w16; a.w16_unscale = s16.unscale; }
    }
    // Split activations exist for conv_h3 / conv_h4 alone: refuse every launch with them that those would not take (the exact kernels it
    // would fall through to read a twin as fp32) -- no w16 on a taking shape, the 4-channel stem, residual AND up, channels not in 16s
    const bool split_act = s16.in16 || s16.ex16 || s16.out16;
    if (split_act) {
        if (!a.w16 || g.cin_conv == 4 || (residual && up) || g.n_true % 16 || (s16.in16 && g.cin_conv % 16) ||
            ((s16.ex16 || s16.out16) && out_ld != g.n_true) || (s16.ex16 && !residual && !up))
            TFAIL(CALD_ERR_INVALID, "split activations need w16 on a shape conv_h3 takes, not residual and up together, channels %% 16 == 0 and out_ld == Cout");
        a.in16 = (const unsigned*)s16.in16; a.ex16 = s16.ex16 ? 1 : 0; a.out16 = (unsigned*)s16.out16;
    }
    const char* name = nullptr;
    if (s16.dgrad && a.w16 && !(name = launch_conv_h3_dgrad(a, cald_internal_stream(c)))) { a.w16 = nullptr; a.in_scale = 0.0f; }      // the exact kernels
    if (!name) name = launch_conv(a, cald_internal_stream(c));
    if (!name) TFAIL(CALD_ERR_UNSUPPORTED, "no conv kernel implements this layer's features");
    if (split_act && strncmp(name, "conv_h", 6) != 0 && strncmp(name, "none", 4) != 0)      // (cannot happen while h3_takes mirrors conv_h3.hip)
        TFAIL(CALD_ERR_STATE, "a launch with split activations ran on %s, which reads them as fp32", name);
    if (kernel) *kernel = name;
    if (mask && !fused) launch_relu_bwd(out, mask, nullptr, (long long)N * Ho * Wo * out_ld / 4, out_ld / 4, cald_internal_stream(c));
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_conv(cald_ctx* c, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                               int KH, int KW, int stride, int pad, int mode, int flags, const float* residual, const float* up,
                               int Hup, int Wup, const float* mask, float* out, int out_ld) {
    return train_conv(c, N, H, W, in, CinK, packed, Cout, Cin, KH, KW, stride, pad, mode, flags, residual, up, Hup, Wup, mask, out, out_ld,
                      Split16{nullptr, 1.0f, nullptr, 0, nullptr, false, 0.0f}, nullptr);
}
extern "C" int cald_train_conv_f16x3(cald_ctx* c, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                                     int KH, int KW, int stride, int pad, int mode, int flags, const float* residual, const float* up,
                                     int Hup, int Wup, const float* mask, float* out, int out_ld, const void* w16, float w16_unscale,
                                     const void* in16, int ex16, void* out16, const char** kernel) {
    return train_conv(c, N, H, W, in, CinK, packed, Cout, Cin, KH, KW, stride, pad, mode, flags, residual, up, Hup, Wup, mask, out, out_ld,
                      Split16{w16, w16_unscale, in16, ex16, out16, false, 0.0f}, kernel);
}
extern "C" int cald_train_conv_dgrad_f16x3(cald_ctx* c, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                                           int KH, int KW, int pad, int mode, const float* residual, const float* mask, float* out, int out_ld,
                                           const void* w16, float w16_unscale, float in_scale, const char** kernel) {
    if (!w16) TFAIL(CALD_ERR_INVALID, "null argument");
    return train_conv(c, N, H, W, in, CinK, packed, Cout, Cin, KH, KW, 1, pad, mode, 0, residual, nullptr, 0, 0, mask, out, out_ld,
                      Split16{w16, w16_unscale, nullptr, 0, nullptr, true, in_scale}, kernel);
}

// The same layer shape applied to several tensors in ONE launch (the pyramid levels under shared-weight heads; problems may carry
// different weights of equal shape, e.g. RetinaNet's two towers): workgroups of the small levels fill the tail of the large ones.
// Falls back to one launch per problem when the shape does not qualify for the grouped kernel (conv_p4.hip launch_conv_p4_group).
static int train_conv_group(cald_ctx* c, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                            int Cout, int Cin, int KH, int KW, int stride, int pad, int mode, int flags, const float* const* masks,
                            float* const* outs, int out_ld, const void* const* w16, const float* w16_unscale, const void* const* in16,
                            const char** kernels, const float* in_scale = nullptr) {
    const bool dgrad = in_scale != nullptr;             // data-gradient packs' twins, one input scale per problem (train_conv's Split16::dgrad)
    if (kernels) for (int i = 0; i < n && i < CALD_MAX_GROUP; i++) kernels[i] = nullptr;
    if (!c || !hw || !ins || !packed || !outs) TFAIL(CALD_ERR_INVALID, "null argument");
    if (n < 1 || n > CALD_MAX_GROUP) TFAIL(CALD_ERR_INVALID, "1..%d problems per group", CALD_MAX_GROUP);
    THIP(hipSetDevice(cald_internal_device(c)));
    SEG_ENTRY();
    const PackGeom g = pack_geom(Cout, Cin, KH, KW, CinK, mode);
    const int kh = mode >= 2 ? 1 : KH, kw = mode >= 2 ? 1 : KW;
    if (out_ld < g.n_true) TFAIL(CALD_ERR_INVALID, "out_ld < Cout");
    if (masks && !p4_takes(g, kh * kw)) TFAIL(CALD_ERR_INVALID, "masks need a shape the tiled kernel covers");
    if (dgrad && (!w16 || !w16_unscale || (mode != 1 && mode != 3) || in16)) TFAIL(CALD_ERR_INVALID, "a data-gradient group needs data-gradient packs with twins and their unscales, and no split inputs");
    if (!dgrad && w16 && (!w16_unscale || (mode != 0 && mode != 2) || masks)) TFAIL(CALD_ERR_INVALID, "w16 belongs to forward packs, comes with its unscale and takes no masks");
    const bool split = w16 && (dgrad ? h3_takes_grad(g, KH * KW, mode) : h3_takes(g, KH * KW, mode));
    if (in16 && (!split || g.cin_conv % 16)) TFAIL(CALD_ERR_INVALID, "split inputs need w16 on a shape conv_h3 takes and channels %% 16 == 0");
    ConvArgs probs[CALD_MAX_GROUP];
    for (int i = 0; i < n; i++) {
        const int H = hw[2 * i], W = hw[2 * i + 1];
        const int Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
        if (H < 1 || W < 1 || Ho < 1 || Wo < 1 || !ins[i] || !outs[i] || !packed[i]) TFAIL(CALD_ERR_INVALID, "bad problem %d", i);
        if (int rc = conv_args(c, probs[i], g, packed[i], flags, N, H, W, Ho, Wo, kh, kw, stride, pad, ins[i], outs[i], out_ld)) return rc;
        probs[i].mask = masks ? masks[i] : nullptr;
        if (split) {
            if (!w16[i]) TFAIL(CALD_ERR_INVALID, "problem %d has no w16", i);
            probs[i].w16 = w16[i]; probs[i].w16_unscale = w16_unscale[i];
            if (in16) probs[i].in16 = (const unsigned*)in16[i];
            if (dgrad) {
                if (!pow2_scale(in_scale[i]) || !pow2_scale(w16_unscale[i])) TFAIL(CALD_ERR_INVALID, "problem %d: in_scale and w16_unscale must be powers of two", i);
                probs[i].in_scale = in_scale[i];
            }
        }
    }
    const char* names[CALD_MAX_GROUP];
    const char* gname = dgrad && split ? launch_conv_h3_dgrad_group(probs, n, cald_internal_stream(c)) : nullptr;
    if (gname) for (int i = 0; i < n; i++) names[i] = gname;
    else {
        if (dgrad) for (int i = 0; i < n; i++) { probs[i].w16 = nullptr; probs[i].in_scale = 0.0f; }      // the exact kernels
        launch_conv_group(probs, n, cald_internal_stream(c), names);
    }
    for (int i = 0; i < n; i++) if (!names[i]) TFAIL(CALD_ERR_UNSUPPORTED, "no conv kernel implements problem %d's features", i);
    if (in16) for (int i = 0; i < n; i++) if (in16[i] && strncmp(names[i], "conv_h", 6) != 0 && strncmp(names[i], "none", 4) != 0)
        TFAIL(CALD_ERR_STATE, "problem %d with a split input ran on %s, which reads it as fp32", i, names[i]);
    if (kernels) for (int i = 0; i < n; i++) kernels[i] = names[i];
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_conv_group(cald_ctx* c, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                                     int Cout, int Cin, int KH, int KW, int stride, int pad, int mode, int flags, const float* const* masks,
                                     float* const* outs, int out_ld) {
    return train_conv_group(c, n, N, hw, ins, CinK, packed, Cout, Cin, KH, KW, stride, pad, mode, flags, masks, outs, out_ld, nullptr, nullptr, nullptr, nullptr);
}
extern "C" int cald_train_conv_group_f16x3(cald_ctx* c, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                                           int Cout, int Cin, int KH, int KW, int stride, int pad, int mode, int flags, const float* const* masks,
                                           float* const* outs, int out_ld, const void* const* w16, const float* w16_unscale,
                                           const void* const* in16, const char** kernels) {
    return train_conv_group(c, n, N, hw, ins, CinK, packed, Cout, Cin, KH, KW, stride, pad, mode, flags, masks, outs, out_ld, w16, w16_unscale, in16, kernels);
}
extern "C" int cald_train_conv_dgrad_group_f16x3(cald_ctx* c, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                                                 int Cout, int Cin, int KH, int KW, int pad, int mode, const float* const* masks, float* const* outs,
                                                 int out_ld, const void* const* w16, const float* w16_unscale, const float* in_scale, const char** kernels) {
    if (!in_scale) TFAIL(CALD_ERR_INVALID, "null argument");
    return train_conv_group(c, n, N, hw, ins, CinK, packed, Cout, Cin, KH, KW, 1, pad, mode, 0, masks, outs, out_ld, w16, w16_unscale, nullptr, kernels, in_scale);
}

// images[i]: device uint8 [H_i][W_i][3]; hw = host {H_0, W_0, Hr_0, Wr_0, ...} (source size, resized size); remainders[i]: optional
// device float [3][H_i][W_i] added to image / 255 (inputs that are not on the uint8 grid), or null.  out [N][Hp][Wp][4] (channel 3 = 0).
extern "C" int cald_train_preprocess(cald_ctx* c, int N, const uint8_t* const* images, const float* const* remainders, const int* hw, int Hp, int Wp,
                                     float* out) {
    if (!c || !images || !hw || !out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (N < 1 || N > CALD_MAX_VIEWS) TFAIL(CALD_ERR_INVALID, "N must be 1..%d", CALD_MAX_VIEWS);
    THIP(hipSetDevice(cald_internal_device(c)));
    SEG_ENTRY();
    hipStream_t st = cald_internal_stream(c);
    std::vector<ViewDesc> hv(N);
    memset(hv.data(), 0, sizeof(ViewDesc) * N);
    for (int v = 0; v < N; v++) {
        hv[v].src = images[v]; hv[v].H = hw[4 * v]; hv[v].W = hw[4 * v + 1]; hv[v].Hr = hw[4 * v + 2]; hv[v].Wr = hw[4 * v + 3];
        hv[v].Ho = hv[v].H; hv[v].Wo = hv[v].W; hv[v].noise = remainders ? remainders[v] : nullptr;
        if (hv[v].Hr > Hp || hv[v].Wr > Wp) TFAIL(CALD_ERR_INVALID, "resized image %d exceeds the padded batch size", v);
    }
    // the descriptors travel through a pinned staging ring: the call returns without waiting for the stream (it used to stop the host
    // twice, and with it the start of every training step until the previous step had left the GPU)
    const void* dv = nullptr; int slot = 0;
    if (int rc = stage_upload(c, hv.data(), sizeof(ViewDesc) * N, st, &dv, &slot)) return rc;
    const LevelSeg* s0;
    if (int rc = dense_seg(c, N, Hp, Wp, &s0)) return rc;
    launch_preprocess((const ViewDesc*)dv, s0, out, N, Hp * Wp, st);
    THIP(hipGetLastError());
    if (int rc = stage_consumed(c, slot, st)) return rc;
    return 0;
}
// max_pool2d(3, 2, 1) and max_pool2d(1, 2, 0) (LastLevelMaxPool: every second pixel): in [N][H][W][C] -> out [N][(H-1)/2+1][(W-1)/2+1][C]
static int pool_stride2(cald_ctx* c, int N, int H, int W, int C, const float* in, float* out, bool window3) {
    if (!c || !in || !out || C % 4) TFAIL(CALD_ERR_INVALID, "bad arguments");
    THIP(hipSetDevice(cald_internal_device(c)));
    SEG_ENTRY();
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const LevelSeg *si, *so;
    if (int rc = dense_seg(c, N, H, W, &si)) return rc;
    if (int rc = dense_seg(c, N, Ho, Wo, &so)) return rc;
    if (window3) launch_maxpool(in, out, si, so, C, N, Ho * Wo, cald_internal_stream(c));
    else launch_subsample2(in, out, si, so, C, N, Ho * Wo, cald_internal_stream(c));
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_maxpool(cald_ctx* c, int N, int H, int W, int C, const float* in, float* out) {
    return pool_stride2(c, N, H, W, C, in, out, true);
}
extern "C" int cald_train_subsample2(cald_ctx* c, int N, int H, int W, int C, const float* in, float* out) {
    return pool_stride2(c, N, H, W, C, in, out, false);
}
