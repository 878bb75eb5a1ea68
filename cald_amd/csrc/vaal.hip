// vaal.hip -- the VAAL sweep (vaal/vaal_helper.py:186-222 AdversarySampler.sample; VAE.forward :78-86, Discriminator :121-143): per image the
// nearest resize to 256 x 256, five [Conv2d(4, 2, 1, bias) -> BatchNorm2d -> ReLU] stages 3 -> 64 -> 128 -> 256 -> 512 -> 1024, fc_mu
// 65 536 -> 256 and the discriminator 256 -> 512 -> 512 -> 1 with a sigmoid; and the C ABI: cald_vaal_*, cald_sweep_vaal, cald_op_vaal_*.
// Exact fp32, NHWC.  Every image's result depends on that image alone: no sum crosses images, and no order below depends on the batch
// size or the launch geometry.
//
// Resize (vaal_resize_kernel): source index = min((dst * in) >> 8, in - 1) per axis -- F.interpolate's default 'nearest' for an output of
// 256.  (u / 255) * 255 == u in float32 for every byte u, so the encoder's input is the uint8 pixel as a float, gathered straight from the
// HWC pool image into [256][256][4] (channel 3 = 0: the conv kernels take channel counts that are multiples of 4).
//
// Convolutions: the exact-mode launchers (launch_conv), chain order conv_k_index, + bias; their arithmetic is oracle.conv2d's.  The
// zero channel of the first layer adds fmaf(0, 0, acc) = acc to its (kh, kw, cin) chain.
//
// BatchNorm2d in train() mode, per (image, channel) over the N = H * W pixels in row-major order -- two passes, the order of lossnet.hip's
// pooling:
//   - chunks of 256 consecutive pixels (the last one may be short); inside a chunk pixel phase q = p mod 4 is summed sequentially in
//     increasing p from +0; chunk sum = (s0 + s1) + (s2 + s3); chunk sums are added sequentially in increasing chunk index from +0;
//   - pass 1 sums x, mean = sum / (float)N; pass 2 sums d * d with d = x - mean (a rounded product, then a rounded add),
//     var = sum / (float)N (biased); istd = 1.0f / sqrtf(var + 1e-5f), both IEEE;
//   - y = max(0, (((x - mean) * istd) * gamma) + beta), every operation rounded.
// The maps have 16 384, 4 096, 1 024, 256 and 64 pixels: 64, 16, 4, 1 and 1 chunks.  A chunk of 256 keeps the sequential part of a sum at
// 64 adds per phase plus at most 64 chunk adds, gives the partial kernel (chunks x C / 64 x images) workgroups -- 64 x 1 down to 1 x 16 per
// image -- and one pixel phase per wave, so a wave reads 64 consecutive channels of one pixel per load.  The statistics are not fused
// into the conv epilogue: a conv workgroup holds 128 rows of a tile grid that ignores the 256-pixel chunks' phases.
// In eval() mode the running statistics are folded at finalize into the conv epilogue's scale / shift (scale = gamma * (1 / sqrt(var +
// eps)), shift = beta - mean * scale, as the detector's FrozenBatchNorm2d), ReLU in the epilogue; no statistics kernel runs.
//
// fc_mu: the weight is repacked at finalize from k = c * 64 + p (View of NCHW) to the activation's order k' = p * 1024 + c, k'-major
// [65536][256].  Two fixed levels: 256 segments of 256 consecutive k'; a segment is one k'-ascending fmaf chain from +0; the segment sums are
// added sequentially in increasing segment index from +0; + bias.  A workgroup owns one segment for 16 images, so a batch reads the 67 MB
// weight once per 16 images (and finds it in the Infinity Cache after the first).
//
// Head: h1 = relu(chain_k(mu[k] * W1[j][k]) + b1[j]), h2 likewise over h1, x = chain(h2[i] * w3[i]) + b3, every chain one k-ascending
// fmaf chain from +0; pred = 1 / (1 + det_expf(-x)) (common.h: the library's deterministic exp).
#include "host.h"

#define VAAL_SIDE 256
#define VAAL_PIX (VAAL_SIDE * VAAL_SIDE)
#define VAAL_LAYERS 5
#define VAAL_Z 256
#define VAAL_FC_K 65536
#define VAAL_FC_SEG 256
#define VAAL_FC_NSEG (VAAL_FC_K / VAAL_FC_SEG)
#define VAAL_FC_TILE 16
#define VAAL_HID 512
#define BN_CHUNK 256
#define BN_EPS 1e-5f

__global__ __launch_bounds__(256) void vaal_resize_kernel(const VaalImage* __restrict__ imgs, float4* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x, dy = i >> 8, dx = i & (VAAL_SIDE - 1);
    const VaalImage im = imgs[blockIdx.y];
    int sy = (int)(((long long)dy * im.H) >> 8), sx = (int)(((long long)dx * im.W) >> 8);
    if (sy > im.H - 1) sy = im.H - 1;
    if (sx > im.W - 1) sx = im.W - 1;
    const uint8_t* p = im.src + ((size_t)sy * im.W + sx) * 3;
    out[(size_t)blockIdx.y * VAAL_PIX + i] = make_float4((float)p[0], (float)p[1], (float)p[2], 0.0f);
}

// grid (chunks, ceil(C / 64), images): wave = pixel phase, lane = channel.  VAR: sums (x - mean)^2, else x
template <bool VAR>
__global__ __launch_bounds__(256) void vaal_bn_partial_kernel(const float* __restrict__ x, const int HW, const int C, const float* __restrict__ mean,
                                                              float* __restrict__ partial) {
    __shared__ float sm[4][64];
    const int chunk = blockIdx.x, img = blockIdx.z, lane = threadIdx.x & 63, phase = threadIdx.x >> 6, c = blockIdx.y * 64 + lane;
    const int p0 = chunk * BN_CHUNK, n = HW - p0 < BN_CHUNK ? HW - p0 : BN_CHUNK;
    const int cnt = n > phase ? (n - phase + 3) >> 2 : 0;
    float acc = 0.0f;
    if (c < C) {
        const float m = VAR ? mean[(size_t)img * C + c] : 0.0f;
        const float* p = x + ((size_t)img * HW + p0 + phase) * C + c;
#pragma unroll 8
        for (int i = 0; i < cnt; i++) {
            const float v = p[(size_t)i * 4 * C];
            if (VAR) { const float d = v - m; acc = acc + d * d; } else acc = acc + v;
        }
    }
    sm[phase][lane] = acc;
    __syncthreads();
    if (phase == 0 && c < C)
        partial[((size_t)img * gridDim.x + chunk) * C + c] = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
}

// grid (ceil(C / 256), images): out[img][c] = the mean (VAR: 1 / sqrt(biased variance + eps))
template <bool VAR>
__global__ __launch_bounds__(256) void vaal_bn_finish_kernel(const float* __restrict__ partial, const int nchunk, const int HW, const int C,
                                                             float* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (c >= C) return;
    const float* p = partial + (size_t)img * nchunk * C + c;
    float sum = 0.0f;
    for (int k = 0; k < nchunk; k++) sum = sum + p[(size_t)k * C];
    const float v = sum / (float)HW;
    out[(size_t)img * C + c] = VAR ? 1.0f / sqrtf(v + BN_EPS) : v;
}

// in place over [images][HW][C], C % 4 == 0; one float4 per thread
__global__ __launch_bounds__(256) void vaal_bn_apply_kernel(float4* __restrict__ x, const long long n4, const int HW, const int C, const float* __restrict__ mean,
                                                            const float* __restrict__ istd, const float* __restrict__ gamma, const float* __restrict__ beta) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const int c4 = C >> 2;
    const int c = (int)(e % c4) * 4;
    const long long img = e / ((long long)HW * c4);
    const float4 v = x[e];
    const float4 m = *reinterpret_cast<const float4*>(mean + img * C + c), s = *reinterpret_cast<const float4*>(istd + img * C + c);
    const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
    float4 y;
    y.x = (((v.x - m.x) * s.x) * g.x) + b.x; y.y = (((v.y - m.y) * s.y) * g.y) + b.y;
    y.z = (((v.z - m.z) * s.z) * g.z) + b.z; y.w = (((v.w - m.w) * s.w) * g.w) + b.w;
    y.x = y.x > 0.0f ? y.x : 0.0f; y.y = y.y > 0.0f ? y.y : 0.0f; y.z = y.z > 0.0f ? y.z : 0.0f; y.w = y.w > 0.0f ? y.w : 0.0f;
    x[e] = y;
}

// grid (256 segments, ceil(n / 16)): thread = output j; partial [n][segment][256]
__global__ __launch_bounds__(256) void vaal_fc_partial_kernel(const float* __restrict__ act, const float* __restrict__ wt, const int n, float* __restrict__ partial) {
    __shared__ float sa[VAAL_FC_TILE][VAAL_FC_SEG];
    const int seg = blockIdx.x, i0 = blockIdx.y * VAAL_FC_TILE, j = threadIdx.x;
    const int ni = n - i0 < VAAL_FC_TILE ? n - i0 : VAAL_FC_TILE;
    for (int t = 0; t < VAAL_FC_TILE; t++)
        sa[t][j] = t < ni ? act[(size_t)(i0 + t) * VAAL_FC_K + (size_t)seg * VAAL_FC_SEG + j] : 0.0f;
    __syncthreads();
    float acc[VAAL_FC_TILE];
#pragma unroll
    for (int t = 0; t < VAAL_FC_TILE; t++) acc[t] = 0.0f;
    const float* w = wt + (size_t)seg * VAAL_FC_SEG * VAAL_Z + j;
#pragma unroll 4
    for (int k = 0; k < VAAL_FC_SEG; k++) {
        const float wv = w[(size_t)k * VAAL_Z];
#pragma unroll
        for (int t = 0; t < VAAL_FC_TILE; t++) acc[t] = fmaf(sa[t][k], wv, acc[t]);
    }
#pragma unroll
    for (int t = 0; t < VAAL_FC_TILE; t++)
        if (t < ni) partial[((size_t)(i0 + t) * VAAL_FC_NSEG + seg) * VAAL_Z + j] = acc[t];
}

// grid (n): mu[i][j] = (segment sums in increasing segment index from +0) + bias[j]
__global__ __launch_bounds__(256) void vaal_fc_finish_kernel(const float* __restrict__ partial, const float* __restrict__ bias, float* __restrict__ mu) {
    const int i = blockIdx.x, j = threadIdx.x;
    const float* p = partial + (size_t)i * VAAL_FC_NSEG * VAAL_Z + j;
    float sum = 0.0f;
    for (int s = 0; s < VAAL_FC_NSEG; s++) sum = sum + p[(size_t)s * VAAL_Z];
    mu[(size_t)i * VAAL_Z + j] = sum + bias[j];
}

// one workgroup of 512 threads per image; w1t [256][512], w2t [512][512] (k-major), w3 [512]
__global__ __launch_bounds__(512) void vaal_head_kernel(const float* __restrict__ mu, const float* __restrict__ w1t, const float* __restrict__ b1,
                                                        const float* __restrict__ w2t, const float* __restrict__ b2, const float* __restrict__ w3, const float b3,
                                                        float* __restrict__ out) {
    __shared__ float sx[VAAL_Z], h1[VAAL_HID], h2[VAAL_HID];
    const int i = blockIdx.x, j = threadIdx.x;
    if (j < VAAL_Z) sx[j] = mu[(size_t)i * VAAL_Z + j];
    __syncthreads();
    float acc = 0.0f;
    for (int k = 0; k < VAAL_Z; k++) acc = fmaf(sx[k], w1t[(size_t)k * VAAL_HID + j], acc);
    acc = acc + b1[j];
    h1[j] = acc > 0.0f ? acc : 0.0f;
    __syncthreads();
    acc = 0.0f;
    for (int k = 0; k < VAAL_HID; k++) acc = fmaf(h1[k], w2t[(size_t)k * VAAL_HID + j], acc);
    acc = acc + b2[j];
    h2[j] = acc > 0.0f ? acc : 0.0f;
    __syncthreads();
    if (j == 0) {
        acc = 0.0f;
        for (int k = 0; k < VAAL_HID; k++) acc = fmaf(h2[k], w3[k], acc);
        acc = acc + b3;
        out[i] = 1.0f / (1.0f + det_expf(-acc));
    }
}

// ---- launchers (kernels.h) ----
void launch_vaal_resize(const VaalImage* imgs, int n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(vaal_resize_kernel, dim3(VAAL_PIX / 256, n), dim3(256), 0, st, imgs, reinterpret_cast<float4*>(out));
}
int vaal_bn_chunks(int HW) { return (HW + BN_CHUNK - 1) / BN_CHUNK; }
void launch_vaal_bn_relu(float* x, int n, int HW, int C, const float* gamma, const float* beta, float* partial, float* mean, float* istd, hipStream_t st) {
    const int nch = vaal_bn_chunks(HW);
    const dim3 gp(nch, (C + 63) / 64, n), gf((C + 255) / 256, n);
    hipLaunchKernelGGL(vaal_bn_partial_kernel<false>, gp, dim3(256), 0, st, x, HW, C, nullptr, partial);
    hipLaunchKernelGGL(vaal_bn_finish_kernel<false>, gf, dim3(256), 0, st, partial, nch, HW, C, mean);
    hipLaunchKernelGGL(vaal_bn_partial_kernel<true>, gp, dim3(256), 0, st, x, HW, C, mean, partial);
    hipLaunchKernelGGL(vaal_bn_finish_kernel<true>, gf, dim3(256), 0, st, partial, nch, HW, C, istd);
    const long long n4 = (long long)n * HW * (C / 4);
    hipLaunchKernelGGL(vaal_bn_apply_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, reinterpret_cast<float4*>(x), n4, HW, C, mean, istd, gamma, beta);
}
void launch_vaal_fc_mu(const float* act, const float* wt, const float* bias, int n, float* partial, float* mu, hipStream_t st) {
    hipLaunchKernelGGL(vaal_fc_partial_kernel, dim3(VAAL_FC_NSEG, (n + VAAL_FC_TILE - 1) / VAAL_FC_TILE), dim3(256), 0, st, act, wt, n, partial);
    hipLaunchKernelGGL(vaal_fc_finish_kernel, dim3(n), dim3(256), 0, st, partial, bias, mu);
}
void launch_vaal_head(const float* mu, const float* w1t, const float* b1, const float* w2t, const float* b2, const float* w3, float b3, int n, float* out,
                      hipStream_t st) {
    hipLaunchKernelGGL(vaal_head_kernel, dim3(n), dim3(512), 0, st, mu, w1t, b1, w2t, b2, w3, b3, out);
}

// =============================================================================================
// handle
// =============================================================================================
static const int kCout[VAAL_LAYERS] = {64, 128, 256, 512, 1024};
static const int kCin[VAAL_LAYERS] = {3, 64, 128, 256, 512};
static const int kLevelPix[VAAL_LAYERS + 1] = {VAAL_PIX, 16384, 4096, 1024, 256, 64};

struct cald_vaal {
    cald_ctx* ctx = nullptr;
    std::map<std::string, HostTensor> sd;
    bool finalized = false;
    struct Layer { float *w = nullptr, *w4 = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr, *gamma = nullptr, *beta = nullptr; int Cin = 0, CoutPad = 0, Kpad = 0; } L[VAAL_LAYERS];
    float *fc_wt = nullptr, *fc_b = nullptr, *w1t = nullptr, *b1 = nullptr, *w2t = nullptr, *b2 = nullptr, *w3 = nullptr; float b3 = 0.0f;
    std::vector<void*> owned;
    void release() { for (void* p : owned) hipFree(p); owned.clear(); finalized = false; }
};

static bool vaal_key_used(const std::string& k) {
    static const char* const suf4[4] = {".weight", ".bias", ".running_mean", ".running_var"};
    for (int l = 0; l < VAAL_LAYERS; l++) {
        for (int s = 0; s < 2; s++) if (k == "encoder." + std::to_string(3 * l) + suf4[s]) return true;
        for (int s = 0; s < 4; s++) if (k == "encoder." + std::to_string(3 * l + 1) + suf4[s]) return true;
    }
    for (const char* p : {"fc_mu", "net.0", "net.2", "net.4"})
        for (int s = 0; s < 2; s++) if (k == std::string(p) + suf4[s]) return true;
    return false;
}

extern "C" int cald_vaal_create(cald_ctx* ctx, cald_vaal** out) {
    if (!ctx || !out) return fail(CALD_ERR_INVALID, "null argument");
    cald_vaal* v = new cald_vaal(); v->ctx = ctx;
    *out = v;
    return 0;
}
extern "C" int cald_vaal_load_tensor(cald_vaal* v, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!v || !key) return fail(CALD_ERR_INVALID, "bad argument");
    if (v->finalized) return fail(CALD_ERR_STATE, "VAAL model already finalized");
    if (!vaal_key_used(key)) return 0;           // the decoder, fc_logvar, num_batches_tracked: not part of the sweep
    if (!data || !shape || ndim < 1 || ndim > 4) return fail(CALD_ERR_INVALID, "%s: bad argument", key);
    HostTensor t; size_t n = 1;
    for (int i = 0; i < ndim; i++) { if (shape[i] < 1 || shape[i] > (1 << 20)) return fail(CALD_ERR_INVALID, "%s: bad shape", key); t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    if (n > ((size_t)1 << 26)) return fail(CALD_ERR_INVALID, "%s: bad shape", key);
    t.data.assign(data, data + n);
    v->sd[key] = std::move(t);
    return 0;
}

template <typename T> static int vaal_upload(cald_vaal* v, const std::vector<T>& h, T** d) {
    HIPCHK(hipMalloc((void**)d, h.size() * sizeof(T)));
    v->owned.push_back(*d);
    HIPCHK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

static int vaal_finalize(cald_vaal* v) {
    int err = 0;
    auto need = [&](const std::string& k, std::initializer_list<int64_t> shape) -> const HostTensor* {
        auto it = v->sd.find(k);
        if (it == v->sd.end()) { err = fail(CALD_ERR_MISSING_WEIGHT, "VAAL tensor '%s' is missing", k.c_str()); return nullptr; }
        if (it->second.shape != std::vector<int64_t>(shape)) { err = fail(CALD_ERR_INVALID, "VAAL tensor '%s' is mis-shaped", k.c_str()); return nullptr; }
        return &it->second;
    };
    int rc;
    for (int l = 0; l < VAAL_LAYERS; l++) {
        const std::string cv = "encoder." + std::to_string(3 * l), bn = "encoder." + std::to_string(3 * l + 1);
        const int Cout = kCout[l], Cin = kCin[l], Cinp = l == 0 ? 4 : Cin;
        const HostTensor* w = need(cv + ".weight", {Cout, Cin, 4, 4}); if (!w) return err;
        const HostTensor* b = need(cv + ".bias", {Cout}); if (!b) return err;
        const HostTensor* g = need(bn + ".weight", {Cout}); if (!g) return err;
        const HostTensor* be = need(bn + ".bias", {Cout}); if (!be) return err;
        const HostTensor* rm = need(bn + ".running_mean", {Cout}); if (!rm) return err;
        const HostTensor* rv = need(bn + ".running_var", {Cout}); if (!rv) return err;
        ConvPack pk;
        pack_conv({w->data.data()}, {Cout}, Cin, Cinp, 4, 4, 2, 1, false, &pk);
        cald_vaal::Layer& L = v->L[l];
        L.Cin = Cinp; L.CoutPad = pk.CoutPad; L.Kpad = pk.Kpad;
        std::vector<float> bias(pk.CoutPad, 0.0f), sc(pk.CoutPad, 0.0f), sh(pk.CoutPad, 0.0f);
        for (int i = 0; i < Cout; i++) {
            bias[i] = b->data[i];
            const float s = g->data[i] * (1.0f / sqrtf(rv->data[i] + BN_EPS));
            sc[i] = s; sh[i] = be->data[i] - rm->data[i] * s;
        }
        if ((rc = vaal_upload(v, pk.w, &L.w)) || (!pk.w4.empty() && (rc = vaal_upload(v, pk.w4, &L.w4))) || (rc = vaal_upload(v, bias, &L.bias)) ||
            (rc = vaal_upload(v, sc, &L.scale)) || (rc = vaal_upload(v, sh, &L.shift)) || (rc = vaal_upload(v, g->data, &L.gamma)) ||
            (rc = vaal_upload(v, be->data, &L.beta))) return rc;
    }
    {
        const HostTensor* w = need("fc_mu.weight", {VAAL_Z, VAAL_FC_K}); if (!w) return err;
        const HostTensor* b = need("fc_mu.bias", {VAAL_Z}); if (!b) return err;
        std::vector<float> wt((size_t)VAAL_FC_K * VAAL_Z);
        for (int j = 0; j < VAAL_Z; j++) {
            const float* src = w->data.data() + (size_t)j * VAAL_FC_K;
            for (int c = 0; c < 1024; c++)
                for (int p = 0; p < 64; p++) wt[((size_t)p * 1024 + c) * VAAL_Z + j] = src[c * 64 + p];
        }
        if ((rc = vaal_upload(v, wt, &v->fc_wt)) || (rc = vaal_upload(v, b->data, &v->fc_b))) return rc;
    }
    const HostTensor* w1 = need("net.0.weight", {VAAL_HID, VAAL_Z}); if (!w1) return err;
    const HostTensor* b1 = need("net.0.bias", {VAAL_HID}); if (!b1) return err;
    const HostTensor* w2 = need("net.2.weight", {VAAL_HID, VAAL_HID}); if (!w2) return err;
    const HostTensor* b2 = need("net.2.bias", {VAAL_HID}); if (!b2) return err;
    const HostTensor* w3 = need("net.4.weight", {1, VAAL_HID}); if (!w3) return err;
    const HostTensor* b3 = need("net.4.bias", {1}); if (!b3) return err;
    std::vector<float> w1t((size_t)VAAL_Z * VAAL_HID), w2t((size_t)VAAL_HID * VAAL_HID);
    for (int j = 0; j < VAAL_HID; j++) {
        for (int k = 0; k < VAAL_Z; k++) w1t[(size_t)k * VAAL_HID + j] = w1->data[(size_t)j * VAAL_Z + k];
        for (int k = 0; k < VAAL_HID; k++) w2t[(size_t)k * VAAL_HID + j] = w2->data[(size_t)j * VAAL_HID + k];
    }
    if ((rc = vaal_upload(v, w1t, &v->w1t)) || (rc = vaal_upload(v, b1->data, &v->b1)) || (rc = vaal_upload(v, w2t, &v->w2t)) ||
        (rc = vaal_upload(v, b2->data, &v->b2)) || (rc = vaal_upload(v, w3->data, &v->w3))) return rc;
    v->b3 = b3->data[0];
    return 0;
}
extern "C" int cald_vaal_finalize(cald_vaal* v) {
    if (!v) return fail(CALD_ERR_INVALID, "null argument");
    if (v->finalized) return 0;
    HIPCHK(hipSetDevice(v->ctx->device));
    const int rc = vaal_finalize(v);
    if (rc) { v->release(); return rc; }
    v->sd.clear();
    v->finalized = true;
    return 0;
}
extern "C" int cald_vaal_destroy(cald_vaal* v) {
    if (!v) return 0;
    hipStreamSynchronize(v->ctx->stream);
    v->release();
    delete v;
    return 0;
}

// =============================================================================================
// the sweep
// =============================================================================================
// the geometry of n equal images at the six levels: seg [6][cap + 1], entry n of a level the sentinel
static void vaal_fill_seg(std::vector<LevelSeg>& seg, int cap) {
    seg.assign((size_t)(VAAL_LAYERS + 1) * (cap + 1), LevelSeg());
    for (int l = 0; l <= VAAL_LAYERS; l++) {
        const int side = VAAL_SIDE >> l, pix = kLevelPix[l], tiles = (pix + 127) / 128;
        for (int i = 0; i <= cap; i++) {
            LevelSeg& s = seg[(size_t)l * (cap + 1) + i];
            s.pix_off = (long long)i * pix; s.H = side; s.W = side; s.tile_start = i * tiles; s.pad_ = 0;
        }
    }
}

extern "C" int cald_sweep_vaal(cald_ctx* c, cald_vaal* v, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                               const cald_vaal_cfg* cfg, float* preds_out, float* mu_out) {
    if (!c || !v || !images_dev || !H || !W || !preds_out || n_images < 0) return fail(CALD_ERR_INVALID, "null argument");
    if (!v->finalized) return fail(CALD_ERR_STATE, "VAAL model not finalized (call cald_vaal_finalize)");
    if (v->ctx != c) return fail(CALD_ERR_INVALID, "the VAAL model belongs to another context");
    const int mode = cfg ? cfg->bn_mode : CALD_VAAL_BN_BATCH;
    if (mode != CALD_VAAL_BN_BATCH && mode != CALD_VAAL_BN_RUNNING) return fail(CALD_ERR_INVALID, "bn_mode %d is not a CALD_VAAL_BN_* value", mode);
    int B = sweep_batch(cfg ? cfg->batch_images : 0, 64);
    if (B > n_images) B = n_images;
    for (int i = 0; i < n_images; i++)
        if (!images_dev[i] || H[i] < 1 || W[i] < 1 || (long long)H[i] * W[i] > (1ll << 28)) return fail(CALD_ERR_INVALID, "image %d is malformed", i);
    if (!n_images) return 0;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    VaalImage* d_imgs = nullptr; LevelSeg* d_seg = nullptr;
    float* act[VAAL_LAYERS + 1] = {};
    float *d_part = nullptr, *d_mean = nullptr, *d_istd = nullptr, *d_fcp = nullptr, *d_mu = nullptr, *d_pred = nullptr;
    int rc;
    std::vector<LevelSeg> seg; vaal_fill_seg(seg, B);
    if ((rc = sd.alloc(&d_imgs, (size_t)B * sizeof(VaalImage))) || (rc = sd.upload(&d_seg, seg.data(), seg.size() * sizeof(LevelSeg)))) return rc;
    for (int l = 0; l <= VAAL_LAYERS; l++)
        if ((rc = sd.alloc(&act[l], (size_t)B * kLevelPix[l] * (l ? kCout[l - 1] : 4) * 4))) return rc;
    // statistics partials: chunks x channels is 64 x 64 at the first layer and no larger after it
    if ((rc = sd.alloc(&d_part, (size_t)B * 4096 * 4)) || (rc = sd.alloc(&d_mean, (size_t)B * 1024 * 4)) || (rc = sd.alloc(&d_istd, (size_t)B * 1024 * 4)) ||
        (rc = sd.alloc(&d_fcp, (size_t)B * VAAL_FC_NSEG * VAAL_Z * 4)) || (rc = sd.alloc(&d_mu, (size_t)B * VAAL_Z * 4)) || (rc = sd.alloc(&d_pred, (size_t)B * 4))) return rc;
    std::vector<VaalImage> h_imgs(B);
    for (int i0 = 0; i0 < n_images; i0 += B) {
        const int nb = n_images - i0 < B ? n_images - i0 : B;
        for (int i = 0; i < nb; i++) { h_imgs[i].src = images_dev[i0 + i]; h_imgs[i].H = H[i0 + i]; h_imgs[i].W = W[i0 + i]; }
        HIPCHK(hipMemcpyAsync(d_imgs, h_imgs.data(), (size_t)nb * sizeof(VaalImage), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));        // h_imgs is pageable and rewritten by the next batch
        launch_vaal_resize(d_imgs, nb, act[0], c->stream);
        for (int l = 0; l < VAAL_LAYERS; l++) {
            const cald_vaal::Layer& L = v->L[l];
            ConvArgs a; memset(&a, 0, sizeof(a));
            a.in = act[l]; a.out = act[l + 1]; a.w = L.w; a.w4 = L.w4; a.bias = L.bias;
            if (mode == CALD_VAAL_BN_RUNNING) { a.scale = L.scale; a.shift = L.shift; a.relu = 1; }
            a.seg_in = d_seg + (size_t)l * (B + 1); a.seg_out = d_seg + (size_t)(l + 1) * (B + 1); a.seg_up = a.seg_out;
            a.V = nb; a.Cin = L.Cin; a.Cout = kCout[l]; a.CoutPad = L.CoutPad; a.Kpad = L.Kpad; a.KH = 4; a.KW = 4; a.stride = 2; a.pad = 1;
            a.total_mtiles = nb * ((kLevelPix[l + 1] + 127) / 128); a.out_ld = kCout[l]; a.zeros = c->d_zeros;
            if ((rc = run_conv(c, a, 2.0 * nb * kLevelPix[l + 1] * (double)kCout[l] * 16.0 * kCin[l]))) return rc;
            if (mode == CALD_VAAL_BN_BATCH)
                launch_vaal_bn_relu(act[l + 1], nb, kLevelPix[l + 1], kCout[l], L.gamma, L.beta, d_part, d_mean, d_istd, c->stream);
        }
        launch_vaal_fc_mu(act[VAAL_LAYERS], v->fc_wt, v->fc_b, nb, d_fcp, d_mu, c->stream);
        launch_vaal_head(d_mu, v->w1t, v->b1, v->w2t, v->b2, v->w3, v->b3, nb, d_pred, c->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(preds_out + i0, d_pred, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
        if (mu_out) HIPCHK(hipMemcpyAsync(mu_out + (size_t)i0 * VAAL_Z, d_mu, (size_t)nb * VAAL_Z * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// =============================================================================================
// operator hooks
// =============================================================================================
extern "C" int cald_op_vaal_resize(cald_ctx* c, const uint8_t* image, int H, int W, float* out) {
    if (!c || !image || !out) return fail(CALD_ERR_INVALID, "null argument");
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 28)) return fail(CALD_ERR_INVALID, "bad size %d x %d", H, W);
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    uint8_t* d_img = nullptr; VaalImage* d_i = nullptr; float* d_out = nullptr; int rc;
    if ((rc = sd.upload(&d_img, image, (size_t)H * W * 3))) return rc;
    const VaalImage hi = {d_img, H, W};
    if ((rc = sd.upload(&d_i, &hi, sizeof(hi))) || (rc = sd.alloc(&d_out, (size_t)VAAL_PIX * 16))) return rc;
    launch_vaal_resize(d_i, 1, d_out, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<float> h((size_t)VAAL_PIX * 4);
    HIPCHK(hipMemcpyAsync(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < VAAL_PIX; i++) for (int k = 0; k < 3; k++) out[(size_t)i * 3 + k] = h[(size_t)i * 4 + k];
    return 0;
}

extern "C" int cald_op_vaal_bn_relu(cald_ctx* c, const float* x, long long x_floats, int n, int HW, int C, const float* gamma, const float* beta, float* out) {
    if (!c || !x || !gamma || !beta || !out) return fail(CALD_ERR_INVALID, "null argument");
    if (n < 1 || n > CALD_MAX_VIEWS || HW < 1 || HW > (1 << 20) || C < 4 || C > 4096 || C % 4) return fail(CALD_ERR_INVALID, "bad shape: n %d (1..%d), HW %d, C %d (a multiple of 4)", n, CALD_MAX_VIEWS, HW, C);
    const long long used = (long long)n * HW * C;
    if (x_floats < used || used > (1ll << 30)) return fail(CALD_ERR_INVALID, "x holds %lld floats, the maps need %lld", x_floats, used);
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    float *d_x = nullptr, *d_g = nullptr, *d_b = nullptr, *d_part = nullptr, *d_mean = nullptr, *d_istd = nullptr; int rc;
    if ((rc = sd.upload(&d_x, x, (size_t)x_floats * 4)) || (rc = sd.upload(&d_g, gamma, (size_t)C * 4)) || (rc = sd.upload(&d_b, beta, (size_t)C * 4)) ||
        (rc = sd.alloc(&d_part, (size_t)n * vaal_bn_chunks(HW) * C * 4)) || (rc = sd.alloc(&d_mean, (size_t)n * C * 4)) || (rc = sd.alloc(&d_istd, (size_t)n * C * 4))) return rc;
    launch_vaal_bn_relu(d_x, n, HW, C, d_g, d_b, d_part, d_mean, d_istd, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_x, (size_t)used * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int cald_op_vaal_fc_mu(cald_vaal* v, int n, const float* act, float* mu_out) {
    if (!v || !act || !mu_out || n < 1 || n > CALD_MAX_VIEWS) return fail(CALD_ERR_INVALID, "bad argument");
    if (!v->finalized) return fail(CALD_ERR_STATE, "VAAL model not finalized (call cald_vaal_finalize)");
    cald_ctx* c = v->ctx;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    float *d_a = nullptr, *d_p = nullptr, *d_mu = nullptr; int rc;
    if ((rc = sd.upload(&d_a, act, (size_t)n * VAAL_FC_K * 4)) || (rc = sd.alloc(&d_p, (size_t)n * VAAL_FC_NSEG * VAAL_Z * 4)) || (rc = sd.alloc(&d_mu, (size_t)n * VAAL_Z * 4))) return rc;
    launch_vaal_fc_mu(d_a, v->fc_wt, v->fc_b, n, d_p, d_mu, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mu_out, d_mu, (size_t)n * VAAL_Z * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int cald_op_vaal_head(cald_vaal* v, int n, const float* mu, float* preds_out) {
    if (!v || !mu || !preds_out || n < 1 || n > (1 << 16)) return fail(CALD_ERR_INVALID, "bad argument");
    if (!v->finalized) return fail(CALD_ERR_STATE, "VAAL model not finalized (call cald_vaal_finalize)");
    cald_ctx* c = v->ctx;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    float *d_mu = nullptr, *d_o = nullptr; int rc;
    if ((rc = sd.upload(&d_mu, mu, (size_t)n * VAAL_Z * 4)) || (rc = sd.alloc(&d_o, (size_t)n * 4))) return rc;
    launch_vaal_head(d_mu, v->w1t, v->b1, v->w2t, v->b2, v->w3, v->b3, n, d_o, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(preds_out, d_o, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
