// train_loss.hip -- the losses, value + gradient in one pass with every sum in a fixed order (block_sum_256): softmax cross-entropy, smooth-L1
// and binary cross-entropy with logits over the whole batch or per image (frcnn_ll.py:29-64, :243-276), and RetinaNet's focal loss
// (retinanet_cal.py:100-133).
#include "train_host.h"

// The three segmented losses: ONE workgroup per segment (the row counts are a few thousand), so the sums are taken in a
// fixed order.  Segment i = rows / gathered entries [off[i], off[i + 1]).  The plain entry points launch one segment over everything
// with a host `gscale` (the upstream gradient of the scalar loss, normally 1); the *_seg entry points launch one segment per IMAGE
// (the learning-loss baseline's task losses, frcnn_ll.py:29-64 and :243-276; ll_train.py:77-85): loss[i], and image i's gradient
// scaled by seg_gscale[i] (device; null = the host gscale).  Same kernel, same thread-strided sum and block_sum_256, so a single
// segment returns the plain entry point's bits.  The segments are the TRUE per-image sample counts: the reference's
// view(len(labels), -1, C) presumes equal counts per image, and with equal counts the two agree.  The table travels in the kernel
// arguments.
#define TRAIN_MAX_SEG 64
struct SegTable { int off[TRAIN_MAX_SEG + 1]; float denom[TRAIN_MAX_SEG]; };
static int seg_table(int N, const int* seg_off, const float* denom, SegTable& t) {
    if (N < 1 || N > TRAIN_MAX_SEG || !seg_off) TFAIL(CALD_ERR_INVALID, "%d segments outside [1, %d]", N, TRAIN_MAX_SEG);
    if (seg_off[0] < 0) TFAIL(CALD_ERR_INVALID, "negative segment offset");
    memset(&t, 0, sizeof(t));
    for (int i = 0; i <= N; i++) {
        if (i && seg_off[i] < seg_off[i - 1]) TFAIL(CALD_ERR_INVALID, "segment offsets must be non-decreasing (segment %d)", i - 1);
        t.off[i] = seg_off[i];
    }
    for (int i = 0; i < N; i++) {
        t.denom[i] = denom ? denom[i] : 1.0f;
        if (!(t.denom[i] > 0.0f)) TFAIL(CALD_ERR_INVALID, "denominator of segment %d is not positive", i);
    }
    return 0;
}
// the plain entry points' table: everything in one segment; their arguments are checked by the entry point, not by seg_table
static SegTable one_segment(int n, float denom) {
    SegTable t;
    memset(&t, 0, sizeof(t));
    t.off[1] = n; t.denom[0] = denom;
    return t;
}
__device__ inline float block_sum_256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v; __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const float r = red[0]; __syncthreads();
    return r;
}
// F.cross_entropy(logits[R][C], labels) (mean over the segment's rows); grad[r][c] = (softmax - onehot) / R; rows have stride ld
__global__ __launch_bounds__(256) void softmax_ce_kernel(const SegTable t, const float* logits, const long long* labels, int C, int ld, float gscale,
                                                         const float* seg_gscale, float* loss, float* grad) {
    __shared__ float red[256];
    const int img = blockIdx.x, r0 = t.off[img], R = t.off[img + 1] - r0;
    const float gs = seg_gscale ? seg_gscale[img] : gscale;
    float local = 0.0f;
    for (int r = threadIdx.x; r < R; r += 256) {
        const float* z = logits + (long long)(r0 + r) * ld;
        float m = z[0];
        for (int k = 1; k < C; k++) m = fmaxf(m, z[k]);
        float s = 0.0f;
        for (int k = 0; k < C; k++) s += det_expf(z[k] - m);
        const int y = (int)labels[r0 + r];
        local += (det_logf(s) + m) - z[y];
        if (grad) {
            float* g = grad + (long long)(r0 + r) * ld;
            const float inv = gs / (float)R;
            for (int k = 0; k < C; k++) g[k] = (det_expf(z[k] - m) / s - (k == y ? 1.0f : 0.0f)) * inv;
        }
    }
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) loss[img] = R > 0 ? tot / (float)R : 0.0f;
}
// det_utils.smooth_l1_loss(pred, target, beta, size_average=False) / denom over a segment's gathered 4-vectors: pred 4-vector i starts
// at float offset idx[i] of `pred` (and of `grad`, which the caller has zeroed).  beta = 0 is the plain L1 loss (retinanet_cal.py:217);
// weights (optional, one per 4-vector) multiply each vector's term (per-image 1 / num_foreground of RetinaNet).
__global__ __launch_bounds__(256) void smooth_l1_kernel(const SegTable t, const float* pred, const long long* idx, const float* target, float beta,
                                                        const float* weights, float gscale, const float* seg_gscale, float* loss, float* grad) {
    __shared__ float red[256];
    const int img = blockIdx.x, e0 = 4 * t.off[img], n = t.off[img + 1] - t.off[img];
    const float gs = seg_gscale ? seg_gscale[img] : gscale, denom = t.denom[img];
    float local = 0.0f;
    for (int e = threadIdx.x; e < 4 * n; e += 256) {
        const long long o = idx[(e0 + e) >> 2] + (e & 3);
        const float d = pred[o] - target[e0 + e], ad = fabsf(d);
        const float w = weights ? weights[(e0 + e) >> 2] : 1.0f;
        local += w * (ad < beta ? 0.5f * d * d / beta : ad - 0.5f * beta);
        if (grad) grad[o] = (ad < beta ? d / beta : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f))) * (w * gs / denom);
    }
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) loss[img] = tot / denom;           // no foreground row: 0 / denom = 0, and no gradient was written
}
// F.binary_cross_entropy_with_logits(x[idx], y) (mean over a segment's gathered logits)
__global__ __launch_bounds__(256) void bce_logits_kernel(const SegTable t, const float* x, const long long* idx, const float* y, float gscale,
                                                         const float* seg_gscale, float* loss, float* grad) {
    __shared__ float red[256];
    const int img = blockIdx.x, e0 = t.off[img], n = t.off[img + 1] - e0;
    const float gs = seg_gscale ? seg_gscale[img] : gscale;
    float local = 0.0f;
    for (int e = threadIdx.x; e < n; e += 256) {
        const long long o = idx[e0 + e];
        const float z = x[o], tt = y[e0 + e];
        // max(z, 0) - z * t + log(1 + exp(-|z|))
        local += ((z > 0.0f ? z : 0.0f) - z * tt) + det_logf(1.0f + det_expf(-fabsf(z)));
        if (grad) grad[o] = (det_sigmoidf(z) - tt) * (gs / (float)n);
    }
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) loss[img] = n > 0 ? tot / (float)n : 0.0f;
}
// all three are launched alike: N segments, one workgroup of 256 threads each
template <typename K, typename... A> static int launch_loss(cald_ctx* c, int N, K kernel, A... args) {
    THIP(hipSetDevice(cald_internal_device(c)));
    hipLaunchKernelGGL(kernel, dim3(N), dim3(256), 0, cald_internal_stream(c), args...);
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_softmax_ce(cald_ctx* c, int R, int C, int ld, const float* logits, const int64_t* labels, float gscale, float* loss_out,
                                     float* grad_out) {
    if (!c || !logits || !labels || !loss_out || R < 1 || C < 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    return launch_loss(c, 1, softmax_ce_kernel, one_segment(R, 1.0f), logits, (const long long*)labels, C, ld, gscale, (const float*)nullptr, loss_out, grad_out);
}
extern "C" int cald_train_smooth_l1(cald_ctx* c, int n, const float* pred, const int64_t* idx, const float* target, float beta, float denom,
                                    const float* weights, float gscale, float* loss_out, float* grad) {
    if (!c || !loss_out || (n > 0 && (!pred || !idx || !target))) TFAIL(CALD_ERR_INVALID, "bad arguments");
    return launch_loss(c, 1, smooth_l1_kernel, one_segment(n, denom), pred, (const long long*)idx, target, beta, weights, gscale, (const float*)nullptr, loss_out, grad);
}
extern "C" int cald_train_bce_logits(cald_ctx* c, int n, const float* logits, const int64_t* idx, const float* labels, float gscale, float* loss_out,
                                     float* grad) {
    if (!c || !loss_out || n < 1 || !logits || !idx || !labels) TFAIL(CALD_ERR_INVALID, "bad arguments");
    return launch_loss(c, 1, bce_logits_kernel, one_segment(n, 1.0f), logits, (const long long*)idx, labels, gscale, (const float*)nullptr, loss_out, grad);
}
extern "C" int cald_train_softmax_ce_seg(cald_ctx* c, int N, const int* seg_off, int C, int ld, const float* logits, const int64_t* labels,
                                         const float* gscale, float* loss_out, float* grad_out) {
    if (!c || !logits || !labels || !loss_out || C < 1 || ld < C) TFAIL(CALD_ERR_INVALID, "bad arguments");
    SegTable t;
    if (int rc = seg_table(N, seg_off, nullptr, t)) return rc;
    return launch_loss(c, N, softmax_ce_kernel, t, logits, (const long long*)labels, C, ld, 1.0f, gscale, loss_out, grad_out);
}
extern "C" int cald_train_smooth_l1_seg(cald_ctx* c, int N, const int* seg_off, const float* pred, const int64_t* idx, const float* target, float beta,
                                        const float* denom, const float* gscale, float* loss_out, float* grad) {
    if (!c || !loss_out || !denom) TFAIL(CALD_ERR_INVALID, "bad arguments");
    SegTable t;
    if (int rc = seg_table(N, seg_off, denom, t)) return rc;
    if (t.off[N] > 0 && (!pred || !idx || !target)) TFAIL(CALD_ERR_INVALID, "bad arguments");
    return launch_loss(c, N, smooth_l1_kernel, t, pred, (const long long*)idx, target, beta, (const float*)nullptr, 1.0f, gscale, loss_out, grad);
}
extern "C" int cald_train_bce_logits_seg(cald_ctx* c, int N, const int* seg_off, const float* logits, const int64_t* idx, const float* labels,
                                         const float* gscale, float* loss_out, float* grad) {
    if (!c || !loss_out || !logits || !idx || !labels) TFAIL(CALD_ERR_INVALID, "bad arguments");
    SegTable t;
    if (int rc = seg_table(N, seg_off, nullptr, t)) return rc;
    return launch_loss(c, N, bce_logits_kernel, t, logits, (const long long*)idx, labels, 1.0f, gscale, loss_out, grad);
}

// RetinaNet classification loss (retinanet_cal.py:100-133): torchvision.ops.sigmoid_focal_loss(alpha 0.25, gamma 2, 'sum') over the
// anchors whose match is not BETWEEN_THRESHOLDS, / max(1, #foreground) per image, mean over images.
//   logits: five level blocks in one buffer, level l = [N][pix_l][ld] with channel a * K + k; anchor order (level, y, x, a).
//   target(n, anchor, k) = matched >= 0 and gt_labels[gt_off[n] + matched] == k;  img_weight[n] = 1 / (max(1, #fg_n) * N).
// One thread per (image, anchor); block partial sums are added in a fixed order by the second kernel.
struct FocalArgs {
    const float* logits; float* grad; const int* matched; const long long* gt_labels; const int* gt_off; const float* img_weight;
    long long lvl_anchor0[6], lvl_off[5]; int lvl_pix[5];
    int N, A, K, ld; long long A_tot; float alpha, gscale;
};
__global__ __launch_bounds__(256) void focal_loss_kernel(FocalArgs a, float* partial) {
    __shared__ float red[256];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    float local = 0.0f;
    if (i < a.N * a.A_tot) {
        const int n = (int)(i / a.A_tot); const long long an = i - (long long)n * a.A_tot;
        const int m = a.matched[i];
        if (m != -2) {
            int l = 0;
            while (l < 4 && an >= a.lvl_anchor0[l + 1]) l++;
            const long long rel = an - a.lvl_anchor0[l];
            const long long pix = rel / a.A; const int aa = (int)(rel - pix * a.A);
            const long long base = a.lvl_off[l] + ((long long)n * a.lvl_pix[l] + pix) * a.ld + (long long)aa * a.K;
            const int cls = m >= 0 ? (int)a.gt_labels[a.gt_off[n] + m] : -1;
            const float w = a.img_weight[n];
            for (int k = 0; k < a.K; k++) {
                const float x = a.logits[base + k];
                const float lse = det_logf(1.0f + det_expf(-fabsf(x)));          // log(1 + exp(-|x|))
                const float logp = -((x < 0.0f ? -x : 0.0f) + lse);               // log sigmoid(x)
                const float log1mp = -((x > 0.0f ? x : 0.0f) + lse);              // log (1 - sigmoid(x))
                const float p = det_sigmoidf(x), q = 1.0f - p;
                float loss, g;
                if (k == cls) { loss = -a.alpha * q * q * logp; g = a.alpha * q * q * (2.0f * p * logp - q); }
                else { loss = -(1.0f - a.alpha) * p * p * log1mp; g = (1.0f - a.alpha) * p * p * (p - 2.0f * q * log1mp); }
                local += w * loss;
                if (a.grad) a.grad[base + k] = g * w * a.gscale;
            }
        }
    }
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* partial, int n, float* out) {
    __shared__ float red[256];
    float local = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) local += partial[i];
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) *out = tot;
}
extern "C" int cald_train_focal_loss(cald_ctx* c, int N, const int* level_pix, int A, int K, int ld, const float* logits, const int* matched,
                                     const int64_t* gt_labels, const int* gt_off, const float* img_weight, float alpha, float gscale,
                                     float* loss_out, float* grad) {
    if (!c || !level_pix || !logits || !matched || !gt_labels || !gt_off || !img_weight || !loss_out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (N < 1 || A < 1 || K < 1 || ld < A * K) TFAIL(CALD_ERR_INVALID, "bad geometry");
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    FocalArgs a; memset(&a, 0, sizeof(a));
    a.logits = logits; a.grad = grad; a.matched = matched; a.gt_labels = (const long long*)gt_labels; a.gt_off = gt_off; a.img_weight = img_weight;
    long long an = 0, off = 0;
    for (int l = 0; l < 5; l++) {
        a.lvl_anchor0[l] = an; a.lvl_off[l] = off; a.lvl_pix[l] = level_pix[l];
        an += (long long)level_pix[l] * A; off += (long long)N * level_pix[l] * ld;
    }
    a.lvl_anchor0[5] = an; a.A_tot = an; a.N = N; a.A = A; a.K = K; a.ld = ld; a.alpha = alpha; a.gscale = gscale;
    const long long total = (long long)N * an;
    const int blocks = (int)((total + 255) / 256);
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, (size_t)blocks * 4 + 64, &scratch)) return rc;
    hipLaunchKernelGGL(focal_loss_kernel, dim3(blocks), dim3(256), 0, st, a, (float*)scratch);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, (const float*)scratch, blocks, loss_out);
    THIP(hipGetLastError());
    return 0;
}

// The same loss per IMAGE (retina_ll.py:100-132): loss[n] = (sum of image n's raw terms) / denom[n], one IEEE division, as the
// reference's sigmoid_focal_loss(..., 'sum') / max(1, num_foreground); grad = g * (gs[n] / denom[n]).  The grid is (blocks per
// image, N): no workgroup covers anchors of two images, block (b, n) sums anchors [256 b, 256 b + 256) of image n and the finishing
// kernel (one workgroup per image) adds image n's partials with the thread-strided sum + block_sum_256 -- so image n's loss and gradient
// bits are those of the same image submitted alone.  Ignored anchors write nothing (the caller zeroed grad); pad columns are not touched.
struct FocalSegArgs { FocalArgs f; float denom[TRAIN_MAX_SEG]; const float* seg_gscale; };
__global__ __launch_bounds__(256) void focal_loss_seg_kernel(const FocalSegArgs s, float* partial) {
    __shared__ float red[256];
    const FocalArgs& a = s.f;
    const int n = blockIdx.y;
    const long long an = (long long)blockIdx.x * 256 + threadIdx.x;
    float local = 0.0f;
    if (an < a.A_tot) {
        const int m = a.matched[(long long)n * a.A_tot + an];
        if (m != -2) {
            int l = 0;
            while (l < 4 && an >= a.lvl_anchor0[l + 1]) l++;
            const long long rel = an - a.lvl_anchor0[l];
            const long long pix = rel / a.A; const int aa = (int)(rel - pix * a.A);
            const long long base = a.lvl_off[l] + ((long long)n * a.lvl_pix[l] + pix) * a.ld + (long long)aa * a.K;
            const int cls = m >= 0 ? (int)a.gt_labels[a.gt_off[n] + m] : -1;
            const float w = (s.seg_gscale ? s.seg_gscale[n] : 1.0f) / s.denom[n];
            for (int k = 0; k < a.K; k++) {
                const float x = a.logits[base + k];
                const float lse = det_logf(1.0f + det_expf(-fabsf(x)));          // log(1 + exp(-|x|))
                const float logp = -((x < 0.0f ? -x : 0.0f) + lse);               // log sigmoid(x)
                const float log1mp = -((x > 0.0f ? x : 0.0f) + lse);              // log (1 - sigmoid(x))
                const float p = det_sigmoidf(x), q = 1.0f - p;
                float loss, g;
                if (k == cls) { loss = -a.alpha * q * q * logp; g = a.alpha * q * q * (2.0f * p * logp - q); }
                else { loss = -(1.0f - a.alpha) * p * p * log1mp; g = (1.0f - a.alpha) * p * p * (p - 2.0f * q * log1mp); }
                local += loss;
                if (a.grad) a.grad[base + k] = g * w;
            }
        }
    }
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) partial[(long long)n * gridDim.x + blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void focal_seg_finish_kernel(const FocalSegArgs s, const float* partial, int per_img, float* loss) {
    __shared__ float red[256];
    const int n = blockIdx.x;
    float local = 0.0f;
    for (int i = threadIdx.x; i < per_img; i += 256) local += partial[(long long)n * per_img + i];
    const float tot = block_sum_256(local, red);
    if (threadIdx.x == 0) loss[n] = tot / s.denom[n];
}
// _sum(losses) / len(targets) of retina_ll.py:132 and :220 in float32: (((l_0 + l_1) + ...) + l_{N-1}) / (float)N, image order
__global__ void seg_mean_kernel(const float* loss, int N, float* mean_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float s = loss[0];
        for (int i = 1; i < N; i++) s += loss[i];
        *mean_out = s / (float)N;
    }
}
extern "C" int cald_train_seg_mean(cald_ctx* c, int N, const float* losses, float* mean_out) {
    if (!c || !losses || !mean_out || N < 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    THIP(hipSetDevice(cald_internal_device(c)));
    hipLaunchKernelGGL(seg_mean_kernel, dim3(1), dim3(64), 0, cald_internal_stream(c), losses, N, mean_out);
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_focal_loss_seg(cald_ctx* c, int N, const int* level_pix, int A, int K, int ld, const float* logits, const int* matched,
                                         const int64_t* gt_labels, const int* gt_off, const float* denom, float alpha, const float* gscale,
                                         float* loss_out, float* mean_out, float* grad) {
    if (!c || !level_pix || !logits || !matched || !gt_labels || !gt_off || !denom || !loss_out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (N < 1 || N > TRAIN_MAX_SEG) TFAIL(CALD_ERR_INVALID, "%d images outside [1, %d]", N, TRAIN_MAX_SEG);
    if (A < 1 || K < 1 || ld < A * K) TFAIL(CALD_ERR_INVALID, "bad geometry");
    FocalSegArgs s; memset(&s, 0, sizeof(s));
    FocalArgs& a = s.f;
    for (int n = 0; n < N; n++) {
        if (!(denom[n] > 0.0f)) TFAIL(CALD_ERR_INVALID, "denominator of image %d is not positive", n);
        s.denom[n] = denom[n];
    }
    s.seg_gscale = gscale;
    a.logits = logits; a.grad = grad; a.matched = matched; a.gt_labels = (const long long*)gt_labels; a.gt_off = gt_off;
    long long an = 0, off = 0;
    for (int l = 0; l < 5; l++) {
        if (level_pix[l] < 0) TFAIL(CALD_ERR_INVALID, "negative level size");
        a.lvl_anchor0[l] = an; a.lvl_off[l] = off; a.lvl_pix[l] = level_pix[l];
        an += (long long)level_pix[l] * A; off += (long long)N * level_pix[l] * ld;
    }
    if (an < 1 || (an + 255) / 256 > 0x7fffffffLL) TFAIL(CALD_ERR_INVALID, "bad geometry");
    a.lvl_anchor0[5] = an; a.A_tot = an; a.N = N; a.A = A; a.K = K; a.ld = ld; a.alpha = alpha; a.gscale = 1.0f;
    const int per_img = (int)((an + 255) / 256);
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, (size_t)N * per_img * 4 + 64, &scratch)) return rc;
    hipLaunchKernelGGL(focal_loss_seg_kernel, dim3(per_img, N), dim3(256), 0, st, s, (float*)scratch);
    hipLaunchKernelGGL(focal_seg_finish_kernel, dim3(N), dim3(256), 0, st, s, (const float*)scratch, per_img, loss_out);
    if (mean_out) hipLaunchKernelGGL(seg_mean_kernel, dim3(1), dim3(64), 0, st, (const float*)loss_out, N, mean_out);
    THIP(hipGetLastError());
    return 0;
}
