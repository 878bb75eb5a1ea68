// lossnet.hip -- the learning-loss baseline sweep (ll_train.py:145-166 get_uncertainty, ll4al/models/lossnet.py:31-65 LossNet): global average
// pooling of four pyramid levels of the ragged NHWC batch, LossNet's five linear layers, and the C ABI on top of the features-only forward
// (forward.hip, host.h FwdFeatures): cald_lossnet_*, cald_sweep_ll, cald_op_gap, cald_op_lossnet.
//
// Pooling order (fixed: bit-reproducible, restated on the CPU by the tests).  Per view, level and channel, N = H * W pixels in row-major order:
//   - chunks of 256 consecutive pixels (the last one may be short);
//   - inside a chunk, pixel phase q = p mod 4 is summed sequentially in increasing p from +0 (at most 64 adds per phase);
//   - chunk sum = (s0 + s1) + (s2 + s3); chunk sums are added sequentially in increasing chunk index from +0;
//   - mean = sum / (float)N, IEEE float32 division.
// gap_partial_kernel: one workgroup of 256 threads per (view, level, chunk); wave = phase, lane = channel quad, so a wave reads one pixel's
// 1 KB with one 16-byte load per lane; the four phases meet in LDS; partials [view][level][chunk][256] leave through plain vector stores -- no
// atomics.  The kernel is HBM-bound (31 MB per P2 of a VOC view) and deliberately not part of the FPN output conv's epilogue.
// A level kept in split form only (CALD_PRECISION_F16X3, h16.h) is read as hi + lo, the value cald_debug_tensor hands out.
//
// Head (the arithmetic contract of the linear layers): each FC_i output is one k-ordered fmaf chain from +0 over the 256 pooled
// values, + bias, ReLU; the result one fmaf chain over the 4 D values in torch.cat order, + bias.
#include "host.h"
#include "h16.h"

#define GAP_CHUNK 256
#define LL_C 256              // channels of every pyramid level

struct GapArgs {
    const float* feat[4];     // per level slot: the level tensor of the batch ([sum pix][256] fp32, or the same bytes in split form)
    const LevelSeg* seg[4];   // device: the level's geometry, V entries
    int split[4];
    int nslot, V, chunk_stride;
    float* partial;           // [V][nslot][chunk_stride][256]
};

__global__ __launch_bounds__(256) void gap_partial_kernel(const GapArgs a) {
    __shared__ float4 sm[4][64];
    const int s = blockIdx.y, v = blockIdx.z, chunk = blockIdx.x;
    const LevelSeg sg = a.seg[s][v];
    const int N = sg.H * sg.W, p0 = chunk * GAP_CHUNK;
    if (p0 >= N) return;                       // the whole workgroup: no barrier is skipped by a part of it
    const int n = N - p0 < GAP_CHUNK ? N - p0 : GAP_CHUNK;
    const int phase = threadIdx.x >> 6, cq = threadIdx.x & 63;
    const int cnt = n > phase ? (n - phase + 3) >> 2 : 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!a.split[s]) {
        const float4* p = reinterpret_cast<const float4*>(a.feat[s] + (sg.pix_off + p0 + phase) * LL_C) + cq;
#pragma unroll 8
        for (int i = 0; i < cnt; i++) {
            const float4 x = p[(size_t)i * LL_C];          // 4 pixels = 4 * 256 floats = 256 float4 further
            acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
        }
    } else {
        // channels 4 cq .. 4 cq + 3 of a pixel: four fp16 hi at chunk + 2 (c & 15), their lo 32 bytes further
        const unsigned char* p = reinterpret_cast<const unsigned char*>(a.feat[s]) + (sg.pix_off + p0 + phase) * (LL_C * 4) + (cq >> 2) * 64 + (cq & 3) * 8;
#pragma unroll 8
        for (int i = 0; i < cnt; i++) {
            const uint2 hi = *reinterpret_cast<const uint2*>(p + (size_t)i * (4 * LL_C * 4));
            const uint2 lo = *reinterpret_cast<const uint2*>(p + (size_t)i * (4 * LL_C * 4) + 32);
            acc.x += h16_join((hi.x & 0xffffu) | (lo.x << 16));
            acc.y += h16_join((hi.x >> 16) | (lo.x & 0xffff0000u));
            acc.z += h16_join((hi.y & 0xffffu) | (lo.y << 16));
            acc.w += h16_join((hi.y >> 16) | (lo.y & 0xffff0000u));
        }
    }
    sm[phase][cq] = acc;
    __syncthreads();
    const int c = threadIdx.x;
    const float* f = reinterpret_cast<const float*>(sm);
    const float s0 = f[c], s1 = f[256 + c], s2 = f[512 + c], s3 = f[768 + c];
    a.partial[(((size_t)v * a.nslot + s) * a.chunk_stride + chunk) * LL_C + c] = (s0 + s1) + (s2 + s3);
}

// grid (nbranch, V): pooled[v][j][c] = the mean of level slot branch_slot[j]
struct GapFinishArgs { int branch_slot[4]; float* pooled; };
__global__ __launch_bounds__(256) void gap_finish_kernel(const GapArgs a, const GapFinishArgs fa) {
    const int j = blockIdx.x, v = blockIdx.y, c = threadIdx.x, s = fa.branch_slot[j];
    const LevelSeg sg = a.seg[s][v];
    const int N = sg.H * sg.W, nch = (N + GAP_CHUNK - 1) / GAP_CHUNK;
    const float* p = a.partial + ((size_t)v * a.nslot + s) * a.chunk_stride * LL_C + c;
    float sum = 0.0f;
    for (int k = 0; k < nch; k++) sum += p[(size_t)k * LL_C];
    fa.pooled[((size_t)v * gridDim.x + j) * LL_C + c] = sum / (float)N;
}

// one workgroup per image: pooled [n][4][256]; wt [4][256][D] (k-major), b [4][D], lw [4 D]
__global__ __launch_bounds__(256) void lossnet_head_kernel(const float* __restrict__ pooled, const float* __restrict__ wt, const float* __restrict__ b,
                                                          const float* __restrict__ lw, const float lb, const int D, float* __restrict__ out) {
    __shared__ float sp[4 * LL_C];
    __shared__ float sh[4 * 256];
    const int v = blockIdx.x, d = threadIdx.x;
    for (int i = d; i < 4 * LL_C; i += 256) sp[i] = pooled[(size_t)v * 4 * LL_C + i];
    __syncthreads();
    if (d < D) {
        for (int j = 0; j < 4; j++) {
            const float* w = wt + (size_t)j * LL_C * D + d;
            float acc = 0.0f;
            for (int k = 0; k < LL_C; k++) acc = fmaf(sp[j * LL_C + k], w[(size_t)k * D], acc);
            acc = acc + b[j * D + d];
            sh[j * D + d] = acc > 0.0f ? acc : 0.0f;
        }
    }
    __syncthreads();
    if (d == 0) {
        float acc = 0.0f;
        for (int i = 0; i < 4 * D; i++) acc = fmaf(sh[i], lw[i], acc);
        out[v] = acc + lb;
    }
}

// the two pooling launches over `a` (partial sized by the caller), timed as one entry each while the profile is on
static int run_gap(cald_ctx* c, const GapArgs& a, const GapFinishArgs& fa, int nbranch, int max_chunks, long long bytes) {
    ProfLaunch t; int rc;
    if ((rc = prof_begin(c, t))) return rc;
    hipLaunchKernelGGL(gap_partial_kernel, dim3(max_chunks, a.nslot, a.V), dim3(256), 0, c->stream, a);
    if ((rc = prof_end(c, t, 0.0, 0, "gap_partial,bytes=%lld", bytes))) return rc;
    ProfLaunch t2;
    if ((rc = prof_begin(c, t2))) return rc;
    hipLaunchKernelGGL(gap_finish_kernel, dim3(nbranch, a.V), dim3(256), 0, c->stream, a, fa);
    if ((rc = prof_end(c, t2, 0.0, 0, "gap_finish"))) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

// =============================================================================================
// LossNet handle
// =============================================================================================
struct cald_lossnet {
    cald_ctx* ctx = nullptr;
    std::map<std::string, HostTensor> sd;
    bool finalized = false;
    int D = 0;
    float *d_wt = nullptr, *d_b = nullptr, *d_lw = nullptr; float lb = 0.0f;
    void release() { hipFree(d_wt); hipFree(d_b); hipFree(d_lw); d_wt = d_b = d_lw = nullptr; finalized = false; }
};

extern "C" int cald_lossnet_create(cald_ctx* ctx, cald_lossnet** out) {
    if (!ctx || !out) return fail(CALD_ERR_INVALID, "null argument");
    cald_lossnet* ln = new cald_lossnet(); ln->ctx = ctx;
    *out = ln;
    return 0;
}
extern "C" int cald_lossnet_load_tensor(cald_lossnet* ln, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!ln || !key || !data || !shape || ndim < 1 || ndim > 2) return fail(CALD_ERR_INVALID, "bad argument");
    if (ln->finalized) return fail(CALD_ERR_STATE, "LossNet already finalized");
    HostTensor t; size_t n = 1;
    for (int i = 0; i < ndim; i++) { if (shape[i] < 1 || shape[i] > (1 << 20)) return fail(CALD_ERR_INVALID, "%s: bad shape", key); t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    ln->sd[key] = std::move(t);
    return 0;
}
extern "C" int cald_lossnet_finalize(cald_lossnet* ln) {
    if (!ln) return fail(CALD_ERR_INVALID, "null argument");
    if (ln->finalized) return 0;
    int err = 0;
    auto need = [&](const std::string& k, int ndim) -> const HostTensor* {
        auto it = ln->sd.find(k);
        if (it == ln->sd.end()) { err = fail(CALD_ERR_MISSING_WEIGHT, "LossNet tensor '%s' is missing", k.c_str()); return nullptr; }
        if ((int)it->second.shape.size() != ndim) { err = fail(CALD_ERR_INVALID, "LossNet tensor '%s' has %d dimensions, not %d", k.c_str(), (int)it->second.shape.size(), ndim); return nullptr; }
        return &it->second;
    };
    const HostTensor* w1 = need("FC1.weight", 2);
    if (!w1) return err;
    const int D = (int)w1->shape[0];
    if (D < 1 || D > 256) return fail(CALD_ERR_INVALID, "LossNet interm_dim %d outside [1, 256]", D);
    std::vector<float> wt((size_t)4 * LL_C * D), b((size_t)4 * D);
    for (int j = 0; j < 4; j++) {
        const std::string fc = "FC" + std::to_string(j + 1);
        const HostTensor* w = need(fc + ".weight", 2); if (!w) return err;
        const HostTensor* bb = need(fc + ".bias", 1); if (!bb) return err;
        if (w->shape[0] != D || w->shape[1] != LL_C) return fail(CALD_ERR_INVALID, "%s.weight is [%lld][%lld], expected [%d][%d]", fc.c_str(), (long long)w->shape[0], (long long)w->shape[1], D, LL_C);
        if (bb->shape[0] != D) return fail(CALD_ERR_INVALID, "%s.bias has %lld entries, expected %d", fc.c_str(), (long long)bb->shape[0], D);
        for (int d = 0; d < D; d++) {
            for (int k = 0; k < LL_C; k++) wt[((size_t)j * LL_C + k) * D + d] = w->data[(size_t)d * LL_C + k];
            b[(size_t)j * D + d] = bb->data[d];
        }
    }
    const HostTensor* l = need("linear.weight", 2); if (!l) return err;
    const HostTensor* lbias = need("linear.bias", 1); if (!lbias) return err;
    if (l->shape[0] != 1 || l->shape[1] != 4 * D) return fail(CALD_ERR_INVALID, "linear.weight is [%lld][%lld], expected [1][%d]", (long long)l->shape[0], (long long)l->shape[1], 4 * D);
    if (lbias->shape[0] != 1) return fail(CALD_ERR_INVALID, "linear.bias has %lld entries, expected 1", (long long)lbias->shape[0]);
    const std::vector<float>& lw = l->data;
    cald_ctx* c = ln->ctx;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc((void**)&ln->d_wt, wt.size() * 4)); HIPCHK(hipMalloc((void**)&ln->d_b, b.size() * 4)); HIPCHK(hipMalloc((void**)&ln->d_lw, lw.size() * 4));
    HIPCHK(hipMemcpy(ln->d_wt, wt.data(), wt.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ln->d_b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ln->d_lw, lw.data(), lw.size() * 4, hipMemcpyHostToDevice));
    ln->lb = lbias->data[0]; ln->D = D; ln->finalized = true;
    return 0;
}
extern "C" int cald_lossnet_destroy(cald_lossnet* ln) {
    if (!ln) return 0;
    hipStreamSynchronize(ln->ctx->stream);
    ln->release();
    delete ln;
    return 0;
}

static void launch_head(const cald_lossnet* ln, int n, const float* d_pooled, float* d_out, hipStream_t st) {
    hipLaunchKernelGGL(lossnet_head_kernel, dim3(n), dim3(256), 0, st, d_pooled, ln->d_wt, ln->d_b, ln->d_lw, ln->lb, ln->D, d_out);
}

// =============================================================================================
// operator hooks
// =============================================================================================
extern "C" int cald_op_gap(cald_ctx* c, const float* x, int H, int W, int C, float* mean_out) {
    if (!c || !x || !mean_out) return fail(CALD_ERR_INVALID, "null argument");
    if (C != LL_C) return fail(CALD_ERR_INVALID, "cald_op_gap pools %d channels, not %d", LL_C, C);
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 22)) return fail(CALD_ERR_INVALID, "bad size %d x %d", H, W);
    HIPCHK(hipSetDevice(c->device));
    const int N = H * W, nch = (N + GAP_CHUNK - 1) / GAP_CHUNK;
    ScopedDev scratch(c->stream);
    float *d_x = nullptr, *d_part = nullptr, *d_mean = nullptr; LevelSeg* d_seg = nullptr;
    int rc;
    if ((rc = scratch.alloc(&d_x, (size_t)N * LL_C * 4)) || (rc = scratch.alloc(&d_part, (size_t)nch * LL_C * 4)) ||
        (rc = scratch.alloc(&d_mean, LL_C * 4)) || (rc = scratch.alloc(&d_seg, 2 * sizeof(LevelSeg)))) return rc;
    LevelSeg sg[2]; memset(sg, 0, sizeof(sg));
    sg[0].H = H; sg[0].W = W; sg[1].pix_off = N; sg[1].tile_start = (N + 127) / 128;
    HIPCHK(hipMemcpyAsync(d_x, x, (size_t)N * LL_C * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_seg, sg, sizeof(sg), hipMemcpyHostToDevice, c->stream));
    GapArgs a; memset(&a, 0, sizeof(a));
    a.feat[0] = d_x; a.seg[0] = d_seg; a.nslot = 1; a.V = 1; a.chunk_stride = nch; a.partial = d_part;
    GapFinishArgs fa; memset(&fa, 0, sizeof(fa)); fa.pooled = d_mean;
    if ((rc = run_gap(c, a, fa, 1, nch, (long long)N * LL_C * 4))) return rc;
    HIPCHK(hipMemcpyAsync(mean_out, d_mean, LL_C * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int cald_op_lossnet(cald_lossnet* ln, int n, const float* pooled, float* out) {
    if (!ln || !pooled || !out || n < 1) return fail(CALD_ERR_INVALID, "bad argument");
    if (!ln->finalized) return fail(CALD_ERR_STATE, "LossNet not finalized (call cald_lossnet_finalize)");
    cald_ctx* c = ln->ctx;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev scratch(c->stream);
    float *d_p = nullptr, *d_o = nullptr; int rc;
    if ((rc = scratch.alloc(&d_p, (size_t)n * 4 * LL_C * 4)) || (rc = scratch.alloc(&d_o, (size_t)n * 4))) return rc;
    HIPCHK(hipMemcpyAsync(d_p, pooled, (size_t)n * 4 * LL_C * 4, hipMemcpyHostToDevice, c->stream));
    launch_head(ln, n, d_p, d_o, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_o, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// =============================================================================================
// pooling in the training forward (ll_train.py:77 task_model(images, targets) -> features; frcnn_ll.py:601-602)
// =============================================================================================
int cald_internal_scratch(cald_ctx* c, size_t bytes, void** out);   // ctx.hip: grow-only per-context device scratch (stream-ordered reuse)

// the geometry of four dense levels, written on the device (no host table has to outlive the call): seg [4][N], LevelSeg.pix_off = n H W
struct DenseHW { int H[4], W[4]; };
__global__ void dense_seg_fill_kernel(LevelSeg* seg, const int N, const DenseHW g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * N) return;
    const int l = i / N, n = i % N, H = g.H[l], W = g.W[l];
    LevelSeg s; s.pix_off = (long long)n * H * W; s.H = H; s.W = W; s.tile_start = n * ((H * W + 127) / 128); s.pad_ = 0;
    seg[i] = s;
}

extern "C" int cald_train_gap(cald_ctx* c, int N, const float* const* maps, const int* level_hw, float* pooled) {
    if (!c || !maps || !level_hw || !pooled) return fail(CALD_ERR_INVALID, "null argument");
    if (N < 1 || N > CALD_MAX_VIEWS) return fail(CALD_ERR_INVALID, "batch of %d images outside [1, %d]", N, CALD_MAX_VIEWS);
    DenseHW g; int max_chunks = 1; long long bytes = 0;
    for (int l = 0; l < 4; l++) {
        const int H = level_hw[2 * l], W = level_hw[2 * l + 1];
        if (!maps[l] || H < 1 || W < 1 || (long long)H * W > (1ll << 22)) return fail(CALD_ERR_INVALID, "level %d: bad map (%d x %d)", l, H, W);
        g.H[l] = H; g.W[l] = W;
        const int ch = (H * W + GAP_CHUNK - 1) / GAP_CHUNK;
        if (ch > max_chunks) max_chunks = ch;
        bytes += (long long)N * H * W * LL_C * 4;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t seg_bytes = ((size_t)4 * N * sizeof(LevelSeg) + 255) / 256 * 256;
    void* scratch = nullptr; int rc;
    if ((rc = cald_internal_scratch(c, seg_bytes + (size_t)N * 4 * max_chunks * LL_C * 4, &scratch))) return rc;
    LevelSeg* d_seg = reinterpret_cast<LevelSeg*>(scratch);
    hipLaunchKernelGGL(dense_seg_fill_kernel, dim3((4 * N + 255) / 256), dim3(256), 0, c->stream, d_seg, N, g);
    GapArgs a; memset(&a, 0, sizeof(a));
    for (int l = 0; l < 4; l++) { a.feat[l] = maps[l]; a.seg[l] = d_seg + (size_t)l * N; }
    a.nslot = 4; a.V = N; a.chunk_stride = max_chunks; a.partial = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + seg_bytes);
    GapFinishArgs fa; for (int j = 0; j < 4; j++) fa.branch_slot[j] = j;
    fa.pooled = pooled;
    return run_gap(c, a, fa, 4, max_chunks, bytes);
}

// =============================================================================================
// the sweep (ll_train.py:145-166)
// =============================================================================================
extern "C" int cald_sweep_ll(cald_model* m, cald_lossnet* ln, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                             const int* group, const cald_ll_cfg* cfg, double* uncertainty_out, float* pooled_out) {
    if (!m || !ln || !images_dev || !H || !W || !group || !uncertainty_out || n_images < 0) return fail(CALD_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CALD_ERR_STATE, "model not finalized");
    if (!ln->finalized) return fail(CALD_ERR_STATE, "LossNet not finalized (call cald_lossnet_finalize)");
    if (ln->ctx != m->ctx) return fail(CALD_ERR_INVALID, "the detector and the LossNet belong to different contexts");
    cald_ctx* c = m->ctx;
    const bool retina = m->cfg.arch == CALD_ARCH_RETINANET;
    // ll_train.py:155-161 hands features[0] (P3) to all four branches of a RetinaNet, as shipped; Faster R-CNN pools '0'..'3' = P2..P5
    int levels[4];
    for (int j = 0; j < 4; j++) levels[j] = cfg ? cfg->levels[j] : (retina ? 0 : j);
    const int n_pyr = retina ? 5 : 4;      // P3..P7 | P2..P5 ('pool' is not a LossNet input)
    bool p7 = false;
    for (int j = 0; j < 4; j++) {
        if (levels[j] < 0 || levels[j] >= n_pyr) return fail(CALD_ERR_INVALID, "level %d of branch %d is outside the pyramid (0..%d)", levels[j], j, n_pyr - 1);
        p7 |= retina && levels[j] == 4;
    }
    const int B = sweep_batch(cfg ? cfg->batch_views : 0, 32);
    // an image is padded to its loader batch's common size: the per-dimension maximum of the members' own padded sizes (a maximum of multiples
    // of 32 is one) -- computed here from the whole group, so a group may straddle launch batches
    std::vector<int> pad((size_t)2 * (n_images ? n_images : 1));
    for (int i = 0; i < n_images; ) {
        if (H[i] <= 0 || W[i] <= 0 || !images_dev[i]) return fail(CALD_ERR_INVALID, "image %d is malformed", i);
        int j = i, Hm = 0, Wm = 0;
        for (; j < n_images && group[j] == group[i]; j++) {
            if (H[j] <= 0 || W[j] <= 0 || !images_dev[j]) return fail(CALD_ERR_INVALID, "image %d is malformed", j);
            int Hr, Wr, Hp, Wp; transform_size(H[j], W[j], m->cfg.min_size, m->cfg.max_size, &Hr, &Wr, &Hp, &Wp);
            if (Hp > Hm) Hm = Hp; if (Wp > Wm) Wm = Wp;
        }
        if (j < n_images && group[j] < group[i]) return fail(CALD_ERR_INVALID, "group ids must be non-decreasing (image %d)", j);
        for (int k = i; k < j; k++) { pad[2 * k] = Hm; pad[2 * k + 1] = Wm; }
        i = j;
    }
    // level slots: each pyramid level in use is pooled once
    int slot_level[4], nslot = 0, branch_slot[4];
    for (int j = 0; j < 4; j++) {
        int s = 0; while (s < nslot && slot_level[s] != levels[j]) s++;
        if (s == nslot) slot_level[nslot++] = levels[j];
        branch_slot[j] = s;
    }
    HIPCHK(hipSetDevice(c->device));
    ScopedDev scratch(c->stream);
    float *d_pooled = nullptr, *d_out = nullptr, *d_part = nullptr; size_t part_cap = 0;
    { int rc0; if ((rc0 = scratch.alloc(&d_pooled, (size_t)B * 4 * LL_C * 4)) || (rc0 = scratch.alloc(&d_out, (size_t)B * 4))) return rc0; }
    std::vector<float> h_out(B), h_pooled(pooled_out ? (size_t)B * 4 * LL_C : 0);
    int rc = 0;
    for (int i0 = 0; i0 < n_images && !rc; i0 += B) {
        const int nb = (n_images - i0 < B) ? n_images - i0 : B;
        std::vector<ViewDesc> views = ref_views(images_dev, H, W, i0, nb);
        FwdFeatures ft; ft.pad_to = reinterpret_cast<const int (*)[2]>(pad.data() + 2 * (size_t)i0); ft.p7 = p7;
        if ((rc = forward_model(m, nb, views.data(), FwdRequest::features(&ft)))) break;
        GapArgs a; memset(&a, 0, sizeof(a));
        int max_chunks = 1; long long bytes = 0;
        for (int s = 0; s < nslot; s++) {
            const int pl = ft.plan_level[slot_level[s]];
            a.feat[s] = ft.P[slot_level[s]]; a.seg[s] = c->d_plan->seg[pl]; a.split[s] = ft.split_only[slot_level[s]] ? 1 : 0;
            for (int v = 0; v < nb; v++) {
                const int ch = (m->plan.seg[pl][v].H * m->plan.seg[pl][v].W + GAP_CHUNK - 1) / GAP_CHUNK;
                if (ch > max_chunks) max_chunks = ch;
            }
            bytes += level_pix(m->plan, pl, nb) * LL_C * 4;
        }
        const size_t need = (size_t)nb * nslot * max_chunks * LL_C * 4;
        if (need > part_cap) {
            if (d_part) { hipStreamSynchronize(c->stream); hipFree(d_part); d_part = nullptr; part_cap = 0; }
            if (hipMalloc((void**)&d_part, need + (need >> 2)) != hipSuccess) { rc = fail(CALD_ERR_HIP, "hipMalloc of the pooling partials failed"); break; }
            part_cap = need + (need >> 2);
        }
        a.nslot = nslot; a.V = nb; a.chunk_stride = max_chunks; a.partial = d_part;
        GapFinishArgs fa; for (int j = 0; j < 4; j++) fa.branch_slot[j] = branch_slot[j];
        fa.pooled = d_pooled;
        if ((rc = run_gap(c, a, fa, 4, max_chunks, bytes))) break;
        launch_head(ln, nb, d_pooled, d_out, c->stream);
        if (hipMemcpyAsync(h_out.data(), d_out, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (pooled_out && hipMemcpyAsync(h_pooled.data(), d_pooled, (size_t)nb * 4 * LL_C * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(CALD_ERR_HIP, "learning-loss scoring failed: %s", hipGetErrorString(hipGetLastError())); break; }
        for (int i = 0; i < nb; i++) uncertainty_out[i0 + i] = (double)h_out[i];
        if (pooled_out) memcpy(pooled_out + (size_t)i0 * 4 * LL_C, h_pooled.data(), (size_t)nb * 4 * LL_C * 4);
    }
    hipStreamSynchronize(c->stream);
    if (d_part) hipFree(d_part);
    return rc;
}
