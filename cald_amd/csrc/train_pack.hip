// train_pack.hip -- weight packing ON THE DEVICE, every step, from the torch-layout parameter tensors into what the inference conv kernels
// (conv_p4.hip / conv_mfma.hip) read: forward packs, and the spatially flipped, channel-transposed filter on which the same kernels compute
// the data gradient, and -- for a forward_precision / backward_precision "f16x3" trainer -- the split-fp16 twin of a forward / data-gradient
// pack that conv_h3.hip / conv_h4.hip read.
// cald_train_packed_floats, cald_train_pack_conv(16), and the cald_train_pack_plan_* family (every layer's packs in two launches).
#include "train_host.h"

// mode 0: forward      K rows = (tap, ci) of a Cin_k-channel input (Cin_k >= Cin, the input buffer's channel stride), N = Cout
// mode 1: data grad    K rows = (flipped tap, co) of a Cin_k-channel dY (Cin_k >= Cout),                      N = Cin
// mode 2: forward of a linear layer whose torch weight is [Cout][Cin][taps] (fc6: [1024][256][7*7]) applied to rows laid out
//         [tap][Cin] (the RoIAlign output [R][49][256]): K rows = tap * Cin + ci
// mode 3: data gradient of a mode-2 layer: K rows = co of a CinK-channel dY, N = tap * Cin + ci
// w16 (or null): the split-fp16 twin conv_h3.hip / conv_h4.hip read, [Kpad/16][2 (hi, lo)][NPad][16] of w * 2^S -- of a data-gradient pack:
// of the values the fp32 pack holds (transposed, flipped, rowscale folded in)
struct PackArgs { const float* w; float* wk; float* w4; int Cout, Cin, taps, CinK, Kpad, NPad, mode; const float* rowscale; unsigned short* w16; int S; };
__device__ __forceinline__ void pack_weight_body(const PackArgs& a, long long blk) {
    const long long i = blk * 256 + threadIdx.x;
    if (i >= (long long)a.Kpad * a.NPad) return;
    const int k = (int)(i / a.NPad), n = (int)(i - (long long)k * a.NPad);
    int tap, ci;
    if (a.mode == 2) { tap = k / a.Cin; ci = k - tap * a.Cin; }
    else if (a.mode == 3) { tap = 0; ci = k; }
    else if (a.CinK % 16 == 0 && a.taps <= 32) { const int chunk = k / (16 * a.taps), rem = k - chunk * 16 * a.taps; tap = rem >> 4; ci = chunk * 16 + (rem & 15); }
    else { tap = k / a.CinK; ci = k - tap * a.CinK; }
    float v = 0.0f;
    if (a.mode == 1) {
        if (tap < a.taps && ci < a.Cout && n < a.Cin) v = a.w[((long long)ci * a.Cin + n) * a.taps + (a.taps - 1 - tap)];
        if (a.rowscale && ci < a.Cout) v = v * a.rowscale[ci];       // FrozenBatchNorm scale of the forward layer's output channel
    } else if (a.mode == 3) {
        const int t = n / a.Cin, cc = n - t * a.Cin;
        if (ci < a.Cout && t < a.taps) v = a.w[((long long)ci * a.Cin + cc) * a.taps + t];
        if (a.rowscale && ci < a.Cout) v = v * a.rowscale[ci];
    } else {
        if (tap < a.taps && ci < a.Cin && n < a.Cout) v = a.w[((long long)n * a.Cin + ci) * a.taps + tap];
    }
    a.wk[i] = v;
    const int kt = k >> 4, kk = k & 15, kq = kk >> 3, j = (kk & 7) >> 1, h = kk & 1;
    a.w4[(((long long)(kt * 2 + kq) * a.NPad + n) * 2 + h) * 4 + j] = v;
    if (!a.w16) return;
    // the split twin of a data-gradient pack, the arithmetic of pack_transpose_body's: hi = fp16(v * 2^S), lo = fp16(v * 2^S - hi)
    const float x = ldexpf(v, a.S);
    const _Float16 hi = (_Float16)x;
    const _Float16 lo = (_Float16)(x - (float)hi);
    const long long o = ((long long)kt * 2 * a.NPad + n) * 16 + kk;
    a.w16[o] = __builtin_bit_cast(unsigned short, hi);
    a.w16[o + (long long)a.NPad * 16] = __builtin_bit_cast(unsigned short, lo);
}
__global__ __launch_bounds__(256) void pack_weight_kernel(PackArgs a) { pack_weight_body(a, blockIdx.x); }
// Forward packs (modes 0, 2) in two coalesced passes: (1) every torch row n (Cin * taps contiguous floats) is read in order and
// written to T[n][k] (k = position in the chain order: neighbours stay inside one 16-channel chunk); (2) a tiled LDS transpose
// T[n][k] -> wk[k][n] + the conv_p4 layout.  (pack_weight_kernel reads with a stride of one whole row between lanes.)
__device__ __forceinline__ void pack_rows_body(const PackArgs& a, float* T, long long blk) {
    const long long i = blk * 256 + threadIdx.x;
    const long long row = (long long)a.Cin * a.taps;
    if (i >= (long long)a.Cout * row) return;
    const int n = (int)(i / row); const int r = (int)(i - (long long)n * row);
    const int ci = r / a.taps, tap = r - ci * a.taps;
    int k;
    if (a.mode == 2) k = tap * a.Cin + ci;
    else k = (a.CinK % 16 == 0 && a.taps <= 32) ? ((ci >> 4) * a.taps + tap) * 16 + (ci & 15) : tap * a.CinK + ci;
    T[(long long)n * a.Kpad + k] = a.w[i];
}
__global__ __launch_bounds__(256) void pack_rows_kernel(PackArgs a, float* T) { pack_rows_body(a, T, blockIdx.x); }
__device__ __forceinline__ void pack_transpose_body(const PackArgs& a, const float* T, int bx, int by) {
    __shared__ float tile[32][33];
    const int k0 = bx * 32, n0 = by * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, k = k0 + tx;
        tile[r][tx] = (n < a.Cout && k < a.Kpad) ? T[(long long)n * a.Kpad + k] : 0.0f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, n = n0 + tx;
        if (k >= a.Kpad || n >= a.NPad) continue;
        const float v = tile[tx][r];
        a.wk[(long long)k * a.NPad + n] = v;
        const int kt = k >> 4, kk = k & 15, kq = kk >> 3, j = (kk & 7) >> 1, h = kk & 1;
        a.w4[(((long long)(kt * 2 + kq) * a.NPad + n) * 2 + h) * 4 + j] = v;
    }
    if (!a.w16) return;
    // the split twin of the same 32 x 32 tile (model.hip pack_w16, byte for byte): hi = fp16(w * 2^S), lo = fp16(w * 2^S - hi).  16 lanes
    // write the 16 k of one (k-tile, n) -- 32 contiguous bytes -- and the 32 n of the tile follow each other: 1 KB runs per plane
    for (int it = 0; it < 4; it++) {
        const int idx = threadIdx.x + 256 * it, kk = idx & 15, nl = (idx >> 4) & 31, ktl = idx >> 9;
        const int k = k0 + ktl * 16 + kk, n = n0 + nl;
        if (k >= a.Kpad || n >= a.NPad) continue;
        const float x = ldexpf(tile[nl][ktl * 16 + kk], a.S);
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        const long long o = ((long long)(k >> 4) * 2 * a.NPad + n) * 16 + kk;
        a.w16[o] = __builtin_bit_cast(unsigned short, hi);
        a.w16[o + (long long)a.NPad * 16] = __builtin_bit_cast(unsigned short, lo);
    }
}
__global__ __launch_bounds__(256) void pack_transpose_kernel(PackArgs a, const float* T) { pack_transpose_body(a, T, blockIdx.x, blockIdx.y); }
__device__ __forceinline__ void pack_vec_body(const float* bias, const float* scale, const float* shift, int n, float* dst, int npad, int blk) {
    const int i = blk * 256 + threadIdx.x;
    if (i >= npad) return;
    dst[i] = (bias && i < n) ? bias[i] : 0.0f;
    dst[npad + i] = (scale && i < n) ? scale[i] : 0.0f;
    dst[2 * npad + i] = (shift && i < n) ? shift[i] : 0.0f;
}
__global__ __launch_bounds__(256) void pack_vec_kernel(const float* bias, const float* scale, const float* shift, int n, float* dst, int npad) {
    pack_vec_body(bias, scale, shift, n, dst, npad, blockIdx.x);
}
// Every trainable layer's packs in TWO launches (cald_train_pack_plan_*): the optimizer changes all weights at once, and ~220 launches of
// 2 - 9 us each kept the side stream busy for 1.5 ms at the start of a step -- longer than the frozen stem + layer 1 the main stream
// runs meanwhile.  A launch covers a list of segments (kind, job, first block); a workgroup finds its segment by bisection.
struct PackJobDev { PackArgs a; float* T; const float *bias, *scale, *shift; float* vec; int n_true, gx; };
struct PackSeg { int kind, job; unsigned first; };          // kind 0 rows (modes 0 / 2), 1 whole pack (modes 1 / 3), 2 epilogue vectors, 3 transpose
__global__ __launch_bounds__(256) void pack_plan_kernel(const PackSeg* __restrict__ segs, int nseg, const PackJobDev* __restrict__ jobs) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (segs[mid].first <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const PackSeg sg = segs[lo];
    const PackJobDev& j = jobs[sg.job];
    const unsigned blk = blockIdx.x - sg.first;
    if (sg.kind == 0) pack_rows_body(j.a, j.T, blk);
    else if (sg.kind == 1) pack_weight_body(j.a, blk);
    else if (sg.kind == 2) pack_vec_body(j.bias, j.scale, j.shift, j.n_true, j.vec, j.a.NPad, (int)blk);
    else pack_transpose_body(j.a, j.T, (int)(blk % (unsigned)j.gx), (int)(blk / (unsigned)j.gx));
}
// CinK is the channel stride of the tensor the pack is applied to: the contracted channels (Cin forward, Cout for a data gradient) padded to
// whole float4s.  Mode 2 contracts [tap][Cin] rows and takes no CinK.
#define CINK_RULE "CinK must be a multiple of 4 and cover the contracted channels"
static bool cink_ok(int Cout, int Cin, int CinK, int mode) { return mode == 2 || (CinK % 4 == 0 && CinK >= (mode == 0 ? Cin : Cout)); }
extern "C" int cald_train_packed_floats(int Cout, int Cin, int KH, int KW, int CinK, int mode, int64_t* floats_out) {
    if (!floats_out || Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || mode < 0 || mode > 3) TFAIL(CALD_ERR_INVALID, "bad arguments");
    *floats_out = pack_geom(Cout, Cin, KH, KW, CinK, mode).floats;
    return 0;
}
// The split twin exists for forward packs of the shapes conv_h3.hip takes (model.hip pack_conv's `tiled`), and for data-gradient packs
// whose data gradient -- a stride-1 conv over CinK channels of dY -- conv_h3.hip takes: 0 bytes otherwise.
static long long w16_bytes(const PackGeom& g, int taps, int mode) {
    return (h3_takes(g, taps, mode) || h3_takes_grad(g, taps, mode)) ? 4ll * g.Kpad * g.NPad : 0;
}
#define W16_RULE "a split twin needs a pack of a shape conv_h3 takes (cald_train_packed16_bytes / cald_train_packed_grad16_bytes > 0) and |S| <= 40"
extern "C" int cald_train_packed16_bytes(int Cout, int Cin, int KH, int KW, int CinK, int mode, int64_t* bytes_out) {
    if (!bytes_out || Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || mode < 0 || mode > 3) TFAIL(CALD_ERR_INVALID, "bad arguments");
    const PackGeom g = pack_geom(Cout, Cin, KH, KW, CinK, mode);
    *bytes_out = h3_takes(g, KH * KW, mode) ? w16_bytes(g, KH * KW, mode) : 0;
    return 0;
}
extern "C" int cald_train_packed_grad16_bytes(int Cout, int Cin, int KH, int KW, int CinK, int mode, int64_t* bytes_out) {
    if (!bytes_out || Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || mode < 0 || mode > 3) TFAIL(CALD_ERR_INVALID, "bad arguments");
    const PackGeom g = pack_geom(Cout, Cin, KH, KW, CinK, mode);
    *bytes_out = h3_takes_grad(g, KH * KW, mode) ? w16_bytes(g, KH * KW, mode) : 0;
    return 0;
}
// model.hip pack_w16's scale: max |w| = f * 2^e, f in [0.5, 1) -> S = 14 - e, clamped to +-40; 0 for an all-zero or non-finite tensor
extern "C" int cald_train_f16x3_scale(float max_abs, int* S_out, float* unscale_out) {
    if (!S_out || !unscale_out) TFAIL(CALD_ERR_INVALID, "null argument");
    int S = 0;
    if (max_abs > 0.0f && std::isfinite(max_abs)) { int e; std::frexp(max_abs, &e); S = 14 - e; }
    if (S > 40) S = 40;
    if (S < -40) S = -40;
    *S_out = S; *unscale_out = std::ldexp(1.0f, -(S + 4));
    return 0;
}
// The input scale of a data-gradient launch on conv_h3.hip from the largest |g| of the gradient tensor it reads (a backward_precision
// "f16x3" trainer reads it on its calibration step): max |g| = f * 2^e, f in [0.5, 1) -> G = 7 - e, so that max |g| * 2^(4 + G) lies in
// [2^10, 2^11) -- x 32 of growth before fp16 overflows at 65 504, x 2^13 of shrink before the tensor's largest entry loses a bit of its lo
// half.  Clamped to +-60; 0 for an all-zero or non-finite tensor.  in_scale = 2^(4 + G).
extern "C" int cald_train_f16x3_grad_scale(float max_abs, int* G_out, float* in_scale_out) {
    if (!G_out || !in_scale_out) TFAIL(CALD_ERR_INVALID, "null argument");
    int G = 0;
    if (max_abs > 0.0f && std::isfinite(max_abs)) { int e; std::frexp(max_abs, &e); G = 7 - e; }
    if (G > 60) G = 60;
    if (G < -60) G = -60;
    *G_out = G; *in_scale_out = std::ldexp(1.0f, 4 + G);
    return 0;
}
static int pack_conv(cald_ctx* c, const float* w, const float* bias, const float* scale, const float* shift,
                     int Cout, int Cin, int KH, int KW, int CinK, int mode, float* packed, void* w16, int S) {
    if (!c || !w || !packed) TFAIL(CALD_ERR_INVALID, "null argument");
    if (mode < 0 || mode > 3) TFAIL(CALD_ERR_INVALID, "mode must be 0 (forward), 1 (data gradient), 2 (tap-major linear) or 3 (its data gradient)");
    if (!cink_ok(Cout, Cin, CinK, mode)) TFAIL(CALD_ERR_INVALID, CINK_RULE);
    THIP(hipSetDevice(cald_internal_device(c)));
    const PackGeom g = pack_geom(Cout, Cin, KH, KW, CinK, mode);
    if (w16 && (!w16_bytes(g, KH * KW, mode) || S < -40 || S > 40)) TFAIL(CALD_ERR_INVALID, W16_RULE);
    PackArgs a{w, packed, packed + (long long)g.Kpad * g.NPad, Cout, Cin, KH * KW, CinK, g.Kpad, g.NPad, mode, (mode == 1 || mode == 3) ? scale : nullptr,
               (unsigned short*)w16, S};
    hipStream_t st = cald_internal_stream(c);
    const long long n = (long long)g.Kpad * g.NPad;
    if (mode == 0 || mode == 2) {
        void* scratch = nullptr;
        const long long tn = (long long)Cout * g.Kpad;
        if (int rc = cald_internal_scratch(c, (size_t)tn * 4, &scratch)) return rc;
        float* T = (float*)scratch;
        if (g.Kpad != Cin * KH * KW)     // k positions no source element maps to (channel / K padding)
            THIP(hipMemsetAsync(T, 0, (size_t)tn * 4, st));
        const long long src = (long long)Cout * Cin * KH * KW;
        hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((src + 255) / 256)), dim3(256), 0, st, a, T);
        hipLaunchKernelGGL(pack_transpose_kernel, dim3((g.Kpad + 31) / 32, (g.NPad + 31) / 32), dim3(256), 0, st, a, (const float*)T);
    } else {
        hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    }
    float* vec = packed + 2 * n;
    const int nt = g.n_true, blocks = (g.NPad + 255) / 256;
    if (mode == 0 || mode == 2)     // the data-gradient packs carry no epilogue vectors (cald_train_conv never reads them: flags 0)
        hipLaunchKernelGGL(pack_vec_kernel, dim3(blocks), dim3(256), 0, st, bias, scale, shift, nt, vec, g.NPad);
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_pack_conv(cald_ctx* c, const float* w, const float* bias, const float* scale, const float* shift,
                                    int Cout, int Cin, int KH, int KW, int CinK, int mode, float* packed) {
    return pack_conv(c, w, bias, scale, shift, Cout, Cin, KH, KW, CinK, mode, packed, nullptr, 0);
}
extern "C" int cald_train_pack_conv16(cald_ctx* c, const float* w, const float* bias, const float* scale, const float* shift,
                                      int Cout, int Cin, int KH, int KW, int CinK, int mode, float* packed, void* w16, int S) {
    if (!w16) TFAIL(CALD_ERR_INVALID, "null argument");
    return pack_conv(c, w, bias, scale, shift, Cout, Cin, KH, KW, CinK, mode, packed, w16, S);
}

struct cald_pack_plan {
    int device; PackSeg *seg1, *seg2; PackJobDev* jobs; int nseg1, nseg2; unsigned blocks1, blocks2;
};
static long long plan_round64(long long x) { return (x + 63) / 64 * 64; }
static int pack_plan_check(int n, const cald_pack_job* jobs) {
    if (n < 1 || !jobs) TFAIL(CALD_ERR_INVALID, "no jobs");
    for (int i = 0; i < n; i++) {
        const cald_pack_job& q = jobs[i];
        if (!q.weight || !q.packed) TFAIL(CALD_ERR_INVALID, "job %d: null weight / packed", i);
        if (q.Cout < 1 || q.Cin < 1 || q.KH < 1 || q.KW < 1 || q.mode < 0 || q.mode > 3) TFAIL(CALD_ERR_INVALID, "job %d: bad shape / mode", i);
        if (!cink_ok(q.Cout, q.Cin, q.CinK, q.mode)) TFAIL(CALD_ERR_INVALID, "job %d: " CINK_RULE, i);
        if (q.w16 && (!w16_bytes(pack_geom(q.Cout, q.Cin, q.KH, q.KW, q.CinK, q.mode), q.KH * q.KW, q.mode) || q.w16_S < -40 || q.w16_S > 40))
            TFAIL(CALD_ERR_INVALID, "job %d: " W16_RULE, i);
    }
    return 0;
}
extern "C" int cald_train_pack_plan_scratch_floats(int n, const cald_pack_job* jobs, int64_t* floats_out) {
    if (!floats_out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (int rc = pack_plan_check(n, jobs)) return rc;
    long long tot = 0;
    for (int i = 0; i < n; i++) {
        const cald_pack_job& q = jobs[i];
        if (q.mode == 0 || q.mode == 2) tot += plan_round64((long long)q.Cout * pack_geom(q.Cout, q.Cin, q.KH, q.KW, q.CinK, q.mode).Kpad);
    }
    *floats_out = tot;
    return 0;
}
extern "C" int cald_train_pack_plan_create(cald_ctx* c, int n, const cald_pack_job* jobs, float* scratch, int64_t scratch_floats, cald_pack_plan** out) {
    if (!c || !out) TFAIL(CALD_ERR_INVALID, "null argument");
    int64_t need = 0;
    if (int rc = cald_train_pack_plan_scratch_floats(n, jobs, &need)) return rc;
    if (need && (!scratch || scratch_floats < need)) TFAIL(CALD_ERR_INVALID, "scratch of %lld floats needed", (long long)need);
    THIP(hipSetDevice(cald_internal_device(c)));
    std::vector<PackJobDev> dj(n);
    std::vector<PackSeg> s1, s2;
    unsigned b1 = 0, b2 = 0;
    long long toff = 0;
    for (int i = 0; i < n; i++) {
        const cald_pack_job& q = jobs[i];
        const PackGeom g = pack_geom(q.Cout, q.Cin, q.KH, q.KW, q.CinK, q.mode);
        const long long nn = (long long)g.Kpad * g.NPad;
        const bool fwd = q.mode == 0 || q.mode == 2;
        PackJobDev& d = dj[i];
        d.a = PackArgs{q.weight, q.packed, q.packed + nn, q.Cout, q.Cin, q.KH * q.KW, q.CinK, g.Kpad, g.NPad, q.mode, fwd ? nullptr : q.bn_scale,
                       (unsigned short*)q.w16, q.w16_S};
        d.T = nullptr; d.bias = q.bias; d.scale = q.bn_scale; d.shift = q.bn_shift; d.vec = q.packed + 2 * nn; d.n_true = g.n_true;
        d.gx = (g.Kpad + 31) / 32;
        if (fwd) {
            d.T = scratch + toff; toff += plan_round64((long long)q.Cout * g.Kpad);
            const long long src = (long long)q.Cout * q.Cin * q.KH * q.KW;
            s1.push_back(PackSeg{0, i, b1}); b1 += (unsigned)((src + 255) / 256);
            s1.push_back(PackSeg{2, i, b1}); b1 += (unsigned)((g.NPad + 255) / 256);
            s2.push_back(PackSeg{3, i, b2}); b2 += (unsigned)(d.gx * ((g.NPad + 31) / 32));
        } else {
            s1.push_back(PackSeg{1, i, b1}); b1 += (unsigned)((nn + 255) / 256);
        }
    }
    cald_pack_plan* p = new cald_pack_plan();
    p->device = cald_internal_device(c); p->seg1 = p->seg2 = nullptr; p->jobs = nullptr;
    p->nseg1 = (int)s1.size(); p->nseg2 = (int)s2.size(); p->blocks1 = b1; p->blocks2 = b2;
    auto fail = [&](hipError_t e) { hipFree(p->seg1); hipFree(p->seg2); hipFree(p->jobs); delete p; return cald_internal_fail(CALD_ERR_HIP, "pack plan: %s", hipGetErrorString(e)); };
    hipError_t e;
    if ((e = hipMalloc((void**)&p->jobs, sizeof(PackJobDev) * n)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&p->seg1, sizeof(PackSeg) * (s1.size() + 1))) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&p->seg2, sizeof(PackSeg) * (s2.size() + 1))) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->jobs, dj.data(), sizeof(PackJobDev) * n, hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(p->seg1, s1.data(), sizeof(PackSeg) * s1.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if (!s2.empty() && (e = hipMemcpy(p->seg2, s2.data(), sizeof(PackSeg) * s2.size(), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    // k positions no source element maps to (channel / K padding) stay zero for the plan's lifetime: the scratch is the plan's own
    // (on the context stream: ordered after whatever used this memory before and before the first cald_train_pack_plan_run)
    if (need && (e = hipMemsetAsync(scratch, 0, (size_t)need * 4, cald_internal_stream(c))) != hipSuccess) return fail(e);
    *out = p;
    return 0;
}
extern "C" int cald_train_pack_plan_run(cald_ctx* c, const cald_pack_plan* p) {
    if (!c || !p) TFAIL(CALD_ERR_INVALID, "null argument");
    if (p->device != cald_internal_device(c)) TFAIL(CALD_ERR_INVALID, "plan belongs to another device");
    THIP(hipSetDevice(p->device));
    hipStream_t st = cald_internal_stream(c);
    hipLaunchKernelGGL(pack_plan_kernel, dim3(p->blocks1), dim3(256), 0, st, (const PackSeg*)p->seg1, p->nseg1, (const PackJobDev*)p->jobs);
    if (p->blocks2) hipLaunchKernelGGL(pack_plan_kernel, dim3(p->blocks2), dim3(256), 0, st, (const PackSeg*)p->seg2, p->nseg2, (const PackJobDev*)p->jobs);
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_pack_plan_destroy(cald_pack_plan* p) {
    if (!p) return 0;
    hipSetDevice(p->device);
    hipFree(p->seg1); hipFree(p->seg2); hipFree(p->jobs);
    delete p;
    return 0;
}
