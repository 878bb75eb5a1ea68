// train_roi.hip -- MultiScaleRoIAlign (7 x 7, sampling_ratio 2, aligned=False; torchvision 0.8.2 ops/poolers.py, roi_align) on a dense batch:
// the forward, and the backward that scatters the bilinear weights with FIXED-POINT integer atomics, so that it is deterministic.
#include "train_host.h"

struct RoiTrainArgs {
    const float* feat[4]; float* gfeat[4]; int H[4], W[4];
    int C, R;
    const float* rois;     // [R][5]: image index, x1, y1, x2, y2 (resized-image coordinates)
    float* out;            // forward: [R][49][C]
    const float* gout;     // backward: [R][49][C]
};
__device__ inline void roi_setup(const RoiTrainArgs& a, int r, RoiSample* sy, RoiSample* sx, int* n_out, int* l_out) {
    const float* rp = a.rois + (long long)r * 5;
    const float4 box = make_float4(rp[1], rp[2], rp[3], rp[4]);
    const int l = roi_level(box), tid = threadIdx.x;
    if (tid < 28) {
        const float scale = 1.0f / (float)(4 << l);
        const float x1 = box.x * scale, y1 = box.y * scale, x2 = box.z * scale, y2 = box.w * scale;
        float rw = x2 - x1; if (!(rw >= 1.0f)) rw = 1.0f;
        float rh = y2 - y1; if (!(rh >= 1.0f)) rh = 1.0f;
        const float bw = rw / 7.0f, bh = rh / 7.0f;
        if (tid < 14) sy[tid] = roi_sample(y1, bh, tid >> 1, tid & 1, a.H[l]);
        else sx[tid - 14] = roi_sample(x1, bw, (tid - 14) >> 1, (tid - 14) & 1, a.W[l]);
    }
    *n_out = (int)rp[0]; *l_out = l;
    __syncthreads();
}
// forward: a thread owns (bin, 4 consecutive channels): 16 float4 gathers in flight per bin, one float4 store
__global__ __launch_bounds__(256) void roi_align_train_kernel(RoiTrainArgs a) {
    __shared__ RoiSample sy[14], sx[14];
    const int r = blockIdx.x, tid = threadIdx.x;
    int n, l;
    roi_setup(a, r, sy, sx, &n, &l);
    const int Hf = a.H[l], Wf = a.W[l], Cq = a.C >> 2;
    const float4* f = reinterpret_cast<const float4*>(a.feat[l]) + (long long)n * Hf * Wf * Cq;
    for (int idx = tid; idx < 49 * Cq; idx += 256) {
        const int bin = idx / Cq, q = idx - bin * Cq;
        const int ph = bin / 7, pw = bin - ph * 7;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int iy = 0; iy < 2; iy++) {
            const RoiSample Y = sy[ph * 2 + iy];
#pragma unroll
            for (int ix = 0; ix < 2; ix++) {
                const RoiSample X = sx[pw * 2 + ix];
                if (!(Y.valid && X.valid)) continue;
                const float w1 = Y.h * X.h, w2 = Y.h * X.l, w3 = Y.l * X.h, w4 = Y.l * X.l;
                const float4 v1 = f[(long long)(Y.lo * Wf + X.lo) * Cq + q], v2 = f[(long long)(Y.lo * Wf + X.hi) * Cq + q];
                const float4 v3 = f[(long long)(Y.hi * Wf + X.lo) * Cq + q], v4 = f[(long long)(Y.hi * Wf + X.hi) * Cq + q];
                acc.x = acc.x + (((w1 * v1.x + w2 * v2.x) + w3 * v3.x) + w4 * v4.x);
                acc.y = acc.y + (((w1 * v1.y + w2 * v2.y) + w3 * v3.y) + w4 * v4.y);
                acc.z = acc.z + (((w1 * v1.z + w2 * v2.z) + w3 * v3.z) + w4 * v4.z);
                acc.w = acc.w + (((w1 * v1.w + w2 * v2.w) + w3 * v3.w) + w4 * v4.w);
            }
        }
        reinterpret_cast<float4*>(a.out)[(long long)r * 49 * Cq + idx] = make_float4(acc.x / 4.0f, acc.y / 4.0f, acc.z / 4.0f, acc.w / 4.0f);
    }
}
static int roi_args(RoiTrainArgs& a, const float* const* feats, float* const* gfeats, const int* level_hw, int C, int R, const float* rois) {
    if (C % 4 || R < 1 || !rois || !level_hw) return cald_internal_fail(CALD_ERR_INVALID, "bad RoIAlign arguments");
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < 4; l++) { a.feat[l] = feats ? feats[l] : nullptr; a.gfeat[l] = gfeats ? gfeats[l] : nullptr; a.H[l] = level_hw[2 * l]; a.W[l] = level_hw[2 * l + 1]; }
    a.C = C; a.R = R; a.rois = rois;
    return 0;
}
extern "C" int cald_train_roi_align(cald_ctx* c, const float* const* feats, const int* level_hw, int C, int R, const float* rois, float* out) {
    if (!c || !feats || !out) TFAIL(CALD_ERR_INVALID, "null argument");
    THIP(hipSetDevice(cald_internal_device(c)));
    RoiTrainArgs a; if (int rc = roi_args(a, feats, nullptr, level_hw, C, R, rois)) return rc;
    a.out = out;
    hipLaunchKernelGGL(roi_align_train_kernel, dim3(R), dim3(256), 0, cald_internal_stream(c), a);
    THIP(hipGetLastError());
    return 0;
}
// Deterministic scatter: contributions are accumulated as 64-bit FIXED-POINT integers (integer addition is associative, so the
// arrival order of the atomics does not matter), scaled by 2^k with k chosen from max|gout| so that the largest single term is
// 2^40 (resolution 2^-40 of it; 2^21 such terms still fit), then converted and added to the float gradient.
__global__ void absmax_kernel(const float* x, long long n, unsigned* out_bits) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float m = 0.0f;
    for (long long j = i; j < n; j += (long long)gridDim.x * blockDim.x) { const float v = fabsf(x[j]); if (v > m && v != INFINITY) m = v; }   // NaN and Inf never win
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(out_bits, __float_as_uint(m));
}
__device__ inline double fixed_scale(unsigned max_bits) {
    const int e = (int)((max_bits >> 23) & 255) - 127;          // max = 1.f x 2^e  (0 if the tensor is all zero)
    return max_bits ? ldexp(1.0, 40 - (e + 1)) : 1.0;
}
struct RoiAccPtrs { long long* p[4]; };
// backward: a thread owns (bin, ONE channel), consecutive lanes = consecutive channels, so that every atomic instruction of a
// wavefront lands on 256 contiguous bytes (two cache lines) of one feature pixel
__global__ __launch_bounds__(256) void roi_align_bwd_fixed_kernel(RoiTrainArgs a, RoiAccPtrs acc, const unsigned* max_bits) {
    __shared__ RoiSample sy[14], sx[14];
    const int r = blockIdx.x, tid = threadIdx.x;
    int n, l;
    roi_setup(a, r, sy, sx, &n, &l);
    const int Hf = a.H[l], Wf = a.W[l], C = a.C;
    unsigned long long* gf = reinterpret_cast<unsigned long long*>(acc.p[l]) + (long long)n * Hf * Wf * C;
    const double scale = fixed_scale(*max_bits);
    for (int idx = tid; idx < 49 * C; idx += 256) {
        const int bin = idx / C, c = idx - bin * C;
        const int ph = bin / 7, pw = bin - ph * 7;
        const float go = a.gout[(long long)r * 49 * C + idx] * 0.25f;
        if (!(go == go) || fabsf(go) == INFINITY) continue;          // non-finite gradients are reported by the loss check, not spread
#pragma unroll
        for (int iy = 0; iy < 2; iy++) {
            const RoiSample Y = sy[ph * 2 + iy];
#pragma unroll
            for (int ix = 0; ix < 2; ix++) {
                const RoiSample X = sx[pw * 2 + ix];
                if (!(Y.valid && X.valid)) continue;
                const float w[4] = {Y.h * X.h, Y.h * X.l, Y.l * X.h, Y.l * X.l};
                const long long o[4] = {(long long)(Y.lo * Wf + X.lo) * C + c, (long long)(Y.lo * Wf + X.hi) * C + c,
                                        (long long)(Y.hi * Wf + X.lo) * C + c, (long long)(Y.hi * Wf + X.hi) * C + c};
#pragma unroll
                for (int k = 0; k < 4; k++)
                    atomicAdd(gf + o[k], (unsigned long long)(long long)rint((double)(w[k] * go) * scale));      // two's complement wrap = signed add
            }
        }
    }
}
// C == 256: the 16 contributions of a (bin, channel) -- 2 x 2 samples x 4 bilinear taps -- fall on far fewer than 16 feature pixels
// (the two samples of a bin are half a bin apart: usually they share a pixel row / column or sit on the same ones).  The integer
// contributions are summed per distinct pixel in registers first -- exact, the accumulation is integer -- and one atomic goes out per
// pixel.  Which samples share rows / columns is the same for the whole workgroup (one bin per pass), so the sharing pattern is a
// scalar branch:  P 0: slots (lo0, hi0, lo1, hi1);  P 1: lo1 == hi0 -> (lo0, hi0, hi1);  P 2: sample 1 on sample 0's pair -> (lo0, hi0).
template <int PR, int PC>
__device__ __forceinline__ void roi_bwd_bin(unsigned long long* const gf, const int Wf, const int c, const float go, const double scale,
                                            const RoiSample Y0, const RoiSample Y1, const RoiSample X0, const RoiSample X1) {
    constexpr int NRS = PR == 0 ? 4 : (PR == 1 ? 3 : 2), NCS = PC == 0 ? 4 : (PC == 1 ? 3 : 2);
    long long acc[NRS][NCS];
#pragma unroll
    for (int i = 0; i < NRS; i++)
#pragma unroll
        for (int j = 0; j < NCS; j++) acc[i][j] = 0;
#pragma unroll
    for (int iy = 0; iy < 2; iy++) {
        const RoiSample Y = iy ? Y1 : Y0;
        const int rl = iy == 0 ? 0 : (PR == 0 ? 2 : (PR == 1 ? 1 : 0)), rh = iy == 0 ? 1 : (PR == 0 ? 3 : (PR == 1 ? 2 : 1));
#pragma unroll
        for (int ix = 0; ix < 2; ix++) {
            const RoiSample X = ix ? X1 : X0;
            const int cl = ix == 0 ? 0 : (PC == 0 ? 2 : (PC == 1 ? 1 : 0)), ch = ix == 0 ? 1 : (PC == 0 ? 3 : (PC == 1 ? 2 : 1));
            if (!(Y.valid && X.valid)) continue;
            acc[rl][cl] += (long long)rint((double)((Y.h * X.h) * go) * scale);
            acc[rl][ch] += (long long)rint((double)((Y.h * X.l) * go) * scale);
            acc[rh][cl] += (long long)rint((double)((Y.l * X.h) * go) * scale);
            acc[rh][ch] += (long long)rint((double)((Y.l * X.l) * go) * scale);
        }
    }
    const int rows[4] = {Y0.lo, Y0.hi, PR == 1 ? Y1.hi : Y1.lo, Y1.hi};
    const int cols[4] = {X0.lo, X0.hi, PC == 1 ? X1.hi : X1.lo, X1.hi};
#pragma unroll
    for (int i = 0; i < NRS; i++)
#pragma unroll
        for (int j = 0; j < NCS; j++)
            if (acc[i][j]) atomicAdd(gf + (long long)(rows[i] * Wf + cols[j]) * 256 + c, (unsigned long long)acc[i][j]);
}
__global__ __launch_bounds__(256) void roi_align_bwd_fixed_merge_kernel(RoiTrainArgs a, RoiAccPtrs acc, const unsigned* max_bits) {
    __shared__ RoiSample sy[14], sx[14];
    const int r = blockIdx.x, tid = threadIdx.x;
    int n, l;
    roi_setup(a, r, sy, sx, &n, &l);
    const int Hf = a.H[l], Wf = a.W[l];
    unsigned long long* gf = reinterpret_cast<unsigned long long*>(acc.p[l]) + (long long)n * Hf * Wf * 256;
    const double scale = fixed_scale(*max_bits);
    for (int bin = 0; bin < 49; bin++) {
        const int ph = bin / 7, pw = bin - ph * 7;
        float go = a.gout[((long long)r * 49 + bin) * 256 + tid] * 0.25f;
        if (!(go == go) || fabsf(go) == INFINITY) go = 0.0f;          // non-finite gradients are reported by the loss check, not spread
        const RoiSample Y0 = sy[ph * 2], Y1 = sy[ph * 2 + 1], X0 = sx[pw * 2], X1 = sx[pw * 2 + 1];
        const int y0l = __builtin_amdgcn_readfirstlane(Y0.lo), y0h = __builtin_amdgcn_readfirstlane(Y0.hi);
        const int y1l = __builtin_amdgcn_readfirstlane(Y1.lo), y1h = __builtin_amdgcn_readfirstlane(Y1.hi);
        const int x0l = __builtin_amdgcn_readfirstlane(X0.lo), x0h = __builtin_amdgcn_readfirstlane(X0.hi);
        const int x1l = __builtin_amdgcn_readfirstlane(X1.lo), x1h = __builtin_amdgcn_readfirstlane(X1.hi);
        const int pr = (y1l == y0l && y1h == y0h) ? 2 : (y1l == y0h ? 1 : 0);
        const int pc = (x1l == x0l && x1h == x0h) ? 2 : (x1l == x0h ? 1 : 0);
        switch (pr * 3 + pc) {
            case 0: roi_bwd_bin<0, 0>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 1: roi_bwd_bin<0, 1>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 2: roi_bwd_bin<0, 2>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 3: roi_bwd_bin<1, 0>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 4: roi_bwd_bin<1, 1>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 5: roi_bwd_bin<1, 2>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 6: roi_bwd_bin<2, 0>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            case 7: roi_bwd_bin<2, 1>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
            default: roi_bwd_bin<2, 2>(gf, Wf, tid, go, scale, Y0, Y1, X0, X1); break;
        }
    }
}
// two accumulators per thread; the scale is a power of two, so multiplying by its reciprocal is the exact division
__global__ void fixed_to_float_kernel(const long long* acc, float* g, long long n, const unsigned* max_bits) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i >= n) return;
    const double inv = 1.0 / fixed_scale(*max_bits);
    if (i + 1 < n) {
        const longlong2 v = *reinterpret_cast<const longlong2*>(acc + i);
        if (v.x | v.y) {
            float2 o = *reinterpret_cast<float2*>(g + i);
            if (v.x) o.x = o.x + (float)((double)v.x * inv);
            if (v.y) o.y = o.y + (float)((double)v.y * inv);
            *reinterpret_cast<float2*>(g + i) = o;
        }
    } else {
        const long long v = acc[i];
        if (v) g[i] = g[i] + (float)((double)v * inv);
    }
}
/* gfeats[l] += scatter of gout through the bilinear weights.  Deterministic (fixed-point accumulation, see above). */
extern "C" int cald_train_roi_align_bwd(cald_ctx* c, int N, float* const* gfeats, const int* level_hw, int C, int R, const float* rois, const float* gout) {
    if (!c || !gfeats || !gout || N < 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    RoiTrainArgs a; if (int rc = roi_args(a, (const float* const*)gfeats, gfeats, level_hw, C, R, rois)) return rc;
    a.gout = gout;
    long long n[4], total = 0;
    for (int l = 0; l < 4; l++) { n[l] = (long long)N * a.H[l] * a.W[l] * C; total += (n[l] + 1) & ~1ll; }
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, (size_t)total * 8 + 256, &scratch)) return rc;
    long long* acc = (long long*)scratch;
    unsigned* d_max = (unsigned*)(acc + total);
    RoiAccPtrs ptrs; long long off = 0;
    for (int l = 0; l < 4; l++) { ptrs.p[l] = acc + off; off += (n[l] + 1) & ~1ll; }     // 16-byte aligned level bases
    THIP(hipMemsetAsync(acc, 0, (size_t)total * 8 + 4, st));
    const long long ng = (long long)R * 49 * C;
    hipLaunchKernelGGL(absmax_kernel, dim3(1024), dim3(256), 0, st, gout, ng, d_max);
    static const bool merge = !(getenv("CALD_ROI_BWD_MERGE") && atoi(getenv("CALD_ROI_BWD_MERGE")) == 0);
    if (merge && C == 256) hipLaunchKernelGGL(roi_align_bwd_fixed_merge_kernel, dim3(R), dim3(256), 0, st, a, ptrs, (const unsigned*)d_max);
    else hipLaunchKernelGGL(roi_align_bwd_fixed_kernel, dim3(R), dim3(256), 0, st, a, ptrs, (const unsigned*)d_max);
    for (int l = 0; l < 4; l++)
        hipLaunchKernelGGL(fixed_to_float_kernel, dim3((unsigned)((n[l] + 511) / 512)), dim3(256), 0, st, (const long long*)ptrs.p[l], gfeats[l], n[l], (const unsigned*)d_max);
    THIP(hipGetLastError());
    return 0;
}
