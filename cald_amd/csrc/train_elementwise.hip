// train_elementwise.hip -- the elementwise passes of the backward pass (ReLU / FrozenBatchNorm backward, gradient joins, the stride-2 data
// gradient's dilation, the FPN top-down backward) and the optimizer, sgd_kernel: torch.optim.SGD (weight decay, momentum, no dampening /
// nesterov; cald_train.py:397) over the flat parameter buffer.  All float4-wide and HBM-bound.
#include "train_host.h"

// g[q][c] = (act[q][c] > 0 ? g[q][c] : 0) * (scale ? scale[c] : 1): ReLU backward (act = the layer's post-ReLU output) and
// the FrozenBatchNorm scale in one pass.  act == null: scale only.
__global__ void relu_bwd_kernel(float* g, const float* act, const float* scale, long long n4, int C4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<float4*>(g)[i];
    if (act) { const float4 y = reinterpret_cast<const float4*>(act)[i]; if (!(y.x > 0.f)) v.x = 0.f; if (!(y.y > 0.f)) v.y = 0.f; if (!(y.z > 0.f)) v.z = 0.f; if (!(y.w > 0.f)) v.w = 0.f; }
    if (scale) { const float4 s = reinterpret_cast<const float4*>(scale)[i % C4]; v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w; }
    reinterpret_cast<float4*>(g)[i] = v;
}
void cald_train_host::launch_relu_bwd(float* g, const float* act, const float* scale, long long n4, int C4, hipStream_t st) {
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, g, act, scale, n4, C4);
}
extern "C" int cald_train_relu_bwd(cald_ctx* c, long long rows, int C, float* g, const float* act, const float* scale) {
    if (!c || !g || C % 4) TFAIL(CALD_ERR_INVALID, "bad arguments (C must be a multiple of 4)");
    THIP(hipSetDevice(cald_internal_device(c)));
    const long long n4 = rows * C / 4;
    if (n4 > 0) launch_relu_bwd(g, act, scale, n4, C / 4, cald_internal_stream(c));
    THIP(hipGetLastError());
    return 0;
}
// dst = a + b (b may be null: copy), float4 granularity
__global__ void add_kernel(float* dst, const float* a, const float* b, long long n4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = reinterpret_cast<const float4*>(a)[i];
    if (b) { const float4 w = reinterpret_cast<const float4*>(b)[i]; v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
    reinterpret_cast<float4*>(dst)[i] = v;
}
extern "C" int cald_train_add(cald_ctx* c, long long n, float* dst, const float* a, const float* b) {
    if (!c || !dst || !a || n % 4) TFAIL(CALD_ERR_INVALID, "bad arguments (n must be a multiple of 4)");
    THIP(hipSetDevice(cald_internal_device(c)));
    if (n > 0) hipLaunchKernelGGL(add_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, cald_internal_stream(c), dst, a, b, n / 4);
    THIP(hipGetLastError());
    return 0;
}
// dst[n][p][c] = (a + b) + g[n][c] / (float)HW: where the RPN branch's and the box head's gradients of a pyramid level are joined, the
// gradient of LossNet's global average pooling of that level (the same for every pixel) rides along -- no further pass over the maps.
// grid (float4s of one image / 256, N); the quotient is one IEEE division per float4 lane, HBM-bound like add_kernel (12 bytes per float).
__global__ void add_bcast_kernel(float* dst, const float* a, const float* b, const float* g, long long g_stride, unsigned per4, unsigned C4, float hw) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per4) return;
    const long long o = (long long)blockIdx.y * per4 + i;
    float4 v = reinterpret_cast<const float4*>(a)[o];
    const float4 w = reinterpret_cast<const float4*>(b)[o];
    const float4 q = reinterpret_cast<const float4*>(g + (long long)blockIdx.y * g_stride)[i % C4];
    v.x = (v.x + w.x) + q.x / hw; v.y = (v.y + w.y) + q.y / hw; v.z = (v.z + w.z) + q.z / hw; v.w = (v.w + w.w) + q.w / hw;
    reinterpret_cast<float4*>(dst)[o] = v;
}
extern "C" int cald_train_add_bcast(cald_ctx* c, int N, long long HW, int C, float* dst, const float* a, const float* b, const float* g, long long g_stride) {
    if (!c || !dst || !a || !b || !g || N < 1 || N > 65535 || HW < 1 || C < 4 || C % 4 || g_stride % 4 || g_stride < 0) TFAIL(CALD_ERR_INVALID, "bad arguments (C and g_stride must be multiples of 4)");
    if (HW > (1ll << 24) || HW * (C / 4) >= (1ll << 31)) TFAIL(CALD_ERR_INVALID, "map of %lld pixels x %d channels is too large", HW, C);
    THIP(hipSetDevice(cald_internal_device(c)));
    const unsigned per4 = (unsigned)(HW * (C / 4));
    hipLaunchKernelGGL(add_bcast_kernel, dim3((per4 + 255) / 256, N), dim3(256), 0, cald_internal_stream(c), dst, a, b, g, g_stride, per4, (unsigned)(C / 4), (float)HW);
    THIP(hipGetLastError());
    return 0;
}
// stride-s data gradient, step 1: scatter g [N][Ho][Wo][C] onto the stride-1 grid [N][Hd][Wd][C] (zeros elsewhere), Hd = (Ho-1)*s+1 + extra
__global__ void dilate_kernel(const float* g, float* out, int N, int Ho, int Wo, int Hd, int Wd, int C4, int s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n4 = (long long)N * Hd * Wd * C4;
    if (i >= n4) return;
    const int c = (int)(i % C4); long long p = i / C4;
    const int x = (int)(p % Wd); p /= Wd; const int y = (int)(p % Hd); const int n = (int)(p / Hd);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (y % s == 0 && x % s == 0 && y / s < Ho && x / s < Wo) v = reinterpret_cast<const float4*>(g)[(((long long)n * Ho + y / s) * Wo + x / s) * C4 + c];
    reinterpret_cast<float4*>(out)[i] = v;
}
extern "C" int cald_train_dilate(cald_ctx* c, int N, int Ho, int Wo, int C, int s, int Hd, int Wd, const float* g, float* out) {
    if (!c || !g || !out || C % 4 || s < 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    THIP(hipSetDevice(cald_internal_device(c)));
    const long long n4 = (long long)N * Hd * Wd * (C / 4);
    hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, cald_internal_stream(c), g, out, N, Ho, Wo, Hd, Wd, C / 4, s);
    THIP(hipGetLastError());
    return 0;
}
// FPN top-down backward: coarse[n][yc][xc][c] += sum of fine[n][yf][xf][c] over the fine pixels whose nearest source is (yc, xc)
// (F.interpolate(size=fine, mode='nearest'): source = floor(dst * coarse / fine))
__global__ void upsample_bwd_kernel(const float* fine, float* coarse, int N, int Hf, int Wf, int Hc, int Wc, int C4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n4 = (long long)N * Hc * Wc * C4;
    if (i >= n4) return;
    const int c = (int)(i % C4); long long p = i / C4;
    const int xc = (int)(p % Wc); p /= Wc; const int yc = (int)(p % Hc); const int n = (int)(p / Hc);
    // fine rows y with floor(y * Hc / Hf) == yc  <=>  y in [ceil(yc * Hf / Hc), ceil((yc + 1) * Hf / Hc))
    const int y0 = (yc * Hf + Hc - 1) / Hc, y1 = ((yc + 1) * Hf + Hc - 1) / Hc;
    const int x0 = (xc * Wf + Wc - 1) / Wc, x1 = ((xc + 1) * Wf + Wc - 1) / Wc;
    float4 s = reinterpret_cast<float4*>(coarse)[i];
    for (int y = y0; y < y1 && y < Hf; y++)
        for (int x = x0; x < x1 && x < Wf; x++) {
            const float4 v = reinterpret_cast<const float4*>(fine)[(((long long)n * Hf + y) * Wf + x) * C4 + c];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    reinterpret_cast<float4*>(coarse)[i] = s;
}
extern "C" int cald_train_upsample_bwd(cald_ctx* c, int N, int Hf, int Wf, int Hc, int Wc, int C, const float* fine, float* coarse) {
    if (!c || !fine || !coarse || C % 4) TFAIL(CALD_ERR_INVALID, "bad arguments");
    THIP(hipSetDevice(cald_internal_device(c)));
    const long long n4 = (long long)N * Hc * Wc * (C / 4);
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, cald_internal_stream(c), fine, coarse, N, Hf, Wf, Hc, Wc, C / 4);
    THIP(hipGetLastError());
    return 0;
}

// optimizer: torch.optim.SGD(lr, momentum, weight_decay), dampening 0, no nesterov (cald_train.py:397)
//   d = grad + wd * p;  buf = first ? d : momentum * buf + d;  p -= lr * buf
__global__ void sgd_kernel(float* p, const float* grad, float* buf, long long n, float lr, float momentum, float wd, int first) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d = grad[i];
    if (wd != 0.0f) d = d + wd * p[i];
    if (momentum != 0.0f) { const float b = first ? d : momentum * buf[i] + d; buf[i] = b; d = b; }
    p[i] = p[i] - lr * d;
}
extern "C" int cald_train_sgd(cald_ctx* c, long long n, float* param, const float* grad, float* momentum_buf, float lr, float momentum,
                              float weight_decay, int first_step) {
    if (!c || !param || !grad || (momentum != 0.0f && !momentum_buf)) TFAIL(CALD_ERR_INVALID, "null argument");
    THIP(hipSetDevice(cald_internal_device(c)));
    if (n > 0) hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, cald_internal_stream(c), param, grad, momentum_buf, n, lr, momentum, weight_decay, first_step);
    THIP(hipGetLastError());
    return 0;
}
