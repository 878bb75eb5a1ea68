// lossnet_train.hip -- training the loss-prediction module beside the detector (ll_train.py:73-141, ll4al/models/lossnet.py:31-65 LossNet,
// ll4al/main.py:64-83 LossPredLoss): LossNet's forward with its hidden activations kept, its backward, and the pairwise hinge loss with its
// gradient.  Operator-level C ABI on device pointers; the parameters live in a torch-owned flat buffer in LossNet.state_dict() layout
// (cald_amd/ll_train.py).  The pooling of the training forward (cald_train_gap) is in lossnet.hip, beside the kernels it launches.
//
// Arithmetic contract.  Forward: the chains of lossnet_head_kernel (lossnet.hip) -- per FC output one k-ordered fmaf chain from +0 over the
// 256 pooled values, + bias, ReLU; the prediction one fmaf chain over the 4 D hidden values in torch.cat order, + bias -- read from the
// [D][256] torch layout instead of the sweep's k-major copy, so a LossNet trained here scores a pool with the bits it was trained on.
// Backward: every sum over the batch runs b ascending from +0 in one thread (product, then add: -ffp-contract=off), the gradient of the
// pooled vector is one d-ordered fmaf chain from +0; no atomics, two runs are bit-identical.  All kernels are launch-bound (B = 4 images,
// 0.5 MB of weights): one workgroup per output row, coalesced over the 256 channels where a tensor is that wide.
#include "train_host.h"

#define LL_C 256              // channels of every pyramid level
#define LPL_MAX_B 2048        // LossPredLoss: one workgroup, the pair terms meet in LDS

// one workgroup per image; thread d = one output of each FC layer
__global__ __launch_bounds__(256) void lossnet_train_fwd_kernel(const cald_lossnet_tensors p, const int D, const float* __restrict__ pooled,
                                                               float* __restrict__ hidden, float* __restrict__ pred) {
    __shared__ float sp[4 * LL_C];
    __shared__ float sh[4 * 256];
    const int v = blockIdx.x, d = threadIdx.x;
    for (int i = d; i < 4 * LL_C; i += 256) sp[i] = pooled[(size_t)v * 4 * LL_C + i];
    __syncthreads();
    if (d < D) {
        for (int j = 0; j < 4; j++) {
            const float* w = p.fc_w[j] + (size_t)d * LL_C;
            float acc = 0.0f;
            for (int k = 0; k < LL_C; k++) acc = fmaf(sp[j * LL_C + k], w[k], acc);
            acc = acc + p.fc_b[j][d];
            const float h = acc > 0.0f ? acc : 0.0f;
            sh[j * D + d] = h;
            hidden[((size_t)v * 4 + j) * D + d] = h;
        }
    }
    __syncthreads();
    if (d == 0) {
        float acc = 0.0f;
        for (int i = 0; i < 4 * D; i++) acc = fmaf(sh[i], p.lin_w[i], acc);
        pred[v] = acc + p.lin_b[0];
    }
}

// grid ceil(4 D / 256): thread i = one hidden unit.  g linear.weight / bias, and g_h [B][4 D] for the two kernels below
__global__ __launch_bounds__(256) void lossnet_bwd_head_kernel(const cald_lossnet_tensors p, const cald_lossnet_tensors g, const int B, const int D,
                                                              const float* __restrict__ hidden, const float* __restrict__ g_pred,
                                                              float* __restrict__ gh, const int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 4 * D) {
        const float lw = p.lin_w[i];
        float s = 0.0f;
        for (int b = 0; b < B; b++) {
            const float gb = g_pred[b], h = hidden[(size_t)b * 4 * D + i];
            s += gb * h;
            gh[(size_t)b * 4 * D + i] = h > 0.0f ? gb * lw : 0.0f;
        }
        g.lin_w[i] = accumulate ? g.lin_w[i] + s : s;
    }
    if (i == 0) {
        float s = 0.0f;
        for (int b = 0; b < B; b++) s += g_pred[b];
        g.lin_b[0] = accumulate ? g.lin_b[0] + s : s;
    }
}

// grid (D, 4): one row of one FC weight per workgroup, thread c = input channel
__global__ __launch_bounds__(256) void lossnet_bwd_fc_kernel(const cald_lossnet_tensors g, const int B, const int D, const float* __restrict__ pooled,
                                                            const float* __restrict__ gh, const int accumulate) {
    const int d = blockIdx.x, j = blockIdx.y, c = threadIdx.x;
    float s = 0.0f, sb = 0.0f;
    for (int b = 0; b < B; b++) {
        const float t = gh[((size_t)b * 4 + j) * D + d];
        s += t * pooled[((size_t)b * 4 + j) * LL_C + c];
        sb += t;
    }
    float* gw = g.fc_w[j] + (size_t)d * LL_C + c;
    *gw = accumulate ? *gw + s : s;
    if (c == 0) { float* gb = g.fc_b[j] + d; *gb = accumulate ? *gb + sb : sb; }
}

// grid (4, B): g_pooled[b][j][c] = sum_d g_h[b][j][d] * FCj.weight[d][c]
__global__ __launch_bounds__(256) void lossnet_bwd_pooled_kernel(const cald_lossnet_tensors p, const int D, const float* __restrict__ gh,
                                                                float* __restrict__ g_pooled) {
    const int j = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    const float* t = gh + ((size_t)b * 4 + j) * D;
    const float* w = p.fc_w[j] + c;
    float acc = 0.0f;
    for (int d = 0; d < D; d++) acc = fmaf(t[d], w[(size_t)d * LL_C], acc);
    g_pooled[((size_t)b * 4 + j) * LL_C + c] = acc;
}

// one workgroup; pair i = (i, B - 1 - i)
__global__ __launch_bounds__(256) void loss_pred_loss_kernel(const int B, const float* __restrict__ input, const float* __restrict__ target, const float margin,
                                                            const int per_pair, const float* __restrict__ g_up, float* __restrict__ loss, float* __restrict__ terms,
                                                            float* __restrict__ grad) {
    __shared__ float st[LPL_MAX_B / 2];
    const int half = B / 2;
    const float up_mean = per_pair ? 0.0f : (g_up ? g_up[0] : 1.0f) / (float)half;
    for (int i = threadIdx.x; i < half; i += 256) {
        const float dt = target[i] - target[B - 1 - i];
        const float one = dt > 0.0f ? 1.0f : -1.0f;             // 2 sign(clamp(dt, min = 0)) - 1: a tie is -1
        const float x = margin - one * (input[i] - input[B - 1 - i]);
        st[i] = x > 0.0f ? x : 0.0f;
        if (terms) terms[i] = st[i];
        if (grad) {
            const float up = per_pair ? (g_up ? g_up[i] : 1.0f) : up_mean;
            const float gi = x >= 0.0f ? -one * up : 0.0f;      // clamp(min = 0) passes the gradient at x == 0
            grad[i] = gi; grad[B - 1 - i] = -gi;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int i = 0; i < half; i++) s += st[i];
        loss[0] = s / (float)half;
    }
}

static bool tensors_ok(const cald_lossnet_tensors* t) {
    if (!t || !t->lin_w || !t->lin_b) return false;
    for (int j = 0; j < 4; j++) if (!t->fc_w[j] || !t->fc_b[j]) return false;
    return true;
}

extern "C" int cald_lossnet_train_fwd(cald_ctx* c, int B, int D, const cald_lossnet_tensors* params, const float* pooled, float* hidden, float* pred) {
    if (!c || !tensors_ok(params) || !pooled || !hidden || !pred || B < 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    if (D < 1 || D > 256) TFAIL(CALD_ERR_INVALID, "LossNet interm_dim %d outside [1, 256]", D);
    THIP(hipSetDevice(cald_internal_device(c)));
    hipLaunchKernelGGL(lossnet_train_fwd_kernel, dim3(B), dim3(256), 0, cald_internal_stream(c), *params, D, pooled, hidden, pred);
    THIP(hipGetLastError());
    return 0;
}

extern "C" int cald_lossnet_train_bwd(cald_ctx* c, int B, int D, const cald_lossnet_tensors* params, const float* pooled, const float* hidden,
                                      const float* g_pred, float* gh_scratch, const cald_lossnet_tensors* grads, int accumulate, float* g_pooled) {
    if (!c || !tensors_ok(params) || !tensors_ok(grads) || !pooled || !hidden || !g_pred || !gh_scratch || B < 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    if (D < 1 || D > 256) TFAIL(CALD_ERR_INVALID, "LossNet interm_dim %d outside [1, 256]", D);
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    hipLaunchKernelGGL(lossnet_bwd_head_kernel, dim3((4 * D + 255) / 256), dim3(256), 0, st, *params, *grads, B, D, hidden, g_pred, gh_scratch, accumulate);
    hipLaunchKernelGGL(lossnet_bwd_fc_kernel, dim3(D, 4), dim3(256), 0, st, *grads, B, D, pooled, (const float*)gh_scratch, accumulate);
    if (g_pooled) hipLaunchKernelGGL(lossnet_bwd_pooled_kernel, dim3(4, B), dim3(256), 0, st, *params, D, (const float*)gh_scratch, g_pooled);
    THIP(hipGetLastError());
    return 0;
}

extern "C" int cald_loss_pred_loss(cald_ctx* c, int B, const float* input, const float* target, float margin, int per_pair, const float* g_up_dev,
                                   float* loss_out, float* terms_out, float* grad_out) {
    if (!c || !input || !target || !loss_out) TFAIL(CALD_ERR_INVALID, "bad arguments");
    if (B < 2 || (B & 1)) TFAIL(CALD_ERR_INVALID, "LossPredLoss: the batch size %d is not even", B);
    if (B > LPL_MAX_B) TFAIL(CALD_ERR_INVALID, "LossPredLoss: batch size %d above %d", B, LPL_MAX_B);
    THIP(hipSetDevice(cald_internal_device(c)));
    hipLaunchKernelGGL(loss_pred_loss_kernel, dim3(1), dim3(256), 0, cald_internal_stream(c), B, input, target, margin, per_pair, g_up_dev, loss_out, terms_out, grad_out);
    THIP(hipGetLastError());
    return 0;
}
