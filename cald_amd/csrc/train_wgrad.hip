// train_wgrad.hip -- the weight gradient of a conv / linear layer (losses.backward(), cald_train.py:40-74; cuDNN / cuBLAS in the reference):
// wgrad_kernel, the GEMM  dW[co][(tap, ci)] = sum over output pixels  dY[q][co] * X[q @ tap][ci]  on v_mfma_f32_32x32x2_f32.  Both operands
// are read in their natural NHWC order (the channel index is the MFMA row / column, the pixel index is k: no transposes), staged through
// LDS, pixels split over workgroups, partial tiles summed in a fixed order (deterministic).  The bias gradient is a column sum of dY.
// cald_train_wgrad_plan says what a shape launches; wgrad_impl launches exactly that.
#include "train_host.h"
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WgradArgs {
    const float* x; const float* g; float* partial;
    int N, H, W, Cin, ldx;
    int Ho, Wo, Cout, ldg;
    int KH, KW, stride, pad;
    int J, JT, MT;
    long long Q, chunk;
};
// grid (MT * JT, S), 256 threads = 4 waves (2 x 2), tile 128 (co) x 128 (j = tap * Cin + ci) x BK output pixels per stage.
// FAST (both tensors < 2 GB): raw buffer loads whose byte offsets advance by additions only; a row outside its image / past the end of
// the split gets the out-of-range offset and loads zeros -- no branches, no 64-bit multiplies in the loop (the fp32 MFMA shares its
// issue slots with the VALU: the first version spent a third of the loop on address arithmetic).
typedef float f32x4v __attribute__((ext_vector_type(4)));
// PW (1 x 1 filter, stride 1, no padding, or a linear layer; implies FAST): both operands are plain row-major matrices over the pixels,
// so the cursors are two additions per row and the buffer descriptors end at the tensors' ends -- rows past the last pixel load zeros
// without a compare (the general path spends ~70 VALU instructions per stage on the pixel cursor and the image-border tests).
// MODE 2 (filters with a spatial extent / strides, Cin % 128 == 0 so that the 128 columns of a tile are ONE tap; implies FAST): the
// byte offset of every pixel under that tap -- or the out-of-range offset outside the image -- is computed 1 024 pixels at a time into
// an LDS table; a stage reads two table words per thread instead of stepping (n, y, x) cursors.
template <bool FAST, int BK, int MODE = 0>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(const WgradArgs a) {
    constexpr bool PW = MODE == 1, TAB = MODE == 2;
    constexpr int TQ = 1024;                                  // MODE 2: pixels per table fill (a multiple of 2 * BK: every fill starts on stage buffer 0)
    __shared__ int tab[TAB ? TQ + 2 * BK : 1];
    constexpr int R = BK / 8;                                    // rows of both tiles staged per thread
    __shared__ __attribute__((aligned(16))) float sA[2][BK][128];
    __shared__ __attribute__((aligned(16))) float sB[2][BK][128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int mt = blockIdx.x / a.JT, jt = blockIdx.x - mt * a.JT;
    const int m0 = mt * 128, j0 = jt * 128;
    const long long q0 = (long long)blockIdx.y * a.chunk;
    long long q1 = q0 + a.chunk; if (q1 > a.Q) q1 = a.Q;
    const int col4 = (tid & 31) * 4, row = tid >> 5;          // this thread stages rows row, row + 8, ... of both tiles
    // B column (fixed for the whole kernel): j -> (tap, ci)
    const int j = j0 + col4;
    const bool jvalid = j < a.J;
    const int tap = jvalid ? j / a.Cin : 0, ci = j - tap * a.Cin;
    const int ky = tap / a.KW, kx = tap - ky * a.KW;
    const bool mvalid = m0 + col4 < a.ldg;
    // pixel cursors of the staged rows
    int pn[R], py[R], px[R];
    long long pq[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        pq[r] = q0 + row + 8 * r;
        const long long hw = (long long)a.Ho * a.Wo;
        pn[r] = (int)(pq[r] / hw);
        const int rem = (int)(pq[r] - (long long)pn[r] * hw);
        py[r] = rem / a.Wo; px[r] = rem - py[r] * a.Wo;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int jn = 0; jn < 2; jn++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][jn][r] = 0.0f;
    float4 ra[R], rb[R];
    // FAST-path cursor: byte offsets from the tensor bases, remaining rows of the split, input coordinates of this thread's tap
    const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc((void*)a.g, 0, (PW || TAB) ? (int)(a.Q * a.ldg * 4) : 0x7FFE0000, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, PW ? (int)(a.Q * a.ldx * 4) : 0x7FFE0000, 0x00020000);
    int voffG[R], voffX[R], left[R], fiy[R], fix[R], fpx[R], fpy[R];
    const int stepG = BK * a.ldg * 4, stepX = BK * a.stride * a.ldx * 4, stepI = BK * a.stride;
    const int rowX = (a.stride * a.W - a.Wo * a.stride) * a.ldx * 4, imgX = (a.H - a.Ho * a.stride) * a.W * a.ldx * 4;
    if (FAST) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            voffG[r] = (int)((pq[r] * a.ldg + m0 + col4) * 4);
            left[r] = (int)(q1 - pq[r]);
            fpy[r] = py[r]; fpx[r] = px[r];
            fiy[r] = py[r] * a.stride + ky - a.pad; fix[r] = px[r] * a.stride + kx - a.pad;
            voffX[r] = (int)(((((long long)pn[r] * a.H + fiy[r]) * a.W + fix[r]) * a.ldx + ci) * 4);
            if (PW || TAB) {                                 // columns beyond the matrix: the out-of-range offset for the whole kernel
                if (!mvalid) voffG[r] = 0x7FFF0000;          // (the cursor advances by less than 2 GB in total: no wrap-around)
                voffX[r] = jvalid ? (int)((pq[r] * a.ldx + ci) * 4) : 0x7FFF0000;
            }
        }
    }
    int ti = row;                                            // MODE 2: table index of this thread's first row of the next stage
    const int ci4 = jvalid ? ci * 4 : 0x7FFF0000;            // added to a table word; any word + 0x7FFF0000 is out of range
    // table words [0, TQ + 2 BK) <-> pixels sub .. : the BK words past TQ are the first stage of the next fill, which the last stage of
    // this one prefetches
    auto fill = [&](long long sub) {
        const int hw = a.Ho * a.Wo;
        for (int e = tid; e < TQ + 2 * BK; e += 256) {
            int off = 0x7FFF0000;
            const long long q = sub + e;
            if (q < q1) {
                const int n = (int)(q / hw), rem = (int)(q - (long long)n * hw);
                const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
                const int iy = oy * a.stride + ky - a.pad, ix = ox * a.stride + kx - a.pad;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) off = (int)(((((long long)n * a.H + iy) * a.W + ix) * a.ldx) * 4);
            }
            tab[e] = off;
        }
        __syncthreads();
    };
    if (TAB) fill(q0);
    auto load = [&]() {
        if (TAB) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int vx = tab[ti + 8 * r] + ci4;
                ra[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsG, voffG[r], 0, 0));
                rb[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsX, vx, 0, 0));
                voffG[r] += stepG;
            }
            ti += BK;
            return;
        }
        if (PW) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                ra[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsG, voffG[r], 0, 0));
                rb[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsX, voffX[r], 0, 0));
                voffG[r] += stepG; voffX[r] += stepX;
            }
            return;
        }
        if (FAST) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const bool live = left[r] > 0;
                const int vg = (live && mvalid) ? voffG[r] : 0x7FFF0000;
                const bool inimg = fiy[r] >= 0 && fiy[r] < a.H && fix[r] >= 0 && fix[r] < a.W;
                const int vx = (live && jvalid && inimg) ? voffX[r] : 0x7FFF0000;
                ra[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsG, vg, 0, 0));
                rb[r] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsX, vx, 0, 0));
                voffG[r] += stepG; left[r] -= BK;
                voffX[r] += stepX; fix[r] += stepI; fpx[r] += BK;
                while (fpx[r] >= a.Wo) {
                    fpx[r] -= a.Wo; fix[r] -= a.Wo * a.stride; voffX[r] += rowX; fiy[r] += a.stride;
                    if (++fpy[r] >= a.Ho) { fpy[r] = 0; fiy[r] -= a.Ho * a.stride; voffX[r] += imgX; }
                }
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            ra[r] = make_float4(0.f, 0.f, 0.f, 0.f); rb[r] = ra[r];
            if (pq[r] < q1) {
                if (mvalid) ra[r] = *reinterpret_cast<const float4*>(a.g + pq[r] * a.ldg + m0 + col4);
                const int iy = py[r] * a.stride + ky - a.pad, ix = px[r] * a.stride + kx - a.pad;
                if (jvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    rb[r] = *reinterpret_cast<const float4*>(a.x + (((long long)pn[r] * a.H + iy) * a.W + ix) * a.ldx + ci);
            }
            // advance the cursor by one stage (BK pixels); stages past the end of the split load nothing and contribute zeros
            pq[r] += BK; px[r] += BK;
            while (px[r] >= a.Wo) { px[r] -= a.Wo; if (++py[r] >= a.Ho) { py[r] = 0; pn[r]++; } }
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            *reinterpret_cast<float4*>(&sA[buf][row + 8 * r][col4]) = ra[r];
            *reinterpret_cast<float4*>(&sB[buf][row + 8 * r][col4]) = rb[r];
        }
    };
    const int kl = lane >> 5, cl = lane & 31;
    const int stages = (int)((q1 - q0 + BK - 1) / BK);
    load(); store(0);
    __syncthreads();
    // one stage; the buffer index is a compile-time constant (two stages per loop turn), so every LDS address below is a register +
    // an immediate -- with a run-time buffer index each of the 16 fragment reads costs a v_add beside the MFMAs
    auto stage = [&](auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        load();                                               // the next stage (zeros past the end)
        // fragments of k-step ks + 1 are read from LDS before the MFMAs of k-step ks issue (the compiler does not hoist them itself)
        float fa0 = sA[buf][kl][wm * 64 + cl], fa1 = sA[buf][kl][wm * 64 + 32 + cl];
        float fb0 = sB[buf][kl][wn * 64 + cl], fb1 = sB[buf][kl][wn * 64 + 32 + cl];
#pragma unroll
        for (int ks = 0; ks < BK / 2; ks++) {
            const float a0 = fa0, a1 = fa1, b0 = fb0, b1 = fb1;
            if (ks + 1 < BK / 2) {
                fa0 = sA[buf][2 * ks + 2 + kl][wm * 64 + cl]; fa1 = sA[buf][2 * ks + 2 + kl][wm * 64 + 32 + cl];
                fb0 = sB[buf][2 * ks + 2 + kl][wn * 64 + cl]; fb1 = sB[buf][2 * ks + 2 + kl][wn * 64 + 32 + cl];
            }
            __builtin_amdgcn_sched_barrier(0);      // keep the reads above the MFMAs: the scheduler otherwise sinks them to their use
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        store(buf ^ 1);
        __syncthreads();
    };
    if (TAB) {
        for (int s0 = 0; s0 < stages; s0 += TQ / BK) {
            if (s0) { fill(q0 + (long long)s0 * BK); ti = row + BK; }      // (the stage before ended on a barrier; stage s0 is already staged)
            const int s1 = s0 + TQ / BK < stages ? s0 + TQ / BK : stages;
            for (int s = s0; s < s1; s += 2) {
                stage(std::integral_constant<int, 0>());
                if (s + 1 < s1) stage(std::integral_constant<int, 1>());
            }
        }
    } else {
        for (int s = 0; s < stages; s += 2) {
            stage(std::integral_constant<int, 0>());
            if (s + 1 < stages) stage(std::integral_constant<int, 1>());
        }
    }
    // partial tile -> partial[S][MT*128][JT*128]
    const long long ldp = (long long)a.JT * 128;
    float* P = a.partial + (long long)blockIdx.y * ((long long)a.MT * 128) * ldp;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int jn = 0; jn < 2; jn++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rr = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
                const int cc = j0 + wn * 64 + jn * 32 + cl;
                P[(long long)rr * ldp + cc] = acc[i][jn][r];
            }
}
// grad[co][ci][tap] (torch layout) (+)= sum over splits, in split order
__global__ void wgrad_reduce_kernel(const float* __restrict__ partial, int S, long long split_stride, long long ldp, int Cout, int Cin, int taps,
                                    float* __restrict__ grad, int accumulate, const float* __restrict__ row_scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long J = (long long)taps * Cin;
    if (i >= (long long)Cout * J) return;
    const int co = (int)(i / J); const int j = (int)(i - (long long)co * J);
    const int tap = j / Cin, ci = j - tap * Cin;
    // the splits are summed in split order (fixed, reproducible); sixteen loads are in flight at a time -- a layer with few outputs
    // and hundreds of splits (the 15-column RPN head: 3 840 outputs x 512 splits) spent 0.47 ms per launch waiting for one load after
    // the other
    float s = 0.0f;
    const float* q = partial + (long long)co * ldp + j;
    int k = 0;
    for (; k + 16 <= S; k += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = q[(long long)(k + u) * split_stride];
#pragma unroll
        for (int u = 0; u < 16; u++) s += v[u];
    }
    for (; k < S; k++) s += q[(long long)k * split_stride];
    if (row_scale) s = s * row_scale[co];
    float* dst = grad + ((long long)co * Cin + ci) * taps + tap;
    *dst = accumulate ? *dst + s : s;
}
// the same for taps > 1 with coalesced stores: one workgroup sums 64 input channels x all taps of one output channel (reads run
// along ci), turns the [tap][ci] block into the torch [ci][tap] order in LDS and stores it as one contiguous run
__global__ __launch_bounds__(256) void wgrad_reduce_taps_kernel(const float* __restrict__ partial, int S, long long split_stride, long long ldp, int Cin,
                                                                int taps, float* __restrict__ grad, int accumulate, const float* __restrict__ row_scale) {
    extern __shared__ float blk[];     // [64][taps]
    const int co = blockIdx.y, c0 = blockIdx.x * 64;
    const int nc = Cin - c0 < 64 ? Cin - c0 : 64;
    const float* P = partial + (long long)co * ldp + c0;
    const float sc = row_scale ? row_scale[co] : 1.0f;
    for (int e = threadIdx.x; e < taps * 64; e += 256) {
        const int t = e >> 6, cl = e & 63;
        if (cl >= nc) continue;
        const float* q = P + (long long)t * Cin + cl;
        float s = 0.0f;
        int k = 0;
        for (; k + 8 <= S; k += 8) {          // split order kept; eight loads in flight
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = q[(long long)(k + u) * split_stride];
#pragma unroll
            for (int u = 0; u < 8; u++) s += v[u];
        }
        for (; k < S; k++) s += q[(long long)k * split_stride];
        if (row_scale) s = s * sc;
        blk[cl * taps + t] = s;
    }
    __syncthreads();
    float* dst = grad + ((long long)co * Cin + c0) * taps;
    for (int e = threadIdx.x; e < taps * nc; e += 256) dst[e] = accumulate ? dst[e] + blk[e] : blk[e];
}
// db[c] = sum over rows of g[q][c]: stage 1 partial sums over row blocks (128 channels x 8 row lanes per workgroup, float4
// loads), stage 2 fixed-order sum over the row blocks
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* g, long long Q, int C, int ld, long long rows_per_block, float* partial) {
    __shared__ float4 red[8][32];
    const int cq = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 128 + cq * 4;
    const long long q0 = (long long)blockIdx.y * rows_per_block;
    long long q1 = q0 + rows_per_block; if (q1 > Q) q1 = Q;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < ld)
        for (long long q = q0 + rl; q < q1; q += 8) {
            const float4 v = *reinterpret_cast<const float4*>(g + q * ld + c);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    red[rl][cq] = s;
    __syncthreads();
    if (rl == 0) {
        for (int r = 1; r < 8; r++) { const float4 v = red[r][cq]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
        float* o = partial + (long long)blockIdx.y * C;
        if (c < C) o[c] = s.x;
        if (c + 1 < C) o[c + 1] = s.y;
        if (c + 2 < C) o[c + 2] = s.z;
        if (c + 3 < C) o[c + 3] = s.w;
    }
}
// 16 channels x 16 split lanes per workgroup: lane l sums splits l, l+16, ... in order, then lane 0 adds the 16 lane sums in order
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* partial, int S, int C, float* out, int accumulate) {
    __shared__ float red[16][17];
    const int cl = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    float s = 0.0f;
    if (c < C)
        for (int k = lane; k < S; k += 16) s += partial[(long long)k * C + c];
    red[lane][cl] = s;
    __syncthreads();
    if (lane == 0 && c < C) {
        for (int l = 1; l < 16; l++) s += red[l][cl];
        out[c] = accumulate ? out[c] + s : s;
    }
}

// The launch plan of one weight gradient: which wgrad_kernel instantiation, how many splits of how many pixels, which reduction,
// how the bias column sum is split, how much scratch.  wgrad_impl launches exactly what this returns; tests query it to pin the variant a
// shape reaches.  Host arithmetic only.
extern "C" int cald_train_wgrad_plan(long long Q, int N, int H, int W, int Cin, int ldx, int Cout, int ldg, int KH, int KW, int stride, int pad,
                                     int red_taps, cald_wgrad_plan* out) {
    if (!out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (Q < 1 || N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0 || red_taps < 1) TFAIL(CALD_ERR_INVALID, "bad geometry");
    if (Cin % 4 || ldx % 4 || ldg % 4 || ldx < Cin || ldg < Cout) TFAIL(CALD_ERR_INVALID, "Cin and the row strides must be multiples of 4 (and cover the channels)");
    memset(out, 0, sizeof(*out));
    const long long J = (long long)KH * KW * Cin;
    out->JT = (int)((J + 127) / 128); out->MT = (Cout + 127) / 128;
    const long long tiles = (long long)out->MT * out->JT;
    const long long tile_floats = tiles * 128 * 128;
    // workgroups aimed at per launch: one resident round (2 per CU).  Measured on the whole step (the kernel shares the chip with the
    // data-gradient stream): 512 -> 34.6 / 33.8 ms (Faster R-CNN / RetinaNet), 384 -> 34.3 / 34.7, 1024 -> 34.9, 2048 -> 35.0 / 35.5
    static const long long target = getenv("CALD_WGRAD_TARGET") ? atoll(getenv("CALD_WGRAD_TARGET")) : 512;
    const long long bytesG = Q * ldg * 4, bytesX = (long long)N * H * W * ldx * 4;
    const bool fast = bytesG < 0x7FFE0000ll && bytesX < 0x7FFE0000ll;
    static const bool pw_env = !(getenv("CALD_WGRAD_PW") && atoi(getenv("CALD_WGRAD_PW")) == 0);
    static const bool tab_env = !(getenv("CALD_WGRAD_TAB") && atoi(getenv("CALD_WGRAD_TAB")) == 0);
    static const int bk_env = getenv("CALD_WGRAD_BK") ? atoi(getenv("CALD_WGRAD_BK")) : 16;     // 32-pixel stages measured slower (109 vs 115 TFLOP/s on the largest layer)
    // pointwise: every pixel row q of g pairs with row q of x (chunks are multiples of 32 pixels, so only the last split runs past Q)
    const bool pw = fast && pw_env && KH == 1 && KW == 1 && stride == 1 && pad == 0 && Q == (long long)N * H * W;
    const bool tabm = fast && tab_env && !pw && Cin % 128 == 0;
    long long S = target / tiles;                         // rounded down: one workgroup over the resident round costs a second round
    const long long maxS_rows = (Q + 255) / 256; if (S > maxS_rows) S = maxS_rows;
    const long long cap = (512ll << 20) / 4 / tile_floats; if (S > cap) S = cap;
    if (S < 1) S = 1;
    out->chunk = ((Q + S - 1) / S + 31) / 32 * 32;
    out->S = (Q + out->chunk - 1) / out->chunk;
    out->csplit = (Q + 255) / 256 > 1024 ? 1024 : (Q + 255) / 256;
    out->rows_per_block = (Q + out->csplit - 1) / out->csplit;
    out->scratch_bytes = (out->S * tile_floats + out->csplit * Cout + 64) * 4;
    out->variant = pw ? CALD_WGRAD_POINTWISE : tabm ? CALD_WGRAD_TABLE : (fast && bk_env == 32) ? CALD_WGRAD_GENERAL32 : fast ? CALD_WGRAD_GENERAL : CALD_WGRAD_WIDE;
    out->reduce = red_taps > 1 && red_taps <= 64 ? CALD_WGRAD_REDUCE_TAPS : CALD_WGRAD_REDUCE_FLAT;
    static const char* const names[] = {"wgrad_kernel<true,16,1>", "wgrad_kernel<true,16,2>", "wgrad_kernel<true,16>", "wgrad_kernel<true,32>", "wgrad_kernel<false,16>"};
    strcpy(out->kernel, names[out->variant]);          // (both fit: the struct was zeroed above)
    strcpy(out->reduce_kernel, out->reduce == CALD_WGRAD_REDUCE_TAPS ? "wgrad_reduce_taps_kernel" : "wgrad_reduce_kernel");
    return 0;
}

// x [N][H][W][ldx] (Cin channels used, Cin % 4 == 0), g [N][Ho][Wo][ldg] (Cout channels used; ldg % 4 == 0 and the pad channels
// readable).  dw: torch layout [Cout][Cin][KH][KW]; for a tap-major linear layer pass KH*KW = taps, H = W = 1 and x rows
// [R][taps * Cin] as N = R... (see cald_train_linear_wgrad).  db: [Cout] or null.
static int wgrad_impl(cald_ctx* c, long long Q, int N, int H, int W, const float* x, int Cin, int ldx, int Ho, int Wo, const float* g,
                      int Cout, int ldg, int KH, int KW, int stride, int pad, int red_taps, int red_cin, float* dw, float* db, int accumulate,
                      const float* row_scale) {
    if (Cin % 4 || ldx % 4 || ldg % 4) TFAIL(CALD_ERR_INVALID, "Cin and the row strides must be multiples of 4");
    if (ldx < Cin || ldg < Cout) TFAIL(CALD_ERR_INVALID, "a row stride is smaller than the channel count");
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    WgradArgs a; memset(&a, 0, sizeof(a));
    a.x = x; a.g = g; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.ldx = ldx; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.ldg = ldg;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.J = KH * KW * Cin; a.JT = (a.J + 127) / 128; a.MT = (Cout + 127) / 128; a.Q = Q;
    cald_wgrad_plan pl;
    if (int rc = cald_train_wgrad_plan(Q, N, H, W, Cin, ldx, Cout, ldg, KH, KW, stride, pad, red_taps, &pl)) return rc;
    const long long tiles = (long long)a.MT * a.JT, tile_floats = tiles * 128 * 128;
    const long long S = pl.S, csplit = pl.csplit;
    a.chunk = pl.chunk;
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, (size_t)pl.scratch_bytes, &scratch)) return rc;
    a.partial = (float*)scratch;
    switch (pl.variant) {
        case CALD_WGRAD_POINTWISE: hipLaunchKernelGGL((wgrad_kernel<true, 16, 1>), dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, st, a); break;
        case CALD_WGRAD_TABLE: hipLaunchKernelGGL((wgrad_kernel<true, 16, 2>), dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, st, a); break;
        case CALD_WGRAD_GENERAL32: hipLaunchKernelGGL((wgrad_kernel<true, 32>), dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, st, a); break;
        case CALD_WGRAD_GENERAL: hipLaunchKernelGGL((wgrad_kernel<true, 16>), dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((wgrad_kernel<false, 16>), dim3((unsigned)tiles, (unsigned)S), dim3(256), 0, st, a); break;
    }
    const long long nred = (long long)Cout * a.J;
    if (pl.reduce == CALD_WGRAD_REDUCE_TAPS)
        hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3((unsigned)((red_cin + 63) / 64), (unsigned)Cout), dim3(256), (size_t)red_taps * 64 * 4, st,
                           a.partial, (int)S, tile_floats, (long long)a.JT * 128, red_cin, red_taps, dw, accumulate, row_scale);
    else
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, st, a.partial, (int)S, tile_floats,
                           (long long)a.JT * 128, Cout, red_cin, red_taps, dw, accumulate, row_scale);
    if (db) {
        float* cp = a.partial + S * tile_floats;
        const long long rpb = pl.rows_per_block;
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((Cout + 127) / 128, (unsigned)csplit), dim3(256), 0, st, g, Q, Cout, ldg, rpb, cp);
        hipLaunchKernelGGL(colsum_final_kernel, dim3((Cout + 15) / 16), dim3(256), 0, st, cp, (int)csplit, Cout, db, accumulate);
    }
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_conv_wgrad(cald_ctx* c, int N, int H, int W, const float* x, int Cin, int ldx, const float* g, int Cout, int ldg,
                                     int KH, int KW, int stride, int pad, const float* row_scale, float* dw, float* db, int accumulate) {
    if (!c || !x || !g || !dw) TFAIL(CALD_ERR_INVALID, "null argument");
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    if (N < 1 || Ho < 1 || Wo < 1) TFAIL(CALD_ERR_INVALID, "bad geometry");
    if (row_scale && db) TFAIL(CALD_ERR_INVALID, "row_scale is for FrozenBatchNorm layers, which carry no bias");
    return wgrad_impl(c, (long long)N * Ho * Wo, N, H, W, x, Cin, ldx, Ho, Wo, g, Cout, ldg, KH, KW, stride, pad, KH * KW, Cin, dw, db, accumulate, row_scale);
}
// linear layer on rows: x [R][K], g [R][ldg] -> dw [Cout][K] torch layout; taps > 1: rows are [tap][K / taps] and the torch
// weight is [Cout][K / taps][taps] (fc6 on the RoIAlign output)
extern "C" int cald_train_linear_wgrad(cald_ctx* c, int R, const float* x, int K, const float* g, int Cout, int ldg, int taps,
                                       float* dw, float* db, int accumulate) {
    if (!c || !x || !g || !dw) TFAIL(CALD_ERR_INVALID, "null argument");
    if (R < 1 || taps < 1 || K % taps) TFAIL(CALD_ERR_INVALID, "bad geometry");
    return wgrad_impl(c, R, 1, 1, R, x, K, K, 1, R, g, Cout, ldg, 1, 1, 1, 0, taps, K / taps, dw, db, accumulate, nullptr);
}
