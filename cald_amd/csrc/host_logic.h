// host_logic.h -- host-side restatements of the reference's non-GPU logic on the sweep path (no device work):
//   * detector-transform size rule (torchvision GeneralizedRCNNTransform)
//   * Python's `random` (MT19937: random.seed(int), random.random(), random.uniform) and cald_helper.cutout's rectangle
//     selection (cald/cald_helper.py:88-132)
//   * np.round(np.linspace(0, n-1, 50)) sub-sampling (cald_train.py:110-113) and numpy's pairwise float64 / float32 sums
//   * Pillow's resampling coefficients (Resample.c precompute_coeffs / normalize_coeffs_8bpc; BILINEAR and BICUBIC)
//   * Pillow's Image.rotate(expand=True) matrix + 16.16 fixed-point coefficients, and cald_helper.rotate's box constants
// Product code; the oracle holds its own independent restatement of each of these.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static inline void transform_size(int H, int W, int min_size, int max_size, int* Hr, int* Wr, int* Hp, int* Wp) {
    double mn = (double)(H < W ? H : W), mx = (double)(H > W ? H : W);
    double scale = (double)min_size / mn;
    if (mx * scale > (double)max_size) scale = (double)max_size / mx;
    *Hr = (int)std::floor((double)H * scale);
    *Wr = (int)std::floor((double)W * scale);
    *Hp = ((*Hr + 31) / 32) * 32;
    *Wp = ((*Wr + 31) / 32) * 32;
}

// ---- Python's random module: MT19937 + random.seed(int) + random.random() ----
struct PyRandom {
    uint32_t mt[624]; int idx;
    void init_genrand(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    void seed(uint64_t a) {
        uint32_t key[2] = {(uint32_t)(a & 0xffffffffu), (uint32_t)(a >> 32)};
        int klen = key[1] ? 2 : 1;
        init_genrand(19650218u);
        int i = 1, j = 0;
        for (int k = 624; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            i++; j++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
            if (j >= klen) j = 0;
        }
        for (int k = 623; k; k--) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            i++;
            if (i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int k = 0; k < 624; k++) {
                uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= (y >> 11); y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= (y >> 18);
        return y;
    }
    double random() { uint32_t a = next() >> 5, b = next() >> 6; return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0); }
    double uniform(double a, double b) { return a + (b - a) * random(); }
    // random.randint(0, n - 1) == randrange(n): _randbelow_with_getrandbits (k = n.bit_length(), rejection sampling)
    int randbelow(int n) {
        int k = 0;
        for (int t = n; t; t >>= 1) k++;
        for (;;) { const uint32_t r = next() >> (32 - k); if ((int)r < n) return (int)r; }
    }
};

// cald_helper.cutout (cald/cald_helper.py:88-132): rectangle selection only; the fill happens in
// the preprocess kernel.  boxes: sub-sampled reference detections, original image coordinates.
// The generator is the caller's: get_uncertainty draws ColorSwap's randint and every cutout call of one image from the
// same global Python generator, in call order (cald_train.py:140-166).
// margin (optional): the smallest distance of any trial's largest overlap ratio to the two accept thresholds (0.4, 0.1) -- the only
// place where the reference boxes decide something discrete here (audit.hip).
static inline int cutout_rects(PyRandom& rng, int H, int W, int N, const float* boxes, int cut_num, int* rects, float* margin = nullptr) {
    int count = 0;
    if (margin) *margin = INFINITY;
    for (int t = 0; t < 50; t++) {
        double sh = rng.uniform(0.05 * H, 0.2 * H);
        double sw = rng.uniform(0.05 * W, 0.2 * W);
        double left = rng.uniform(0.0, (double)W - sw), right = left + sw;
        double top = rng.uniform(0.0, (double)H - sh), bottom = top + sh;
        int il = (int)left, it = (int)top, ir = (int)right, ib = (int)bottom;
        float c[4] = {(float)il, (float)it, (float)ir, (float)ib};
        float rmax = 0.0f; bool any_nan = false;
        for (int i = 0; i < N; i++) {
            const float* b = boxes + 4 * i;
            float iw = std::fmin(c[2], b[2]) - std::fmax(c[0], b[0]); if (iw < 0.0f) iw = 0.0f;
            float ih = std::fmin(c[3], b[3]) - std::fmax(c[1], b[1]); if (ih < 0.0f) ih = 0.0f;
            float area = (b[2] - b[0]) * (b[3] - b[1]);
            float ratio = (iw * ih) / area;
            if (ratio != ratio) any_nan = true;
            if (i == 0 || ratio > rmax) rmax = ratio;
        }
        if (margin && !any_nan) { const float d = std::fmin(std::fabs(rmax - 0.4f), std::fabs(rmax - 0.1f)); if (d < *margin) *margin = d; }
        if (!any_nan && (rmax > 0.4f || rmax < 0.1f)) continue;
        rects[4 * count] = il; rects[4 * count + 1] = it; rects[4 * count + 2] = ir; rects[4 * count + 3] = ib;
        if (++count >= cut_num) break;
    }
    return count;
}
static inline int cutout_rects(uint64_t seed, int H, int W, int N, const float* boxes, int cut_num, int* rects) {
    PyRandom rng; rng.seed(seed);
    return cutout_rects(rng, H, W, N, boxes, cut_num, rects);
}

// np.round(np.linspace(0, n-1, 50)).astype(int)  (cald_train.py:110-113)
static inline int subsample_indices(int n, int* inds) {
    if (n <= 40) { for (int i = 0; i < n; i++) inds[i] = i; return n; }
    double step = (double)(n - 1) / 49.0;
    for (int i = 0; i < 50; i++) {
        double v = (i == 49) ? (double)(n - 1) : (double)i * step;
        inds[i] = (int)std::nearbyint(v);
    }
    return 50;
}

// numpy pairwise summation of float64 (np.mean over a 1-D array)
static inline double np_sum(const double* a, int n) {
    if (n < 8) { double r = 0.0; for (int i = 0; i < n; i++) r += a[i]; return r; }
    if (n <= 128) {
        double r[8];
        for (int k = 0; k < 8; k++) r[k] = a[k];
        int i;
        for (i = 8; i < n - (n % 8); i += 8) for (int k = 0; k < 8; k++) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    int n2 = n / 2; n2 -= n2 % 8;
    return np_sum(a, n2) + np_sum(a + n2, n - n2);
}

// Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc; fid 0 = BILINEAR (support 1), 1 = BICUBIC (support 2, a = -0.5)
static inline double pil_filter(int fid, double x) {
    if (x < 0.0) x = -x;
    if (fid == 0) return x < 1.0 ? 1.0 - x : 0.0;
    if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * -0.5;
    return 0.0;
}
static inline int pil_coeffs(int inSize, int outSize, int fid, std::vector<int>& bounds, std::vector<int>& kk) {
    double scale = (double)inSize / (double)outSize, filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    double support = (fid == 0 ? 1.0 : 2.0) * filterscale;
    int ksize = (int)std::ceil(support) * 2 + 1;
    std::vector<double> pre((size_t)outSize * ksize);
    bounds.assign((size_t)outSize * 2, 0); kk.assign((size_t)outSize * ksize, 0);
    for (int xx = 0; xx < outSize; xx++) {
        double center = (xx + 0.5) * scale, ww = 0.0, ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5); if (xmax > inSize) xmax = inSize;
        xmax -= xmin;
        double* k = &pre[(size_t)xx * ksize];
        int x;
        for (x = 0; x < xmax; x++) {
            double w = pil_filter(fid, (x + xmin - center + 0.5) * ss);
            k[x] = w; ww += w;
        }
        for (x = 0; x < xmax; x++) if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; x++) k[x] = 0;
        bounds[2 * xx] = xmin; bounds[2 * xx + 1] = xmax;
    }
    for (size_t i = 0; i < pre.size(); i++)
        kk[i] = pre[i] < 0 ? (int)(-0.5 + pre[i] * (double)(1 << 22)) : (int)(0.5 + pre[i] * (double)(1 << 22));
    return ksize;
}

// torch.randn(3, H, W) on fewer than 16 elements takes torch's scalar path (another draw pattern, double arithmetic) instead of the
// 16-chunk Box-Muller fill noise_stream_kernel restates: every entry point that draws Gaussian noise refuses such an image.
static inline bool randn_unsupported(int H, int W) { return (long long)H * W * 3 < 16; }

// PIL Image.rotate(angle, expand=True): matrix arithmetic of Image.rotate (python floats, round(., 15)),
// then the FIX()ed 16.16 coefficients of Geometry.c affine_fixed.  (cald_helper.py:153)
static inline double py_round15(double v) { char buf[64]; snprintf(buf, sizeof(buf), "%.15f", v); return strtod(buf, nullptr); }
static inline int pil_fix(double v) { double t = v * 65536.0 + 0.5; return t < 0.0 ? (int)std::floor(t) : (int)t; }
static inline void pil_rotate_setup(int H, int W, double angle_deg, int fix[6], int* nH, int* nW) {
    double angle = std::fmod(angle_deg, 360.0); if (angle < 0) angle += 360.0;
    const double w = (double)W, h = (double)H, cx = w / 2.0, cy = h / 2.0;
    const double ang = -(angle * (3.141592653589793 / 180.0));
    double m[6] = {py_round15(std::cos(ang)), py_round15(std::sin(ang)), 0.0, py_round15(-std::sin(ang)), py_round15(std::cos(ang)), 0.0};
    if (angle == 90.0 || angle == 270.0) {
        // Image.rotate returns transpose(ROTATE_90 / ROTATE_270) for these two angles when expand is set: out[y][x] = in[x][W-1-y] resp.
        // in[H-1-x][y], a W x H image.  The same index permutation as the exact affine map the nearest-neighbour loop evaluates.
        if (angle == 90.0) { m[0] = 0; m[1] = -1; m[2] = w; m[3] = 1; m[4] = 0; m[5] = 0; }
        else { m[0] = 0; m[1] = 1; m[2] = 0; m[3] = -1; m[4] = 0; m[5] = h; }
        fix[0] = pil_fix(m[0]); fix[1] = pil_fix(m[1]); fix[3] = pil_fix(m[3]); fix[4] = pil_fix(m[4]);
        fix[2] = pil_fix(m[2] + m[0] * 0.5 + m[1] * 0.5); fix[5] = pil_fix(m[5] + m[3] * 0.5 + m[4] * 0.5);
        *nH = W; *nW = H;
        return;
    }
    double m2 = m[0] * -cx + m[1] * -cy + m[2], m5 = m[3] * -cx + m[4] * -cy + m[5];
    m[2] = m2 + cx; m[5] = m5 + cy;
    const double xs[4] = {0, w, w, 0}, ys[4] = {0, 0, h, h};
    double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
    for (int i = 0; i < 4; i++) {
        const double X = m[0] * xs[i] + m[1] * ys[i] + m[2], Y = m[3] * xs[i] + m[4] * ys[i] + m[5];
        if (i == 0 || X < xmin) xmin = X; if (i == 0 || X > xmax) xmax = X;
        if (i == 0 || Y < ymin) ymin = Y; if (i == 0 || Y > ymax) ymax = Y;
    }
    const int nw = (int)std::ceil(xmax) - (int)std::floor(xmin), nh = (int)std::ceil(ymax) - (int)std::floor(ymin);
    const double px = -(nw - W) / 2.0, py = -(nh - H) / 2.0;
    m2 = m[0] * px + m[1] * py + m[2]; m5 = m[3] * px + m[4] * py + m[5];
    m[2] = m2; m[5] = m5;
    fix[0] = pil_fix(m[0]); fix[1] = pil_fix(m[1]); fix[3] = pil_fix(m[3]); fix[4] = pil_fix(m[4]);
    fix[2] = pil_fix(m[2] + m[0] * 0.5 + m[1] * 0.5); fix[5] = pil_fix(m[5] + m[3] * 0.5 + m[4] * 0.5);
    *nH = nh; *nW = nw;
}
// cald_helper.rotate box transform constants (cald_helper.py:135-222): float32 affine matrix, scale, clamp bounds
static inline void rotate_box_params(int H, int W, double angle_deg, int pilW, int pilH, float* p /*12*/) {
    const double ang = angle_deg * (3.141592653589793 / 180.0);
    const double alpha = std::cos(ang), beta = std::sin(ang), cx = W / 2.0, cy = H / 2.0;
    double m02 = (1 - alpha) * cx - beta * cy, m12 = beta * cx + (1 - alpha) * cy;
    const double c_ = std::fabs(alpha), s_ = std::fabs(beta);
    const int nW = (int)((H * s_) + (W * c_)), nH = (int)((H * c_) + (W * s_));
    m02 += (nW / 2.0) - cx; m12 += (nH / 2.0) - cy;
    p[0] = (float)alpha; p[1] = (float)beta; p[2] = (float)m02; p[3] = (float)(-beta); p[4] = (float)alpha; p[5] = (float)m12;
    p[6] = (float)((double)pilW / (double)W); p[7] = (float)((double)pilH / (double)H); p[8] = (float)W; p[9] = (float)H;
    p[10] = p[11] = 0.0f;
}

// cald_helper.rotate box transform (cald_helper.py:160-222) on the host, same float32 arithmetic as score.hip kind 3
static inline void rotate_boxes_host(const float* p /*rotate_box_params*/, const float* boxes, int N, float* out) {
    for (int i = 0; i < N; i++) {
        const float* b = boxes + 4 * i;
        const float bw = b[2] - b[0], bh = b[3] - b[1];
        const float xs[4] = {b[0], b[0] + bw, b[0], b[2]}, ys[4] = {b[1], b[1], b[1] + bh, b[3]};
        float xmin = 0.f, xmax = 0.f, ymin = 0.f, ymax = 0.f;
        for (int q = 0; q < 4; q++) {
            const float X = (p[0] * xs[q] + p[1] * ys[q]) + p[2] * 1.0f;
            const float Y = (p[3] * xs[q] + p[4] * ys[q]) + p[5] * 1.0f;
            if (q == 0 || X < xmin) xmin = X; if (q == 0 || X > xmax) xmax = X;
            if (q == 0 || Y < ymin) ymin = Y; if (q == 0 || Y > ymax) ymax = Y;
        }
        auto cl = [](float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); };
        out[4 * i] = cl(xmin / p[6], 0.0f, p[8]); out[4 * i + 1] = cl(ymin / p[7], 0.0f, p[9]);
        out[4 * i + 2] = cl(xmax / p[6], 0.0f, p[8]); out[4 * i + 3] = cl(ymax / p[7], 0.0f, p[9]);
    }
}

// numpy pairwise summation of float32 (np.sum over a 1-D float32 array)
static inline float np_sum_f32(const float* a, int n) {
    if (n < 8) { float r = 0.0f; for (int i = 0; i < n; i++) r += a[i]; return r; }
    if (n <= 128) {
        float r[8];
        for (int k = 0; k < 8; k++) r[k] = a[k];
        int i;
        for (i = 8; i < n - (n % 8); i += 8) for (int k = 0; k < 8; k++) r[k] += a[i + k];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    int n2 = n / 2; n2 -= n2 % 8;
    return np_sum_f32(a, n2) + np_sum_f32(a + n2, n - n2);
}


// What a pair's aug_param holds for the augmentations that move boxes (score.hip aug_box; kind as ScoreArgs::aug_kind): 1 flip {W},
// 2 resize {ratio} -- boxes * ratio is a float32 tensor times the scalar --, 3 rotate {the constants of rotate_box_params over Pillow's
// expanded canvas}; anything else: zeros.
static inline void pair_params(int kind, int H, int W, double param, float* par /*12*/) {
    for (int q = 0; q < 12; q++) par[q] = 0.0f;
    if (kind == 1) par[0] = (float)W;
    else if (kind == 2) par[0] = (float)param;
    else if (kind == 3) { int fx[6], nh, nw; pil_rotate_setup(H, W, param, fx, &nh, &nw); rotate_box_params(H, W, param, nw, nh, par); }
}

// ---- host tail of the ls_c sweep (ls_c_train.py:118-153) ----
// the reference boxes that are scored: all n while n <= 30, otherwise the top 30 by prob_max (value descending, index ascending).
// sel [30]; returns how many
static inline int ls_select(int n, const float* pm, int* sel) {
    std::vector<int> idx(n); for (int k = 0; k < n; k++) idx[k] = k;
    if (n > 30) {
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return pm[x] > pm[y]; });
        idx.resize(30);
    }
    for (size_t k = 0; k < idx.size(); k++) sel[k] = idx[k];
    return (int)idx.size();
}
// the float64 / float32 numpy arithmetic of ls_c_train.py:151-153: pm [N] the selected boxes' prob_max, rows[r][k] the maximum IoU of
// selected box k in noisy view r (n_rows views; the mean is over six whatever n_rows is).  No box: 0.0
static inline double ls_tail(int N, const float* pm, int n_rows, const float* const* rows) {
    if (N <= 0) return 0.0;
    std::vector<double> st(N, 0.0), prod(N);
    float U = 0.0f;
    for (int k = 0; k < N; k++) {
        const float u = 1.0f - pm[k];
        if (k == 0 || u > U) U = u;
    }
    for (int r = 0; r < n_rows; r++) for (int k = 0; k < N; k++) st[k] += (double)rows[r][k];
    for (int k = 0; k < N; k++) { st[k] = st[k] / 6.0; prod[k] = (double)pm[k] * st[k]; }
    return np_sum(prod.data(), N) / (double)np_sum_f32(pm, N) - (double)U;
}


// ---- cut_out view reuse (cutout_reuse.hip CutPlanner::cut_plan): the pixels of each backbone tensor that can differ from the reference view's ----
// The cut_out view is the reference view with up to CALD_MAX_CUT rectangles filled, same size, same transform.  Every conv output is one
// fixed k-ordered fma chain over its window, so an output whose window misses every filled input pixel has the reference's bits.  A set
// is a union of rectangles (inclusive bounds), one per cutout rectangle, each carried through the layers on its own; supersets are safe
// (a recomputed clean pixel gets the reference's bits again), so the resize step takes one extra source row / column on each side.
#define CUT_SET_MAX 4
struct CutRect { int x0, y0, x1, y1; };
struct CutSet { int n; CutRect r[CUT_SET_MAX]; };
static inline int cut_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// outputs o of a k-wide, stride-s, pad-p window that meet input span [a, b], clipped to [0, n - 1]; false if none
static inline bool cut_span(int a, int b, int k, int s, int p, int n, int* lo, int* hi) {
    int l = -cut_floor_div(-(a + p - k + 1), s), h = cut_floor_div(b + p, s);
    if (l < 0) l = 0;
    if (h > n - 1) h = n - 1;
    *lo = l; *hi = h;
    return l <= h;
}
static inline CutSet cut_map(const CutSet& in, int k, int s, int p, int Ho, int Wo) {
    CutSet o; o.n = 0;
    for (int i = 0; i < in.n; i++) {
        CutRect r;
        if (cut_span(in.r[i].x0, in.r[i].x1, k, s, p, Wo, &r.x0, &r.x1) && cut_span(in.r[i].y0, in.r[i].y1, k, s, p, Ho, &r.y0, &r.y1)) o.r[o.n++] = r;
    }
    return o;
}
// the input pixels a 3 x 3, stride-s, pad-1 conv reads to produce `out` (conv2's operand T1 = conv1's compute set)
static inline CutSet cut_window(const CutSet& out, int s, int Hi, int Wi) {
    CutSet o; o.n = 0;
    for (int i = 0; i < out.n; i++) {
        CutRect r = {out.r[i].x0 * s - 1, out.r[i].y0 * s - 1, out.r[i].x1 * s + 1, out.r[i].y1 * s + 1};
        if (r.x0 < 0) r.x0 = 0; if (r.y0 < 0) r.y0 = 0;
        if (r.x1 > Wi - 1) r.x1 = Wi - 1; if (r.y1 > Hi - 1) r.y1 = Hi - 1;
        if (r.x0 <= r.x1 && r.y0 <= r.y1) o.r[o.n++] = r;
    }
    return o;
}
// resized pixels (preprocess_kernel) whose bilinear taps meet source span [a, b]: tap y0 = floor(max(sh (y + 0.5) - 0.5, 0)) and y0 + 1,
// widened by one source index on each side against float / double rounding; padding (>= nr) is zeros in both views
static inline bool cut_resize_span(int a, int b, int n_src, int nr, int* lo, int* hi) {
    const double sc = (double)n_src / (double)nr;
    int l = nr, h = -1;
    for (int y = 0; y < nr; y++) {
        double f = sc * ((double)y + 0.5) - 0.5; if (f < 0.0) f = 0.0;
        const int t0 = (int)f;
        if (t0 + 2 >= a && t0 - 1 <= b) { if (y < l) l = y; h = y; }
    }
    *lo = l; *hi = h;
    return l <= h;
}
// nblk blocks (stride of conv2 each, levels from the pooled stem output at /4) -> per block the dirty set of its output (= what conv2,
// conv3 and the downsample conv recompute) and conv1's compute set; *pool1 = the dirty set of the pooled stem output.  Level sizes are the
// plan's (Hp >> l, Wp >> l).
static inline void cut_geometry(int H, int W, int Hr, int Wr, int Hp, int Wp, int nrect, const int* rects, int nblk, const int* stride,
                                CutSet* pool1, CutSet* out, CutSet* t1) {
    CutSet s; s.n = 0;
    for (int i = 0; i < nrect && i < CUT_SET_MAX; i++) {
        const int* q = rects + 4 * i;           // source pixels [q0, q2) x [q1, q3)
        if (q[2] <= q[0] || q[3] <= q[1]) continue;
        CutRect r;
        if (cut_resize_span(q[0], q[2] - 1, W, Wr, &r.x0, &r.x1) && cut_resize_span(q[1], q[3] - 1, H, Hr, &r.y0, &r.y1)) s.r[s.n++] = r;
    }
    s = cut_map(s, 7, 2, 3, Hp >> 1, Wp >> 1);         // stem 7 x 7 / 2
    s = cut_map(s, 3, 2, 1, Hp >> 2, Wp >> 2);         // max-pool 3 x 3 / 2
    *pool1 = s;
    int l = 2;
    for (int b = 0; b < nblk; b++) {
        const int lo = l + (stride[b] == 2 ? 1 : 0);
        out[b] = cut_map(s, 3, stride[b], 1, Hp >> lo, Wp >> lo);
        t1[b] = cut_window(out[b], stride[b], Hp >> l, Wp >> l);
        s = out[b]; l = lo;
    }
}
// The FPN of Faster R-CNN on the cut_out view (forward.hip fpn): c[0..3] = the dirty sets of C2..C5 (the `out` sets of the stages' last
// blocks), levels 2..5 of the plan.  Lateral l is a 1 x 1 conv of C_l plus the 2 x nearest upsample of lateral l + 1, so
//   inner P5 dirty = C5 dirty;   inner P_l dirty = dirty(C_l) U upsample(inner P_{l + 1} dirty);   output P_l = the 3 x 3 pad-1 map of inner P_l.
// Padded sizes are multiples of 32: every level is exactly twice the one above, and the upsample of [x0, x1] is [2 x0, 2 x1 + 1].  Each
// cutout rectangle is carried on its own, as everywhere here: its rectangle of dirty(C_l) lies inside the upsample of its rectangle one
// level up (a stride-2 3 x 3 map and its 2 x upsample cover the span they came from, later blocks only widen it), so the union per
// rectangle is the hull of the two.  A set pair that does not line up rectangle by rectangle (none does) takes the whole level.
static inline CutRect cut_hull(const CutRect& a, const CutRect& b) {
    return {a.x0 < b.x0 ? a.x0 : b.x0, a.y0 < b.y0 ? a.y0 : b.y0, a.x1 > b.x1 ? a.x1 : b.x1, a.y1 > b.y1 ? a.y1 : b.y1};
}
static inline void cut_fpn_geometry(int Hp, int Wp, const CutSet* c, CutSet* inner, CutSet* outp) {
    inner[3] = c[3];
    for (int i = 2; i >= 0; i--) {
        const int Hl = Hp >> (2 + i), Wl = Wp >> (2 + i);
        const CutSet& up = inner[i + 1];
        CutSet s; s.n = 0;
        if (up.n == c[i].n) {
            for (int q = 0; q < up.n; q++) {
                CutRect u = {2 * up.r[q].x0, 2 * up.r[q].y0, 2 * up.r[q].x1 + 1, 2 * up.r[q].y1 + 1};
                if (u.x1 > Wl - 1) u.x1 = Wl - 1; if (u.y1 > Hl - 1) u.y1 = Hl - 1;
                s.r[s.n++] = cut_hull(u, c[i].r[q]);
            }
        } else if (up.n || c[i].n) {
            s.n = 1; s.r[0] = {0, 0, Wl - 1, Hl - 1};
        }
        inner[i] = s;
    }
    for (int i = 0; i < 4; i++) outp[i] = cut_map(inner[i], 3, 1, 1, Hp >> (2 + i), Wp >> (2 + i));
}
// a set as disjoint rectangles, row bands top to bottom (a band's runs merged, a run that continues one of the band above extends it);
// -1 if more than cap
static inline int cut_disjoint(const CutSet& s, CutRect* o, int cap) {
    int ys[2 * CUT_SET_MAX], ny = 0;
    for (int i = 0; i < s.n; i++) { ys[ny++] = s.r[i].y0; ys[ny++] = s.r[i].y1 + 1; }
    for (int i = 1; i < ny; i++) for (int j = i; j > 0 && ys[j] < ys[j - 1]; j--) { const int t = ys[j]; ys[j] = ys[j - 1]; ys[j - 1] = t; }
    int n = 0;
    for (int k = 0; k + 1 < ny; k++) {
        const int ya = ys[k], yb = ys[k + 1] - 1;
        if (ya > yb) continue;
        int x0[CUT_SET_MAX], x1[CUT_SET_MAX], nx = 0;
        for (int i = 0; i < s.n; i++)
            if (s.r[i].y0 <= ya && s.r[i].y1 >= yb) { x0[nx] = s.r[i].x0; x1[nx] = s.r[i].x1; nx++; }
        for (int i = 1; i < nx; i++) for (int j = i; j > 0 && x0[j] < x0[j - 1]; j--) {
            int t = x0[j]; x0[j] = x0[j - 1]; x0[j - 1] = t; t = x1[j]; x1[j] = x1[j - 1]; x1[j - 1] = t;
        }
        for (int i = 0; i < nx;) {
            const int a = x0[i];
            int b = x1[i++];
            while (i < nx && x0[i] <= b + 1) { if (x1[i] > b) b = x1[i]; i++; }
            bool ext = false;
            for (int q = 0; q < n && !ext; q++)
                if (o[q].x0 == a && o[q].x1 == b && o[q].y1 == ya - 1) { o[q].y1 = yb; ext = true; }
            if (ext) continue;
            if (n == cap) return -1;
            o[n++] = {a, ya, b, yb};
        }
    }
    return n;
}
