// ssm.hip -- the SSM tail: RoIHeads.ssm_postprocess_detections (detection/frcnn_ssm.py:44-102) + transform.postprocess of V views.
//   ssm_softmax_kernel    per proposal the softmax of post_softmax_kernel (roi.hip: det_expf, the same summation order -- the same bits), and
//                         the view's largest foreground probability as an orderable key (atomicMax on integers: order-free).
//   ssm_class_nms_kernel  one workgroup per (foreground class, view): all proposals of the view sorted by (probability of the class desc,
//                         proposal index asc), decoded with weights (10, 10, 5, 5) and clipped as post_nms_kernel does, greedy NMS at 0.3
//                         on the boxes + c * (maxc + 1) in float32 (batched_nms with every label equal to c: maxc is the maximum over THIS
//                         class's boxes), the first `cap` survivors, of those the prefix with probability > score_thr.
//                         A view with al = 1 (largest foreground probability < 0.5, or no proposals) does nothing and gives no rows.
//   ssm_offsets_kernel    exclusive prefix sums of the per-class row counts over (view, class): one workgroup, integer sums, no atomics on
//                         a cursor -- the row order is (view, class, kept order) in every run.
//   ssm_emit_kernel       the rows: box scaled to the original image (post_nms_kernel's expression), the proposal's C - 1 foreground
//                         probabilities, and the labels +1 iff probability > 0.5 (judge_y, frcnn_ssm.py:29-39).
// LDS of a class workgroup: 1 024 keys (8 KB) + raw and offset boxes (16 KB each) + the max reduction (4 KB) + the kept list (24 B a box):
// 46.4 KB at cap = 100, so three workgroups fit a CU's 160 KB and the 1 024-thread workgroups, two a CU, are what bounds the occupancy.
#include "sortnms.h"
#include "kernels.h"

__global__ __launch_bounds__(256) void ssm_softmax_kernel(SsmArgs a) {
    const int v = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    int n = a.prop_count[v]; if (n > CALD_ROI_CAP) n = CALD_ROI_CAP;
    if (r >= n) return;
    const int C = a.C;
    const float* lg = a.pred + ((long long)v * CALD_ROI_CAP + r) * a.pred_ld;
    float* pr = a.prob + ((long long)v * CALD_ROI_CAP + r) * C;
    float m = lg[0];
    for (int c = 1; c < C; c++) if (lg[c] > m) m = lg[c];
    float s = 0.0f;
    for (int c = 0; c < C; c++) { const float e = det_expf(lg[c] - m); pr[c] = e; s = s + e; }
    float pm = 0.0f;
    for (int c = 0; c < C; c++) {
        const float p = pr[c] / s;
        pr[c] = p;
        if (c == 1 || (c > 1 && p > pm)) pm = p;
    }
    atomicMax(&a.vmax[v], det_orderable(pm));
}

#define SSM_LDS_FIXED (1024 * (8 + 16 + 16 + 4))
__global__ __launch_bounds__(1024) void ssm_class_nms_kernel(SsmArgs a) {
    __shared__ int s_nk, s_m;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];      // SSM_LDS_FIXED bytes, then the kept list
    const int cap = a.cap;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(dyn);
    float4* cbox = reinterpret_cast<float4*>(dyn + 1024 * 8);
    float4* obox = cbox + 1024;
    float* red = reinterpret_cast<float*>(obox + 1024);
    float4* kept_box = reinterpret_cast<float4*>(dyn + SSM_LDS_FIXED);
    float* kept_area = reinterpret_cast<float*>(kept_box + cap);
    int* keep_idx = reinterpret_cast<int*>(kept_area + cap);
    const int c = blockIdx.x + 1, v = blockIdx.y, tid = threadIdx.x, C = a.C;
    const long long vc = (long long)v * (C - 1) + (c - 1);
    int n = a.prop_count[v]; if (n > CALD_ROI_CAP) n = CALD_ROI_CAP;
    if (n <= 0 || a.vmax[v] < det_orderable(a.conf_thr)) {       // al = 1: the whole grid row of the view leaves (uniform per workgroup)
        if (tid == 0) a.cls_count[vc] = 0;
        return;
    }
    const float* prob = a.prob + (long long)v * CALD_ROI_CAP * C;
    keys[tid] = tid < n ? (((unsigned long long)det_orderable(prob[(long long)tid * C + c]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)tid)) : 0ull;
    if (tid == 0) s_m = 0;
    __syncthreads();
    block_bitonic_sort_desc(keys, 1024);
    const ViewDesc vd = a.views[v];
    const float Wr = (float)vd.Wr, Hr = (float)vd.Hr;
    float mx = -INFINITY;
    if (tid < n) {
        const int r = (int)(0xFFFFFFFFu - (unsigned)(keys[tid] & 0xFFFFFFFFull));
        const float4 p = reinterpret_cast<const float4*>(a.proposals)[(long long)v * CALD_ROI_CAP + r];
        const float pb[4] = {p.x, p.y, p.z, p.w};
        const float* dl = a.pred + ((long long)v * CALD_ROI_CAP + r) * a.pred_ld + C + 4 * c;
        const float d[4] = {dl[0], dl[1], dl[2], dl[3]};
        float o[4];
        det_box_decode(pb, d, 10.0f, 10.0f, 5.0f, 5.0f, o);
        float4 b;
        b.x = det_clamp(o[0], 0.0f, Wr); b.z = det_clamp(o[2], 0.0f, Wr);
        b.y = det_clamp(o[1], 0.0f, Hr); b.w = det_clamp(o[3], 0.0f, Hr);
        cbox[tid] = b;
        mx = fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w));
    }
    red[tid] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
    const float off = (float)c * (red[0] + 1.0f);
    if (tid < n) { const float4 b = cbox[tid]; obox[tid] = make_float4(b.x + off, b.y + off, b.z + off, b.w + off); }
    __syncthreads();
    block_nms_sorted(obox, n, a.nms_thr, cap, kept_box, kept_area, nullptr, keep_idx, &s_nk);
    const int nk = s_nk;
    const float rh = (float)((double)vd.Ho / (double)vd.Hr), rw = (float)((double)vd.Wo / (double)vd.Wr);
    // kept order is score order: the rows above the threshold are a prefix, and its length is their number
    if (tid < nk) {
        const int k = keep_idx[tid];
        const int r = (int)(0xFFFFFFFFu - (unsigned)(keys[k] & 0xFFFFFFFFull));
        if (prob[(long long)r * C + c] > a.score_thr) {
            atomicAdd(&s_m, 1);
            const float4 b = cbox[k];
            a.kept_prop[vc * cap + tid] = r;
            reinterpret_cast<float4*>(a.kept_box)[vc * cap + tid] = make_float4(b.x * rw, b.y * rh, b.z * rw, b.w * rh);
        }
    }
    __syncthreads();
    if (tid == 0) a.cls_count[vc] = s_m;
}

// one workgroup: thread t sums the classes of views t, t + 256, ...; thread 0 chains the views
__global__ __launch_bounds__(256) void ssm_offsets_kernel(SsmArgs a) {
    __shared__ int s_base[CALD_MAX_VIEWS + 1];
    const int K = a.C - 1;
    for (int v = threadIdx.x; v < a.V; v += 256) {
        int s = 0;
        for (int k = 0; k < K; k++) { a.row_off[(long long)v * K + k] = s; s += a.cls_count[(long long)v * K + k]; }
        a.count[v] = s;
        int n = a.prop_count[v]; if (n > CALD_ROI_CAP) n = CALD_ROI_CAP;
        a.al[v] = (n <= 0 || a.vmax[v] < det_orderable(a.conf_thr)) ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int v = 0; v < a.V; v++) { s_base[v] = s; s += a.count[v]; }
        *a.total = s;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < a.V; v += 256)
        for (int k = 0; k < K; k++) a.row_off[(long long)v * K + k] += s_base[v];
}

__global__ __launch_bounds__(256) void ssm_emit_kernel(SsmArgs a) {
    const int K = a.C - 1, v = blockIdx.y, C = a.C;
    const long long vc = (long long)v * K + blockIdx.x;
    const int cnt = a.cls_count[vc];
    const long long row0 = a.row_off[vc];
    const float* prob = a.prob + (long long)v * CALD_ROI_CAP * C;
    for (int i = threadIdx.x; i < cnt; i += 256)
        reinterpret_cast<float4*>(a.boxes)[row0 + i] = reinterpret_cast<const float4*>(a.kept_box)[vc * a.cap + i];
    for (int e = threadIdx.x; e < cnt * K; e += 256) {
        const int i = e / K, q = e - i * K;
        const float p = prob[(long long)a.kept_prop[vc * a.cap + i] * C + 1 + q];
        a.scores[(row0 + i) * K + q] = p;
        a.labels[(row0 + i) * K + q] = p > a.conf_thr ? 1 : -1;
    }
}

void launch_ssm_postprocess(const SsmArgs& a, hipStream_t st) {
    hipMemsetAsync(a.vmax, 0, sizeof(unsigned) * a.V, st);
    hipLaunchKernelGGL(ssm_softmax_kernel, dim3((CALD_ROI_CAP + 255) / 256, a.V), dim3(256), 0, st, a);
    static PerDeviceOnce once;
    allow_big_lds(once, ssm_class_nms_kernel);      // cap above ~800 takes the workgroup past the default 64 KB
    hipLaunchKernelGGL(ssm_class_nms_kernel, dim3(a.C - 1, a.V), dim3(1024), SSM_LDS_FIXED + (size_t)a.cap * (16 + 4 + 4), st, a);
    hipLaunchKernelGGL(ssm_offsets_kernel, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(ssm_emit_kernel, dim3(a.C - 1, a.V), dim3(256), 0, st, a);
}
