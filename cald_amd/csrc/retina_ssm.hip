// retina_ssm.hip -- the SSM tail of RetinaNet: RetinaNet.ssm_postprocess_detections (detection/retina_ssm.py:487-584) + transform.postprocess
// of V views.  The reference sub-samples every class's candidates with random.shuffle in the middle of the tail; the shuffle needs one
// number per (view, class) -- how many anchors passed the score threshold -- so the tail is two device phases around one host stop.
// Phase A (launch_retina_ssm_phase_a):
//   rssm_compact_kernel<false>  one thread per anchor, one det_sigmoidf per (anchor, class) -- the bits retina_emit_kernel stores in scores_cls.
//                               Per class a 64-bit __ballot of `score > score_thr` per wave; the block's count of the class goes to
//                               blk_off[view][class][block].  The view's largest score over ALL K classes as an orderable key
//                               (atomicMax on integers: order-free).
//   rssm_scan_kernel            per (class, view) the exclusive prefix sum of the block counts (integers, a fixed order), the class's count
//                               n_c, and the view's flag al = (largest score < 0.5).
//   rssm_compact_kernel<true>   the same ballots again; a candidate's slot is (candidates of the blocks before) + (of the waves before in
//                               the block) + (popcount of the lower lanes): the list holds the anchor indices in ascending order in every
//                               run, without a sort and without an atomic cursor.
// The host reads n_c and al, draws per class up to CALD_SSM_RETINA_TAKE positions into the class's list (cald_ssm_pick_fn), checks and uploads them.
// Phase B (launch_retina_ssm_phase_b):
//   rssm_class_nms_kernel       one workgroup per (class, view): the picked candidates sorted by (score desc, pick position asc) -- among
//                               equal scores the one earlier in the shuffled list wins --, decoded and clipped (retina_decode), boxes with a
//                               side < 1e-2 skipped (they used up a pick), greedy NMS, the first per_class survivors.
//   rssm_offsets_kernel         exclusive prefix sums of the per-class row counts over (view, class): one workgroup, no cursor atomics.
//   rssm_emit_kernel            the rows: box scaled to the original image (retina_emit_kernel's float32 ratios), the score of the row's
//                               class, the labels +1 iff sigmoid > 0.5 over classes 1..K-1 (judge_y on scores[1:]).
// A view with al = 1 does nothing in phase B and gives no rows.
#include "../../include/cald_hip.h"
#include "sortnms.h"
#include "kernels.h"

#define RSSM_MAXK 256                       // classes (cald_op_retina_ssm_postprocess and the model both refuse more)
#define RSSM_TAKE CALD_SSM_RETINA_TAKE
#define RSSM_SLOTS 512                      // power of two >= RSSM_TAKE: the keys one workgroup sorts in LDS

__device__ inline const float* rssm_logits(const RetinaArgs& r, int v, int i) {
    int li;
    const int l = retina_level_of(r, v, i, &li);
    const LevelSeg sg = r.seg[l][v];
    const int pix = li / r.A, an = li - pix * r.A;
    return r.cls[l] + (sg.pix_off + pix) * (long long)r.cls_ld + an * r.K;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void rssm_compact_kernel(RetinaSsmArgs a) {
    __shared__ unsigned long long s_bal[4][RSSM_MAXK];
    const RetinaArgs& r = a.r;
    const int v = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K = r.K;
    const int i = b * 256 + tid;
    int total = 0;
#pragma unroll
    for (int t = 0; t < 5; t++) total += r.seg[t][v].H * r.seg[t][v].W * r.A;
    const bool valid = i < total;           // no early return: every lane takes part in the ballots
    const float* lg = valid ? rssm_logits(r, v, i) : nullptr;
    unsigned best = 0u;
    for (int k = 0; k < K; k++) {
        bool pass = false;
        if (valid) {
            const float s = det_sigmoidf(lg[k]);
            pass = s > r.score_thr;
            if (!WRITE) { const unsigned key = det_orderable(s); if (key > best) best = key; }
        }
        const unsigned long long m = __ballot(pass);
        if (lane == 0) s_bal[wave][k] = m;
    }
    __syncthreads();
    if (!WRITE) {
        for (int k = tid; k < K; k += 256)
            a.blk_off[((long long)v * K + k) * a.nblk + b] = __popcll(s_bal[0][k]) + __popcll(s_bal[1][k]) + __popcll(s_bal[2][k]) + __popcll(s_bal[3][k]);
        for (int s = 32; s > 0; s >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)best, s, 64); if (o > best) best = o; }
        if (lane == 0 && best) atomicMax(&a.vmax[v], best);
    } else {
        if (!valid) return;
        for (int k = 0; k < K; k++) {
            const unsigned long long m = s_bal[wave][k];
            if (!((m >> lane) & 1ull)) continue;
            const long long slot = (long long)v * K + k;
            int off = a.blk_off[slot * a.nblk + b];
            for (int w = 0; w < wave; w++) off += __popcll(s_bal[w][k]);
            off += __popcll(m & ((1ull << lane) - 1ull));
            if (off < r.cand_cap) a.list[slot * r.cand_cap + off] = i;
        }
    }
}

// thread t sums blocks [t * per, (t + 1) * per); thread 0 chains the 256 partial sums; every thread then rewrites its blocks as offsets
__global__ __launch_bounds__(256) void rssm_scan_kernel(RetinaSsmArgs a) {
    __shared__ int s_part[256];
    const int k = blockIdx.x, v = blockIdx.y, tid = threadIdx.x, nblk = a.nblk, K = a.r.K;
    int* bo = a.blk_off + ((long long)v * K + k) * nblk;
    const int per = (nblk + 255) / 256;
    const int b0 = tid * per < nblk ? tid * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    int s = 0;
    for (int b = b0; b < b1; b++) s += bo[b];
    s_part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; t++) { const int c = s_part[t]; s_part[t] = run; run += c; }
        a.r.cand_count[v * K + k] = run;
        if (k == 0) a.al[v] = a.vmax[v] < det_orderable(a.conf_thr) ? 1 : 0;
    }
    __syncthreads();
    int run = s_part[tid];
    for (int b = b0; b < b1; b++) { const int c = bo[b]; bo[b] = run; run += c; }
}

__global__ __launch_bounds__(RSSM_SLOTS) void rssm_class_nms_kernel(RetinaSsmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ int s_nk;
    const RetinaArgs& r = a.r;
    const int per = r.per_class;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(dyn);
    float4* cbox = reinterpret_cast<float4*>(dyn + RSSM_SLOTS * 8);
    float4* kept_box = cbox + RSSM_SLOTS;
    float* kept_area = reinterpret_cast<float*>(kept_box + per);
    int* keep_idx = reinterpret_cast<int*>(kept_area + per);
    int* s_anchor = keep_idx + per;
    unsigned char* s_skip = reinterpret_cast<unsigned char*>(s_anchor + RSSM_SLOTS);
    const int k = blockIdx.x, v = blockIdx.y, tid = threadIdx.x, K = r.K;
    const long long slot = (long long)v * K + k;
    if (a.al[v]) {                            // uniform per workgroup
        if (tid == 0) r.kept_count[slot] = 0;
        return;
    }
    // the host has checked every pick against the count; the clamps keep an index inside the list whatever arrives
    const int cnt = r.cand_count[slot] < r.cand_cap ? r.cand_count[slot] : r.cand_cap;
    int np = a.n_picks[slot];
    if (np > RSSM_TAKE) np = RSSM_TAKE;
    if (np > cnt) np = cnt;
    if (np < 0) np = 0;
    const int* list = a.list + slot * r.cand_cap;
    const int* picks = a.picks + slot * RSSM_TAKE;
    unsigned long long key = 0ull;
    if (tid < np) {
        int pos = picks[tid]; pos = pos < 0 ? 0 : (pos >= cnt ? cnt - 1 : pos);
        const float s = det_sigmoidf(rssm_logits(r, v, list[pos])[k]);
        key = ((unsigned long long)det_orderable(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)tid);
    }
    keys[tid] = key;
    __syncthreads();
    block_bitonic_sort_desc(keys, RSSM_SLOTS);
    const ViewDesc vd = r.views[v];
    const float Wr = (float)vd.Wr, Hr = (float)vd.Hr;
    if (tid < np) {
        const int p = (int)(0xFFFFFFFFu - (unsigned)(keys[tid] & 0xFFFFFFFFull));
        int pos = picks[p]; pos = pos < 0 ? 0 : (pos >= cnt ? cnt - 1 : pos);
        const int ai = list[pos];
        const float4 b = retina_decode(r, v, ai, Wr, Hr);
        s_skip[tid] = ((b.z - b.x) >= r.min_box && (b.w - b.y) >= r.min_box) ? 0 : 1;   // remove_small_boxes, after the cut at RSSM_TAKE
        cbox[tid] = b;
        s_anchor[tid] = ai;
    }
    __syncthreads();
    block_nms_sorted(cbox, np, r.nms_thr, per, kept_box, kept_area, nullptr, keep_idx, &s_nk, s_skip);
    const int nk = s_nk;
    for (int i = tid; i < nk; i += RSSM_SLOTS) {
        const int ci = keep_idx[i];
        r.kept_anchor[slot * per + i] = s_anchor[ci];
        reinterpret_cast<float4*>(r.kept_box)[slot * per + i] = cbox[ci];
    }
    if (tid == 0) r.kept_count[slot] = nk;
}

// one workgroup: thread t sums the classes of views t, t + 256, ...; thread 0 chains the views (ssm_offsets_kernel's pattern)
__global__ __launch_bounds__(256) void rssm_offsets_kernel(RetinaSsmArgs a) {
    __shared__ int s_base[CALD_MAX_VIEWS + 1];
    const int K = a.r.K, V = a.r.V;
    for (int v = threadIdx.x; v < V; v += 256) {
        int s = 0;
        for (int k = 0; k < K; k++) { a.row_off[(long long)v * K + k] = s; s += a.r.kept_count[(long long)v * K + k]; }
        a.count[v] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int v = 0; v < V; v++) { s_base[v] = s; s += a.count[v]; }
        *a.total = s;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256)
        for (int k = 0; k < K; k++) a.row_off[(long long)v * K + k] += s_base[v];
}

__global__ __launch_bounds__(256) void rssm_emit_kernel(RetinaSsmArgs a) {
    const RetinaArgs& r = a.r;
    const int k = blockIdx.x, v = blockIdx.y, K = r.K, per = r.per_class, L = K - 1;
    const long long slot = (long long)v * K + k;
    const int nk = r.kept_count[slot];
    const long long row0 = a.row_off[slot];
    const ViewDesc vd = r.views[v];
    const float rh = (float)vd.Ho / (float)vd.Hr, rw = (float)vd.Wo / (float)vd.Wr;   // stock resize_boxes: fp32 ratio
    for (int i = threadIdx.x; i < nk; i += 256) {
        const float4 b = reinterpret_cast<const float4*>(r.kept_box)[slot * per + i];
        reinterpret_cast<float4*>(a.boxes)[row0 + i] = make_float4(b.x * rw, b.y * rh, b.z * rw, b.w * rh);
        a.scores[row0 + i] = det_sigmoidf(rssm_logits(r, v, r.kept_anchor[slot * per + i])[k]);
    }
    for (int e = threadIdx.x; e < nk * L; e += 256) {
        const int i = e / L, q = e - i * L;
        const float s = det_sigmoidf(rssm_logits(r, v, r.kept_anchor[slot * per + i])[1 + q]);
        a.labels[(row0 + i) * L + q] = s > a.conf_thr ? 1 : -1;
    }
}

void launch_retina_ssm_phase_a(const RetinaSsmArgs& a, hipStream_t st) {
    hipMemsetAsync(a.vmax, 0, sizeof(unsigned) * a.r.V, st);
    hipLaunchKernelGGL(rssm_compact_kernel<false>, dim3(a.nblk, a.r.V), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rssm_scan_kernel, dim3(a.r.K, a.r.V), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rssm_compact_kernel<true>, dim3(a.nblk, a.r.V), dim3(256), 0, st, a);
}

void launch_retina_ssm_phase_b(const RetinaSsmArgs& a, hipStream_t st) {
    const size_t lds = (size_t)RSSM_SLOTS * (8 + 16 + 4 + 1) + (size_t)a.r.per_class * (16 + 4 + 4);      // 14.5 KB + 24 B a kept box: below 64 KB at per_class <= 1024
    hipLaunchKernelGGL(rssm_class_nms_kernel, dim3(a.r.K, a.r.V), dim3(RSSM_SLOTS), lds, st, a);
    hipLaunchKernelGGL(rssm_offsets_kernel, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rssm_emit_kernel, dim3(a.r.K, a.r.V), dim3(256), 0, st, a);
}
