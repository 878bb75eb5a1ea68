// audit.hip -- decision margins of one forward (cald_sweep_audit; the cascade of DESIGN.md section 6b): Faster R-CNN first, RetinaNet's
// tail (its own set of decisions) at the end of the file.
//
// The sweep's result is a continuous function of the GEMM outputs EXCEPT at its discrete decisions: the per-level top-k cut and the
// NMS of the RPN (detection/frcnn_ll.py:284-321), the post-NMS top-n, the RoI level mapper and RoIAlign's border rule
// (torchvision MultiScaleRoIAlign, detection/frcnn_la.py:205-209), the score threshold / class-batched NMS / top-100 of
// postprocess_detections (detection/frcnn_la.py:72-80), and -- in the scoring loop -- argmax over the IoU row and the linspace
// sub-sample of a sorted list (cald_train.py:110-113, :214).  A forward computed with slightly different rounding (precision f16x3)
// reproduces the exact mode's result to ~1e-6 unless one of those decisions comes out differently.  These kernels record, per view
// and per kind of decision, the smallest distance of any RELEVANT decision to its flip point; a view whose margins all exceed the
// rounding noise took the same decisions in both modes.
//
// Relevance: the merged post-NMS proposal list is cut at post_n entries by score.  A decision that only concerns boxes whose score
// lies more than `delta` below that cut cannot change the output (a box is affected only by higher-scored boxes, and everything
// below the cut is dropped), so it is ignored -- otherwise the top-k cut of the finest level alone (60 800 x 3 logits, gaps of 1e-4
// at rank 1000) would flag every other view.  Likewise a near-threshold (proposal, class) score matters only if the box would
// survive NMS, and candidates behind the top-100 cut never matter.
//
// Nothing here feeds the detections: the audit reads the forward's own scratch buffers after the fact.
#include "common.h"
#include "kernels.h"

namespace {
__device__ __forceinline__ float key_score(unsigned long long key) {       // inverse of det_orderable on the key's high word
    const unsigned k = (unsigned)(key >> 32);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ void upd(float* slot, float m) {
    if (!(m >= 0.0f)) m = 0.0f;                                              // NaN or negative: flag
    atomicMin(reinterpret_cast<unsigned*>(slot), __float_as_uint(m));       // non-negative floats order like their bit patterns
}
// the IoU torchvision's nms computes (sortnms.h nms_overlaps, same operation order)
__device__ __forceinline__ float nms_iou(const float4 bi, const float4 bj) {
    const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y);
    const float xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    const float ai = (bi.z - bi.x) * (bi.w - bi.y), aj = (bj.z - bj.x) * (bj.w - bj.y);
    return inter / ((ai + aj) - inter);
}
__global__ void audit_fill_kernel(float* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = INFINITY;
}

// ---------------------------------------------------------------------------------------------
// RPN: grid (5 levels, V), block 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void audit_rpn_kernel(AuditArgs a) {
    __shared__ float4 kb[1024];
    __shared__ float ks[1024];
    __shared__ int kidx[1024];
    __shared__ int s_nk;
    const int l = blockIdx.x, v = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int pre = a.pre_n;
    const long long base = (long long)v * 5 * pre + (long long)l * pre;
    const unsigned long long* ck = a.cand_key + base;
    const float4* cb = reinterpret_cast<const float4*>(a.cand_box) + base;
    const float4* sb = reinterpret_cast<const float4*>(a.sorted_box) + base;       // level offset applied: what NMS compared
    const unsigned char* skip = a.flags + (long long)v * 10 * pre + (long long)l * pre;
    const unsigned char* keep = skip + 5 * pre;
    float* out = a.out + (long long)v * CALD_VM;
    const unsigned long long t0 = a.trunc_key[2 * v], t1 = a.trunc_key[2 * v + 1];
    const float s_cut = t0 ? key_score(t0) - a.delta : -INFINITY;                  // scores below this cannot reach the output
    if (tid == 0) s_nk = 0;
    __syncthreads();
    if (tid < 64) {          // kept boxes of the level, in score order (one wave: ballots keep the order)
        int nk = 0;
        for (int c0 = 0; c0 < pre && c0 < 1024; c0 += 64) {
            const int j = c0 + lane;
            const bool kp = j < pre && keep[j];
            const unsigned long long m = __ballot(kp);
            if (kp) { const int p = nk + __popcll(m & ((1ull << lane) - 1ull)); kb[p] = sb[j]; ks[p] = key_score(ck[j]); kidx[p] = j; }
            nk += __popcll(m);
        }
        if (lane == 0) s_nk = nk;
    }
    __syncthreads();
    const int nk = s_nk;
    if (tid == 0) {
        const unsigned long long k1 = a.next_key[((long long)v * 5 + l) * 2], k2 = a.next_key[((long long)v * 5 + l) * 2 + 1];
        if (k1 && k2) { const float sk = key_score(k1); if (sk >= s_cut) upd(out + VM_RPN_TOPK, sk - key_score(k2)); }
        if (l == 0 && t1) upd(out + VM_RPN_TRUNC, key_score(t0) - key_score(t1));
    }
    float m_small = INFINITY, m_iou = INFINITY, m_ord = INFINITY;
    for (int j = tid; j < pre; j += 256) {
        const float4 b = cb[j];
        if (b.x != 0.0f || b.y != 0.0f || b.z != 0.0f || b.w != 0.0f)              // slots beyond the level's anchors hold zeros
            m_small = fminf(m_small, fminf(fabsf((b.z - b.x) - a.min_size), fabsf((b.w - b.y) - a.min_size)));
        if (skip[j] || ck[j] == 0ull) continue;
        const float sj = key_score(ck[j]);
        if (!(sj >= s_cut)) continue;
        const float4 bj = sb[j];
        float mx = 0.0f;
        for (int i = 0; i < nk && kidx[i] < j; i++) {
            const float iou = nms_iou(kb[i], bj);
            if (iou > mx) mx = iou;
            if (iou > a.rpn_nms_thr) m_ord = fminf(m_ord, ks[i] - sj);              // i suppresses j: had j scored higher, j would suppress i
        }
        m_iou = fminf(m_iou, fabsf(mx - a.rpn_nms_thr));
    }
    if (m_small < INFINITY) upd(out + VM_RPN_SMALL, m_small);
    if (m_iou < INFINITY) upd(out + VM_RPN_IOU, m_iou);
    if (m_ord < INFINITY) upd(out + VM_RPN_ORDER, m_ord);
}

// ---------------------------------------------------------------------------------------------
// RoI level mapper and RoIAlign border rule: grid V, block 256.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void audit_roi_kernel(AuditArgs a) {
    const int v = blockIdx.x, tid = threadIdx.x;
    const int n = a.prop_count[v];
    float m_lvl = INFINITY, m_edge = INFINITY;
    for (int r = tid; r < n; r += 256) {
        const float4 box = reinterpret_cast<const float4*>(a.proposals)[(long long)v * CALD_ROI_CAP + r];
        const float area = (box.z - box.x) * (box.w - box.y);
        const float val = (4.0f + det_log2f(sqrtf(area) / 224.0f)) + 1e-6f;         // roi_level(): floor(val) clamped to [2, 5]
        if (val == val) m_lvl = fminf(m_lvl, fminf(fabsf(val - 3.0f), fminf(fabsf(val - 4.0f), fabsf(val - 5.0f))));
        const int l = roi_level(box);
        const LevelSeg sg = a.seg[l][v];
        const float scale = 1.0f / (float)(4 << l);
        const float x1 = box.x * scale, y1 = box.y * scale, x2 = box.z * scale, y2 = box.w * scale;
        float rw = x2 - x1; if (!(rw >= 1.0f)) rw = 1.0f;
        float rh = y2 - y1; if (!(rh >= 1.0f)) rh = 1.0f;
        const float bw = rw / 7.0f, bh = rh / 7.0f;
        for (int s = 0; s < 14; s++) {                                               // roi_sample(): a sample outside [-1, size] reads zero
            const float ty = y1 + (float)(s >> 1) * bh + ((float)(s & 1) + 0.5f) * bh / 2.0f;
            const float tx = x1 + (float)(s >> 1) * bw + ((float)(s & 1) + 0.5f) * bw / 2.0f;
            m_edge = fminf(m_edge, fminf(fminf(fabsf(ty + 1.0f), fabsf(ty - (float)sg.H)), fminf(fabsf(tx + 1.0f), fabsf(tx - (float)sg.W))));
        }
    }
    if (m_lvl < INFINITY) upd(a.out + (long long)v * CALD_VM + VM_ROI_LEVEL, m_lvl);
    if (m_edge < INFINITY) upd(a.out + (long long)v * CALD_VM + VM_ROI_EDGE, m_edge);
}

// ---------------------------------------------------------------------------------------------
// postprocess_detections: grid V, block 256.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 audit_cand_box(const AuditArgs& a, int v, int r, int c, float Wr, float Hr, float maxc) {
    const float4 p = reinterpret_cast<const float4*>(a.proposals)[(long long)v * CALD_ROI_CAP + r];
    const float pb[4] = {p.x, p.y, p.z, p.w};
    const float* dl = a.pred + ((long long)v * CALD_ROI_CAP + r) * a.pred_ld + a.C + 4 * c;
    const float d[4] = {dl[0], dl[1], dl[2], dl[3]};
    float o[4];
    det_box_decode(pb, d, 10.0f, 10.0f, 5.0f, 5.0f, o);
    const float off = (float)c * (maxc + 1.0f);
    return make_float4(det_clamp(o[0], 0.0f, Wr) + off, det_clamp(o[1], 0.0f, Hr) + off, det_clamp(o[2], 0.0f, Wr) + off, det_clamp(o[3], 0.0f, Hr) + off);
}
__global__ __launch_bounds__(256) void audit_post_kernel(AuditArgs a) {
    __shared__ float4 kb[AUDIT_MAX_DET];
    __shared__ float ks[AUDIT_MAX_DET];
    __shared__ int kc[AUDIT_MAX_DET];
    __shared__ unsigned long long kk[AUDIT_MAX_DET];
    __shared__ unsigned char picked[AUDIT_MAX_DET];
    const int v = blockIdx.x, tid = threadIdx.x, C = a.C;
    float* out = a.out + (long long)v * CALD_VM;
    int n = a.key_count[v]; if (n > a.key_cap) n = a.key_cap;
    int nk = a.det_count[v]; if (nk > AUDIT_MAX_DET) nk = AUDIT_MAX_DET;
    const int np = a.prop_count[v];
    const ViewDesc vd = a.views[v];
    const float Wr = (float)vd.Wr, Hr = (float)vd.Hr;
    const float maxc = a.post_maxc[v];
    const bool full = nk >= a.cap;
    for (int i = tid; i < nk; i += 256) {
        const unsigned long long key = a.kept_key[(long long)v * a.cap + i];
        const int pos = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        const int r = pos / (C - 1), c = pos - r * (C - 1) + 1;
        kk[i] = key; ks[i] = key_score(key); kc[i] = c; kb[i] = audit_cand_box(a, v, r, c, Wr, Hr, maxc);
        picked[i] = 0;
    }
    __syncthreads();
    float m_thr = INFINITY, m_iou = INFINITY, m_ord = INFINITY, m_cap = INFINITY;
    // (a) scores next to the threshold, on either side: relevant unless a kept detection of the class covers the box anyway
    if (!full) {
        for (int idx = tid; idx < np * (C - 1); idx += 256) {
            const int r = idx / (C - 1), c = idx - r * (C - 1) + 1;
            const float p = a.prob[((long long)v * CALD_ROI_CAP + r) * C + c];
            const float d = fabsf(p - a.score_thr);
            if (!(d < 1e-3f) || !(d < m_thr)) continue;
            const float4 b = audit_cand_box(a, v, r, c, Wr, Hr, maxc);
            bool covered = false;
            for (int i = 0; i < nk && !covered; i++) covered = kc[i] == c && nms_iou(kb[i], b) > a.post_nms_thr + 0.01f;
            if (!covered) m_thr = d;
        }
    }
    // (b) every candidate against the kept detections of its class that precede it
    const unsigned long long last = full && nk > 0 ? kk[nk - 1] : 0ull;
    for (int q = tid; q < n; q += 256) {
        const unsigned long long key = a.keys[(long long)v * a.key_cap + q];
        const float sj = key_score(key);
        if (full && key < last) { m_cap = fminf(m_cap, ks[nk - 1] - sj); continue; }      // behind the top-n cut
        const int pos = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        const int r = pos / (C - 1), c = pos - r * (C - 1) + 1;
        const float4 b = audit_cand_box(a, v, r, c, Wr, Hr, maxc);
        float mx = 0.0f;
        for (int i = 0; i < nk; i++) {
            if (kc[i] != c || !(kk[i] > key)) continue;
            const float iou = nms_iou(kb[i], b);
            if (iou > mx) mx = iou;
            if (iou > a.post_nms_thr) m_ord = fminf(m_ord, ks[i] - sj);
        }
        m_iou = fminf(m_iou, fabsf(mx - a.post_nms_thr));
    }
    if (m_thr < INFINITY) upd(out + VM_POST_THR, m_thr);
    if (m_iou < INFINITY) upd(out + VM_POST_IOU, m_iou);
    if (m_ord < INFINITY) upd(out + VM_POST_ORDER, m_ord);
    if (m_cap < INFINITY) upd(out + VM_POST_CAP, m_cap);
    // (c) output order: the gap between the first two detections (argmax over an all-zero IoU row picks detection 0), and -- were this a
    // reference view with more than 40 detections -- the gaps between neighbours of which np.round(np.linspace(0, n - 1, 50)) picks one
    if (tid == 0) {
        if (nk >= 2) upd(out + VM_POST_TOP2, ks[0] - ks[1]);
        if (nk > 40) {
            const double step = (double)(nk - 1) / 49.0;
            for (int i = 0; i < 50; i++) { const int k = i == 49 ? nk - 1 : (int)nearbyint((double)i * step); if (k >= 0 && k < nk) picked[k] = 1; }
            float m = INFINITY;
            for (int i = 0; i + 1 < nk; i++) if (picked[i] != picked[i + 1]) m = fminf(m, ks[i] - ks[i + 1]);
            if (m < INFINITY) upd(out + VM_POST_SUBORDER, m);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// RetinaNet.postprocess_detections (retina.hip; detection/retinanet_cal.py:402-490): grid (K classes, V), block 256, like the tail's NMS
// kernel.  The decisions are per class: `>` at the score threshold over all anchors, remove_small_boxes(1e-2), one NMS, the first
// per_class survivors; the output list is the classes' lists one after the other.  The workgroup holds its class's kept detections
// (<= per_class <= AUDIT_MAX_DET, in the tail's order) in LDS and walks ALL anchors of the view: only an anchor above the threshold or
// within 1e-3 of it is decoded, and compared by a whole wavefront.  "i precedes j" is the tail's sort order -- key orderable(score) << 32 | ~anchor, descending:
// the higher score, on equal scores the lower anchor index -- so nothing here depends on where the tail sorted.
//   VM_POST_THR    |s - thr| < 1e-3, unless the class is full (a score at the threshold ranks last and is cut), the box is small, or another
//                  kept detection of the class covers the box with IoU > nms_thr + 0.01 (it is suppressed on either side of the threshold)
//   VM_POST_SMALL  min(|w - min_box|, |h - min_box|) over every anchor above the threshold
//   VM_POST_CAP    class full: last kept score - score, over the candidates (above the threshold, not small) behind the last kept one
//   VM_POST_IOU    every other candidate: |mx - nms_thr|, mx its largest IoU with the kept boxes that precede it (0 if none does)
//   VM_POST_ORDER  ... and for each of those with IoU > nms_thr: its score - the candidate's (had the candidate ranked first, it would suppress)
//   VM_POST_TOP2   scores[0] - scores[1] of the view's list when both rows are of one class: this workgroup's, if no lower class kept a box
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float retina_score(const RetinaArgs& a, int v, int i, int k) {
    int li;
    const int l = retina_level_of(a, v, i, &li);
    const LevelSeg sg = a.seg[l][v];
    const int pix = li / a.A, an = li - pix * a.A;
    return det_sigmoidf(a.cls[l][(sg.pix_off + pix) * (long long)a.cls_ld + an * a.K + k]);
}
__device__ __forceinline__ int retina_kept(const RetinaArgs& a, long long slot) {
    int nk = a.kept_count[slot];
    if (nk > a.per_class) nk = a.per_class;
    return nk > AUDIT_MAX_DET ? AUDIT_MAX_DET : (nk < 0 ? 0 : nk);
}
__global__ __launch_bounds__(256) void audit_retina_kernel(RetinaArgs a, float* vm) {
    __shared__ float4 kb[AUDIT_MAX_DET];
    __shared__ float ks[AUDIT_MAX_DET];
    __shared__ int ka[AUDIT_MAX_DET];
    const int k = blockIdx.x, v = blockIdx.y, tid = threadIdx.x, per = a.per_class;
    const long long slot = (long long)v * a.K + k;
    float* out = vm + (long long)v * CALD_VM;
    const int nk = retina_kept(a, slot);
    const bool full = nk >= per;
    int total = 0;
#pragma unroll
    for (int t = 0; t < 5; t++) total += a.seg[t][v].H * a.seg[t][v].W * a.A;
    for (int i = tid; i < nk; i += 256) {
        const int ai = a.kept_anchor[slot * per + i];
        ka[i] = ai; kb[i] = reinterpret_cast<const float4*>(a.kept_box)[slot * per + i];
        ks[i] = (ai >= 0 && ai < total) ? retina_score(a, v, ai, k) : NAN;
    }
    __syncthreads();
    const ViewDesc vd = a.views[v];
    const float Wr = (float)vd.Wr, Hr = (float)vd.Hr;
    const float s_last = nk > 0 ? ks[nk - 1] : 0.0f;
    const int a_last = nk > 0 ? ka[nk - 1] : 0;
    float m_thr = INFINITY, m_small = INFINITY, m_iou = INFINITY, m_ord = INFINITY, m_cap = INFINITY;
    // A wavefront scans 64 anchors, one per lane; the few that have something to compare (above the threshold or inside its window, not
    // small) are then taken one at a time by the WHOLE wavefront, 64 kept boxes per step -- a lane walking its own anchor's kept list
    // would leave the other 63 idle.  Everything below is a min or a max: the order the lanes contribute in does not show.
    const int lane = tid & 63;
    const float cover = a.nms_thr + 0.01f;
    for (int i0 = (tid >> 6) * 64; i0 < total; i0 += 256) {
        const int i = i0 + lane;
        float s = 0.0f, d = 0.0f; float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f); int what = 0;      // 1: above the threshold, 2: in the window
        if (i < total) {
            s = retina_score(a, v, i, k);
            d = fabsf(s - a.score_thr);
            what = (s > a.score_thr ? 1 : 0) | (d < 1e-3f ? 2 : 0);
            if (what) {
                b = retina_decode(a, v, i, Wr, Hr);
                const float w = b.z - b.x, h = b.w - b.y;
                if (what & 1) m_small = fminf(m_small, fminf(fabsf(w - a.min_box), fabsf(h - a.min_box)));
                if (!(w >= a.min_box && h >= a.min_box)) what = 0;                                  // a small box takes no part in anything else
            }
        }
        unsigned long long todo = __ballot(what != 0);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int hi = i0 + src, hw = __shfl(what, src, 64);
            const float hs = __shfl(s, src, 64), hd = __shfl(d, src, 64);
            const float4 hb = make_float4(__shfl(b.x, src, 64), __shfl(b.y, src, 64), __shfl(b.z, src, 64), __shfl(b.w, src, 64));
            const bool behind = (hw & 1) && full && (s_last > hs || (s_last == hs && a_last < hi));     // behind the class's cut
            const bool thr = (hw & 2) && !full, nms = (hw & 1) && !behind;
            if (behind) m_cap = fminf(m_cap, s_last - hs);
            if (!thr && !nms) continue;
            bool covered = false; float mx = 0.0f;
            for (int j = lane; j < nk; j += 64) {
                const float iou = nms_iou(kb[j], hb);
                if (thr && ka[j] != hi && iou > cover) covered = true;
                if (nms && (ks[j] > hs || (ks[j] == hs && ka[j] < hi))) {                              // kept entry j precedes the candidate
                    if (iou > mx) mx = iou;
                    if (iou > a.nms_thr) m_ord = fminf(m_ord, ks[j] - hs);
                }
            }
            if (thr && __ballot(covered) == 0ull) m_thr = fminf(m_thr, hd);
            if (nms) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
                m_iou = fminf(m_iou, fabsf(mx - a.nms_thr));
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        m_thr = fminf(m_thr, __shfl_xor(m_thr, o, 64)); m_small = fminf(m_small, __shfl_xor(m_small, o, 64)); m_iou = fminf(m_iou, __shfl_xor(m_iou, o, 64));
        m_ord = fminf(m_ord, __shfl_xor(m_ord, o, 64)); m_cap = fminf(m_cap, __shfl_xor(m_cap, o, 64));
    }
    if (lane == 0) {
        if (m_thr < INFINITY) upd(out + VM_POST_THR, m_thr);
        if (m_small < INFINITY) upd(out + VM_POST_SMALL, m_small);
        if (m_iou < INFINITY) upd(out + VM_POST_IOU, m_iou);
        if (m_ord < INFINITY) upd(out + VM_POST_ORDER, m_ord);
        if (m_cap < INFINITY) upd(out + VM_POST_CAP, m_cap);
    }
    if (tid == 0 && nk >= 2) {
        bool first = true;
        for (int q = 0; q < k && first; q++) first = retina_kept(a, (long long)v * a.K + q) == 0;
        if (first) upd(out + VM_POST_TOP2, ks[0] - ks[1]);
    }
}
// VM_POST_SUBORDER of a RetinaNet view: grid V, one wavefront.  Were this a reference view with more than 40 detections,
// np.round(np.linspace(0, n - 1, 50)) picks 50 rows of its list; inside a class the rows are in score order, so a neighbour pair of one class
// of which exactly one is picked swaps at a score tie.  Across a class boundary the order is fixed by the class index: no record.
__global__ __launch_bounds__(64) void audit_retina_suborder_kernel(RetinaArgs a, float* vm) {
    __shared__ int pk[50];
    const int v = blockIdx.x, t = threadIdx.x, K = a.K;
    int n = 0;
    for (int q = 0; q < K; q++) n += retina_kept(a, (long long)v * K + q);
    if (n <= 40) return;
    const double step = (double)(n - 1) / 49.0;
    if (t < 50) pk[t] = t == 49 ? n - 1 : (int)nearbyint((double)t * step);
    __syncthreads();
    float m = INFINITY;
    if (t < 50) {
        const int r = pk[t];
        for (int d = -1; d <= 1; d += 2) {
            const int nb = r + d;
            if (nb < 0 || nb >= n) continue;
            bool picked = false;
            for (int u = 0; u < 50; u++) picked |= pk[u] == nb;
            if (picked) continue;
            const int lo = d < 0 ? nb : r;                      // rows lo, lo + 1
            int q = 0, off = 0, cnt = retina_kept(a, (long long)v * K);
            while (lo >= off + cnt && q + 1 < K) { off += cnt; q++; cnt = retina_kept(a, (long long)v * K + q); }
            if (lo + 1 >= off + cnt) continue;                  // the pair straddles a class boundary
            const int* an = a.kept_anchor + ((long long)v * K + q) * a.per_class + (lo - off);
            m = fminf(m, retina_score(a, v, an[0], q) - retina_score(a, v, an[1], q));
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    if (t == 0 && m < INFINITY) upd(vm + (long long)v * CALD_VM + VM_POST_SUBORDER, m);
}
}   // namespace

void launch_audit_retina(const RetinaArgs& a, float* out, hipStream_t st) {      // callers guarantee per_class <= AUDIT_MAX_DET; after launch_retina_postprocess
    const int n = a.V * CALD_VM;
    hipLaunchKernelGGL(audit_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out, n);
    hipLaunchKernelGGL(audit_retina_kernel, dim3(a.K, a.V), dim3(256), 0, st, a, out);
    hipLaunchKernelGGL(audit_retina_suborder_kernel, dim3(a.V), dim3(64), 0, st, a, out);
}

void launch_audit(const AuditArgs& a, hipStream_t st) {      // callers guarantee pre_n <= 1024 and det cap <= AUDIT_MAX_DET
    const int n = a.V * CALD_VM;
    hipLaunchKernelGGL(audit_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a.out, n);
    hipLaunchKernelGGL(audit_rpn_kernel, dim3(5, a.V), dim3(256), 0, st, a);
    hipLaunchKernelGGL(audit_roi_kernel, dim3(a.V), dim3(256), 0, st, a);
    hipLaunchKernelGGL(audit_post_kernel, dim3(a.V), dim3(256), 0, st, a);
}
