// eval.hip -- cald_op_coco_match / cald_op_voc_match: the detection-to-ground-truth matching of the two AP evaluators on the device.
// Both kernels restate host code of this package (cald_amd/coco_eval.py COCOeval.evaluate_img + bbox_iou; cald_amd/voc_eval.py
// best_overlaps + mark_detections) in IEEE double, every expression in the host's operation order; with -ffp-contract=off no product is
// fused into a sum, so every comparison falls as it does in numpy and the integer-valued outputs are equal, not close.
//
// Shape of both kernels: one 64-lane wavefront (= one workgroup) per segment, one lane per variant of the greedy loop -- (area range,
// IoU threshold) for COCO, IoU threshold for VOC.  The loop over the segment's detections and ground truths is sequential in every lane
// and uniform across the wavefront (all lanes look at the same pair at the same time, so the boxes come in as wave-uniform loads and the
// overlap is computed once per pair); what differs per lane is only which ground truths are ignored, the threshold and the matched flags.
// The flags are bit words in LDS, one column per lane; no lane reads another lane's column, so the kernels need no barrier, no atomics,
// and a lane without a variant simply leaves.  Every loop is bounded by the segment's own counts, which the host has checked against
// CALD_EVAL_MAX_DT / CALD_EVAL_MAX_GT before anything is uploaded.
//
// evaluate_img visits the ground truths sorted stably by their ignore flag and breaks at the first ignored one once a regular match
// exists.  So the regular group and the ignored group never compete: the ignored group is looked at only while no regular ground truth
// has passed, and then still against the untouched threshold.  The kernel therefore walks the ground truths ONCE in their original order
// with one (best IoU, index) pair per group and takes the regular pair if it holds a match, else the ignored one -- the same result as
// the two-pass walk, pair for pair (`ious < iou` skips, so an equal IoU replaces the earlier ground truth in either statement).
#include "host.h"

namespace {
const int EVAL_GT_WORDS = CALD_EVAL_MAX_GT / 32;

// np.minimum / np.maximum: a NaN operand is the result (fmin / fmax would drop it)
__device__ __forceinline__ double np_min(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

__global__ __launch_bounds__(64) void coco_match_kernel(const long long* __restrict__ dt_off, const long long* __restrict__ gt_off,
                                                        const double* __restrict__ dt_box, const double* __restrict__ dt_area,
                                                        const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                        const uint8_t* __restrict__ gt_crowd, const uint8_t* __restrict__ gt_ign,
                                                        int T, const double* __restrict__ thrs, int A, const double* __restrict__ rng,
                                                        long long D_total, long long G_total,
                                                        int* __restrict__ dt_match, uint8_t* __restrict__ dt_ignore, uint8_t* __restrict__ gt_ignore) {
    __shared__ uint32_t s_matched[EVAL_GT_WORDS][64];
    const int seg = blockIdx.x, lane = threadIdx.x;
    const long long d0 = dt_off[seg], g0 = gt_off[seg];
    const int D = (int)(dt_off[seg + 1] - d0), G = (int)(gt_off[seg + 1] - g0);
    // gtIgnore of every area range: ignore, or the ANNOTATION area outside [a0, a1]
    for (int aa = 0; aa < A; aa++) {
        const double r0 = rng[2 * aa], r1 = rng[2 * aa + 1];
        for (int g = lane; g < G; g += 64) {
            const double ar = gt_area[g0 + g];
            gt_ignore[(long long)aa * G_total + g0 + g] = (gt_ign[g0 + g] || ar < r0 || ar > r1) ? 1 : 0;
        }
    }
    if (lane >= A * T) return;                                // no barrier below: a lane without a variant is done
    const int a = lane / T, t = lane - a * T;
    const double a0 = rng[2 * a], a1 = rng[2 * a + 1];
    const double cap = 1 - 1e-10;
    const double thr = cap < thrs[t] ? cap : thrs[t];         // min(t, 1 - 1e-10)
    for (int w = 0; w < (G + 31) >> 5; w++) s_matched[w][lane] = 0u;
    const long long out0 = (long long)lane * D_total + d0;     // lane == a * T + t
    for (int d = 0; d < D; d++) {
        const double dx = dt_box[(d0 + d) * 4 + 0], dy = dt_box[(d0 + d) * 4 + 1], dw = dt_box[(d0 + d) * 4 + 2], dh = dt_box[(d0 + d) * 4 + 3];
        const double da = dw * dh;
        double iou_r = thr, iou_i = thr;
        int m_r = -1, m_i = -1;
        for (int g = 0; g < G; g++) {
            const double gx = gt_box[(g0 + g) * 4 + 0], gy = gt_box[(g0 + g) * 4 + 1], gw = gt_box[(g0 + g) * 4 + 2], gh = gt_box[(g0 + g) * 4 + 3];
            const bool crowd = gt_crowd[g0 + g] != 0;
            const double w = np_min(dx + dw, gx + gw) - np_max(dx, gx);
            const double h = np_min(dy + dh, gy + gh) - np_max(dy, gy);
            const double inter = (w > 0 && h > 0) ? w * h : 0.0;
            const double ga = gw * gh;
            const double uni = crowd ? da + 0 * ga : (da + ga) - inter;
            const double v = inter > 0 ? inter / uni : 0.0;
            const double ar = gt_area[g0 + g];
            const bool ign = gt_ign[g0 + g] || ar < a0 || ar > a1;
            const bool taken = (s_matched[g >> 5][lane] >> (g & 31)) & 1u;
            if (taken && !crowd) continue;                    // already matched, and not a crowd
            if (ign) {
                if (v < iou_i) continue;
                iou_i = v; m_i = g;
            } else {
                if (v < iou_r) continue;
                iou_r = v; m_r = g;
            }
        }
        const int m = m_r >= 0 ? m_r : m_i;
        const double ar = dt_area[d0 + d];
        dt_match[out0 + d] = m;
        dt_ignore[out0 + d] = m >= 0 ? (m_r >= 0 ? 0 : 1) : ((ar < a0 || ar > a1) ? 1 : 0);
        if (m >= 0) s_matched[m >> 5][lane] |= 1u << (m & 31);
    }
}

__global__ __launch_bounds__(64) void voc_match_kernel(const long long* __restrict__ dt_off, const long long* __restrict__ gt_off,
                                                       const double* __restrict__ gt_box, const uint8_t* __restrict__ gt_difficult,
                                                       const double* __restrict__ dt_box, const long long* __restrict__ dt_index,
                                                       int T, const double* __restrict__ thrs, long long nd,
                                                       double* __restrict__ ovmax, long long* __restrict__ jmax,
                                                       uint8_t* __restrict__ tp, uint8_t* __restrict__ fp) {
    __shared__ uint32_t s_claimed[EVAL_GT_WORDS][64];
    const int seg = blockIdx.x, lane = threadIdx.x;
    if (lane >= T) return;                                    // no barrier below
    const long long d0 = dt_off[seg], g0 = gt_off[seg];
    const int D = (int)(dt_off[seg + 1] - d0), G = (int)(gt_off[seg + 1] - g0);
    const double thr = thrs[lane];
    for (int w = 0; w < (G + 31) >> 5; w++) s_claimed[w][lane] = 0u;
    for (int d = 0; d < D; d++) {
        const double b0 = dt_box[(d0 + d) * 4 + 0], b1 = dt_box[(d0 + d) * 4 + 1], b2 = dt_box[(d0 + d) * 4 + 2], b3 = dt_box[(d0 + d) * 4 + 3];
        const long long idx = dt_index[d0 + d];
        double best = -INFINITY;                              // no box of the class in the image
        int j = 0;
        for (int g = 0; g < G; g++) {
            const double x0 = gt_box[(g0 + g) * 4 + 0], y0 = gt_box[(g0 + g) * 4 + 1], x1 = gt_box[(g0 + g) * 4 + 2], y1 = gt_box[(g0 + g) * 4 + 3];
            const double iw = np_max((np_min(x1, b2) - np_max(x0, b0)) + 1., 0.);
            const double ih = np_max((np_min(y1, b3) - np_max(y0, b1)) + 1., 0.);
            const double inters = iw * ih;
            const double uni = (((b2 - b0) + 1.) * ((b3 - b1) + 1.) + ((x1 - x0) + 1.) * ((y1 - y0) + 1.)) - inters;
            const double ov = inters / uni;
            // np.max / np.argmax: the FIRST maximum; a NaN, once met, is the maximum
            if (g == 0 || (!(best != best) && (ov > best || ov != ov))) { best = ov; j = g; }
        }
        if (lane == 0) { ovmax[idx] = best; jmax[idx] = j; }
        uint8_t vtp = 0, vfp = 0;
        if (best > thr) {                                     // strict: an overlap equal to the threshold is no match
            if (!gt_difficult[g0 + j]) {
                const uint32_t bit = 1u << (j & 31);
                if (!(s_claimed[j >> 5][lane] & bit)) { vtp = 1; s_claimed[j >> 5][lane] |= bit; }
                else vfp = 1;
            }
        } else vfp = 1;
        tp[(long long)lane * nd + idx] = vtp;
        fp[(long long)lane * nd + idx] = vfp;
    }
}

// offsets of n_seg segments: [n_seg + 1], from 0, non-decreasing, no segment above `cap`
int check_offsets(const char* fn, const char* what, int n_seg, const int64_t* off, int cap) {
    if (off[0] != 0) return fail(CALD_ERR_INVALID, "%s: %s offsets must start at 0", fn, what);
    for (int s = 0; s < n_seg; s++) {
        if (off[s + 1] < off[s]) return fail(CALD_ERR_INVALID, "%s: %s offsets decrease at segment %d", fn, what, s);
        if (off[s + 1] - off[s] > cap)
            return fail(CALD_ERR_UNSUPPORTED, "%s: segment %d has %lld %s, the kernel takes %d", fn, s, (long long)(off[s + 1] - off[s]), what, cap);
    }
    return 0;
}

template <typename T> int put(ScopedDev& sd, T** out, const T* h, size_t count) {
    if (int rc = sd.alloc(out, count * sizeof(T))) return rc;
    if (count) HIPCHK(hipMemcpy((void*)*out, h, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
}  // namespace

extern "C" int cald_op_coco_match(cald_ctx* c, int n_seg, const int64_t* dt_off, const int64_t* gt_off,
                                  const double* dt_box, const double* dt_area,
                                  const double* gt_box, const double* gt_area, const uint8_t* gt_iscrowd, const uint8_t* gt_ignore_in,
                                  int T, const double* iou_thrs, int A, const double* area_rng,
                                  int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore) {
    const char* fn = "cald_op_coco_match";
    if (!c || n_seg < 0 || !dt_off || !gt_off || !iou_thrs || !area_rng || T < 1 || A < 1) return fail(CALD_ERR_INVALID, "%s: bad arguments", fn);
    if ((long long)T * A > 64) return fail(CALD_ERR_UNSUPPORTED, "%s: T * A = %lld variants, the kernel takes 64", fn, (long long)T * A);
    int rc;
    if ((rc = check_offsets(fn, "detections", n_seg, dt_off, CALD_EVAL_MAX_DT)) || (rc = check_offsets(fn, "ground truths", n_seg, gt_off, CALD_EVAL_MAX_GT)))
        return rc;
    const int64_t Dt = dt_off[n_seg], Gt = gt_off[n_seg];
    if ((Dt && (!dt_box || !dt_area || !dt_match || !dt_ignore)) || (Gt && (!gt_box || !gt_area || !gt_iscrowd || !gt_ignore_in || !gt_ignore)))
        return fail(CALD_ERR_INVALID, "%s: null array", fn);
    if (n_seg == 0 || (Dt == 0 && Gt == 0)) return 0;
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    long long *d_dt_off, *d_gt_off; double *d_dt_box, *d_dt_area, *d_gt_box, *d_gt_area, *d_thr, *d_rng; uint8_t *d_crowd, *d_ign, *d_dtig, *d_gtig; int* d_dtm;
    if ((rc = put(sd, &d_dt_off, (const long long*)dt_off, (size_t)n_seg + 1)) || (rc = put(sd, &d_gt_off, (const long long*)gt_off, (size_t)n_seg + 1)) ||
        (rc = put(sd, &d_dt_box, dt_box, (size_t)Dt * 4)) || (rc = put(sd, &d_dt_area, dt_area, (size_t)Dt)) ||
        (rc = put(sd, &d_gt_box, gt_box, (size_t)Gt * 4)) || (rc = put(sd, &d_gt_area, gt_area, (size_t)Gt)) ||
        (rc = put(sd, &d_crowd, gt_iscrowd, (size_t)Gt)) || (rc = put(sd, &d_ign, gt_ignore_in, (size_t)Gt)) ||
        (rc = put(sd, &d_thr, iou_thrs, (size_t)T)) || (rc = put(sd, &d_rng, area_rng, (size_t)A * 2)) ||
        (rc = sd.alloc(&d_dtm, (size_t)A * T * Dt * 4)) || (rc = sd.alloc(&d_dtig, (size_t)A * T * Dt)) || (rc = sd.alloc(&d_gtig, (size_t)A * Gt)))
        return rc;
    hipLaunchKernelGGL(coco_match_kernel, dim3(n_seg), dim3(64), 0, c->stream, d_dt_off, d_gt_off, d_dt_box, d_dt_area, d_gt_box, d_gt_area, d_crowd, d_ign,
                       T, d_thr, A, d_rng, (long long)Dt, (long long)Gt, d_dtm, d_dtig, d_gtig);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    if (Dt) {
        HIPCHK(hipMemcpy(dt_match, d_dtm, (size_t)A * T * Dt * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dt_ignore, d_dtig, (size_t)A * T * Dt, hipMemcpyDeviceToHost));
    }
    if (Gt) HIPCHK(hipMemcpy(gt_ignore, d_gtig, (size_t)A * Gt, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int cald_op_voc_match(cald_ctx* c, int n_seg, const int64_t* dt_off, const int64_t* gt_off,
                                 const double* gt_box, const uint8_t* gt_difficult, const double* dt_box, const int64_t* dt_index,
                                 int T, const double* thrs, int64_t nd, double* ovmax, int64_t* jmax, uint8_t* tp, uint8_t* fp) {
    const char* fn = "cald_op_voc_match";
    if (!c || n_seg < 0 || !dt_off || !gt_off || !thrs || T < 1 || nd < 0) return fail(CALD_ERR_INVALID, "%s: bad arguments", fn);
    if (T > 64) return fail(CALD_ERR_UNSUPPORTED, "%s: T = %d thresholds, the kernel takes 64", fn, T);
    int rc;
    if ((rc = check_offsets(fn, "detections", n_seg, dt_off, CALD_EVAL_MAX_DT)) || (rc = check_offsets(fn, "ground truths", n_seg, gt_off, CALD_EVAL_MAX_GT)))
        return rc;
    const int64_t Gt = gt_off[n_seg];
    if (dt_off[n_seg] != nd) return fail(CALD_ERR_INVALID, "%s: the segments hold %lld detections, nd is %lld", fn, (long long)dt_off[n_seg], (long long)nd);
    if ((nd && (!dt_box || !dt_index || !ovmax || !jmax || !tp || !fp)) || (Gt && (!gt_box || !gt_difficult))) return fail(CALD_ERR_INVALID, "%s: null array", fn);
    if (nd == 0) return 0;
    {   // every output slot is written exactly once: dt_index is a permutation of 0 .. nd - 1
        std::vector<char> seen((size_t)nd, 0);
        for (int64_t i = 0; i < nd; i++) {
            if (dt_index[i] < 0 || dt_index[i] >= nd || seen[(size_t)dt_index[i]]) return fail(CALD_ERR_INVALID, "%s: dt_index is no permutation of 0..nd-1 (entry %lld)", fn, (long long)i);
            seen[(size_t)dt_index[i]] = 1;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    ScopedDev sd(c->stream);
    long long *d_dt_off, *d_gt_off, *d_idx, *d_jmax; double *d_gt_box, *d_dt_box, *d_thr, *d_ov; uint8_t *d_diff, *d_tp, *d_fp;
    if ((rc = put(sd, &d_dt_off, (const long long*)dt_off, (size_t)n_seg + 1)) || (rc = put(sd, &d_gt_off, (const long long*)gt_off, (size_t)n_seg + 1)) ||
        (rc = put(sd, &d_gt_box, gt_box, (size_t)Gt * 4)) || (rc = put(sd, &d_diff, gt_difficult, (size_t)Gt)) ||
        (rc = put(sd, &d_dt_box, dt_box, (size_t)nd * 4)) || (rc = put(sd, &d_idx, (const long long*)dt_index, (size_t)nd)) ||
        (rc = put(sd, &d_thr, thrs, (size_t)T)) ||
        (rc = sd.alloc(&d_ov, (size_t)nd * 8)) || (rc = sd.alloc(&d_jmax, (size_t)nd * 8)) || (rc = sd.alloc(&d_tp, (size_t)T * nd)) || (rc = sd.alloc(&d_fp, (size_t)T * nd)))
        return rc;
    hipLaunchKernelGGL(voc_match_kernel, dim3(n_seg), dim3(64), 0, c->stream, d_dt_off, d_gt_off, d_gt_box, d_diff, d_dt_box, d_idx, T, d_thr, (long long)nd,
                       d_ov, d_jmax, d_tp, d_fp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(ovmax, d_ov, (size_t)nd * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(jmax, d_jmax, (size_t)nd * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(tp, d_tp, (size_t)T * nd, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(fp, d_fp, (size_t)T * nd, hipMemcpyDeviceToHost));
    return 0;
}
