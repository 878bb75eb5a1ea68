// train_targets.hip -- from the heads' outputs to what the losses read: region proposals in training mode (torchvision
// RegionProposalNetwork.filter_proposals with pre/post_nms_top_n_train = 2000, detection/frcnn_la.py:154-158: the inference kernels of
// rpn.hip at the larger capacity), the RoI sampler on the host (roi_heads.select_training_samples), Matcher, AnchorGenerator, BoxCoder.encode
// (torchvision 0.8.2 _utils.py) and the gather that follows the sampler on the device.
#include "train_host.h"
#include <algorithm>

// heads[l]: [N][Hl][Wl][head_ld], channel a = objectness logit of anchor a, channel A + 4a + j = delta j.  image_sizes: host [N][2]
// (resized, unpadded h, w).  proposals_out: device [N][post_n][4], counts_out: device int [N].
extern "C" int cald_train_rpn_proposals(cald_ctx* c, int N, int Hp, int Wp, const int* image_sizes, const float* const* heads,
                                        const int* level_hw, int head_ld, int pre_n, int post_n, float nms_thr, float min_size,
                                        float* proposals_out, int* counts_out) {
    if (!c || !image_sizes || !heads || !level_hw || !proposals_out || !counts_out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (N < 1 || N > CALD_MAX_VIEWS || pre_n < 1 || pre_n > 2048 || post_n < 1 || post_n > 2048) TFAIL(CALD_ERR_INVALID, "N <= %d, pre/post top-n <= 2048", CALD_MAX_VIEWS);
    THIP(hipSetDevice(cald_internal_device(c)));
    SEG_ENTRY();
    hipStream_t st = cald_internal_stream(c);
    RpnArgs ra; memset(&ra, 0, sizeof(ra));
    const LevelSeg* s0;
    if (int rc = dense_seg(c, N, Hp, Wp, &s0)) return rc;
    ra.seg0 = s0;
    for (int l = 0; l < 5; l++) {
        const LevelSeg* sl;
        if (int rc = dense_seg(c, N, level_hw[2 * l], level_hw[2 * l + 1], &sl)) return rc;
        ra.seg[l] = sl; ra.head[l] = heads[l];
    }
    const size_t ntot = (size_t)N * 5 * pre_n;
    const size_t b_views = (sizeof(ViewDesc) * N + 255) & ~(size_t)255, b_anch = 256, b_key = (ntot * 8 + 255) & ~(size_t)255, b_box = (ntot * 16 + 255) & ~(size_t)255;
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, b_views + b_anch + b_key + 3 * b_box + 256, &scratch)) return rc;
    char* p = (char*)scratch;
    ViewDesc* d_views = (ViewDesc*)p; p += b_views;
    float* d_base = (float*)p; p += b_anch;
    ra.cand_key = (unsigned long long*)p; p += b_key;
    ra.cand_box = (float*)p; p += b_box; ra.sorted_box = (float*)p; p += b_box; ra.sorted_raw = (float*)p; p += b_box;
    ra.sorted_count = (int*)p;
    std::vector<ViewDesc> hv(N);
    memset(hv.data(), 0, sizeof(ViewDesc) * N);
    for (int v = 0; v < N; v++) { hv[v].Hr = image_sizes[2 * v]; hv[v].Wr = image_sizes[2 * v + 1]; }
    float base[5 * 3 * 4];
    base_anchors_host(0, base);
    // the two host tables go through the pinned staging ring (one blob: base anchors, then the view descriptors), so the call returns with
    // the proposal kernels enqueued instead of first waiting for everything before them on the stream (the whole body + FPN + RPN head)
    std::vector<char> blob(256 + sizeof(ViewDesc) * N);
    memcpy(blob.data(), base, sizeof(base)); memcpy(blob.data() + 256, hv.data(), sizeof(ViewDesc) * N);
    const bool ring = blob.size() <= kStageSlot;
    const void* dv = nullptr; int slot = 0;
    if (ring) {
        if (int rc = stage_upload(c, blob.data(), blob.size(), st, &dv, &slot)) return rc;
        d_base = (float*)dv; d_views = (ViewDesc*)((const char*)dv + 256);
    } else {
        THIP(hipMemcpyAsync(d_views, hv.data(), sizeof(ViewDesc) * N, hipMemcpyHostToDevice, st));
        THIP(hipMemcpyAsync(d_base, base, sizeof(base), hipMemcpyHostToDevice, st));
        THIP(hipStreamSynchronize(st));   // the host arrays above are stack / vector storage
    }
    ra.views = d_views; ra.base_anchors = d_base; ra.head_ld = head_ld; ra.A = 3; ra.V = N; ra.pre_n = pre_n; ra.post_n = post_n;
    ra.nms_thr = nms_thr; ra.min_size = min_size; ra.proposals = proposals_out; ra.prop_stride = post_n; ra.prop_count = counts_out;
    launch_rpn(ra, st);
    THIP(hipGetLastError());
    if (ring) return stage_consumed(c, slot, st);
    return 0;
}

// RoI sampling on the host (roi_heads.select_training_samples: labels from the match results, BalancedPositiveNegativeSampler, the
// index lists the loss kernels read) for all images of a batch in one call.  The forward pass stops for this -- the GPU waits while
// the host turns match results into sample indices -- and the numpy version of the loop cost 0.6 ms per step.
// Candidate table of image i: `slots[i]` proposal rows (the first counts[i] are used) followed by n_gt[i] ground-truth rows; images
// back to back.  The sampler keeps the k candidates with the smallest keys of each class (keys: iid uniform draws handed in by the
// caller, one per table row: every k-subset is equally likely -- what randperm(n)[:k] selects).
extern "C" int cald_train_roi_sample_host(int N, const int* slots, const int* n_gt, const int* counts, const int32_t* matched,
                                          const int64_t* gt_labels, const double* keys, int batch, double pos_fraction, int pred_ld, int num_classes,
                                          int64_t* keep_rows, int64_t* gt_sel, int64_t* labels_out, float* img_col, int64_t* pos_rows,
                                          int64_t* pred_idx, int* R_out, int* n_pos_out, int* per_image_out) {
    if (N < 1 || !slots || !n_gt || !matched || !keys || !keep_rows || !gt_sel || !labels_out || !img_col || !pos_rows || !pred_idx || !R_out || !n_pos_out)
        TFAIL(CALD_ERR_INVALID, "null argument");
    if (batch < 1 || pos_fraction < 0.0 || pos_fraction > 1.0) TFAIL(CALD_ERR_INVALID, "bad sampler parameters");
    long long row0 = 0, g0 = 0, gtot = 0;
    for (int i = 0; i < N; i++) gtot += n_gt[i];
    int R = 0, npos_all = 0;
    std::vector<std::pair<double, int>> pos, neg;
    std::vector<int> kept;
    std::vector<int64_t> lab;
    for (int i = 0; i < N; i++) {
        const int used = counts ? counts[i] : slots[i];
        if (used < 0 || used > slots[i] || n_gt[i] < 0) TFAIL(CALD_ERR_INVALID, "image %d: bad counts", i);
        const int rows = slots[i] + n_gt[i];
        pos.clear(); neg.clear(); lab.assign(rows, -1);
        for (int r = 0; r < rows; r++) {
            if (r >= used && r < slots[i]) continue;                       // an unused proposal slot: not a candidate
            const int m = matched[row0 + r];
            int64_t l;
            if (n_gt[i] == 0) l = 0;
            else if (m >= 0) { if (m >= n_gt[i]) TFAIL(CALD_ERR_INVALID, "image %d: match index out of range", i); l = gt_labels ? gt_labels[g0 + m] : 1; }
            else l = m == -1 ? 0 : -1;                                     // below the low threshold: background; between thresholds: ignored
            lab[r] = l;
            if (l >= 1) pos.emplace_back(keys[row0 + r], r); else if (l == 0) neg.emplace_back(keys[row0 + r], r);
        }
        int num_pos = (int)(batch * pos_fraction); if (num_pos > (int)pos.size()) num_pos = (int)pos.size();
        int num_neg = batch - num_pos; if (num_neg > (int)neg.size()) num_neg = (int)neg.size();
        if (num_pos < (int)pos.size()) std::nth_element(pos.begin(), pos.begin() + num_pos, pos.end());
        if (num_neg < (int)neg.size()) std::nth_element(neg.begin(), neg.begin() + num_neg, neg.end());
        kept.clear();
        for (int k = 0; k < num_pos; k++) kept.push_back(pos[k].second);
        for (int k = 0; k < num_neg; k++) kept.push_back(neg[k].second);
        std::sort(kept.begin(), kept.end());
        for (int r : kept) {
            const int m = matched[row0 + r];
            keep_rows[R] = row0 + r; labels_out[R] = lab[r]; img_col[R] = (float)i;
            gt_sel[R] = n_gt[i] ? g0 + (m > 0 ? m : 0) : gtot;           // images without ground truth point at the extra all-zero box
            if (lab[r] > 0) { pos_rows[npos_all] = R; pred_idx[npos_all] = (int64_t)R * pred_ld + num_classes + 4 * lab[r]; npos_all++; }
            R++;
        }
        if (per_image_out) per_image_out[i] = (int)kept.size();
        row0 += rows; g0 += n_gt[i];
    }
    *R_out = R; *n_pos_out = npos_all;
    return 0;
}

// Matcher (torchvision 0.8.2 _utils.Matcher): IoU of every candidate box with every ground-truth box, best ground truth per
// candidate, thresholds, optional low-quality matches.  out[i] = ground-truth index, -1 below `lo`, -2 between `lo` and `hi`.
__device__ inline float box_iou_tv(const float4 a, const float4 b) {   // torchvision.ops.box_iou
    const float aa = (a.z - a.x) * (a.w - a.y), ab = (b.z - b.x) * (b.w - b.y);
    float w = fminf(a.z, b.z) - fmaxf(a.x, b.x), h = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    w = w < 0.0f ? 0.0f : w; h = h < 0.0f ? 0.0f : h;
    const float inter = w * h;
    return inter / ((aa + ab) - inter);
}
__global__ void match_gtmax_kernel(const float4* boxes, int nB, const float4* gt, int nG, unsigned* gtmax_bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nB) return;
    const float4 b = boxes[i];
    for (int g = 0; g < nG; g++) {
        const float v = box_iou_tv(gt[g], b);
        if (v > 0.0f) atomicMax(&gtmax_bits[g], __float_as_uint(v));   // IoU >= 0: the bit pattern orders like the value
    }
}
__global__ void match_assign_kernel(const float4* boxes, int nB, const float4* gt, int nG, const unsigned* gtmax_bits, float hi, float lo,
                                    int allow_low, int* out, float* best_iou) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nB) return;
    const float4 b = boxes[i];
    float best = -1.0f; int arg = 0; bool low = false;
    for (int g = 0; g < nG; g++) {
        const float v = box_iou_tv(gt[g], b);
        if (v > best) { best = v; arg = g; }                         // first maximum, as torch.max(dim=0)
        if (allow_low && v == __uint_as_float(gtmax_bits[g])) low = true;
    }
    int m = arg;
    if (best < lo) m = -1; else if (best < hi) m = -2;
    if (low) m = arg;
    out[i] = m;
    if (best_iou) best_iou[i] = best;
}
extern "C" int cald_train_match(cald_ctx* c, int n_boxes, const float* boxes, int n_gt, const float* gt, float hi, float lo,
                                int allow_low_quality, int* matched_out, float* best_iou_out) {
    if (!c || !boxes || !gt || !matched_out) TFAIL(CALD_ERR_INVALID, "null argument");
    if (n_boxes < 1 || n_gt < 1) TFAIL(CALD_ERR_INVALID, "needs at least one box and one ground-truth box");
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, (size_t)n_gt * 4 + 256, &scratch)) return rc;
    unsigned* gm = (unsigned*)scratch;
    THIP(hipMemsetAsync(gm, 0, (size_t)n_gt * 4, st));
    const int blocks = (n_boxes + 255) / 256;
    if (allow_low_quality)
        hipLaunchKernelGGL(match_gtmax_kernel, dim3(blocks), dim3(256), 0, st, (const float4*)boxes, n_boxes, (const float4*)gt, n_gt, gm);
    hipLaunchKernelGGL(match_assign_kernel, dim3(blocks), dim3(256), 0, st, (const float4*)boxes, n_boxes, (const float4*)gt, n_gt, gm, hi, lo,
                       allow_low_quality, matched_out, best_iou_out);
    THIP(hipGetLastError());
    return 0;
}

// all anchors of one image, in torchvision's order (level, y, x, anchor): [sum_l Hl*Wl*A][4]
__global__ void anchors_kernel(float4* out, int Hl, int Wl, int sy, int sx, const float* base, int A, long long off) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)Hl * Wl * A) return;
    const int an = (int)(i % A); const long long pix = i / A;
    const int x = (int)(pix % Wl), y = (int)(pix / Wl);
    out[off + i] = make_float4((float)(x * sx) + base[an * 4], (float)(y * sy) + base[an * 4 + 1], (float)(x * sx) + base[an * 4 + 2], (float)(y * sy) + base[an * 4 + 3]);
}
// kind 0: Faster R-CNN AnchorGenerator, sizes (32, 64, 128, 256, 512) x ratios (0.5, 1, 2), A = 3 (frcnn_la.py:185-187)
// kind 1: RetinaNet, sizes (x, int(x 2^(1/3)), int(x 2^(2/3))) for x in the same five, A = 9, index = ratio * 3 + size (retinanet_cal.py:346-351)
int cald_train_host::base_anchors_host(int kind, float* base) {
    const float ratios[3] = {0.5f, 1.0f, 2.0f};
    for (int l = 0; l < 5; l++) {
        const int x = 32 << l;
        const float sizes[3] = {(float)x, (float)(int)((double)x * pow(2.0, 1.0 / 3)), (float)(int)((double)x * pow(2.0, 2.0 / 3))};
        const int ns = kind == 1 ? 3 : 1;
        for (int r = 0; r < 3; r++) {
            const float hr = sqrtf(ratios[r]), wr = 1.0f / hr;
            for (int si = 0; si < ns; si++) {
                const float ws = wr * sizes[si], hs = hr * sizes[si];
                float* b = &base[((l * 3 + r) * ns + si) * 4];
                b[0] = rintf(-ws / 2.0f); b[1] = rintf(-hs / 2.0f); b[2] = rintf(ws / 2.0f); b[3] = rintf(hs / 2.0f);
            }
        }
    }
    return kind == 1 ? 9 : 3;
}
extern "C" int cald_train_anchors(cald_ctx* c, int kind, int Hp, int Wp, const int* level_hw, float* anchors_out) {
    if (!c || !level_hw || !anchors_out || kind < 0 || kind > 1) TFAIL(CALD_ERR_INVALID, "bad arguments");
    THIP(hipSetDevice(cald_internal_device(c)));
    hipStream_t st = cald_internal_stream(c);
    float base[5 * 9 * 4];
    const int A = base_anchors_host(kind, base);
    void* scratch = nullptr;
    if (int rc = cald_internal_scratch(c, sizeof(base), &scratch)) return rc;
    THIP(hipMemcpyAsync(scratch, base, sizeof(base), hipMemcpyHostToDevice, st));
    THIP(hipStreamSynchronize(st));
    long long off = 0;
    for (int l = 0; l < 5; l++) {
        const int Hl = level_hw[2 * l], Wl = level_hw[2 * l + 1];
        const long long n = (long long)Hl * Wl * A;
        hipLaunchKernelGGL(anchors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (float4*)anchors_out, Hl, Wl, Hp / Hl, Wp / Wl,
                           (const float*)scratch + l * A * 4, A, off);
        off += n;
    }
    THIP(hipGetLastError());
    THIP(hipStreamSynchronize(st));   // the scratch holding the base anchors may be reused by the next call
    return 0;
}

// BoxCoder.encode_single (torchvision 0.8.2 _utils.py): regression targets of `proposals` towards `reference` boxes
__device__ __forceinline__ float4 box_encode_one(const float4 r, const float4 p, float wx, float wy, float ww, float wh) {
    const float ex_w = p.z - p.x, ex_h = p.w - p.y, ex_cx = p.x + 0.5f * ex_w, ex_cy = p.y + 0.5f * ex_h;
    const float gt_w = r.z - r.x, gt_h = r.w - r.y, gt_cx = r.x + 0.5f * gt_w, gt_cy = r.y + 0.5f * gt_h;
    return make_float4(wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * det_logf(gt_w / ex_w), wh * det_logf(gt_h / ex_h));
}
__global__ void box_encode_kernel(const float4* reference, const float4* proposals, int n, float wx, float wy, float ww, float wh, float4* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = box_encode_one(reference[i], proposals[i], wx, wy, ww, wh);
}
// What follows the RoI sampler on the device, in one launch: the sampled boxes gathered into RoIAlign's [R][5] rows (image index, box)
// and the regression targets of the foreground rows.  idx: the sampler's int64 block with stride `cap` between its lists
// (cald_train_roi_sample_host's outputs uploaded as they are: table rows | ground-truth rows | labels | pred_idx | pos_rows | image
// index as float32 in the first 4 * R bytes of the sixth list).
__global__ void roi_gather_kernel(const float4* __restrict__ table, const float4* __restrict__ gts, const long long* __restrict__ idx, int cap, int R, int n_pos,
                                  float wx, float wy, float ww, float wh, float* __restrict__ rois, float4* __restrict__ box_tgt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < R) {
        const float4 b = table[idx[i]];
        float* o = rois + (long long)i * 5;
        o[0] = reinterpret_cast<const float*>(idx + 5ll * cap)[i]; o[1] = b.x; o[2] = b.y; o[3] = b.z; o[4] = b.w;
    }
    if (i < n_pos) {
        const long long r = idx[4ll * cap + i];
        box_tgt[i] = box_encode_one(gts[idx[(long long)cap + r]], table[idx[r]], wx, wy, ww, wh);
    }
}
extern "C" int cald_train_roi_gather(cald_ctx* c, const float* table, const float* gts, const int64_t* idx, int cap, int R, int n_pos,
                                     float wx, float wy, float ww, float wh, float* rois_out, float* box_tgt_out) {
    if (!c || !table || !gts || !idx || !rois_out || (n_pos > 0 && !box_tgt_out)) TFAIL(CALD_ERR_INVALID, "null argument");
    if (R < 0 || n_pos < 0 || n_pos > R || R > cap) TFAIL(CALD_ERR_INVALID, "0 <= n_pos <= R <= cap");
    THIP(hipSetDevice(cald_internal_device(c)));
    if (R > 0) hipLaunchKernelGGL(roi_gather_kernel, dim3((R + 255) / 256), dim3(256), 0, cald_internal_stream(c), (const float4*)table, (const float4*)gts,
                                  (const long long*)idx, cap, R, n_pos, wx, wy, ww, wh, rois_out, (float4*)box_tgt_out);
    THIP(hipGetLastError());
    return 0;
}
extern "C" int cald_train_box_encode(cald_ctx* c, int n, const float* reference, const float* proposals, float wx, float wy, float ww, float wh,
                                     float* out) {
    if (!c || (n > 0 && (!reference || !proposals || !out))) TFAIL(CALD_ERR_INVALID, "null argument");
    THIP(hipSetDevice(cald_internal_device(c)));
    if (n > 0) hipLaunchKernelGGL(box_encode_kernel, dim3((n + 255) / 256), dim3(256), 0, cald_internal_stream(c), (const float4*)reference,
                                  (const float4*)proposals, n, wx, wy, ww, wh, (float4*)out);
    THIP(hipGetLastError());
    return 0;
}
