/* cald_hip.h -- C ABI of libcaldhip.so: the MI355X (gfx950) implementation of CALD's unlabeled-pool
 * consistency sweep.  Plain pointers and sizes only; no torch types cross this boundary.
 *
 * The reference (we1pingyu/CALD) has no FFI: its boundary for this path is two in-process Python
 * call signatures.  Each entry point below names the reference interface it stands behind; the
 * Python shim that binds them (cald_amd/_ffi.py, ctypes) and the stub a maintainer would add to the
 * reference are shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative code on failure; cald_last_error() gives the
 *     thread-local message (the Python shim raises RuntimeError with it).
 *   - pointers named *_dev are device (HBM) pointers on the context's GPU, everything else is host.
 *   - the caller owns and allocates all outputs; the library owns only ctx / model / workspace.
 *   - one context per device, one HIP stream per context, not thread-safe per context;
 *     one process per GPU for multi-GPU (the pool is sharded by the caller, see cald_amd/sweep.py).
 */
#ifndef CALD_HIP_H
#define CALD_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cald_ctx cald_ctx;
typedef struct cald_model cald_model;

#define CALD_OK 0
#define CALD_ERR_INVALID (-1)
#define CALD_ERR_HIP (-2)
#define CALD_ERR_STATE (-3)
#define CALD_ERR_MISSING_WEIGHT (-4)
#define CALD_ERR_UNSUPPORTED (-5)   /* input outside the supported set (e.g. a CMYK JPEG) */

/* arithmetic of the conv / linear GEMMs.
 *   FP32   exact: one k-ordered fp32 fma chain per output (v_mfma_f32_32x32x2_f32), bit-identical to the oracle.
 *   F16X3  the "fp16 MFMA path" of BASELINE.json configs[4]: operands split into fp16 hi + lo, three
 *          v_mfma_f32_32x32x16_f16 per product into fp32 accumulators (22-bit operands, ~1e-6 end to end): fp32-grade but
 *          NOT bit-identical -- ~1 % of images change through a flipped borderline detection, so the identical-top-k
 *          bar is met only by FP32; |activations| must stay below 4094. */
#define CALD_PRECISION_FP32 0
#define CALD_PRECISION_F16X3 1

#define CALD_ARCH_FRCNN 0      /* detection/frcnn_la.py FRCNN_Feature */
#define CALD_ARCH_RETINANET 1  /* detection/retinanet_cal.py RetinaNet */

const char* cald_last_error(void);
int cald_version(void);

/* stream: a hipStream_t to launch on (e.g. torch.cuda.current_stream().cuda_stream), or NULL for
 * a private stream.  Replaces torch.cuda.set_device(0) + default stream (cald_train.py:275). */
int cald_ctx_create(int device, void* stream, cald_ctx** out);
int cald_ctx_destroy(cald_ctx* ctx);
int cald_ctx_sync(cald_ctx* ctx);

/* Constructor arguments of fasterrcnn_resnet50_fpn_feature(num_classes, min_size, max_size)
 * (detection/frcnn_la.py:148-169, :278-289; call sites cald_train.py:340-347). */
typedef struct cald_model_cfg {
    int arch;               /* CALD_ARCH_* */
    int depth;              /* 50 | 101 */
    int num_classes;        /* incl. background for FRCNN */
    int min_size, max_size; /* 600/1000 VOC, 800/1333 COCO */
    float box_score_thresh; /* 0.05 */
    float box_nms_thresh;   /* 0.5 */
    int detections_per_img; /* 100 */
    int rpn_pre_nms_top_n;  /* 1000 */
    int rpn_post_nms_top_n; /* 1000 */
    float rpn_nms_thresh;   /* 0.7 */
    int precision;          /* CALD_PRECISION_* (0 = exact fp32, the default and the parity contract) */
} cald_model_cfg;

int cald_model_create(cald_ctx* ctx, const cald_model_cfg* cfg, cald_model** out);
/* model.load_state_dict() (cald_train.py:356): one call per tensor, torchvision key layout
 * ("backbone.body.layer1.0.conv1.weight", ...), float32 host data, row-major. */
int cald_model_load_tensor(cald_model* m, const char* key, const float* data, const int64_t* shape, int ndim);
/* folds FrozenBatchNorm into per-channel scale/shift, repacks weights K-major for the MFMA kernels */
int cald_model_finalize(cald_model* m);
/* Exact (CALD_PRECISION_FP32) Faster R-CNN sweeps evaluate the RPN head of P2 / P3 exactly only at the pixels that can hold one of a
 * level's rpn_pre_nms_top_n anchors, found by a split-fp16 look-ahead whose error bound is derived from a bit-exact statement of the matrix
 * instruction (oracle/mfma_f16_model.h, pinned to the hardware by the tests) and is checked at run time on every anchor evaluated both
 * ways (rpn_prune.hip): same detections bit for bit, ~1/8 less fp32 work.  A sweep whose data leave the look-ahead's
 * range (an activation of |x| >= 4094, a non-finite one) or exceed the bound is repeated with the dense head (cald_profile_prune_fallbacks
 * counts them).  On by default (environment CALD_RPN_PRUNE=0 turns it off for the process); this call switches it per model and returns
 * the previous state in *was (may be null).  cald_forward runs the dense head (unless capture mode is on, below). */
int cald_model_set_rpn_prune(cald_model* m, int on, int* was);
/* test hooks of the pruning: capture mode makes cald_forward take the pruned path too and keep the look-ahead's head maps as debug tensors
 * ("rpn_look0/1": [H][W][15], logits = channels 0..2, channels 3..14 the look-ahead's box deltas under cald_model_set_look_fuse mode 0 and zero
 * where the fused look-ahead ran, which evaluates the logits only; "rpn_pnorm0/1": the per-pixel |3 x 3 patch|_2; "rpn0/1": the maps the top-k reads, exact
 * at selected pixels and -FLT_MAX elsewhere); cald_model_rpn_prune_bound returns the constants of B_a(p) = c1[a] * pnorm(p) + c0[a], a < 3 */
int cald_model_set_rpn_prune_capture(cald_model* m, int on);
int cald_model_rpn_prune_bound(cald_model* m, float* c1, float* c0);
/* test hook, the setter twin: replaces the bound's constants from the next forward on.  This VOIDS THE CERTIFICATE -- the constants of
 * cald_model_finalize are the theorem's, any others are not -- and exists so that a test can make the sweep's ratio tripwire fire (a bound
 * scaled far below the look-ahead's error, a NaN constant).  Sweeps of a model whose bound was set this way still check and fall back, but
 * their ratio is not entered into cald_profile_prune's worst_bound_ratio, which speaks about the certified bound only. */
int cald_model_set_rpn_prune_bound(cald_model* m, const float* c1, const float* c0);
int cald_model_destroy(cald_model* m);

/* One detector input: task_model([tensor]) in cald_train.py:107 / :186.  The view is described by
 * its uint8 HWC source image in HBM plus the augmentation to apply on the fly. */
typedef struct cald_view {
    const uint8_t* image_dev; /* [H][W][3] uint8 */
    int H, W;
    int flip;                 /* cald_helper.HorizontalFlip */
    int nrect;                /* cald_helper.cutout rectangles (left, top, right, bottom), <= 4 */
    int rects[16];
    const float* noise_dev;   /* optional float32 [3][H][W] (CHW) added to image/255 before normalisation, or NULL.  With it a
                               * view carries ANY float input tensor exactly (the reference model accepts arbitrary floats,
                               * e.g. a caller-made GaussianNoise image): image = rounded uint8 grid, noise = x - image/255. */
} cald_view;

/* Result dict of the detector (detection/frcnn_la.py:131-141): device buffers, `cap` rows per view. */
typedef struct cald_dets {
    float* boxes_dev;      /* [n_views][cap][4] */
    float* scores_dev;     /* [n_views][cap] */
    int64_t* labels_dev;   /* [n_views][cap] */
    float* props_dev;      /* [n_views][cap][4] */
    float* prob_max_dev;   /* [n_views][cap] */
    float* scores_cls_dev; /* [n_views][cap][num_classes] */
    int32_t* count_dev;    /* [n_views] */
    int cap;
} cald_dets;

/* model(list_of_images) in eval mode, for up to 128 views at once (batch-1 semantics per view). */
int cald_forward(cald_model* m, int n_views, const cald_view* views, const cald_dets* out);

/* get_uncertainty(task_model, unlabeled_loader, augs, num_cls) (cald_train.py:91-231) over
 * n_images already resident in HBM.  consistency_out[n_images], cls_corr_out[n_images][num_classes-1].
 *
 * The augmented views of an image are given as an ordered list (the Python shim expands the reference's aug names
 * in the reference's order, cald_train.py:123-183).  Randomness: the reference draws GaussianNoise / SaltPepperNoise
 * from torch's global CPU generator and ColorSwap / cutout from Python's global `random`, in call order; here both
 * generators are re-seeded per image with base_seed * 1000003 + pool_pos[i] and consumed in list order, so results
 * do not depend on sharding or batching. */
#define CALD_AUG_FLIP 1          /* HorizontalFlip(image, boxes)            cald_train.py:123-126 */
#define CALD_AUG_GAUSS 2         /* GaussianNoise(image, std = param)       :127-135 ('ga' 16; 'multi_ga' 8..48) */
#define CALD_AUG_COLOR_ADJUST 3  /* ColorAdjust(image, factor = param)      :136-139 ('color_adjust' 1.5) */
#define CALD_AUG_COLOR_SWAP 4    /* ColorSwap(image)                        :140-143 */
#define CALD_AUG_SALT_PEPPER 5   /* SaltPepperNoise(image, prob = param)    :149-157 ('sp' 0.1; 'multi_sp' 0.05..0.3) */
#define CALD_AUG_CUTOUT 6        /* cutout(image, boxes, labels, cut_num = param) :158-166 ('cut_out' 2; 'multi_cut_out' 1..4) */
#define CALD_AUG_RESIZE 7        /* resize(image, boxes, ratio = param)     :167-179 ('smaller_resize' .8, 'larger_resize' 1.2, 'multi_resize' .7 .8 .9) */
#define CALD_AUG_ROTATE 8        /* rotate(image, boxes, angle = param)     :180-183 ('rotation' 5) */
#define CALD_MAX_AUGS 32
typedef struct cald_aug_spec {
    int kind;
    double param;          /* a Python float in the reference (e.g. 7 * 0.1 for multi_resize): kept in double */
} cald_aug_spec;
typedef struct cald_sweep_cfg {
    uint64_t base_seed;
    float bp;              /* args.bp, 1.3 */
    int batch_images;      /* images per batched launch sequence (0 = default 64; capped at CALD_MAX_VIEWS = 128) */
    int n_augs;
    cald_aug_spec augs[CALD_MAX_AUGS];
} cald_sweep_cfg;
int cald_sweep(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
               const int64_t* pool_pos, const cald_sweep_cfg* cfg, double* consistency_out, double* cls_corr_out);

/* ---- cascade support: cald_sweep plus a record of how close every discrete decision of the path came to flipping ----
 * get_uncertainty's result is a continuous function of the detector's GEMM outputs except at its discrete decisions (RPN top-k /
 * NMS / post-NMS cut, RoI level, score threshold, class NMS, top-100, argmax over the IoU row, the linspace sub-sample, cutout's
 * accept test; cald_train.py:110-113, :158-166, :214, detection/frcnn_la.py:72-80, detection/frcnn_ll.py:284-321).  margins_out
 * [n_images][CALD_N_MARGINS] receives, per image and per kind of decision, the smallest distance of any decision THAT CAN REACH THE
 * OUTPUT to its flip point, over all views of the image (+inf where the kind did not occur).  An image whose margins all exceed the
 * rounding noise of a faster precision took the same decisions there as in CALD_PRECISION_FP32, and its scores differ by rounding
 * only; the others are re-scored exactly (cald_amd/sweep.py get_uncertainty_cascade, cald_cascade_plan).  Both detectors: a RetinaNet
 * (detection/retinanet_cal.py:402-490: per-class threshold, remove_small_boxes, per-class NMS and cap, output in class order) leaves the RPN
 * and RoI kinds at +inf, a Faster R-CNN leaves POST_SMALL there.  CALD_ERR_UNSUPPORTED: Faster R-CNN with rpn_pre_nms_top_n > 1024, more
 * than 512 detections per image or box_min_size > 0; RetinaNet with detections_per_img (per class) > 512. */
#define CALD_N_MARGINS 16
#define CALD_MARGIN_RPN_TOPK 0       /* logit: k-th vs (k+1)-th objectness of a level's top-k cut */
#define CALD_MARGIN_RPN_IOU 1        /* IoU:   |max IoU with the kept boxes before it - rpn_nms_thresh| */
#define CALD_MARGIN_RPN_ORDER 2      /* logit: score gap of a (suppressor, suppressed) pair */
#define CALD_MARGIN_RPN_TRUNC 3      /* logit: post_nms_top_n-th vs next kept proposal */
#define CALD_MARGIN_RPN_SMALL 4      /* pixel: |w or h - 1e-3| of a clipped candidate */
#define CALD_MARGIN_ROI_LEVEL 5      /* log2:  distance of 4 + log2(sqrt(area) / 224) + 1e-6 to 3, 4 or 5 */
#define CALD_MARGIN_ROI_EDGE 6       /* feature pixel: distance of a RoIAlign sample to -1 or to the map size */
#define CALD_MARGIN_POST_THR 7       /* prob:  |class score - box_score_thresh| of a box NMS would keep */
#define CALD_MARGIN_POST_IOU 8       /* IoU:   |max IoU with kept same-class detections before it - box_nms_thresh| */
#define CALD_MARGIN_POST_ORDER 9     /* prob:  score gap of a (suppressor, suppressed) pair */
#define CALD_MARGIN_POST_CAP 10      /* prob:  detections_per_img-th detection vs the best candidate behind it */
#define CALD_MARGIN_REF_SUBSAMPLE 11 /* prob:  score gap of neighbours of which np.round(np.linspace(0, n - 1, 50)) picks one (n > 40) */
#define CALD_MARGIN_ARGMAX 12        /* IoU:   best vs best-of-another-proposal in a reference box's IoU row */
#define CALD_MARGIN_ZERO_ROW 13      /* prob:  score gap of an augmented view's first two detections when a row is all zero */
#define CALD_MARGIN_CUTOUT 14        /* ratio: |largest overlap ratio - 0.4 or 0.1| of a cutout trial */
#define CALD_MARGIN_POST_SMALL 15    /* pixel: |w or h - 1e-2| of a decoded, clipped RetinaNet candidate (remove_small_boxes) */
int cald_sweep_audit(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                     const int64_t* pool_pos, const cald_sweep_cfg* cfg, double* consistency_out, double* cls_corr_out,
                     float* margins_out);

/* ---- the baseline sweeps of the same repo that share the detector forward ---- */
/* lt_c_train.py:105-121 get_uncertainty(task_model, unlabeled_loader) -> one float per image */
int cald_sweep_ltc(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                   int batch_images, double* uncertainty_out);
/* ssm/ssm_helper.py:9-33 get_uncertainty on a Faster R-CNN model: one forward per image with the SSM tail (cald_op_ssm_postprocess) in
 * place of the ordinary one, batch_images images a forward (0 = 64; results do not depend on it).  al_out / count_out [n_images]; the rows
 * of all images consecutively in image order: boxes_out [rows][4], scores_out [rows][C - 1], labels_out [rows][C - 1].  *rows_needed_out
 * receives the total; if it exceeds rows_cap the call returns CALD_ERR_INVALID ("... needs N rows"), al_out / count_out are complete and
 * the row arrays hold nothing to rely on.  A RetinaNet model (cald_sweep_ssm_retina is its sweep) or a null argument: CALD_ERR_INVALID. */
int cald_sweep_ssm(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W, int batch_images,
                   int64_t rows_cap, int* al_out, int* count_out, float* boxes_out, float* scores_out, int8_t* labels_out,
                   int64_t* rows_needed_out);
/* ---- SSM on RetinaNet (detection/retina_ssm.py:487-584).  The reference sub-samples every class's candidates (the anchors scoring above
 * box_score_thresh, in anchor order: level P3..P7, pixel row-major, anchor) with random.shuffle on Python's global generator and keeps the
 * first 500.  The tail therefore stops once on the host: after the device has counted and listed the candidates, the library asks the
 * caller's cald_ssm_pick_fn which of them to keep, then finishes on the device. ----
 * pick(user, image, K, counts, picks, n_picks): counts[k] = candidates of class k; the callee writes n_picks[k] <= min(counts[k],
 * CALD_SSM_RETINA_TAKE) and picks[k * CALD_SSM_RETINA_TAKE + j] = the position (0 .. counts[k] - 1) of the j-th kept candidate, in the order
 * the reference's list would have (an earlier pick wins an exact score tie), and returns 0.  Called once per image with al == 0, in image
 * order, for every class (counts of 0 and 1 included); never for an image with al == 1.  A pick outside its range, an n_picks outside
 * its range or a non-zero return ends the call with CALD_ERR_INVALID naming the image and the class; no pick is read by the device before
 * it has been checked. */
#define CALD_SSM_RETINA_TAKE 500
typedef int (*cald_ssm_pick_fn)(void* user, int image, int K, const int* counts /*[K]*/,
                                int* picks /*[K][CALD_SSM_RETINA_TAKE]*/, int* n_picks /*[K]*/);
/* A cald_ssm_pick_fn that IS the reference's draw: per class `keep = list(range(n)); random.shuffle(keep); keep[:500]` of CPython (3.x:
 * for i in reversed(range(1, n)): j = _randbelow(i + 1); swap -- _randbelow(m) draws genrand_uint32() >> (32 - m.bit_length()) until it is
 * below m) on the MT19937 state `user` points at: uint32_t[625], the 624 words and then the index, as random.getstate()[1] lists them.
 * The state is advanced in place.  Host only.  Non-zero for a null argument, an index outside 0..624 or a negative count. */
int cald_ssm_pick_mt19937(void* user, int image, int K, const int* counts, int* picks, int* n_picks);
/* ssm/ssm_helper.py:9-33 get_uncertainty on a RetinaNet model (num_classes = K >= 2): cald_sweep_ssm's batch loop, checks and error texts
 * with the RetinaNet SSM tail (cald_op_retina_ssm_postprocess); `pick` is called between the two device phases of each batch, for the
 * batch's images in order (image = its index in this call).  Every image gets its own rows (the reference's accumulation across the
 * images of a batch is not reproduced).  Rows per image <= K * detections_per_img: boxes_out [rows][4], scores_out [rows] (the score of
 * the row's class), labels_out [rows][K - 1] (+1 / -1 over classes 1..K-1).  Results do not depend on batch_images.  A Faster R-CNN
 * model or a null argument (user may be null): CALD_ERR_INVALID. */
int cald_sweep_ssm_retina(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W, int batch_images,
                          cald_ssm_pick_fn pick, void* user, int64_t rows_cap, int* al_out, int* count_out, float* boxes_out,
                          float* scores_out, int8_t* labels_out, int64_t* rows_needed_out);
/* ls_c_train.py:108-155 get_uncertainty(task_model, unlabeled_loader) -> one float per image (six GaussianNoise views) */
int cald_sweep_lsc(cald_model* m, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                   const int64_t* pool_pos, uint64_t base_seed, int batch_images, double* stability_out);

/* ---- the learning-loss baseline (ll_train.py, ll4al/models/lossnet.py): the detector's forward stops after the FPN, four pyramid levels
 * are average-pooled over the whole PADDED map (AdaptiveAvgPool2d(1) of the batched ImageList tensor, frcnn_ll.py:601-602), and LossNet --
 * relu(FC_i) 256 -> D per level, concatenation, linear 4 D -> 1 -- scores every image (lossnet.hip). ---- */
typedef struct cald_lossnet cald_lossnet;
int cald_lossnet_create(cald_ctx* ctx, cald_lossnet** out);
/* LossNet.state_dict() keys: "FC1.weight" [D][256] ... "FC4.bias" [D], "linear.weight" [1][4*D], "linear.bias" [1]; D = interm_dim, 1..256 */
int cald_lossnet_load_tensor(cald_lossnet* ln, const char* key, const float* data, const int64_t* shape, int ndim);
/* CALD_ERR_MISSING_WEIGHT for a missing tensor, CALD_ERR_INVALID for a mis-shaped one */
int cald_lossnet_finalize(cald_lossnet* ln);
int cald_lossnet_destroy(cald_lossnet* ln);
typedef struct cald_ll_cfg {
    int batch_views;       /* views per launch sequence (0 = default 32; capped at 128); results do not depend on it */
    int levels[4];         /* pyramid index per LossNet branch: Faster R-CNN 0..3 = P2..P5, RetinaNet 0..4 = P3..P7 */
} cald_ll_cfg;
/* ll_train.py:145-166 get_uncertainty(task_model, ll_model, unlabeled_loader).  group[i]: loader-batch id of image i (non-decreasing);
 * an image is padded to its group's common size -- the per-dimension maximum of the members' resized sizes, rounded up to 32 -- so its
 * score depends on its loader batch, as in the reference.  cfg NULL: batch_views 0 and the reference's levels as shipped: {0,1,2,3} for
 * Faster R-CNN, {0,0,0,0} for RetinaNet (ll_train.py:155-161 feeds features[0] = P3 to all four branches).  A cfg's levels are taken as given.
 * uncertainty_out [n] (the float32 value, widened); pooled_out: NULL or [n][4][256] float32, the four pooled vectors per image. */
int cald_sweep_ll(cald_model* m, cald_lossnet* ln, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                  const int* group, const cald_ll_cfg* cfg, double* uncertainty_out, float* pooled_out);

/* ---- training the loss-prediction module (ll_train.py:55-142, ll4al/models/lossnet.py, ll4al/main.py:64-83; lossnet_train.hip).  All
 * pointers are DEVICE pointers unless said otherwise; everything is enqueued on the context's stream; every sum has a fixed order. ---- */
/* The training forward's pooling: maps[l] = dense [N][H_l][W_l][256] (level_hw = host {H_0, W_0, ..., H_3, W_3}), the batch's PADDED maps
 * (frcnn_ll.py:601-602) -> pooled [N][4][256], with the sweep's two pooling kernels, hence cald_op_gap's summation order and bits. */
int cald_train_gap(cald_ctx* ctx, int N, const float* const* maps, const int* level_hw, float* pooled);
/* LossNet parameters (or their gradients) in LossNet.state_dict() layout */
typedef struct cald_lossnet_tensors {
    float* fc_w[4];        /* FCj.weight [D][256] */
    float* fc_b[4];        /* FCj.bias [D] */
    float* lin_w;          /* linear.weight [1][4 D] */
    float* lin_b;          /* linear.bias [1] */
} cald_lossnet_tensors;
/* pooled [B][4][256] -> hidden [B][4][D] = relu(FCj), pred [B]: the arithmetic of cald_op_lossnet (one k-ordered fmaf chain from +0 per FC
 * output, + bias, ReLU; one chain over 4 D, + bias), so pred carries cald_op_lossnet's bits.  D = 1..256. */
int cald_lossnet_train_fwd(cald_ctx* ctx, int B, int D, const cald_lossnet_tensors* params, const float* pooled, float* hidden, float* pred);
/* g_pred [B] = d loss / d pred.  grads (same layout as params): g linear.weight[i] = sum_b g_b * hidden[b][i] and g linear.bias = sum_b g_b,
 * b ascending from +0; g_h = hidden > 0 ? g_b * lw[i] : 0; g FCj.weight[d][c] = sum_b g_h[b][j][d] * pooled[b][j][c] and g FCj.bias[d] =
 * sum_b g_h[b][j][d], b ascending; accumulate != 0 adds to what grads holds.  g_pooled [B][4][256] (null when the features are detached):
 * one d-ordered fmaf chain from +0 per element.  gh_scratch [B][4 D]. */
int cald_lossnet_train_bwd(cald_ctx* ctx, int B, int D, const cald_lossnet_tensors* params, const float* pooled, const float* hidden,
                           const float* g_pred, float* gh_scratch, const cald_lossnet_tensors* grads, int accumulate, float* g_pooled);
/* ll4al/main.py:64-83 LossPredLoss(input, target, margin): pairs (i, B-1-i), i < B/2; one = t_i - t_(B-1-i) > 0 ? +1 : -1 (a tie is -1);
 * term_i = max(0, margin - one * (p_i - p_(B-1-i))); loss_out [1] = (sum of the terms, i ascending from +0) / (B/2); terms_out (or null)
 * [B/2] = reduction='none'.  grad_out (or null) [B]: per_pair == 0 (reduction='mean') g_up / (B/2) * d sum / d input with g_up = *g_up_dev
 * (null: 1); per_pair != 0 (reduction='none') pair i's upstream gradient is g_up_dev[i] (null: 1) and nothing is divided.  At term == 0
 * exactly the gradient passes (torch.clamp's backward).  B odd or > 2048: CALD_ERR_INVALID before any launch. */
int cald_loss_pred_loss(cald_ctx* ctx, int B, const float* input, const float* target, float margin, int per_pair, const float* g_up_dev,
                        float* loss_out, float* terms_out, float* grad_out);

/* ---- the VAAL sweep (vaal/vaal_helper.py:186-222 AdversarySampler.sample): nearest resize of the uint8 pool image to 256 x 256, the VAE's
 * five 4 x 4 / 2 / 1 convolutions each followed by BatchNorm2d and ReLU, fc_mu 65 536 -> 256, and the discriminator 256 -> 512 -> 512 -> 1
 * with a sigmoid (vaal.hip).  Every image's result depends on that image alone. ---- */
typedef struct cald_vaal cald_vaal;
int cald_vaal_create(cald_ctx* ctx, cald_vaal** out);
/* state_dict() keys of VAE and Discriminator: "encoder.{0,3,6,9,12}.{weight,bias}", "encoder.{1,4,7,10,13}.{weight,bias,running_mean,
 * running_var}", "fc_mu.{weight,bias}", "net.{0,2,4}.{weight,bias}".  Any other key (the decoder, fc_logvar, num_batches_tracked) is
 * accepted and ignored. */
int cald_vaal_load_tensor(cald_vaal* v, const char* key, const float* data, const int64_t* shape, int ndim);
/* CALD_ERR_MISSING_WEIGHT for a missing tensor, CALD_ERR_INVALID for a mis-shaped one */
int cald_vaal_finalize(cald_vaal* v);
int cald_vaal_destroy(cald_vaal* v);
#define CALD_VAAL_BN_BATCH 0     /* the module in train(): every BatchNorm normalises with the statistics of its one image */
#define CALD_VAAL_BN_RUNNING 1   /* the module in eval(): running statistics, folded into the convolution's scale / shift */
typedef struct cald_vaal_cfg {
    int bn_mode;           /* CALD_VAAL_BN_* */
    int batch_images;      /* images per launch sequence (0 = default 64; capped at 128); results do not depend on it */
} cald_vaal_cfg;
/* images_dev[i]: uint8 HWC image of H[i] x W[i] in device memory.  cfg NULL: batch statistics, 64 images per launch sequence.
 * preds_out [n]: the discriminator's output; mu_out: NULL or [n][256]. */
int cald_sweep_vaal(cald_ctx* ctx, cald_vaal* v, int n_images, const uint8_t* const* images_dev, const int* H, const int* W,
                    const cald_vaal_cfg* cfg, float* preds_out, float* mu_out);

/* ---- operator-level entry points (used by the parity tests; same kernels as the paths above) ---- */
/* pieces of the VAAL sweep; host pointers.  resize: uint8 [H][W][3] -> float32 [256][256][3].  bn_relu: x holds x_floats >= n HW C floats of
 * which [n][HW][C] are the maps (the rest is uploaded too and must not be read); out [n][HW][C].  fc_mu: act [n][64][1024] (pixel-major,
 * NHWC) -> mu [n][256].  head: mu [n][256] -> preds [n]. */
int cald_op_vaal_resize(cald_ctx* ctx, const uint8_t* image, int H, int W, float* out);
int cald_op_vaal_bn_relu(cald_ctx* ctx, const float* x, long long x_floats, int n, int HW, int C, const float* gamma, const float* beta,
                         float* out);
int cald_op_vaal_fc_mu(cald_vaal* v, int n, const float* act, float* mu_out);
int cald_op_vaal_head(cald_vaal* v, int n, const float* mu, float* preds_out);
/* the learning-loss sweep's pooling of one [H][W][C] tensor (C == 256) in its fixed order (lossnet.hip), and LossNet on n x [4][256] pooled
 * vectors; host pointers */
int cald_op_gap(cald_ctx* ctx, const float* x, int H, int W, int C, float* mean_out);
int cald_op_lossnet(cald_lossnet* ln, int n, const float* pooled, float* out);
/* scoring of ONE (reference, augmentation) pair, cald_train.py:189-224 */
int cald_op_consistency(cald_ctx* ctx, int N, const float* aug_box, const float* ref_scores_cls, const float* ref_pm,
                        int M, const float* boxes, const float* scores_cls, const float* pm, int C, float bp,
                        float* consistency_out);
/* cald_train.py:114-117 */
int cald_op_cls_corr(cald_ctx* ctx, int n, const float* scores, const int64_t* labels, int C, float* out);
/* The scoring stage of ONE sweep batch in the sweeps' own layout, on the sweeps' own table filling and launches (score.hip's five
 * kernels in one call); host arrays in, host arrays out.  V views of `cap` detection slots each (count[v] <= cap of them live), n_img
 * images, P (reference view, augmented view) pairs.  Rejected with CALD_ERR_INVALID, nothing written: a null pointer, C outside 2..256,
 * cap < 1, a count outside 0..cap, ref_n outside 0..50, a live ref_sel slot outside 0..cap - 1, a view or image index out of range, an
 * aug_kind outside 0..3. */
typedef struct cald_score_probe {
    int V, cap, C, n_img, P;
    float bp;
    /* in, per view */
    const float* boxes;        /* [V][cap][4] */
    const float* props;        /* [V][cap][4] the proposal each detection stems from */
    const float* scores;       /* [V][cap] */
    const int64_t* labels;     /* [V][cap] */
    const float* scores_cls;   /* [V][cap][C] */
    const float* prob_max;     /* [V][cap] */
    const int* count;          /* [V] */
    const int* view_img;       /* [V] image of the view */
    const int* view_isref;     /* [V] != 0: a reference view (cls_corr reads its sub-sampled detections only) */
    /* in, per image */
    const int* ref_sel;        /* [n_img][50] the scored detections of the image's reference view */
    const int* ref_n;          /* [n_img] how many of the 50 slots are live */
    /* in, per pair */
    const int* ref_view;       /* [P] */
    const int* aug_view;       /* [P] */
    const int* pair_img;       /* [P] */
    const int* aug_kind;       /* [P] 0 boxes unchanged, 1 flip, 2 resize, 3 rotate */
    const float* aug_param;    /* [P][12] cald_op_pair_params */
    /* out */
    float* cons;               /* [P] consistency_kernel */
    float* cls_corr;           /* [V][C - 1] cls_corr_kernel */
    float* pair_audit;         /* [P][2] pair_audit_kernel: {argmax gap, zero-row flag} */
    float* max_iou;            /* [P][50] max_iou_kernel (boxes NOT transformed, as in ls_c); slots from ref_n on are left as they are */
    float* lt;                 /* [V] lt_uncertainty_kernel */
} cald_score_probe;
int cald_op_score_batch(cald_ctx* ctx, cald_score_probe* p);
/* host only: the aug_param row the sweep gives the scoring kernels for a pair of an H x W image; kind as aug_kind above (1: param unused,
 * 2: the ratio, 3: the angle in degrees; 0: zeros).  par12_out [12] */
int cald_op_pair_params(int kind, int H, int W, double param, float* par12_out);
/* host only: the host tail of cald_sweep_lsc.  prob_max [n] of the reference view's detections -> sel_out [30] / *n_sel_out, the scored
 * boxes (all while n <= 30, else the top 30: value descending, index ascending).  score_out (NULL: selection only): the image's float64
 * score from max_iou [n_rows][*n_sel_out], row r = the maximum IoUs of the selected boxes in noisy view r; n == 0 gives 0.0 */
int cald_op_ls_tail(int n, const float* prob_max, int n_rows, const float* max_iou, int* sel_out, int* n_sel_out, double* score_out);
/* ---- detection-to-ground-truth matching of the AP evaluators (eval.hip).  Host arrays in, host arrays out; IEEE double in the host
 * code's operation order, so every output equals what the Python statement gives.  A segment is one unit of the greedy matching; its
 * detections / ground truths are rows dt_off[s] .. dt_off[s + 1] - 1 / gt_off[s] .. gt_off[s + 1] - 1 of the flat arrays (offsets
 * [n_seg + 1], from 0).  A segment with more than CALD_EVAL_MAX_DT detections or CALD_EVAL_MAX_GT ground truths, or more than 64
 * variants (T * A, or T), returns CALD_ERR_UNSUPPORTED before anything is uploaded or written. */
#define CALD_EVAL_MAX_DT 128
#define CALD_EVAL_MAX_GT 256
/* cald_amd/coco_eval.py COCOeval.evaluate_img for every segment = (image, category), every area range and every IoU threshold at once.
 * dt_box [D][4] xywh in score order (stable, descending, already cut at maxDets), dt_area [D]; gt_box [G][4] xywh in annotation order,
 * gt_area [G] the annotation's area, gt_iscrowd / gt_ignore_in [G]; iou_thrs [T]; area_rng [A][2].  Out: dt_match [A][T][D] = position
 * of the matched ground truth inside its segment (annotation order) or -1; dt_ignore [A][T][D] = the matched ground truth's ignore flag,
 * or for an unmatched detection "dt_area outside the range"; gt_ignore [A][G] = gt_ignore_in or the annotation area outside the range. */
int cald_op_coco_match(cald_ctx* ctx, int n_seg, const int64_t* dt_off, const int64_t* gt_off,
                       const double* dt_box, const double* dt_area,
                       const double* gt_box, const double* gt_area, const uint8_t* gt_iscrowd, const uint8_t* gt_ignore_in,
                       int T, const double* iou_thrs, int A, const double* area_rng,
                       int32_t* dt_match, uint8_t* dt_ignore, uint8_t* gt_ignore);
/* cald_amd/voc_eval.py best_overlaps + mark_detections of one class at T thresholds; a segment = one image.  gt_box [G][4] x1 y1 x2 y2
 * and gt_difficult [G] per image; dt_box [nd][4] grouped by segment, inside a segment in the class's confidence order; dt_index [nd] =
 * each detection's place in that order (a permutation of 0 .. nd - 1).  Out, at the place dt_index names: ovmax [nd] (-inf without a
 * box of the class), jmax [nd] (the first maximum; 0 without a box), tp / fp [T][nd] (strict ovmax > thrs[t]). */
int cald_op_voc_match(cald_ctx* ctx, int n_seg, const int64_t* dt_off, const int64_t* gt_off,
                      const double* gt_box, const uint8_t* gt_difficult, const double* dt_box, const int64_t* dt_index,
                      int T, const double* thrs, int64_t nd, double* ovmax, int64_t* jmax, uint8_t* tp, uint8_t* fp);
/* cald_helper.resize: PIL.Image.resize((ow, oh), BILINEAR) on uint8 RGB */
int cald_op_pil_resize(cald_ctx* ctx, const uint8_t* src_dev, int H, int W, uint8_t* dst_dev, int oh, int ow);
/* cald_helper.cutout rectangle selection (host side RNG = Python random seeded per image) */
int cald_op_cutout_rects(uint64_t seed, int H, int W, int N, const float* boxes, int cut_num, int* rects_out, int* n_out);
/* The cut_out view's dirty sets (host only; what cald_sweep's cut_out reuse recomputes).  H x W source image, detector sizes min_size /
 * max_size, nrect cutout rectangles (left, top, right, bottom; right / bottom exclusive), nblk bottleneck blocks with the stride of each
 * block's 3 x 3 conv, starting at the pooled stem output (/4).  out: (1 + nblk) x 2 sets of 17 ints {n, then n x (x0, y0, x1, y1),
 * inclusive}: set 0 of entry 0 = the pooled stem output; entry 1 + b = block b's output (set 0) and the pixels its conv1 computes (set 1).
 * A pixel outside a dirty set has the reference view's bits. */
int cald_op_cutout_geometry(int H, int W, int min_size, int max_size, int nrect, const int* rects, int nblk, const int* strides, int* out);
/* The same through the FPN of Faster R-CNN (host only): strides of ALL nblk blocks of the backbone (a stage ends before the next stride-2
 * block; there must be four).  out: 8 sets of 17 ints in the form above: the dirty sets of the laterals (inner P2..P5: C_l's dirty set
 * joined with the 2 x upsample of the lateral above), then of the 3 x 3 output convs (P2..P5: one ring around the lateral's set). */
int cald_op_cutout_fpn_geometry(int H, int W, int min_size, int max_size, int nrect, const int* rects, int nblk, const int* strides, int* out);
/* one augmented view outside the sweep (helper API of cald/cald_helper.py; same kernels as inside cald_sweep).  A fresh
 * generator is seeded with `seed` (torch's CPU generator for GAUSS / SALT_PEPPER, Python's `random` for COLOR_SWAP).
 *   CALD_AUG_GAUSS        GaussianNoise :72-75    dst_dev = float [3][H][W], the additive term randn * param / 255
 *   CALD_AUG_SALT_PEPPER  SaltPepperNoise :78-85  dst_dev = uint8 [H][W][3]
 *   CALD_AUG_COLOR_ADJUST ColorAdjust :65-69      dst_dev = uint8 [H][W][3]
 *   CALD_AUG_COLOR_SWAP   ColorSwap :56-62        aux_out[0] = index of the drawn channel permutation (no device work)
 *   CALD_AUG_ROTATE       rotate :135-223         dst_dev = uint8 [H][W][3], boxes_out[n_boxes][4] (host)
 * Two edges of the Pillow / torch calls behind these:
 *   - GAUSS needs 3 * H * W >= 16.  Below that torch.randn takes its scalar path (another draw pattern), which is not implemented:
 *     cald_op_augment, cald_op_noise_stream, cald_sweep (with a GAUSS augmentation) and cald_sweep_lsc return CALD_ERR_UNSUPPORTED
 *     for such an image and write nothing.  A 1 x 6 image is the smallest accepted.  SALT_PEPPER has no such limit.
 *   - ROTATE by 90 or 270 degrees (mod 360) follows Pillow's short-cut: Image.rotate(expand=True) returns the exact transpose
 *     (a W x H image) instead of running the affine loop, whose expanded canvas would be one pixel larger each way.  Every other
 *     angle, 0 and 180 included, takes the affine path, which equals Pillow's result there. */
int cald_op_augment(cald_ctx* ctx, int kind, double param, uint64_t seed, const uint8_t* src_dev, int H, int W,
                    int n_boxes, const float* boxes, void* dst_dev, float* boxes_out, int* aux_out);
/* parity hook of the noise kernel: nseg (1..16) GaussianNoise / SaltPepperNoise views of ONE image drawn in order from ONE generator
 * seeded with `seed`, in one launch -- what cald_sweep issues per image ('multi_ga', 'multi_sp', cald_sweep_lsc), without a model.
 * kinds[g] = CALD_AUG_GAUSS or CALD_AUG_SALT_PEPPER, params[g] and the layout of the device buffer dsts[g] as in cald_op_augment
 * (kinds, params and the pointer array dsts are host memory). */
int cald_op_noise_stream(cald_ctx* ctx, uint64_t seed, const uint8_t* src_dev, int H, int W, int nseg, const int* kinds,
                         const double* params, void* const* dsts);
/* RoIHeads.postprocess_detections + GeneralizedRCNNTransform.postprocess of one view (detection/frcnn_la.py:32-87, :292-315) on the
 * forward's own kernels: logits [R][C], deltas [R][4C] (class-major), proposals [R][4] in resized-image coordinates (host); outputs
 * (host, det_max rows each; scores_cls [det_max][C]) and the number of detections.  R <= 1000. */
int cald_op_frcnn_postprocess(cald_ctx* ctx, int R, int C, const float* logits, const float* deltas, const float* proposals,
                              int Hr, int Wr, int Ho, int Wo, float score_thr, float nms_thr, int det_max,
                              float* boxes_out, float* scores_out, int64_t* labels_out, float* props_out, float* prob_max_out,
                              float* scores_cls_out, int* n_out);
/* The same with torchvision's stock remove_small_boxes between the score threshold and NMS (cald_model_set_box_min_size): candidates whose
 * clipped width or height is < box_min_size are dropped and do not count towards batched_nms's maximum coordinate.  0 = the call above. */
int cald_op_frcnn_postprocess_min(cald_ctx* ctx, int R, int C, const float* logits, const float* deltas, const float* proposals,
                                  int Hr, int Wr, int Ho, int Wo, float score_thr, float nms_thr, int det_max, float box_min_size,
                                  float* boxes_out, float* scores_out, int64_t* labels_out, float* props_out, float* prob_max_out,
                                  float* scores_cls_out, int* n_out);
/* RoIHeads.ssm_postprocess_detections + GeneralizedRCNNTransform.postprocess of one view (detection/frcnn_ssm.py:44-102, :367, :400) on the
 * SSM forward's own kernels (ssm.hip); inputs as above.  *al_out = 1 when the largest foreground probability is < 0.5 (or R == 0, where the
 * reference raises): no rows then.  Else per foreground class NMS at IoU 0.3 over all R proposals, the first det_max survivors, of those the
 * ones scoring > score_thr: *n_out <= (C - 1) * det_max rows in (class, kept) order -- boxes_out [n][4] on the original image, scores_out
 * [n][C - 1] the proposal's foreground probabilities, labels_out [n][C - 1] = +1 where the probability is > 0.5, else -1.  The output
 * arrays hold (C - 1) * det_max rows.  R <= 1000, det_max <= 512. */
int cald_op_ssm_postprocess(cald_ctx* ctx, int R, int C, const float* logits, const float* deltas, const float* proposals,
                            int Hr, int Wr, int Ho, int Wo, float score_thr, int det_max,
                            int* al_out, int* n_out, float* boxes_out, float* scores_out, int8_t* labels_out);
/* RetinaNet.postprocess_detections + the stock GeneralizedRCNNTransform.postprocess of one view (detection/retinanet_cal.py:402-490) on
 * the forward's own kernels: cls[l] = [H_l][W_l][A*K] logits (channel a*K + k), reg[l] = [H_l][W_l][A*4] deltas for the five levels
 * P3..P7 (host), level_hw = {H0, W0, ..., H4, W4}, base_anchors [5][A][4], padded size Hp x Wp (anchor strides Hp / H_l, Wp / W_l),
 * resized size Hr x Wr (clip), original size Ho x Wo.  Outputs (host, K * per_class rows each; scores_cls [K * per_class][K]) in class
 * order and the number of detections.  per_class <= 1024, at most 2^20 anchors. */
int cald_op_retina_postprocess(cald_ctx* ctx, const float* const* cls, const float* const* reg, const int* level_hw, int A, int K,
                               const float* base_anchors, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo,
                               float score_thr, float nms_thr, int per_class,
                               float* boxes_out, float* scores_out, int64_t* labels_out, float* prob_max_out,
                               float* scores_cls_out, int* n_out);
/* The stock RetinaNet tail of one view as in cald_op_retina_postprocess (same inputs), then the decision-margin audit of that view
 * (audit.hip audit_retina_kernel): *n_out = the number of detections, margins_out [CALD_N_MARGINS] = the view's records in the public
 * numbering -- POST_THR / POST_IOU / POST_ORDER / POST_CAP (7-10) and POST_SMALL (15); REF_SUBSAMPLE (11) as if the view were a reference
 * view; ZERO_ROW (13) = the gap of the list's first two rows when they are of one class; +inf everywhere else.  per_class <= 512. */
int cald_op_retina_audit(cald_ctx* ctx, const float* const* cls, const float* const* reg, const int* level_hw, int A, int K,
                         const float* base_anchors, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo,
                         float score_thr, float nms_thr, int per_class, int* n_out, float* margins_out);
/* RetinaNet.ssm_postprocess_detections + the stock transform.postprocess of one view (detection/retina_ssm.py:487-584) on the SSM forward's
 * own kernels (retina_ssm.hip); inputs as for cald_op_retina_postprocess, K >= 2.  *al_out = 1 when the largest score over all K classes
 * is < 0.5: no rows, counts_out zero, `pick` not called.  Else counts_out[k] = anchors with score[k] > score_thr, `pick` is called once
 * (image 0), and per class the picked candidates are decoded, clipped, those with a side < 1e-2 dropped, NMS at nms_thr, the first
 * per_class survivors: *n_out rows in (class, score desc) order -- boxes_out [n][4] on the original image, scores_out [n], labels_out
 * [n][K - 1] = +1 where the anchor's score of class 1..K-1 is > 0.5, else -1.  The output arrays hold K * per_class rows.
 * per_class <= 1024, at most 2^20 anchors. */
int cald_op_retina_ssm_postprocess(cald_ctx* ctx, const float* const* cls, const float* const* reg, const int* level_hw, int A, int K,
                                   const float* base_anchors, int Hp, int Wp, int Hr, int Wr, int Ho, int Wo,
                                   float score_thr, float nms_thr, int per_class, cald_ssm_pick_fn pick, void* user,
                                   int* al_out, int* n_out, int* counts_out, float* boxes_out, float* scores_out, int8_t* labels_out);
/* The certified pruning's three kernels outside any model (rpn_prune.hip: select stage 0, select stage 1, scatter, in the forward's order;
 * tests/test_gpu_rpn_prune_edges.py).  The hook plays the gathered exact convs itself: after each select it reads nsel / row_map back and
 * gathers that stage's exact head rows from `exact` by row_map -- compact per view at the view's pixel offset, as the gathered launch
 * writes them; rows past nsel hold NaN.  All arrays are host memory.  Per level l < 2 and view v < V the geometry is hw[l][v] = {H, W}
 * (ragged views; level 1 need not be smaller than level 0); pix_l = sum of H * W.  Every per-pixel array holds pix_l + guard pixels and
 * tau_key / nsel[s] hold 2 * V + guard words: in / out arrays are copied to the device whole and back whole, so sentinels the caller put
 * into unused slots and guard words show any stray store. */
#define CALD_PRUNE_PROBE_MAX_VIEWS 8
typedef struct {
    int V, guard;
    int hw[2][CALD_PRUNE_PROBE_MAX_VIEWS][2];
    int pre_n, head_ld;                 /* head_ld >= 3: logits are channels 0..2 */
    float c1[3], c0[3];                 /* B_a(p) = c1[a] * pnorm(p) + c0[a] */
    const float* energy[2];             /* in  [pix_l][4] (no guard) */
    const float* exact[2];              /* in  [pix_l][head_ld]: the dense exact head map (no guard) */
    float* head[2];                     /* in: the look-ahead's map, out: the final map; [pix_l + guard][head_ld] */
    float* pnorm[2];                    /* in / out [pix_l + guard] */
    uint32_t* tau_key;                  /* in / out [2 * V + guard], read back after stage 0 */
    int* row_map[2][2];                 /* in / out [stage][level] [pix_l + guard] */
    int* nsel[2];                       /* in / out [stage] [2 * V + guard] */
    float check[2];                     /* in: the initial check words, out: the final ones */
    uint64_t stat[4];                   /* out: selected / total pixels of level 0, of level 1 (from zero) */
} cald_rpn_prune_probe;
int cald_op_rpn_prune(cald_ctx* ctx, cald_rpn_prune_probe* p);
/* MultiScaleRoIAlign(output 7, sampling_ratio 2, aligned=False; detection/frcnn_la.py:205-209) of one view on the forward's own
 * kernels: feats[l] = [H_l][W_l][C] (host) for P2..P5, level_hw = {H0, W0, ..., H3, W3}, rois [R][4]; out [R][49][C] (host) */
int cald_op_roi_align(cald_ctx* ctx, const float* const* feats, const int* level_hw, int C, int R, const float* rois, float* out);
/* The same stage on V views (1..CALD_MAX_VIEWS = 128) in the forward's own layout: one buffer a level with the views' maps one after the
 * other, 1000 proposal slots and 1000 output rows a view.  feats[4 v + l] = [H][W][C] (host) of view v's level l, level_hw [V][4][2]
 * (views may differ), counts [V] in 0..1000, rois = the views' RoIs one after the other ([sum counts][4], finite).  C a multiple of 4
 * up to 1024 (of 16 when out16).  out16 1: the rows in split form (one 32-bit word an element: per 16 channels 16 fp16 hi, then 16 fp16
 * lo of 16 x).  kernel 0: what the forward runs (the row walk at C == 256 unless CALD_ROI_ROWS=0), 1: the gather kernel.  out
 * [V][rows_back][49][C] words (1 <= rows_back <= 1000), in AND out: uploaded into the first rows_back rows of each view's slot before
 * the launch, downloaded after it -- rows from counts[v] on come back as they went.  order_out (NULL or [V][1024]): the processing
 * order of each view, its first counts[v] entries a permutation of the view's RoIs.  Rejected with CALD_ERR_INVALID, nothing written:
 * a null pointer, a size, count or flag out of range, a non-finite RoI. */
int cald_op_roi_align_views(cald_ctx* ctx, int V, const float* const* feats, const int* level_hw, const int* counts, const float* rois,
                            int C, int out16, int kernel, int rows_back, uint32_t* out, int* order_out);
/* NHWC convolution on the MFMA kernel; weights in torch layout [Cout][Cin][KH][KW] (host) */
int cald_op_conv2d(cald_ctx* ctx, const float* in, int H, int W, int Cin, const float* weight, int Cout, int KH, int KW,
                   int stride, int pad, const float* bias, const float* bn_scale, const float* bn_shift,
                   const float* residual, int relu, float* out);
/* the same convolution in CALD_PRECISION_F16X3 (conv_h3.hip); falls back to the exact kernels for shapes it does not
 * cover (Cin % 16 != 0 or Cout not tiled by 128), exactly as inside a model */
int cald_op_conv2d_f16x3(cald_ctx* ctx, const float* in, int H, int W, int Cin, const float* weight, int Cout, int KH, int KW,
                         int stride, int pad, const float* bias, const float* bn_scale, const float* bn_shift,
                         const float* residual, int relu, float* out);
/* Test-only conv probe (tests/test_gpu_conv_variants.py): ONE launch of the product's conv launchers, weights packed by the product's own
 * packing, on a ragged batch of V views laid out as a forward lays them out (per-view pixel offsets and 128-row tile starts).  All arrays
 * are host memory.  `path` pins the kernel family (0 auto = the product's choice, 1 conv_p4, 2 conv_p4 grouped, 3 conv_p4 fused layer-1
 * pair, 4 generic conv_mfma, 5 conv_stem, 6 conv_h3, 7 conv_h3 grouped, 8 conv_h4, 9 conv_h4 grouped), `tile` the conv_p4 tile (0 auto,
 * 1 narrow 128 x 64, 2 wide 128 x 128).  n > 1 problems go through the grouped launcher; the fused mode takes n = 2 (conv2, conv3; conv3's
 * `in` is conv2's output).  A pinned launcher that cannot take the problem returns CALD_ERR_UNSUPPORTED -- it never hands the problem to
 * another kernel.  out / out16 / energy4 are copied to the device whole and back whole: words the caller put past what a kernel may write
 * (guard rows, channels Cout..out_ld) show any stray store.  `kernel` receives the launched instantiation(s), ';'-separated. */
#define CALD_PROBE_MAX_VIEWS 8
#define CALD_PROBE_MAX_RECTS 8
typedef struct cald_conv_probe {
    int V;
    int in_hw[CALD_PROBE_MAX_VIEWS][2];    /* input H, W per view (0 x 0: an empty view) */
    int up_hw[CALD_PROBE_MAX_VIEWS][2];    /* `up`: the coarser level's H, W per view */
    int dyn_rows[CALD_PROBE_MAX_VIEWS];    /* per-view row counts, used when has_dyn */
    int has_dyn;
    int gather;                            /* 1: only the rows of each view's rectangles (x0, y0, w, h in output pixels) */
    int nrect[CALD_PROBE_MAX_VIEWS];
    int rect[CALD_PROBE_MAX_VIEWS][CALD_PROBE_MAX_RECTS][4];
    int Cin, Cout, KH, KW, stride, pad, relu, in_relu, out_ld;
    int cin_true;                          /* input channels of `weight` (0: Cin); the rest are zero-padded, as the stem's 3 -> 4 */
    const float* weight;                   /* torch layout [Cout][cin_true][KH][KW] */
    const float* bias;                     /* [Cout] or null */
    const float* bn_scale;                 /* FrozenBN [Cout] or null */
    const float* bn_shift;
    const float* in;                       /* [sum H W][Cin] */
    const uint32_t* in16;                  /* the same input in split form (CALD_PRECISION_F16X3) or null */
    const float* residual;                 /* [sum Ho Wo][out_ld] or null (split words when ex16) */
    const float* up;                       /* [sum Hu Wu][out_ld] or null (split words when ex16) */
    int ex16;
    const float* mask;                     /* [sum Ho Wo][out_ld] or null: out = mask > 0 ? out : 0 */
    const int* row_map;                    /* [sum Ho Wo] or null: compact row m of a view is the output pixel row_map[pix_off + m] */
    float* out; int64_t out_n;             /* words, >= sum Ho Wo * out_ld; null = split-form output only */
    uint32_t* out16; int64_t out16_n;      /* split-form output or null */
    float* energy4; int64_t energy4_n;     /* [pixel][4] partial sums of squares or null */
    /* conv_h4 grouped (path 9) only, optional: the look-ahead's head epilogue.  head_w [3][Cout] and head_b [3] of a 1 x 1 head on this conv's
     * output (Cout == 256); head_out [>= sum Ho Wo][head_ld] receives the three logits in channels 0..2 and the conv's own output is not
     * written (out / out16 may be null).  head_out null = no head */
    const float* head_w; const float* head_b;
    float* head_out; int64_t head_out_n; int head_ld;
    /* conv_p4's row tiles: 0 auto = the product's choice (packed wherever a forward would pack this launch, unless CALD_CONV_PACK=0),
     * 1 = per-view tiles, 2 = packed tiles (CALD_ERR_INVALID for a problem that cannot be packed: dyn_rows, row_map, gather, mask,
     * Cin == 4, the fused pair).  Kernel families other than conv_p4 tile per view whatever this says. */
    int row_packing;
} cald_conv_probe;
#define CALD_PROBE_PACK_AUTO 0
#define CALD_PROBE_PACK_OFF 1
#define CALD_PROBE_PACK_ON 2
int cald_op_conv_probe(cald_ctx* ctx, int precision, cald_conv_probe* probs, int n, int path, int tile, char* kernel, int kernel_cap);
/* Host-only test hook of the packed row tiles (tests/test_row_packing_lookup.py; needs no GPU): on a level of V views with the given input
 * and output sizes ([V][2] H, W; 0 x 0 = empty), for each of n rows of the output level's flat row space the view that holds it and the row
 * inside that view, by the kernels' own bisection (largest v with pix_off[v] <= row); *packed_rows_out = the row count a launch with Cin
 * input channels and row stride out_ld may be packed with, or 0 where a straddling tile would leave the 32-bit offset range. */
int cald_op_row_pack_lookup(int V, const int* in_hw, const int* out_hw, int Cin, int out_ld, int64_t n, const int64_t* rows,
                            int* view_out, int64_t* local_out, int64_t* packed_rows_out);
/* Parity hook of CALD_PRECISION_F16X3's arithmetic primitive: n independent dot products D[i] = C[i] + sum_{k<16} A[i][k] B[i][k], each
 * evaluated by the hardware as ONE output element of v_mfma_f32_32x32x16_f16 (the instruction conv_h3.hip / conv_h4.hip are built on;
 * there is no reference function -- the reference has no fp16 path).  A, B: fp16 bit patterns [n][16], C / D: fp32
 * bit patterns [n] (host).  tests/ hold oracle/mfma_f16_model.h, the CPU statement of that instruction, against it bit for bit. */
int cald_op_mfma_f16(cald_ctx* ctx, const uint16_t* A, const uint16_t* B, const uint32_t* C, uint32_t* D, int64_t n);
/* kernel-tuning aid (tools/bench_conv.py): average time of ONE conv layer shape (the model's own kernel selection) over a
 * ragged batch of n_views equal views filled with pseudo-random data; `group` > 1 issues that many independent copies as one
 * grouped launch (FPN / RPN style).  tflops_out counts algorithmic FLOPs (2 * M * Cout * KH*KW*Cin).  relu: bit 0 = ReLU in the
 * epilogue. */
int cald_op_conv_bench(cald_ctx* ctx, int n_views, int H, int W, int Cin, int Cout, int KH, int stride, int pad, int residual,
                       int relu, int iters, int group, double* ms_out, double* tflops_out);
/* detector-transform size (GeneralizedRCNNTransform): resized and padded sizes */
int cald_op_transform_size(int H, int W, int min_size, int max_size, int* Hr, int* Wr, int* Hp, int* Wp);
/* intermediate tensors of the LAST cald_forward (parity debugging): name in
 * {"input","conv1","pool1","C2".."C5","P2".."P6","rpn0".."rpn4","proposals","roi","fc6","fc7","pred"} */
int cald_debug_tensor(cald_model* m, const char* name, int view, float* host_out, int64_t capacity, int64_t* shape3);

/* ---- input side: PIL.Image.open(path).convert('RGB') of torchvision's VOCDetection /
 * CocoDetection __getitem__ (detection/voc_utils.py:47-58, detection/coco_utils.py; DataLoader at cald_train.py:434).
 * Bit-identical to Pillow / libjpeg-turbo defaults (ISLOW IDCT, fancy upsampling; IDCT outputs beyond the sample range
 * saturate as turbo's SIMD code does).  Outside the promise: files whose dequantised values (coefficient x quantiser)
 * do not fit int16, where turbo saturates 16-bit intermediates; no encoder makes one from 8-bit samples.  Three kinds of file:
 *   BASELINE      8-bit sequential Huffman (SOF0 / SOF1), grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan,
 *                 restart intervals allowed.  This is the strict set of cald_jpeg_info / cald_jpeg_decode_batch: they
 *                 return CALD_ERR_UNSUPPORTED for anything else and decode nothing on the CPU.
 *   GPU_EXTENDED  decoded on the GPU by cald_jpeg_decode_batch_any only: 8-bit progressive Huffman (SOF2), same colour
 *                 and sampling set, whose scan script follows T.81 G.1.1.1 and brings every coefficient of every
 *                 component to Al = 0 (DC scans interleaved over all components or single-component; restart intervals
 *                 allowed; tables may change between scans); and 3-component files coded as R, G, B (Adobe transform 0,
 *                 or component ids 'R','G','B' without JFIF), sequential or progressive.
 *   HOST_ONLY     a JPEG the GPU path does not decode; the caller decodes it on the host (cald_amd.pool falls back to
 *                 Pillow): 4-component CMYK / YCCK, arithmetic coding, lossless, hierarchical, 12-bit, other sampling
 *                 factors, sequential files with more than one scan, and progressive files that are truncated, whose
 *                 script is incomplete (libjpeg smooths what is missing) or breaks the progression rules. ---- */
#define CALD_JPEG_BASELINE 0
#define CALD_JPEG_GPU_EXTENDED 1
#define CALD_JPEG_HOST_ONLY 2
/* host-only header parse: image size and component count */
int cald_jpeg_info(const uint8_t* data, size_t size, int* H, int* W, int* ncomp);
/* decodes n JPEG files (host bytes) into caller-allocated device images out_dev[i] = uint8 [H][W][3] (RGB) */
int cald_jpeg_decode_batch(cald_ctx* ctx, int n, const uint8_t* const* data, const size_t* sizes, uint8_t* const* out_dev);
/* host-only classification.  CALD_OK with *kind = one of CALD_JPEG_*; CALD_ERR_INVALID for bytes that are not a JPEG.
 * H, W and ncomp are filled whenever a frame header was read (also for HOST_ONLY). */
int cald_jpeg_probe(const uint8_t* data, size_t size, int* H, int* W, int* ncomp, int* kind);
/* cald_jpeg_decode_batch for BASELINE and GPU_EXTENDED files mixed in one call; CALD_ERR_UNSUPPORTED (naming the image
 * index) for a HOST_ONLY file.  A batch of BASELINE files runs exactly the launches of cald_jpeg_decode_batch. */
int cald_jpeg_decode_batch_any(cald_ctx* ctx, int n, const uint8_t* const* data, const size_t* sizes, uint8_t* const* out_dev);
/* CPU restatement: decodes one BASELINE or GPU_EXTENDED file into host memory [H][W][3] by driving the kernels' own
 * __host__ __device__ functions from plain loops.  Needs no GPU. */
int cald_jpeg_decode_host(const uint8_t* data, size_t size, uint8_t* out_host);

/* ---- measurement: HIP-event timing of every conv/linear launch on the context stream ---- */
int cald_profile_enable(cald_ctx* ctx, int on);
/* gemm_flops = algorithmic FLOPs of the timed launches; the RoI-head layers (fc6 / fc7 / predictor) are counted on the
 * MEASURED proposal rows (device-side count after RPN NMS), not on the row capacity */
int cald_profile_read(cald_ctx* ctx, double* gemm_ms, double* gemm_flops, int64_t* gemm_launches, double* total_ms);
/* the exact sweep's certified RPN pruning: time and algorithmic FLOPs of its split-fp16 look-ahead launches
 * (NOT part of cald_profile_read's figures, which then count the exact kernels only, the gathered launches on their selected rows) and
 * the fraction of P2 / P3 pixels whose head was recomputed exactly; worst_bound_ratio = the largest |look-ahead - exact| / bound any sweep of
 * this context has observed on the anchors evaluated both ways (every sweep checks it and repeats itself with the dense head if it exceeds 1);
 * pruned_flops = the dense head's exact FLOPs that were not executed */
int cald_profile_prune(cald_ctx* ctx, double* lookahead_ms, double* lookahead_flops, double* selected_fraction_p2_p3, double* worst_bound_ratio,
                       double* pruned_flops);
/* sweeps of this context that were repeated with the dense head (bound exceeded, or an activation outside the look-ahead's range) */
int cald_profile_prune_fallbacks(cald_ctx* ctx, int64_t* n);
/* cut_out reuse for one model: -1 = the process default (on unless CALD_CUTOUT_REUSE=0), 0 = off, 1 = on, 2 = on with every reused stage
 * run dense over the retained tensors (test hook).  Returns the previous setting in *was. */
int cald_model_set_cutout_reuse(cald_model* m, int mode, int* was);
/* the certified pruning's look-ahead for one model: 0 = two launches (the split-fp16 3 x 3 conv writes the hidden tensor, the exact 1 x 1 head
 * reads it), 1 = one launch wherever conv_h4 takes the look-ahead by its own rule, its epilogue evaluating the three objectness logits with the
 * exact head's fma chain (default; same bits, the hidden tensor is never written), 2 = one launch wherever conv_h4 can run at all (test hook
 * for small views).  Returns the previous setting in *was. */
int cald_model_set_look_fuse(cald_model* m, int mode, int* was);
/* packed row tiles of the dense conv_p4 launches of one model's forwards: -1 = the process default (on unless
 * CALD_CONV_PACK=0), 0 = every view is tiled on its own (each view ends with a partly empty 128-row tile), 1 = the tiles cover the level's
 * flat row space across view ends.  Same bits either way.  Returns the previous setting in *was. */
int cald_model_set_row_packing(cald_model* m, int mode, int* was);
/* torchvision's stock remove_small_boxes in the Faster R-CNN tail: with min_size > 0, candidates above the score threshold whose clipped
 * width or height is < min_size are dropped before NMS (and before batched_nms takes its maximum coordinate).  Default 0: the tail of
 * detection/frcnn_la.py, which has no such step.  The decision-margin audit does not cover it (cald_sweep_audit: CALD_ERR_UNSUPPORTED).
 * Returns the previous value in *was (may be null). */
int cald_model_set_box_min_size(cald_model* m, float min_size, float* was);
/* cut_out reuse of the exact sweeps (CALD_CUTOUT_REUSE=0 disables it): per reused stage (layer1..layer3) the conv output rows the cut_out
 * forwards computed and the rows the dense stages would have (summed over the stage's convs), the batches that reused the reference
 * forward, and the batches whose cut_out views ran dense for want of retention memory.  Accumulated over the context's life. */
int cald_profile_cutout(cald_ctx* ctx, double* rows3, double* dense_rows3, int64_t* batches, int64_t* fallbacks);
/* the same per stage of the cut_out forward -- layer1, layer2, layer3, layer4, the FPN laterals, the FPN output convs (layer4 and the
 * laterals run dense) -- with the 128-row tiles issued and the dense stage's; kept3: the batches whose reference forward retained the
 * three stages and the FPN outputs, the three stages only (the extended slot was refused), nothing (the cut_out views ran dense). */
int cald_profile_cutout_stages(cald_ctx* ctx, double* rows6, double* dense_rows6, double* tiles6, double* dense_tiles6, int64_t* kept3);
/* test hook: an extended retention slot (three stages + FPN outputs) above `bytes` counts as refused, so the sweep falls back to the
 * three-stage retention (0 = no cap, the default).  Returns the previous value in *was (may be null). */
int cald_model_set_cutout_retention_cap(cald_model* m, int64_t bytes, int64_t* was);
/* test hook: a sweep batch's cut_out forward on its own.  The views without their rectangles run as the reference forward (retaining what
 * the model's cut_out reuse mode retains), then the views as given (no flip, no noise) as the cut_out forward over it; with the reuse off,
 * a plain dense forward.  prune != 0: both take the certified pruning's path.  `out` and cald_debug_tensor show the cut_out forward. */
int cald_debug_cutout_forward(cald_model* m, int n_views, const cald_view* views, const cald_dets* out, int prune);
/* mean proposals per view (R of SURVEY 8d) over the Faster R-CNN forwards profiled since cald_profile_enable */
int cald_profile_roi_rows(cald_ctx* ctx, double* mean_rows_per_view, int64_t* views);
/* per-launch CSV (shape, algorithmic GFLOP, ms, TFLOP/s) of the launches recorded since cald_profile_enable */
int cald_profile_dump(cald_ctx* ctx, const char* path);

/* ---- training step: the device operators behind task_model(images, targets) / losses.backward() /
 * optimizer.step() of cald_train.py:40-74 (detection/engine.py:19-61), which the reference delegates to torchvision 0.8.2 +
 * cuDNN autograd.  cald_amd/train.py strings them into the Faster R-CNN training graph.  All pointers are DEVICE pointers,
 * activations are dense NHWC batches [N][H][W][C], every call is asynchronous on the context stream EXCEPT cald_train_anchors and
 * cald_train_rpn_proposals, which stage small host tables (base anchors, proposal counts) and synchronise the context stream before
 * they return (cald_train_preprocess sends its view descriptors through a pinned staging ring and does not wait).
 * Threading: the cald_train_* entry points share one process-wide cache of batch-geometry tables; they are NOT thread-safe, not even across
 * contexts -- call them from one thread per process (one process per GPU is the model everywhere in this library). ---- */
/* size in floats of the packed form of a torch-layout weight [Cout][Cin][KH][KW] (see cald_train_pack_conv) */
int cald_train_packed_floats(int Cout, int Cin, int KH, int KW, int CinK, int mode, int64_t* floats_out);
/* packs weight (+ optional bias / FrozenBatchNorm scale, shift: [Cout]) for the MFMA conv kernels, on the device.
 *   mode 0  forward over an input whose channel stride is CinK >= Cin (multiple of 4; extra channels must be zero or finite)
 *   mode 1  data gradient: the flipped, transposed filter applied to dY with channel stride CinK >= Cout; bn_scale (or null) is
 *           folded in (row co times bn_scale[co]): dY is then the gradient wrt the FrozenBatchNorm output
 *   mode 2  linear layer on rows laid out [tap][Cin] whose torch weight is [Cout][Cin * taps] (box_head.fc6 on RoIAlign rows)
 *   mode 3  data gradient of a mode-2 layer (dY rows with channel stride CinK >= Cout -> rows laid out [tap][Cin]) */
int cald_train_pack_conv(cald_ctx* ctx, const float* weight, const float* bias, const float* bn_scale, const float* bn_shift,
                         int Cout, int Cin, int KH, int KW, int CinK, int mode, float* packed);
/* The forward of a forward_precision "f16x3" trainer runs on the split-fp16 kernels of CALD_PRECISION_F16X3 (conv_h3 / conv_h4); the
 * backward stays the exact fp32 one.  A forward pack (mode 0 or 2) then has a split twin w16, [Kpad/16][2 (hi, lo)][CoutPad][16] fp16 with
 * hi = fp16(w * 2^S), lo = fp16(w * 2^S - hi): byte for byte what cald_model_finalize packs for an inference model at the same S.
 *   cald_train_packed16_bytes  size of the twin; 0 for a shape those kernels do not take (such a layer runs the exact kernels)
 *   cald_train_f16x3_scale     finalize's scale policy from max |w|: S = 14 - exponent, clamped to +-40, 0 for an all-zero or
 *                              non-finite tensor; unscale = 2^-(S + 4), what cald_train_conv_f16x3 takes
 *   cald_train_pack_conv16     cald_train_pack_conv that also writes the twin, in the same launches
 * S is the caller's: the kernels take the unscale by value, so a step cannot derive it from the device without stopping the host. */
int cald_train_packed16_bytes(int Cout, int Cin, int KH, int KW, int CinK, int mode, int64_t* bytes_out);
int cald_train_f16x3_scale(float max_abs, int* S_out, float* unscale_out);
int cald_train_pack_conv16(cald_ctx* ctx, const float* weight, const float* bias, const float* bn_scale, const float* bn_shift,
                           int Cout, int Cin, int KH, int KW, int CinK, int mode, float* packed, void* w16, int S);
/* Every trainable layer's packs in two launches: the optimizer step changes all weights at once (cald_train.py:62-64), and one
 * cald_train_pack_conv per layer and form is ~220 launch-bound launches at the start of every step.  A plan records the jobs (the
 * arguments of cald_train_pack_conv, device pointers that stay valid for the plan's lifetime); cald_train_pack_plan_run packs them
 * all on the context stream, bit for bit what the per-layer calls write.  scratch: device memory of
 * cald_train_pack_plan_scratch_floats floats owned by the plan until it is destroyed (zeroed by create on ctx's stream: run the
 * plan on that stream, or on one ordered after it). */
typedef struct cald_pack_job {
    const float *weight, *bias, *bn_scale, *bn_shift;
    int Cout, Cin, KH, KW, CinK, mode;
    float* packed;
    void* w16;      /* optional split-fp16 twin of the pack (cald_train_pack_conv16; a data-gradient pack's: see cald_train_conv_dgrad_f16x3), or null */
    int w16_S;      /* its weight scale 2^S */
} cald_pack_job;
typedef struct cald_pack_plan cald_pack_plan;
int cald_train_pack_plan_scratch_floats(int n, const cald_pack_job* jobs, int64_t* floats_out);
int cald_train_pack_plan_create(cald_ctx* ctx, int n, const cald_pack_job* jobs, float* scratch, int64_t scratch_floats, cald_pack_plan** plan_out);
int cald_train_pack_plan_run(cald_ctx* ctx, const cald_pack_plan* plan);
int cald_train_pack_plan_destroy(cald_pack_plan* plan);
/* out[N][Ho][Wo][out_ld] = epilogue(conv(in[N][H][W][CinK], packed)); flags: 1 bias, 2 scale/shift, 4 ReLU; residual (same
 * shape as out) and up ([N][Hup][Wup][Cout], nearest-upsampled) are added before the ReLU.  With mode 1 the call computes the
 * data gradient of a stride-1 conv (pad = K - 1 - forward pad); Cout / Cin are always those of the FORWARD weight.  mask (or
 * null; same shape as out): out = mask > 0 ? out : 0 at the very end -- the ReLU backward of the layer whose saved output it is. */
int cald_train_conv(cald_ctx* ctx, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                    int KH, int KW, int stride, int pad, int mode, int flags, const float* residual, const float* up,
                    int Hup, int Wup, const float* mask, float* out, int out_ld);
/* cald_train_conv of ONE layer shape on n tensors in one launch (pyramid levels under shared-weight heads; packed[i] may differ per
 * problem as long as the shape is the same).  hw = {H_0, W_0, ...}; no residual / upsample inputs.  n <= 10. */
int cald_train_conv_group(cald_ctx* ctx, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                          int Cout, int Cin, int KH, int KW, int stride, int pad, int mode, int flags, const float* const* masks,
                          float* const* outs, int out_ld);
/* The two calls above with the split twin of a forward pack: w16 / w16_unscale (or null: the exact kernels, as above) send the launch to
 * conv_h3 / conv_h4 where they take it and to the exact kernels where they refuse.  Activations may carry split twins (h16.h's layout, 4
 * bytes per element like the fp32 tensor; they need w16, Cout % 16 == 0 and out_ld == Cout): in16 = the input's, out16 = one the launch
 * writes beside out, ex16 != 0 = residual / up POINT AT the split twin of that tensor -- the epilogue then adds the 22-bit value an
 * inference model of CALD_PRECISION_F16X3 adds.  Data-gradient packs and mask take no w16.  kernel / kernels (or null) receive the name
 * of the kernel that took the launch / each problem (static strings). */
int cald_train_conv_f16x3(cald_ctx* ctx, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                          int KH, int KW, int stride, int pad, int mode, int flags, const float* residual, const float* up,
                          int Hup, int Wup, const float* mask, float* out, int out_ld, const void* w16, float w16_unscale,
                          const void* in16, int ex16, void* out16, const char** kernel);
int cald_train_conv_group_f16x3(cald_ctx* ctx, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                                int Cout, int Cin, int KH, int KW, int stride, int pad, int mode, int flags, const float* const* masks,
                                float* const* outs, int out_ld, const void* const* w16, const float* w16_unscale,
                                const void* const* in16, const char** kernels);
/* The data gradients of a backward_precision "f16x3" trainer on conv_h3: a data-gradient pack (mode 1 or 3) whose data gradient -- a
 * stride-1 conv over CinK channels of dY -- is a shape conv_h3 takes has a split twin too (cald_train_packed_grad16_bytes > 0; written by
 * cald_train_pack_conv16 / a plan job with w16 set, in the launch that writes the fp32 pack): the split of the values the fp32 pack holds
 * (transposed, flipped, bn_scale folded in) times 2^S, S by cald_train_f16x3_scale from max |w * bn_scale|.  Gradient entries are 1e-3 ..
 * 1e-8, so the kernel stages dY at in_scale = 2^(4 + G) instead of 2^4, G per gradient tensor:
 *   cald_train_f16x3_grad_scale  the policy, host-only: max |g| = f * 2^e, f in [0.5, 1) -> G = 7 - e (max |g| * in_scale in [2^10, 2^11)),
 *                                clamped to +-60, 0 for an all-zero or non-finite tensor; in_scale = 2^(4 + G)
 * and the launch takes w16_unscale = 2^-(S + 4 + G): out is the true, unscaled fp32 gradient.  residual (or null) is added, then mask (or
 * null) applied, in the kernel's epilogue.  pad is the data gradient's own (K - 1 - forward pad), the stride 1.  A shape conv_h3 does not
 * take runs the exact kernels, which never read the twin.  A gradient that outgrew a stale G splits as (inf, -inf): non-finite outputs,
 * no error.  kernel / kernels as above. */
int cald_train_packed_grad16_bytes(int Cout, int Cin, int KH, int KW, int CinK, int mode, int64_t* bytes_out);
int cald_train_f16x3_grad_scale(float max_abs, int* G_out, float* in_scale_out);
int cald_train_conv_dgrad_f16x3(cald_ctx* ctx, int N, int H, int W, const float* in, int CinK, const float* packed, int Cout, int Cin,
                                int KH, int KW, int pad, int mode, const float* residual, const float* mask, float* out, int out_ld,
                                const void* w16, float w16_unscale, float in_scale, const char** kernel);
int cald_train_conv_dgrad_group_f16x3(cald_ctx* ctx, int n, int N, const int* hw, const float* const* ins, int CinK, const float* const* packed,
                                      int Cout, int Cin, int KH, int KW, int pad, int mode, const float* const* masks, float* const* outs,
                                      int out_ld, const void* const* w16, const float* w16_unscale, const float* in_scale, const char** kernels);
/* dw[Cout][Cin][KH][KW] (=, or += when accumulate) sum over output pixels of g[q][co] * x[q @ tap][ci]; db[Cout] likewise (or
 * null).  x [N][H][W][ldx], g [N][Ho][Wo][ldg]; Cin, ldx, ldg multiples of 4.  Deterministic (fixed-order split reduction).
 * row_scale (or null): dw[co] is multiplied by row_scale[co] -- g is then the gradient wrt the FrozenBatchNorm OUTPUT of the layer. */
int cald_train_conv_wgrad(cald_ctx* ctx, int N, int H, int W, const float* x, int Cin, int ldx, const float* g, int Cout, int ldg,
                          int KH, int KW, int stride, int pad, const float* row_scale, float* dw, float* db, int accumulate);
/* linear layer: x [R][K], g [R][ldg] -> dw [Cout][K]; taps > 1: x rows are [tap][K / taps], dw is [Cout][K / taps][taps] */
int cald_train_linear_wgrad(cald_ctx* ctx, int R, const float* x, int K, const float* g, int Cout, int ldg, int taps,
                            float* dw, float* db, int accumulate);
/* The launch plan of the two calls above, as a host-only query (nothing is launched, no context needed): cald_train_conv_wgrad /
 * cald_train_linear_wgrad launch exactly what it returns.  Q = output pixels (N * Ho * Wo; a linear layer: Q = R, N = H = 1, W = R, KH = KW
 * = 1, Cin = ldx = K, red_taps = taps); red_taps = KH * KW for a conv.  `variant`: the wgrad_kernel instantiation -- pointwise (1 x 1,
 * stride 1: both operands plain matrices), offset table (Cin % 128 == 0), general, general with 32-pixel stages (CALD_WGRAD_BK=32 only),
 * wide (a tensor of 0x7FFE0000 bytes or more: 64-bit addressing).  The pixels are cut into S splits of `chunk` (a multiple of 32; the last
 * one may be ragged), reduced in split order by `reduce`; the bias gradient sums `csplit` blocks of `rows_per_block` rows.
 * Pad channels (Cout..ldg of g, Cin..ldx of x) may hold anything finite: they are read and never reach dw / db. */
enum { CALD_WGRAD_POINTWISE = 0, CALD_WGRAD_TABLE = 1, CALD_WGRAD_GENERAL = 2, CALD_WGRAD_GENERAL32 = 3, CALD_WGRAD_WIDE = 4 };
enum { CALD_WGRAD_REDUCE_FLAT = 0, CALD_WGRAD_REDUCE_TAPS = 1 };
typedef struct cald_wgrad_plan {
    int variant, reduce;                   /* CALD_WGRAD_*, CALD_WGRAD_REDUCE_* */
    int MT, JT;                            /* 128 x 128 tiles over Cout and over KH * KW * Cin */
    long long S, chunk;                    /* splits and pixels per split */
    long long csplit, rows_per_block;      /* bias gradient: row blocks and rows per block */
    long long scratch_bytes;
    char kernel[48], reduce_kernel[32];    /* the same as names */
} cald_wgrad_plan;
int cald_train_wgrad_plan(long long Q, int N, int H, int W, int Cin, int ldx, int Cout, int ldg, int KH, int KW, int stride, int pad,
                          int red_taps, cald_wgrad_plan* out);
/* g = (act > 0 ? g : 0) * scale[c]  (ReLU backward on the layer's output + FrozenBatchNorm scale); act / scale may be null */
int cald_train_relu_bwd(cald_ctx* ctx, long long rows, int C, float* g, const float* act, const float* scale);
/* dst = a + b (b null: copy); n floats, multiple of 4 */
int cald_train_add(cald_ctx* ctx, long long n, float* dst, const float* a, const float* b);
/* scatter g [N][Ho][Wo][C] onto the stride-1 grid out [N][Hd][Wd][C] (zeros elsewhere): first step of a strided data gradient */
int cald_train_dilate(cald_ctx* ctx, int N, int Ho, int Wo, int C, int s, int Hd, int Wd, const float* g, float* out);
/* FPN top-down backward: coarse += sum of the fine pixels that nearest-upsampling reads from each coarse pixel */
int cald_train_upsample_bwd(cald_ctx* ctx, int N, int Hf, int Wf, int Hc, int Wc, int C, const float* fine, float* coarse);
/* RegionProposalNetwork.filter_proposals at training sizes (pre / post_nms_top_n <= 2048): heads[l] = [N][Hl][Wl][head_ld] with
 * channel a = objectness of anchor a (A = 3), channel 3 + 4a + j = delta j; level_hw = {H0, W0, ..., H4, W4}; image_sizes = host
 * [N][2] resized (h, w).  proposals_out [N][post_n][4] and counts_out [N] are device buffers. */
int cald_train_rpn_proposals(cald_ctx* ctx, int N, int Hp, int Wp, const int* image_sizes, const float* const* heads,
                             const int* level_hw, int head_ld, int pre_n, int post_n, float nms_thr, float min_size,
                             float* proposals_out, int* counts_out);
/* roi_heads.select_training_samples on the HOST for a whole batch (labels from Matcher results, BalancedPositiveNegativeSampler,
 * the index lists of the loss kernels): torchvision 0.8.2's RoIHeads as frcnn_la.py:198-222 builds it.  All pointers are HOST
 * pointers.  Candidate table: per image slots[i] proposal rows (the first counts[i] used; counts null = all) then n_gt[i]
 * ground-truth rows, images back to back; matched = cald_train_match values per table row; gt_labels = the images' labels back to
 * back; keys = one iid uniform draw per table row (the k smallest of a class are kept: every k-subset equally likely).  Outputs
 * (capacity N * batch): table row, ground-truth row (sum n_gt = the extra zero box of images without boxes), label, image index per
 * sampled RoI in (image, table row) order; pos_rows / pred_idx (row * pred_ld + num_classes + 4 * label) of the foreground RoIs;
 * per_image_out[N] (may be null) = RoIs sampled per image. */
int cald_train_roi_sample_host(int N, const int* slots, const int* n_gt, const int* counts, const int32_t* matched,
                               const int64_t* gt_labels, const double* keys, int batch, double pos_fraction, int pred_ld, int num_classes,
                               int64_t* keep_rows, int64_t* gt_sel, int64_t* labels_out, float* img_col, int64_t* pos_rows,
                               int64_t* pred_idx, int* R_out, int* n_pos_out, int* per_image_out);
/* The device side of the RoI sampling in one launch: idx = cald_train_roi_sample_host's six output lists uploaded with stride cap
 * (table rows | ground-truth rows | labels | pred_idx | pos_rows | image index as float32); table = the candidate boxes [rows][4],
 * gts = all ground-truth boxes + one zero box.  rois_out [R][5] (image index, box) for cald_train_roi_align; box_tgt_out [n_pos][4] =
 * BoxCoder.encode of the foreground rows (weights wx..wh), the arithmetic of cald_train_box_encode. */
int cald_train_roi_gather(cald_ctx* ctx, const float* table, const float* gts, const int64_t* idx, int cap, int R, int n_pos,
                          float wx, float wy, float ww, float wh, float* rois_out, float* box_tgt_out);
/* AnchorGenerator: all anchors of one padded image over five levels, order (level, y, x, anchor): anchors_out [sum Hl*Wl*A][4].
 * kind 0 = Faster R-CNN (A = 3, frcnn_la.py:185-187), kind 1 = RetinaNet (A = 9, retinanet_cal.py:346-351) */
int cald_train_anchors(cald_ctx* ctx, int kind, int Hp, int Wp, const int* level_hw, float* anchors_out);
/* det_utils.Matcher: matched_out[i] = index of the best ground-truth box (torchvision.ops.box_iou), -1 if its IoU < lo, -2 if
 * lo <= IoU < hi; allow_low_quality restores every box that is some ground truth's best.  best_iou_out may be null. */
int cald_train_match(cald_ctx* ctx, int n_boxes, const float* boxes, int n_gt, const float* gt, float hi, float lo,
                     int allow_low_quality, int* matched_out, float* best_iou_out);
/* det_utils.BoxCoder.encode_single */
int cald_train_box_encode(cald_ctx* ctx, int n, const float* reference, const float* proposals, float wx, float wy, float ww,
                          float wh, float* out);
/* MultiScaleRoIAlign(7, sampling_ratio 2) over four dense levels feats[l] = [N][Hl][Wl][C]; rois [R][5] = (image, x1, y1, x2,
 * y2); out [R][49][C].  _bwd scatters gout into gfeats[l] = [N][Hl][Wl][C] (+=): deterministic -- the contributions are summed as
 * 64-bit fixed-point integers (scale from max|gout|), so the arrival order of the atomics does not matter. */
int cald_train_roi_align(cald_ctx* ctx, const float* const* feats, const int* level_hw, int C, int R, const float* rois, float* out);
int cald_train_roi_align_bwd(cald_ctx* ctx, int N, float* const* gfeats, const int* level_hw, int C, int R, const float* rois,
                             const float* gout);
/* F.cross_entropy over R rows of stride ld (mean); grad_out (same layout, may be null) = gscale * d loss / d logits */
int cald_train_softmax_ce(cald_ctx* ctx, int R, int C, int ld, const float* logits, const int64_t* labels, float gscale,
                          float* loss_out, float* grad_out);
/* det_utils.smooth_l1_loss(size_average=False) / denom over n 4-vectors starting at float offsets idx[i] of pred; beta = 0 is the L1
 * loss; weights (one per 4-vector, or null) scale each term; grad (zeroed by the caller, same offsets) may be null */
int cald_train_smooth_l1(cald_ctx* ctx, int n, const float* pred, const int64_t* idx, const float* target, float beta, float denom,
                         const float* weights, float gscale, float* loss_out, float* grad);
/* RetinaNet classification loss (retinanet_cal.py:100-133): sigmoid focal loss (gamma 2) summed over the anchors not between the
 * matcher thresholds, weighted per image by img_weight[n] = 1 / (max(1, #foreground) * N).  logits / grad: five level blocks
 * [N][level_pix[l]][ld] back to back, channel a * K + k; matched [N][sum level_pix * A] (cald_train_match values);
 * gt_labels[gt_off[n] + m] = class index (0-based logit column) of image n's ground-truth box m. */
int cald_train_focal_loss(cald_ctx* ctx, int N, const int* level_pix, int A, int K, int ld, const float* logits, const int* matched,
                          const int64_t* gt_labels, const int* gt_off, const float* img_weight, float alpha, float gscale,
                          float* loss_out, float* grad);
/* F.binary_cross_entropy_with_logits over n logits at float offsets idx[i] (mean) */
int cald_train_bce_logits(cald_ctx* ctx, int n, const float* logits, const int64_t* idx, const float* labels, float gscale,
                          float* loss_out, float* grad);
/* The three losses above per IMAGE (frcnn_ll.py:29-64, :243-276): N <= 64 segments, segment i = rows / gathered entries
 * [seg_off[i], seg_off[i + 1]) (seg_off: HOST, N + 1 non-decreasing entries), loss_out [N], image i's gradient scaled by gscale[i] (DEVICE,
 * N floats; null = 1).  One workgroup per image with the single-segment kernel's thread-strided sum, so N = 1 returns that kernel's bits.
 * Segments are the TRUE per-image sample counts; the reference's view(len(labels), -1, C) presumes equal counts, where the two agree.
 * softmax_ce: mean over the image's rows.  smooth_l1: sum / denom[i] (denom: HOST, N floats > 0); an empty segment gives 0 and no
 * gradient.  bce_logits: mean over the image's entries.  An empty cross-entropy / BCE segment gives loss 0. */
int cald_train_softmax_ce_seg(cald_ctx* ctx, int N, const int* seg_off, int C, int ld, const float* logits, const int64_t* labels,
                              const float* gscale, float* loss_out, float* grad_out);
int cald_train_smooth_l1_seg(cald_ctx* ctx, int N, const int* seg_off, const float* pred, const int64_t* idx, const float* target, float beta,
                             const float* denom, const float* gscale, float* loss_out, float* grad);
int cald_train_bce_logits_seg(cald_ctx* ctx, int N, const int* seg_off, const float* logits, const int64_t* idx, const float* labels,
                              const float* gscale, float* loss_out, float* grad);
/* cald_train_focal_loss per IMAGE (retina_ll.py:100-132), same logit layout and target rule: loss_out[n] = (sum of image n's raw terms)
 * / denom[n] with one IEEE division (denom: HOST, N floats > 0, normally max(1, #foreground)); grad = d term * (gscale[n] / denom[n])
 * (gscale: DEVICE, N floats; null = 1).  An ignored anchor's gradient words are not written (the caller zeroes grad); the pad columns
 * A * K .. ld - 1 are neither read nor written.  N <= 64.  No workgroup covers two images and no atomics are used: the results repeat bit
 * for bit, and image n's loss and gradient are those of the same image submitted alone.  mean_out (1 float, may be null) =
 * (((l_0 + l_1) + ...) + l_{N-1}) / (float)N; cald_train_seg_mean is that sum alone, for any per-image loss vector. */
int cald_train_focal_loss_seg(cald_ctx* ctx, int N, const int* level_pix, int A, int K, int ld, const float* logits, const int* matched,
                              const int64_t* gt_labels, const int* gt_off, const float* denom, float alpha, const float* gscale,
                              float* loss_out, float* mean_out, float* grad);
int cald_train_seg_mean(cald_ctx* ctx, int N, const float* losses, float* mean_out);
/* dst[n][p][c] = (a[n][p][c] + b[n][p][c]) + g[n * g_stride + c] / (float)HW: the join of two gradient maps [N][HW][C] (C a multiple of 4)
 * with the gradient of a global average pooling of the same map (IEEE division), in one pass */
int cald_train_add_bcast(cald_ctx* ctx, int N, long long HW, int C, float* dst, const float* a, const float* b, const float* g,
                         long long g_stride);
/* GeneralizedRCNNTransform of a training batch: images[i] = device uint8 [H_i][W_i][3]; hw = host {H_i, W_i, Hr_i, Wr_i} per image
 * (source and resized sizes); remainders[i] (or null) = device float [3][H_i][W_i] added to image / 255.  out [N][Hp][Wp][4]:
 * normalized, bilinearly resized, zero-padded; channel 3 is zero. */
int cald_train_preprocess(cald_ctx* ctx, int N, const uint8_t* const* images, const float* const* remainders, const int* hw,
                          int Hp, int Wp, float* out);
/* max_pool2d(3, 2, 1) and max_pool2d(1, 2, 0) on [N][H][W][C] */
int cald_train_maxpool(cald_ctx* ctx, int N, int H, int W, int C, const float* in, float* out);
int cald_train_subsample2(cald_ctx* ctx, int N, int H, int W, int C, const float* in, float* out);
/* torch.optim.SGD step over a flat buffer: d = grad + wd * p; buf = first_step ? d : momentum * buf + d; p -= lr * buf */
int cald_train_sgd(cald_ctx* ctx, long long n, float* param, const float* grad, float* momentum_buf, float lr, float momentum,
                   float weight_decay, int first_step);
/* ---- multi-GPU: the sweep's one collective.  Replaces detection/utils.py:75-115 (`all_gather`: pickle, pad to the longest
 * rank, gather) and :302-324 (`init_distributed_mode`, NCCL process group).  One process per GPU; RCCL is bound at first use
 * (dlopen librccl.so.1), the single-GPU path never touches it.
 *   rank 0:      cald_comm_unique_id(id)  -> ship the 128 bytes to every rank by any means (file, socket, the host's own launcher)
 *   every rank:  cald_comm_init_rank(ctx, id, world, rank, &comm)       (or cald_comm_adopt() around an ncclComm_t the host owns)
 *   every rank:  cald_allgather_scores(comm, send_dev, recv_dev, rows_per_rank, row_len)   -- rows of float64, device buffers;
 *                recv_dev [world * rows_per_rank][row_len], rank r's rows at r * rows_per_rank.  Asynchronous on the context's stream.
 * With the strided shard (rank r scores pool positions p % world == r, padded to ceil(pool / world) rows) row j of rank r IS pool
 * position r + j * world: no index column and no padding protocol travel. */
typedef struct cald_comm cald_comm;
int cald_comm_unique_id(void* id128_out);
int cald_comm_init_rank(cald_ctx* ctx, const void* id128, int world_size, int rank, cald_comm** out);
int cald_comm_adopt(cald_ctx* ctx, void* rccl_comm, cald_comm** out);
int cald_comm_info(const cald_comm* comm, int* world_size, int* rank);
int cald_comm_destroy(cald_comm* comm);
int cald_allgather_scores(cald_comm* comm, const double* send_dev, double* recv_dev, int64_t rows_per_rank, int row_len);

/* Number of dense-batch geometry tables the training operators keep cached on the device (all contexts).  The cache is bounded
 * (1024 tables, CALD_SEG_CACHE_CAP overrides); it is emptied between operator calls, never inside one.  Diagnostic. */
int cald_train_seg_cache_size(void);

#ifdef __cplusplus
}
#endif
#endif
