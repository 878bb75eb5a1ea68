// host.h -- what the host files of the C ABI (ctx.hip, ops.hip, eval.hip, model.hip, forward.hip, cutout_reuse.hip, sweep.hip, lossnet.hip, vaal.hip) share: the
// context and the model behind the opaque handles of include/cald_hip.h, a forward's request (FwdRequest), the cut_out reuse planner (CutPlanner), and the host
// functions that cross a file boundary.  Host-only, and included by those nine alone: the train_*.hip files (train_host.h), jpeg.hip and comm.hip reach the context through ctx.hip's cald_internal_* accessors.
#pragma once
#include "../../include/cald_hip.h"
#include "common.h"
#include "kernels.h"
#include "host_logic.h"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

// Everything but the two handle types lives in this namespace, so the library's cald_* symbols stay the C ABI plus cald_internal_*.
namespace cald_host {
int fail(int code, const char* fmt, ...);      // ctx.hip: sets the thread's cald_last_error() text, returns `code`
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(CALD_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

struct PilCoef { int ksize; int* d_bounds; int* d_kk; };
struct PilKey { int in, out, fid; bool operator<(const PilKey& o) const { return in != o.in ? in < o.in : (out != o.out ? out < o.out : fid < o.fid); } };
// one timed launch of the event profile (prof_begin / prof_end)
struct ProfLaunch {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double flops = 0.0;
    int tag = 0;            // 0: the model's own arithmetic; 1: the split-fp16 look-ahead pass of rpn_prune.hip (booked apart)
    std::string desc;
};
}  // namespace cald_host
using namespace cald_host;      // the host files work inside it

#define CALD_PRUNE_LOG 4096     // profiled forwards whose selected-pixel counts are kept per forward (cald_profile_dump)
struct cald_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    char* arena = nullptr; size_t arena_cap = 0, arena_off = 0;
    BatchPlan* d_plan = nullptr;
    ViewDesc* d_views = nullptr;
    float* d_zeros = nullptr;
    // pinned host staging ring for the per-forward plan + view descriptors (keeps the source of the
    // stream-ordered H2D copies alive without a host sync)
    static const int NSTAGE = 8;
    char* h_stage[NSTAGE] = {nullptr}; hipEvent_t stage_ev[NSTAGE] = {nullptr}; int stage_i = 0;
    bool prof = false;
    std::vector<ProfLaunch> prof_launches;
    double prof_flops = 0.0; int64_t prof_extra_launches = 0;
    int prof_tag_now = 0;                           // set around the look-ahead launches of rpn_prune.hip (per context: ADVICE r5)
    double prof_prune_flops_cap[2] = {0.0, 0.0};    // FLOPs the gathered P2 / P3 launches are booked with (every pixel, once per selection stage; rescaled to the selected rows at read time)
    hipEvent_t tot0 = nullptr, tot1 = nullptr; bool tot_open = false; double tot_ms = 0.0;
    // RoI-head GEMMs run on a device-side row count (proposals after NMS): the profile counts their algorithmic FLOPs on the
    // MEASURED rows, accumulated on the device while profiling (no host sync inside a forward)
    float prune_worst = 0.0f;                     // largest ratio any sweep of this context has seen (cald_profile_prune)
    long long prune_fallbacks = 0;                // sweeps repeated with the dense head (bound exceeded / activation outside the split's range)
    float* d_prune_check = nullptr;               // rpn_prune.hip: running max of |look-ahead - exact| / bound (reset by every sweep call)
    unsigned long long* d_prune_stat = nullptr;   // rpn_prune.hip: selected / total pixels of P2, P3 while profiling
    // per profiled forward [sel P2, total P2, sel P3, total P3]: lets cald_profile_dump book each gathered launch on the rows it really computed
    unsigned long long* d_prune_log = nullptr; int prune_log_n = 0;
    struct GatherNote { int log; double cap[2]; };
    std::map<size_t, GatherNote> prof_gather;     // launch index -> which log slot, and the FLOPs its P2 / P3 problems would cost on every pixel
    unsigned long long* d_roi_rows = nullptr; double prof_roi_rows_cap = 0.0, prof_roi_flops_cap = 0.0; long long prof_roi_views = 0;
    std::map<PilKey, PilCoef> pil;
    char* train_scratch = nullptr; size_t train_scratch_cap = 0;   // cald_internal_scratch: the training operators' scratch (train_wgrad.hip: split-K partial tiles of the weight gradients)
    // cut_out reuse (cald_profile_cutout): per reused stage the conv output rows the cut_out forwards computed and what the dense forwards
    // would have; batches whose cut_out views reused the reference forward, batches that could not (the retention did not fit)
    double cut_rows[3] = {0.0, 0.0, 0.0}, cut_dense[3] = {0.0, 0.0, 0.0};
    long long cut_batches = 0, cut_fallbacks = 0;
    // the same per stage of the cut_out forward (cald_profile_cutout_stages; CUT_STAGE_*: layer1..layer4, FPN laterals, FPN output convs): rows
    // computed, rows of the dense stage, 128-row tiles issued and the dense stage's; batches by retention (CUT_KEPT_*)
    double cut_st_rows[6] = {}, cut_st_dense[6] = {}, cut_st_tiles[6] = {}, cut_st_dense_tiles[6] = {};
    long long cut_kept[3] = {0, 0, 0};
};

namespace cald_host {
// device scratch that lives for one API call: everything is released when the call returns, on every path
struct ScopedDev {
    std::vector<void*> ptrs;
    hipStream_t st;
    explicit ScopedDev(hipStream_t s) : st(s) {}
    ~ScopedDev() { if (!ptrs.empty()) { hipStreamSynchronize(st); for (void* p : ptrs) hipFree(p); } }
    void release() { ptrs.clear(); }      // the caller keeps what was allocated so far
    template <typename T> int alloc(T** out, size_t bytes) {
        HIPCHK(hipMalloc((void**)out, bytes ? bytes : 1));
        ptrs.push_back((void*)*out);
        return 0;
    }
    template <typename T> int upload(T** out, const void* h, size_t bytes) {      // device copy of a host array (null stays null)
        *out = nullptr;
        if (!h) return 0;
        if (int rc = alloc(out, bytes)) return rc;
        HIPCHK(hipMemcpy((void*)*out, h, bytes, hipMemcpyHostToDevice));
        return 0;
    }
};
struct Bump {
    char* base; size_t off = 0; bool dry;
    explicit Bump(char* b, bool d) : base(b), dry(d) {}
    template <typename T> T* get(size_t count) {
        size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        T* p = dry ? nullptr : reinterpret_cast<T*>(base + off);
        off += bytes;
        return p;
    }
};

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };
struct ConvLayer {
    float *w = nullptr, *w4 = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr;
    float* wstem = nullptr;                              // conv_stem.hip packing (the 7 x 7 / 2, 3 -> 64 stem only)
    uint16_t* w16 = nullptr; float w16_unscale = 1.0f;   // CALD_PRECISION_F16X3 only
    int Cin = 0, Cout = 0, CoutPad = 0, K = 0, Kpad = 0, KH = 1, KW = 1, stride = 1, pad = 0;
    int CinTrue = 0;   // un-padded input channels (algorithmic FLOP accounting)
};
struct Bottleneck { ConvLayer c1, c2, c3, down; bool has_down = false; bool layer_end = false; };
struct DebugEntry { const float* ptr; int level; int C; int kind; };  // kind 0: level tensor, 1: roi rows [cap][C]
}  // namespace cald_host

struct cald_model {
    cald_ctx* ctx = nullptr;
    cald_model_cfg cfg;
    std::map<std::string, HostTensor> sd;
    bool finalized = false;
    ConvLayer conv1; std::vector<Bottleneck> blocks;
    ConvLayer fpn_inner[4], fpn_layer[4], rpn_conv, rpn_head, fc6, fc7, pred;
    // certified RPN pruning of the exact sweep (rpn_prune.hip): the 3 x 3 RPN conv once more with split-fp16 weights, the bound's constants
    ConvLayer rpn_conv16; bool prune = false; float prune_c1[3] = {0, 0, 0}, prune_c0[3] = {0, 0, 0};
    bool prune_allowed = false;     // finalize's verdict: the look-ahead layer exists and the bound's constants are finite (cald_model_set_rpn_prune* AND it in)
    // the look-ahead's 1 x 1 objectness head in conv_h4.hip's epilogue (cald_model_set_look_fuse): 0 off (two launches), 1 where conv_h4 takes the
    // look-ahead launch by its own rule, 2 wherever conv_h4 is correct (test hook for small views); the head's first three channels [3][256] + bias
    int look_fuse = 1; float* look_head_w = nullptr; float look_head_b[3] = {0, 0, 0};
    int row_packing = -1;           // cald_model_set_row_packing: -1 the process default (conv_pack_default), 0 per-view row tiles, 1 packed row tiles
    bool prune_bound_voided = false;   // test hook cald_model_set_rpn_prune_bound replaced finalize's constants: the sweeps' ratios are not the certificate's
    bool prune_capture = false;     // test hook: cald_forward takes the pruned path too and keeps the look-ahead's logit map (cald_model_set_rpn_prune_capture)
    ConvLayer p6, p7, cls_tower[4], reg_tower[4], cls_out, reg_out;   // RetinaNet
    int det_cap() const { return cfg.arch == CALD_ARCH_RETINANET ? cfg.num_classes * cfg.detections_per_img : cfg.detections_per_img; }
    float* d_anchors = nullptr;
    std::vector<void*> owned;
    std::map<std::string, DebugEntry> dbg;
    BatchPlan plan; int last_V = 0;
    // CALD_PRECISION_F16X3: activation tensors that also (or only) exist in conv_h3.hip's split form (ConvArgs::in16 / out16), keyed by
    // the fp32 buffer of the running forward.  fp32_dead: every consumer is a conv_h3 layer -- the fp32 tensor is not written at all
    // and the split words live in the same buffer.
    struct SplitFmt { unsigned* s16; bool fp32_dead; };
    std::map<const float*, SplitFmt> split;
    std::vector<ViewDesc> last_views;
    // batch-level detection buffers used by the sweeps (cald_sweep alternates between the two sets: batch k + 1's reference forward
    // is in flight while batch k's views are being scored)
    DetBuffers sweep_det; int sweep_det_views = 0;
    DetBuffers sweep_det2; int sweep_det2_views = 0;
    // cald_sweep's scratch lives with the model, grown on demand, never freed between calls (round 3 allocated and freed six device
    // buffers per call -- each hipFree an implicit device synchronisation -- and copied through pageable host memory)
    struct SweepScratch {
        size_t dev_bytes = 0, pin_bytes = 0, aug_cap = 0;
        char* dev = nullptr; char* pin = nullptr; uint8_t* d_aug = nullptr;
        hipEvent_t ev_ref[2] = {nullptr, nullptr}, ev_score[2] = {nullptr, nullptr};
    } ss;
    float box_min_size = 0.0f;   // cald_model_set_box_min_size: stock remove_small_boxes in the ordinary tail (0 = off, frcnn_la.py)
    int key_cap = 32768;   // FRCNN candidate (proposal, class) list capacity per view, sized from box_score_thresh at create
    // cut_out reuse (cutout_reuse.hip CutPlanner): the reference forward's block outputs of the first three stages, one slot per batch parity (batch k + 1's
    // reference forward runs before batch k's cut_out forward), and the gather plans of the cut_out forwards (pinned by parity + device)
    struct CutReuse {
        int mode = -1;              // cald_model_set_cutout_reuse: -1 the process default (CALD_CUTOUT_REUSE), 0 off, 1 on, 2 on with every stage dense
        char* slot[2] = {nullptr, nullptr}; size_t cap[2] = {0, 0};
        bool ext_refused = false;   // the extended slot (+ the FPN outputs) could not be allocated once: later batches keep the three stages only
        size_t ext_cap = 0;         // test hook cald_model_set_cutout_retention_cap: an extended slot above this many bytes counts as refused (0: no cap)
        char* h_gp[2] = {nullptr, nullptr}; char* d_gp = nullptr;
    } cr;
};

namespace cald_host {
// Every weight packing the conv kernels read (model.hip pack_conv)
struct ConvPack {
    std::vector<float> w, w4, wstem;
    std::vector<uint16_t> w16; float w16_unscale = 1.0f;
    int Cout = 0, CoutPad = 0, K = 0, Kpad = 0;
};
// independent convolutions (bias / BN / ReLU epilogue only) issued as ONE launch when they fit the same tiled kernel (forward.hip conv_group_on)
struct ConvSpec { const ConvLayer* L; const float* in; float* out; int level; bool relu; const int* dyn = nullptr; const int* row_map = nullptr; const unsigned* in16 = nullptr;
                  unsigned* out16 = nullptr; float* energy4 = nullptr; };      // out16 / energy4: conv_p4.hip's pruning extras (P2 / P3 of the FPN output convs)

// ---- cut_out reuse: the cut_out views of a sweep batch run as a forward of their own, in the reference forward's image order (same plan),
// and their first three stages recompute only the pixels the filled rectangles reach (host_logic.h cut_geometry), patching the reference
// forward's retained block outputs in place ----
#define CUT_MAX_BLOCKS 36          // blocks of the backbone (ResNet-101: 3 + 4 + 23 + 3); the first three stages are retained and gathered
#define CUT_STAGE_LATERAL 4
#define CUT_STAGE_OUTPUT 5
#define CUT_KEPT_FPN 0             // cut_kept[]: batches that retained the three stages and the FPN outputs, the three stages only, nothing
#define CUT_KEPT_STAGES 1
#define CUT_KEPT_NONE 2
struct FwdReuse {
    int mode = 0;                  // 1: reference forward, the block outputs of the first nblk blocks go to out[]; 2: the cut_out forward
    int nblk = 0;
    float* out[CUT_MAX_BLOCKS] = {};
    // mode 2: per stage gathered launches or dense ones (also written over out[]); the device gather plan (cut_plan_set_bytes): per block b and
    // set k (0: the block output's dirty set -- downsample conv, conv2, conv3; 1: conv1's compute set) LevelSeg[V + 1] (the level's
    // geometry, tile_start counting the set's tiles) then GatherSet[V]
    bool gather[3] = {false, false, false};
    const char* d_gp = nullptr;
    int tiles[CUT_MAX_BLOCKS][2] = {};
    double rows[CUT_MAX_BLOCKS][2] = {};
    // the FPN output convs (Faster R-CNN, P2..P5): retained as well -- mode 1 writes them (and, under the certified pruning, P2 / P3's split
    // copy and energy) to pf[] / p16[] / energy[], mode 2 patches them on the output dirty sets: gather sets 2 nblk + i of the plan, as ONE
    // grouped gathered launch (gather_fpn), or runs the dense group over them
    bool fpn = false, gather_fpn = false;
    float* pf[4] = {}; unsigned* p16[2] = {}; float* energy[2] = {};
    int fpn_tiles[4] = {};
    double fpn_rows[4] = {};
};
// ---- features-only forward (the learning-loss sweep, lossnet.hip): the forward stops after the FPN -- Faster R-CNN after the grouped output
// convs (P2..P5), RetinaNet after P6 (P3..P6; P7 too when p7 is set) ----
struct FwdFeatures {
    const int (*pad_to)[2] = nullptr;   // per view {Hp, Wp}, multiples of 32 and >= the view's own padded size, which they replace (null: the view's own).
                                        // Hr / Wr stay the view's own; the area beyond the resized image is zero
    bool p7 = false;
    // filled by forward_model, per pyramid index: the level tensor in the arena (valid until the context's next forward), whether it exists in
    // split form only (h16.h), and its level in the plan
    const float* P[5] = {}; bool split_only[5] = {}; int plan_level[5] = {};
};
// ---- the tail stages that the forward (forward.hip ForwardRun) and the hooks cald_op_roi_align / _frcnn_postprocess / _retina_postprocess (ops.hip) both run:
// the stage's scratch, laid out from the sizes alone, and the filler of its kernel arguments.  `plan` / `views` are device pointers. ----
struct ProposalBufs { float* proposals = nullptr; int* prop_count = nullptr; void layout(Bump& B, int V); };   // RPN -> RoIAlign, post-processing: CALD_ROI_CAP rows a view
struct RoiBufs { float* roi = nullptr; int* order = nullptr; void layout(Bump& B, int V, int C); };
struct PostBufs {
    float *prob = nullptr, *pmax = nullptr, *cbox = nullptr; unsigned long long* keys = nullptr; int* key_count = nullptr; int key_cap = 0;
    unsigned char* skip = nullptr;      // remove_small_boxes marks (PostArgs::skip)
    void layout(Bump& B, int V, int C, int key_cap);
};
// what either SSM tail leaves on the device for the host to collect (ssm_collect_rows): per view al and count, the batch's total, its rows
struct SsmRows { const int *al, *count, *total; const float *boxes, *scores; const signed char* labels; };
// the SSM tail (ssm.hip): scratch and results of V views; the results hold (C - 1) * cap rows a view, the most a view can give
struct SsmBufs {
    float *prob = nullptr, *kept_box = nullptr, *boxes = nullptr, *scores = nullptr; unsigned* vmax = nullptr; signed char* labels = nullptr;
    int *kept_prop = nullptr, *cls_count = nullptr, *row_off = nullptr, *al = nullptr, *count = nullptr, *total = nullptr;
    void layout(Bump& B, int V, int C, int cap);
    SsmRows rows() const { return {al, count, total, boxes, scores, labels}; }
};
// ---- the SSM forward (cald_sweep_ssm): Faster R-CNN up to the box predictor, then ssm_postprocess() in place of postprocess().  Filled by
// forward_model: the tail's buffers in the arena (valid until the context's next forward) ----
struct FwdSsm { SsmBufs out; };
#define SSM_NMS_THR 0.3f     // frcnn_ssm.py:88
#define SSM_CONF_THR 0.5f    // frcnn_ssm.py:60 CONF_THRESH
struct RetinaTailBufs {
    int *cand_count = nullptr, *kept_anchor = nullptr, *kept_count = nullptr, cand_cap = 0, max_anchors = 0; unsigned long long* cand_key = nullptr;
    float *cand_box = nullptr, *kept_box = nullptr; unsigned char* cand_skip = nullptr;
    void layout(Bump& B, int V, int K, int per_class, int max_anchors);      // max_anchors: the largest anchor count of a view
};
// the SSM tail of RetinaNet (retina_ssm.hip): scratch and results of V views; the results hold K * per_class rows a view
struct RetinaSsmBufs {
    int *cand_count = nullptr, *blk_off = nullptr, *list = nullptr, *al = nullptr, *picks = nullptr, *n_picks = nullptr, *kept_anchor = nullptr, *kept_count = nullptr,
        *row_off = nullptr, *count = nullptr, *total = nullptr, cand_cap = 0, nblk = 0;
    unsigned* vmax = nullptr; float *kept_box = nullptr, *boxes = nullptr, *scores = nullptr; signed char* labels = nullptr;
    void layout(Bump& B, int V, int K, int per_class, int max_anchors);      // max_anchors: the largest anchor count of a view
    SsmRows rows() const { return {al, count, total, boxes, scores, labels}; }
};
// ---- the SSM forward of RetinaNet (cald_sweep_ssm_retina): the heads, then phase A, the host stop (`pick` once per image with al == 0;
// image = image0 + view) and phase B in place of the stock tail.  Filled by forward_model: the tail's buffers in the arena (valid until the
// context's next forward) ----
struct FwdRetinaSsm { cald_ssm_pick_fn pick = nullptr; void* user = nullptr; int image0 = 0; RetinaSsmBufs out; };
// ---- what one forward is run for: ONE tail, and only what that tail reads.  STOCK: the detections into stock.det (+ the decision-margin
// records of audit_out, the certified pruning where the model has it and prune_ok allows it, the cut_out reuse of `ru`); FEATURES / SSM /
// RETINA_SSM: the struct above of that name, which forward_model fills.  What a maker's argument points to outlives the call. ----
struct FwdRequest {
    enum Tail { STOCK, FEATURES, SSM, RETINA_SSM } tail;
    struct Stock { DetBuffers det; float* audit_out; bool prune_ok; const FwdReuse* ru; };
    union { Stock stock; FwdFeatures* feat; FwdSsm* ssm; FwdRetinaSsm* rssm; };
    static FwdRequest detect(const DetBuffers& det, bool prune_ok = false, const FwdReuse* ru = nullptr) { FwdRequest r; r.tail = STOCK; r.stock = Stock{det, nullptr, prune_ok, ru}; return r; }
    FwdRequest audited(float* out) const { FwdRequest r = *this; r.stock.audit_out = out; return r; }      // a stock request with the audit's records (null: none)
    static FwdRequest features(FwdFeatures* f) { FwdRequest r; r.tail = FEATURES; r.feat = f; return r; }
    static FwdRequest ssm_tail(FwdSsm* s) { FwdRequest r; r.tail = SSM; r.ssm = s; return r; }
    static FwdRequest retina_ssm_tail(FwdRetinaSsm* s) { FwdRequest r; r.tail = RETINA_SSM; r.rssm = s; return r; }
};
// ---- the cut_out reuse planner (cutout_reuse.hip) of one run over model m: which blocks are retained and gathered, the retention slot of a
// reference forward (one per batch parity, grown on demand) and the gather plan of the cut_out forward over it.  Books the context's cut_*
// counters (cald_profile_cutout / _stages). ----
struct CutPlanner {
    CutPlanner() {}                                     // off, until a run builds its own
    CutPlanner(cald_model* m, bool prune_ok);           // the block tables of m
    void enable(bool has_cutout, bool audit);           // is the reuse on for this model?  The caller's own terms: the run has a cut_out augmentation, and it is no audit
    // the retention slot `parity` for a reference forward of nb views, and `ru` over it: returns what the forward retains (CUT_KEPT_*), or an error
    int retain(int parity, int nb, const ViewDesc* views, FwdReuse& ru);
    // gather plan of the cut_out forward (V views in the reference forward's order) over slot `parity` into the pinned set `parity`, one H2D, and `ru`
    int cut_plan(int parity, bool kept_fpn, int V, const ViewDesc* views, FwdReuse& ru);
private:
    cald_model* m = nullptr; bool prune_ok = false, retina = false;
    bool on = false;        // enable()'s verdict: off, every retain() keeps nothing and books nothing
    // blocks of the first three stages (retained and gathered)
    int nblk = 0, blk_lin[CUT_MAX_BLOCKS], blk_lout[CUT_MAX_BLOCKS], blk_stage[CUT_MAX_BLOCKS], blk_stride[CUT_MAX_BLOCKS];
    // the whole backbone for the geometry (ngeo >= nblk blocks, geo_stride = conv2's strides; the first nblk are blk_stride) and the blocks
    // whose outputs are C2..C5; fpn_ok: Faster R-CNN with four stages -- the FPN output convs can be retained and patched
    int ngeo = 0, geo_stride[CUT_MAX_BLOCKS], c_blk[4] = {0, 0, 0, 0};
    bool fpn_ok = false;
    BatchPlan rplan;        // the plan of the views at hand (plan_of)
    void plan_of(int nv, const ViewDesc* vs);
    size_t retain_layout(int nv, bool fpn, char* base, FwdReuse* ru) const;
};
RetinaSsmArgs retina_ssm_args(const RetinaSsmBufs& S, const float* const* cls, const float* const* reg, const BatchPlan* plan, const ViewDesc* views,
                              const float* base_anchors, int A, int K, int V, float score_thr, float nms_thr, int per_class);
// the host stop between the two phases: waits for phase A, reads al and the counts, asks `pick` for every view with al == 0 (in view order),
// checks every answer and uploads the picks.  h_counts (optional) receives the counts [V][K]
int retina_ssm_pick_stop(cald_ctx* c, const RetinaSsmBufs& S, int V, int K, cald_ssm_pick_fn pick, void* user, int image0, int* h_counts);
RoiArgs roi_args(const RoiBufs& S, const float* const* feat, const BatchPlan* plan, int C, int V, const ProposalBufs& P, bool out16);
PostArgs post_args(const PostBufs& S, const float* pred, int pred_ld, int C, int V, const ProposalBufs& P, const ViewDesc* views,
                   float score_thr, float nms_thr, const DetBuffers& det);
SsmArgs ssm_args(const SsmBufs& S, const float* pred, int pred_ld, int C, int V, const ProposalBufs& P, const ViewDesc* views, float score_thr, int cap);
RetinaArgs retina_args(const RetinaTailBufs& S, const float* const* cls, const float* const* reg, const BatchPlan* plan, const ViewDesc* views,
                       const float* base_anchors, int A, int K, int V, float score_thr, float nms_thr, int per_class, const DetBuffers& det);
inline size_t cut_plan_set_bytes(int V) { return (size_t)(V + 1) * sizeof(LevelSeg) + (size_t)V * sizeof(GatherSet); }
inline long long level_pix(const BatchPlan& P, int l, int V) { return P.seg[l][V].pix_off; }

// ctx.hip
int arena_reserve(cald_ctx* c, size_t bytes);
int prof_begin(cald_ctx* c, ProfLaunch& t);                                                  // no-ops while the profile is off
int prof_end(cald_ctx* c, ProfLaunch& t, double flops, int tag, const char* fmt, ...);
int conv_refused(const ConvArgs& a);
int run_conv(cald_ctx* c, const ConvArgs& a, double flops);
// ops.hip
int pil_resize(cald_ctx* c, const uint8_t* src, int H, int W, uint8_t* dst, int oh, int ow, uint8_t* tmp, int fid = 0);
// model.hip
std::vector<float> pack_w4(const std::vector<float>& w, int Kpad, int CoutPad);
void pack_conv(const std::vector<const float*>& ts, const std::vector<int>& couts, int cin, int cinp, int kh, int kw, int stride, int pad,
               bool want16, ConvPack* P);
// forward.hip
void build_plan(BatchPlan& P, int V, const ViewDesc* views, const int (*hp)[2], bool retina);
bool stem_grid_exact(const LevelSeg* seg, int V);
bool conv_pack_default();       // packed row tiles (ConvArgs::packed_rows) in the dense conv_p4 launches: on unless CALD_CONV_PACK=0
int forward_model(cald_model* m, int V, ViewDesc* views, const FwdRequest& rq);
// the caller's output buffers as DetBuffers of C classes; every one must be there
inline int dets_from_abi(const cald_dets* abi, int C, DetBuffers* det) {
    if (!abi || !abi->boxes_dev || !abi->scores_dev || !abi->labels_dev || !abi->props_dev || !abi->prob_max_dev || !abi->scores_cls_dev || !abi->count_dev)
        return fail(CALD_ERR_INVALID, "output buffers must all be provided");
    *det = DetBuffers{abi->boxes_dev, abi->scores_dev, (long long*)abi->labels_dev, abi->props_dev, abi->prob_max_dev, abi->scores_cls_dev, abi->count_dev, abi->cap, C};
    return 0;
}
// sweep.hip
void free_det(DetBuffers& d);
int alloc_det(DetBuffers& d, int V, int cap, int C);
// detection buffers that live for one API call
struct ScopedDet { DetBuffers d{}; ~ScopedDet() { free_det(d); } int alloc(int V, int cap, int C) { return alloc_det(d, V, cap, C); } };
// the untouched view of one image, and the reference views of images [i0, i0 + nb)
inline ViewDesc plain_view(const uint8_t* src, int H, int W) { ViewDesc d; memset(&d, 0, sizeof(d)); d.src = src; d.H = H; d.W = W; return d; }
inline std::vector<ViewDesc> ref_views(const uint8_t* const* images_dev, const int* H, const int* W, int i0, int nb) {
    std::vector<ViewDesc> views(nb);
    for (int i = 0; i < nb; i++) views[i] = plain_view(images_dev[i0 + i], H[i0 + i], W[i0 + i]);
    return views;
}
// images per batch of a sweep: the caller's request, `dflt` where it gives none, CALD_MAX_VIEWS at the most
inline int sweep_batch(int requested, int dflt) { const int B = requested > 0 ? requested : dflt; return B > CALD_MAX_VIEWS ? CALD_MAX_VIEWS : B; }
// The rows of one batch of an SSM tail (V views): drains the stream, reads al and count of every view into al_out / count_out [V] and the
// batch's total into *total_out, checks them (a view has 0..view_rows rows, none with al set; the counts add up to the total), and copies the
// rows to row `row0` of boxes_out / scores_out [score_cols] / labels_out [label_cols] where row0 + total <= rows_cap.  hook: the one-view
// hooks of ops.hip word the refusal in their own way (null: the sweeps' words, naming image image0 + view)
int ssm_collect_rows(hipStream_t st, const char* hook, int image0, const SsmRows& R, int V, size_t score_cols, size_t label_cols, int64_t view_rows,
                     int64_t row0, int64_t rows_cap, int* al_out, int* count_out, float* boxes_out, float* scores_out, int8_t* labels_out, int* total_out);
// ---- the scoring stage's tables, shared by the sweeps (sweep.hip) and the hook cald_op_score_batch (ops.hip) ----
// The `ints` block of a scoring stage, the same words on the host and on the device: per pair ref_view | aug_view | aug_kind | pair_img
// (P_MAX each), ref_sel [B][50], ref_n [B], then per view view_img | view_isref (VT each; VT = 0: no per-view tail -- ls_c has no cls_corr).
struct PairLayout {
    int P_MAX, B, VT;
    struct Ptrs { int *ref_view, *aug_view, *aug_kind, *pair_img, *ref_sel, *ref_n, *view_img, *view_isref; };
    size_t n_ints() const { return (size_t)P_MAX * 4 + (size_t)B * 51 + (size_t)VT * 2; }
    Ptrs at(int* base) const {
        Ptrs p;
        p.ref_view = base; p.aug_view = p.ref_view + P_MAX; p.aug_kind = p.aug_view + P_MAX; p.pair_img = p.aug_kind + P_MAX;
        p.ref_sel = p.pair_img + P_MAX; p.ref_n = p.ref_sel + (size_t)B * 50; p.view_img = p.ref_n + B; p.view_isref = p.view_img + VT;
        return p;
    }
    // the scoring kernels' arguments over the device copy of the block
    ScoreArgs score_args(int* d_base, const DetBuffers& D, const float* d_par, int P, float bp, float* cons) const {
        const Ptrs p = at(d_base);
        ScoreArgs sa; sa.det = D;
        sa.ref_view = p.ref_view; sa.aug_view = p.aug_view; sa.aug_kind = p.aug_kind; sa.pair_img = p.pair_img;
        sa.ref_sel = p.ref_sel; sa.ref_n = p.ref_n; sa.aug_param = d_par; sa.P = P; sa.bp = bp; sa.cons = cons;
        return sa;
    }
};
}  // namespace cald_host
