// train_host.h -- what the host code of the training operators (train_*.hip, lossnet_train.hip) shares: the cald_internal_* accessors of ctx.hip
// through which these files reach the context, the error macros, and the few host functions that cross a file boundary.  Host-only: no kernel
// is referenced across translation units (the build is not RDC), a file that needs another file's kernel calls its host launcher.
//
// The training step of the detector (cald_train.py:40-74 train_one_epoch -> task_model(images, targets) /
// losses.backward() / optimizer.step(); the arithmetic the reference delegates to torchvision 0.8.2 + cuDNN/cuBLAS autograd) is an
// operator-level C ABI on device pointers; the host side that strings the operators into the training graph is cald_amd/train.py.
//   train_geom.hip         geometry tables of the dense batches, pinned staging ring
//   train_pack.hip         weights packed on the device every step
//   train_conv.hip         forward conv / linear, data gradient, input side: the inference kernels
//   train_wgrad.hip        weight gradient (MFMA GEMM over the output pixels, fixed-order split reduction)
//   train_elementwise.hip  elementwise backward passes, SGD
//   train_targets.hip      proposals, RoI sampler, matcher, anchors, box coder, RoI gather
//   train_roi.hip          RoIAlign forward and fixed-point backward
//   train_loss.hip         segmented losses, focal loss
#pragma once
#include "common.h"
#include "kernels.h"
#include "../../include/cald_hip.h"
#include <cstdlib>
#include <cstring>
#include <vector>

int cald_internal_fail(int code, const char* fmt, ...);
hipStream_t cald_internal_stream(cald_ctx* c);
int cald_internal_device(cald_ctx* c);
const float* cald_internal_zeros(cald_ctx* c);
int cald_internal_scratch(cald_ctx* c, size_t bytes, void** out);   // grow-only per-context device scratch (stream-ordered reuse)
void cald_internal_train_release(cald_ctx* c);                      // train_geom.hip: frees the context's geometry tables and staging ring

#define TFAIL(code, ...) return cald_internal_fail(code, __VA_ARGS__)
#define THIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return cald_internal_fail(CALD_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

// Everything else lives in this namespace, so the library's cald_* symbols stay the C ABI plus cald_internal_* (as host.h's cald_host).
namespace cald_train_host {
// train_geom.hip: the dense-batch geometry of N equal views of H x W, cached on the device per (context, N, H, W).  An entry point that takes
// tables opens with SEG_ENTRY() (the deferred eviction), then calls dense_seg() once per table.
int seg_entry();
#define SEG_ENTRY() do { const int rc_ = seg_entry(); if (rc_) return rc_; } while (0)
int dense_seg(cald_ctx* c, int N, int H, int W, const LevelSeg** out);
// train_geom.hip: small host tables on their way to the device without stopping the host (a ring of pinned slots + device slots per context).
// stage_consumed() goes behind the last launch that reads the slot.
const size_t kStageSlot = sizeof(ViewDesc) * CALD_MAX_VIEWS;
int stage_upload(cald_ctx* c, const void* src, size_t bytes, hipStream_t st, const void** dev_out, int* slot_out);
int stage_consumed(cald_ctx* c, int slot, hipStream_t st);

// the layout of a packed weight buffer (train_pack.hip writes it, train_conv.hip reads it): wk [Kpad][NPad] | conv_p4 layout, as large | bias,
// scale, shift [3][NPad].  mode as in cald_train_pack_conv.
struct PackGeom { int K, Kpad, NPad, n_true, cin_conv; long long floats; };
inline PackGeom pack_geom(int Cout, int Cin, int KH, int KW, int CinK, int mode) {
    PackGeom g;
    const int taps = KH * KW;
    if (mode == 2) { g.K = taps * Cin; g.n_true = Cout; g.cin_conv = taps * Cin; }
    else if (mode == 3) { g.K = CinK; g.n_true = taps * Cin; g.cin_conv = CinK; }
    else { g.K = taps * CinK; g.n_true = mode == 1 ? Cin : Cout; g.cin_conv = CinK; }
    g.Kpad = round_up(g.K, 16);
    g.NPad = cout_pad(g.n_true);
    g.floats = 2ll * g.Kpad * g.NPad + 3ll * g.NPad;
    return g;
}
// Whether conv_h3.hip / conv_h4.hip take a FORWARD launch on this pack (the geometric part of conv_h3.hip's h3_refuses, model.hip pack_conv's
// `tiled`): only such a pack has a split twin (train_pack.hip), and only such a launch may carry split activations (train_conv.hip).
// taps: KH * KW of the pack's torch weight; a mode-2 pack is applied as a 1 x 1 conv over taps * Cin channels.
inline bool h3_takes(const PackGeom& g, int taps, int mode) {
    if (mode != 0 && mode != 2) return false;
    return g.NPad % 64 == 0 && ((g.cin_conv % 16 == 0 && (mode == 2 ? 1 : taps) <= 32) || g.cin_conv == 4);
}
// Whether conv_h3.hip takes the DATA GRADIENT on this pack (modes 1 / 3: a stride-1 conv / 1 x 1 conv over cin_conv = CinK channels of dY
// with n_true = Cin (x taps) outputs): only such a pack has a split twin, only such a launch reads it (conv_h3.hip launch_conv_h3_dgrad).
inline bool h3_takes_grad(const PackGeom& g, int taps, int mode) {
    if (mode != 1 && mode != 3) return false;
    return g.NPad % 64 == 0 && g.cin_conv % 16 == 0 && (mode == 3 ? 1 : taps) <= 32;
}
inline bool p4_takes(const PackGeom& g, int taps) { return g.NPad % 64 == 0 && g.cin_conv % 16 == 0 && taps <= 32; }   // the tiled kernel (conv_p4.hip) covers the shape

// train_targets.hip: the AnchorGenerator base anchors of the five levels, base[5][A][4]; returns A (kind 0: Faster R-CNN, 3; kind 1: RetinaNet, 9)
int base_anchors_host(int kind, float* base);
// train_elementwise.hip: relu_bwd_kernel over n4 float4s of rows of C4 float4s (act / scale may be null)
void launch_relu_bwd(float* g, const float* act, const float* scale, long long n4, int C4, hipStream_t st);
}  // namespace cald_train_host
using namespace cald_train_host;      // the training files work inside it
