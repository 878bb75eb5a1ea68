// train_geom.hip -- the two per-context host tables of the training operators: the dense-batch geometry cache (N equal views of H x W as
// LevelSeg[N + 1] on the device, keyed by (context, N, H, W): torchvision pads a training batch to one common size,
// GeneralizedRCNNTransform.batch_images) with its deferred eviction, and the pinned staging ring.  cald_train_seg_cache_size,
// cald_internal_train_release.
#include "train_host.h"
#include <map>
#include <mutex>
#include <tuple>

static std::mutex g_seg_stage_mu;      // guards the geometry cache (g_seg, g_seg_evict) and the staging ring (g_stage)
static std::map<std::tuple<cald_ctx*, int, int, int>, LevelSeg*> g_seg;
static bool g_seg_evict = false;      // the cache went over its bound: empty it at the NEXT entry point, never inside one
static size_t seg_cache_cap() {       // CALD_SEG_CACHE_CAP: tests lower it to exercise the eviction
    static const size_t cap = [] { const char* e = getenv("CALD_SEG_CACHE_CAP"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 1024); }();
    return cap;
}
// A public entry point takes several tables from consecutive dense_seg() calls (input / output / up-sampling geometry, s0 plus five
// pyramid levels, ...) before it launches anything, so a table must never be freed while an entry point is running: dense_seg() only
// flags the overflow (the cache then exceeds its bound by the few tables of one call), and the NEXT entry point that uses tables
// empties the cache first thing -- after the launches that may still read the old tables have drained; a rare, synchronous event.
int cald_train_host::seg_entry() {
    std::lock_guard<std::mutex> lk(g_seg_stage_mu);
    if (!g_seg_evict) return 0;
    THIP(hipDeviceSynchronize());
    for (auto& kv : g_seg) hipFree(kv.second);
    g_seg.clear();
    g_seg_evict = false;
    return 0;
}
int cald_train_host::dense_seg(cald_ctx* c, int N, int H, int W, const LevelSeg** out) {
    std::lock_guard<std::mutex> lk(g_seg_stage_mu);
    auto key = std::make_tuple(c, N, H, W);
    auto it = g_seg.find(key);
    if (it == g_seg.end()) {
        if (g_seg.size() >= seg_cache_cap()) g_seg_evict = true;   // a long run over variable padded sizes x pyramid levels x contexts
        std::vector<LevelSeg> h(N + 1);
        const int tiles = (H * W + 127) / 128;
        for (int v = 0; v <= N; v++) { h[v].pix_off = (long long)v * H * W; h[v].H = H; h[v].W = W; h[v].tile_start = v * tiles; h[v].pad_ = 0; }
        LevelSeg* d = nullptr;
        THIP(hipMalloc((void**)&d, sizeof(LevelSeg) * (N + 1)));
        THIP(hipMemcpy(d, h.data(), sizeof(LevelSeg) * (N + 1), hipMemcpyHostToDevice));
        it = g_seg.emplace(key, d).first;
    }
    *out = it->second;
    return 0;
}

// Small host tables on their way to the device without stopping the host: a ring of pinned slots + device slots per context.  A slot
// is reused only after the stream has passed the event recorded behind its last consumer (in practice never waited for).
struct StageRing { char* host; char* dev; hipEvent_t ev[8]; bool used[8]; int next; };
static std::map<cald_ctx*, StageRing> g_stage;
int cald_train_host::stage_upload(cald_ctx* c, const void* src, size_t bytes, hipStream_t st, const void** dev_out, int* slot_out) {
    if (bytes > kStageSlot) TFAIL(CALD_ERR_INVALID, "staging slot too small");
    std::lock_guard<std::mutex> lk(g_seg_stage_mu);
    auto it = g_stage.find(c);
    if (it == g_stage.end()) {
        StageRing r; memset(&r, 0, sizeof(r));
        THIP(hipHostMalloc((void**)&r.host, kStageSlot * 8, hipHostMallocDefault));
        THIP(hipMalloc((void**)&r.dev, kStageSlot * 8));
        for (int i = 0; i < 8; i++) THIP(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming));
        it = g_stage.emplace(c, r).first;
    }
    StageRing& r = it->second;
    const int s = r.next; r.next = (s + 1) & 7;
    if (r.used[s]) THIP(hipEventSynchronize(r.ev[s]));
    memcpy(r.host + kStageSlot * s, src, bytes);
    THIP(hipMemcpyAsync(r.dev + kStageSlot * s, r.host + kStageSlot * s, bytes, hipMemcpyHostToDevice, st));
    *dev_out = r.dev + kStageSlot * s; *slot_out = s;
    return 0;
}
int cald_train_host::stage_consumed(cald_ctx* c, int slot, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_seg_stage_mu);
    StageRing& r = g_stage[c];
    THIP(hipEventRecord(r.ev[slot], st));
    r.used[slot] = true;
    return 0;
}

extern "C" int cald_train_seg_cache_size(void) { std::lock_guard<std::mutex> lk(g_seg_stage_mu); return (int)g_seg.size(); }
void cald_internal_train_release(cald_ctx* c) {
    std::lock_guard<std::mutex> lk(g_seg_stage_mu);
    for (auto it = g_seg.begin(); it != g_seg.end();) {
        if (std::get<0>(it->first) == c) { hipFree(it->second); it = g_seg.erase(it); } else ++it;
    }
    auto sr = g_stage.find(c);
    if (sr != g_stage.end()) {
        for (int i = 0; i < 8; i++) hipEventDestroy(sr->second.ev[i]);
        hipHostFree(sr->second.host); hipFree(sr->second.dev);
        g_stage.erase(sr);
    }
}
