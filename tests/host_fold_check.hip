// Stand-alone check of the pure-host pieces the sweeps share (cald_amd/csrc/host.h): sweep_batch and dets_from_abi's refusals.  Built as a
// program of its own, with the host sanitizers, by tests/test_cpu_host.py; calls nothing of the HIP runtime.  Exit 0: every check held.
#include "../cald_amd/csrc/host.h"

static int n_failed = 0;
static char last_text[256];
int cald_host::fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(last_text, sizeof(last_text), fmt, ap); va_end(ap);
    return code;
}
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); n_failed++; } } while (0)

int main() {
    // sweep_batch: the default for a request <= 0, the cap above CALD_MAX_VIEWS, the request otherwise
    for (int dflt : {32, 64}) {
        for (int r : {0, -1, INT_MIN}) CHECK(sweep_batch(r, dflt) == dflt);
        for (int r : {1, 2, dflt, CALD_MAX_VIEWS - 1, CALD_MAX_VIEWS}) CHECK(sweep_batch(r, dflt) == r);
        for (int r : {CALD_MAX_VIEWS + 1, 1000, INT_MAX}) CHECK(sweep_batch(r, dflt) == CALD_MAX_VIEWS);
    }
    CHECK(sweep_batch(0, CALD_MAX_VIEWS + 5) == CALD_MAX_VIEWS);

    // dets_from_abi: every buffer must be there; a complete set comes back field by field
    float f[4]; int64_t l[1]; int n[1];
    const cald_dets full = {f, f + 1, l, f + 2, f + 3, f, n, 7};
    DetBuffers d; memset(&d, 0, sizeof(d));
    last_text[0] = 0;
    CHECK(dets_from_abi(&full, 21, &d) == 0 && last_text[0] == 0);
    CHECK(d.boxes == f && d.scores == f + 1 && d.labels == (long long*)l && d.props == f + 2 && d.prob_max == f + 3 && d.scores_cls == f && d.count == n);
    CHECK(d.cap == 7 && d.C == 21);
    CHECK(dets_from_abi(nullptr, 21, &d) == CALD_ERR_INVALID);
    for (int hole = 0; hole < 7; hole++) {
        cald_dets a = full;
        if (hole == 0) a.boxes_dev = nullptr; else if (hole == 1) a.scores_dev = nullptr; else if (hole == 2) a.labels_dev = nullptr;
        else if (hole == 3) a.props_dev = nullptr; else if (hole == 4) a.prob_max_dev = nullptr; else if (hole == 5) a.scores_cls_dev = nullptr;
        else a.count_dev = nullptr;
        DetBuffers e; memset(&e, 0, sizeof(e));
        last_text[0] = 0;
        CHECK(dets_from_abi(&a, 21, &e) == CALD_ERR_INVALID);
        CHECK(strcmp(last_text, "output buffers must all be provided") == 0);
        CHECK(e.boxes == nullptr && e.count == nullptr && e.cap == 0);      // a refusal writes nothing
    }
    printf(n_failed ? "%d checks failed\n" : "ok\n", n_failed);
    return n_failed ? 1 : 0;
}
