"""The decisions of the certified RPN pruning (cald_amd/csrc/rpn_prune.hip) in plain numpy: no radix select, no bit mask, no scan.

Keys are sorted; selected pixels are np.flatnonzero of a boolean map.  Every value the kernels compute is a short, fixed sequence of
float32 operations (the library is built with -ffp-contract=off; sqrt and division are correctly rounded on both sides), so each one is
restated operation by operation on numpy float32 scalars / arrays and compared BIT FOR BIT by tests/test_gpu_rpn_prune_edges.py.

A case is a dict: V, hw [2][V] of (H, W), pre_n, ld, c1[3], c0[3], check[2] (initial), and per level l energy[l] [pix][4],
look[l] [pix][ld] (the look-ahead's map), exact[l] [pix][ld] (the dense exact map); views are consecutive in every per-pixel array.
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
RANGE = F32(4094.0)


def orderable(x):
    """det_orderable (common.h): larger float -> larger uint32, -0.0 and +0.0 folded, +NaN above +inf."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).copy()
    u[(u & np.uint32(0x7FFFFFFF)) == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def patch_norm(en, H, W):
    """(float32 in the kernel's order, float64 without the 1.0001) of one view's [H * W][4] energies."""
    q = np.ascontiguousarray(en, F32).reshape(H, W, 4)
    with np.errstate(all="ignore"):
        t = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])                   # float32
        s = np.zeros((H, W), F32)
        s64 = np.zeros((H, W), np.float64)
        yy, xx = np.mgrid[0:H, 0:W]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y2, x2 = yy + dy, xx + dx
                ok = (y2 >= 0) & (y2 < H) & (x2 >= 0) & (x2 < W)
                nb = t[np.clip(y2, 0, H - 1), np.clip(x2, 0, W - 1)]
                s = np.where(ok, s + nb, s).astype(F32)
                s64 = s64 + np.where(ok, q.astype(np.float64).sum(axis=2)[np.clip(y2, 0, H - 1), np.clip(x2, 0, W - 1)], 0.0)
        pn = (np.sqrt(s) * F32(1.0001)).astype(F32)
    return pn.reshape(-1), np.sqrt(s64).reshape(-1)


def bound(pn, c1, c0):
    """B[p][a] = c1[a] * pn[p] + c0[a]: two float32 roundings."""
    with np.errstate(all="ignore"):
        return ((np.asarray(c1, F32)[None, :] * pn[:, None]).astype(F32) + np.asarray(c0, F32)[None, :]).astype(F32)


def kth_largest(keys, k):
    return int(np.sort(keys.reshape(-1))[::-1][k - 1])


def select_view(look3, exact3, pn, c1, c0, pre_n):
    """The two selection stages of one (level, view): look3 / exact3 [npx][3].  Returns tau, threshold of stage 1, keep0, keep1 (bool [npx])."""
    npx = look3.shape[0]; n = 3 * npx; k = min(pre_n, n)
    B = bound(pn, c1, c0)
    with np.errstate(all="ignore"):
        lb = (look3 - B).astype(F32); ub = (look3 + B).astype(F32)
    klb, kub = orderable(lb), orderable(ub)
    tau = 0 if n <= k else kth_largest(klb, k)
    keep0 = (np.isnan(lb) | (klb >= tau)).any(axis=1)
    if n <= k:
        thr = tau
    else:
        kex = orderable(exact3[keep0])
        assert kex.size >= k, "stage 0 keeps at least k anchors"
        tau2 = kth_largest(kex, k)
        thr = tau2 if tau2 > tau else tau
    keep1 = ~keep0 & (np.isnan(ub) | (kub >= thr)).any(axis=1)
    return tau, thr, keep0, keep1


def run(case):
    V, ld = case["V"], case["ld"]
    c1, c0 = np.asarray(case["c1"], F32), np.asarray(case["c0"], F32)
    out = dict(pnorm=[], pnorm64=[], head=[], row_map=[[None, None], [None, None]], tau_key=np.zeros((2, V), np.uint32), thr_key=np.zeros((2, V), np.uint32),
               nsel=np.zeros((2, 2, V), np.int32), keep=[[[], []], [[], []]], stat=np.zeros(4, np.uint64))
    chk0 = np.asarray(case["check"], F32).view(np.uint32).copy()
    worst = F32(0.0); flag = False
    for l in range(2):
        off = 0
        pnl, pn64l = [], []
        head = np.array(case["look"][l], F32, copy=True)
        exact = np.ascontiguousarray(case["exact"][l], F32)
        maps = [[], []]
        for v in range(V):
            H, W = case["hw"][l][v]; npx = H * W
            pn, pn64 = patch_norm(case["energy"][l][off:off + npx], H, W)
            pnl.append(pn); pn64l.append(pn64)
            flag = flag or bool((~(pn < RANGE)).any())
            look3 = head[off:off + npx, :3].copy(); ex = exact[off:off + npx]
            tau, thr, k0, k1 = select_view(look3, ex[:, :3], pn, c1, c0, case["pre_n"])
            out["tau_key"][l, v] = tau; out["thr_key"][l, v] = thr
            for s, keep in enumerate((k0, k1)):
                idx = np.flatnonzero(keep).astype(np.int32)
                out["nsel"][s, l, v] = idx.size; maps[s].append((off, idx)); out["keep"][s][l].append(keep)
            out["stat"][2 * l] += np.uint64(int(k0.sum() + k1.sum())); out["stat"][2 * l + 1] += np.uint64(npx)
            parked = ~k0 & ~k1
            view = head[off:off + npx]
            view[parked, :3] = -FLT_MAX
            sel = k0 | k1
            view[sel] = ex[sel]
            B = bound(pn, c1, c0)
            with np.errstate(all="ignore"):
                ratio = (np.abs((look3[sel] - ex[sel, :3]).astype(F32)) / B[sel]).astype(F32).reshape(-1)
            ratio = np.where(np.isnan(ratio), F32(np.inf), ratio)
            if ratio.size:
                worst = max(worst, F32(ratio.max()))
            off += npx
        out["pnorm"].append(np.concatenate(pnl)); out["pnorm64"].append(np.concatenate(pn64l)); out["head"].append(head)
        for s in range(2):
            out["row_map"][s][l] = maps[s]
    wb = np.array([worst], F32).view(np.uint32)[0]
    if worst > 0 and chk0[0] < wb:                   # non-negative floats order like their bit patterns
        chk0[0] = wb
    one = np.array([1.0], F32).view(np.uint32)[0]
    if flag and chk0[1] < one:
        chk0[1] = one
    out["check"] = chk0.view(F32)
    out["worst"] = worst
    return out
