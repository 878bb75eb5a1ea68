"""CPU restatement of the learning-loss sweep's arithmetic, numpy float32, for tests/test_ll_sweep.py and tests/test_gpu_ll_sweep.py.

Written from the stated order, not from the kernels, and sharing no code with the product:

pooling, per channel, N = H * W pixels in row-major order
  - chunks of 256 consecutive pixels (the last may be short);
  - inside a chunk, phase q = p mod 4 summed sequentially in increasing p from +0;
  - chunk sum (s0 + s1) + (s2 + s3); chunk sums added sequentially in increasing chunk index from +0;
  - mean = sum / float32(N).
LossNet (the contract of oracle.linear): FC_i = one k-ordered fmaf chain from +0 over the 256 pooled values, + bias, ReLU; the output one fmaf
chain over the 4 D values in torch.cat order, + bias.

The a-priori bound against float64 is the running-error bound of the longest chain: pooling gamma_d * mean|x_c| with d = 64 + 2 + n_chunks + 1,
carried through the two linear layers with gamma_257 and gamma_513 and the absolute weights.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24


def gamma(d):
    return d * U / (1.0 - d * U)


def fma32(a, b, c):
    """Correctly rounded float32 a * b + c, elementwise.  The product of two float32 is exact in float64; the float64 sum is made
    round-to-odd (TwoSum gives its error exactly), after which the rounding to float32 is the rounding of the exact value."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0.0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


def gap(x):
    """x: [H][W][C] or [N][C] float32 -> the pooled vector [C] float32 in the stated order."""
    x = np.ascontiguousarray(x, F32)
    C = x.shape[-1]
    x = x.reshape(-1, C)
    N = x.shape[0]
    nch = (N + 255) // 256
    pad = np.zeros((nch * 256, C), F32)          # +0 beyond the last pixel: x + (+0) is x for every x an accumulator that started at +0 can hold
    pad[:N] = x
    pad = pad.reshape(nch, 64, 4, C)
    ph = np.zeros((nch, 4, C), F32)
    for i in range(64):
        ph = (ph + pad[:, i]).astype(F32)
    cs = ((ph[:, 0] + ph[:, 1]).astype(F32) + (ph[:, 2] + ph[:, 3]).astype(F32)).astype(F32)
    tot = np.zeros(C, F32)
    for k in range(nch):
        tot = (tot + cs[k]).astype(F32)
    return (tot / F32(N)).astype(F32)


def gap_bound(x):
    """gamma_d * mean|x_c| per channel, d = 64 + 2 + n_chunks + 1."""
    x = np.asarray(x, np.float64).reshape(-1, x.shape[-1])
    nch = (x.shape[0] + 255) // 256
    return gamma(64 + 2 + nch + 1) * np.abs(x).mean(axis=0)


def gap64(x):
    x = np.asarray(x, np.float64)
    return x.reshape(-1, x.shape[-1]).mean(axis=0)


def _chain(x, w):
    """x [n][K], w [D][K] -> [n][D]: one k-ordered fmaf chain from +0 per output."""
    x = np.ascontiguousarray(x, F32); w = np.ascontiguousarray(w, F32)
    acc = np.zeros((x.shape[0], w.shape[0]), F32)
    for k in range(x.shape[1]):
        acc = fma32(x[:, k:k + 1], w[None, :, k], acc)
    return acc


def lossnet(sd, pooled):
    """sd: LossNet's state dict as float32 arrays; pooled [n][4][256] float32 -> [n] float32."""
    pooled = np.ascontiguousarray(pooled, F32)
    hs = []
    for j in range(4):
        h = (_chain(pooled[:, j], sd["FC%d.weight" % (j + 1)]) + np.asarray(sd["FC%d.bias" % (j + 1)], F32)[None]).astype(F32)
        hs.append(np.where(h > 0, h, F32(0)).astype(F32))
    cat = np.concatenate(hs, axis=1)
    return (_chain(cat, sd["linear.weight"])[:, 0] + F32(np.asarray(sd["linear.bias"], F32)[0])).astype(F32)


def lossnet64(sd, pooled):
    """float64 evaluation on float64 pooled vectors [n][4][256]; returns (out [n], hidden [n][4 D])."""
    pooled = np.asarray(pooled, np.float64)
    hs = [np.maximum(pooled[:, j] @ np.asarray(sd["FC%d.weight" % (j + 1)], np.float64).T + np.asarray(sd["FC%d.bias" % (j + 1)], np.float64), 0.0)
          for j in range(4)]
    cat = np.concatenate(hs, axis=1)
    return cat @ np.asarray(sd["linear.weight"], np.float64)[0] + float(np.asarray(sd["linear.bias"])[0]), cat


def lossnet_bound(sd, pooled64, pooled_err):
    """Bound on |float32 result - float64 result| per image: the pooled vectors' own error bound pooled_err [n][4][256] carried through
    |W|, plus gamma_257 on each FC chain (256 products and the bias add) and gamma_513 on the output chain; ReLU is 1-Lipschitz."""
    pooled64 = np.abs(np.asarray(pooled64, np.float64)); pooled_err = np.asarray(pooled_err, np.float64)
    eh, hm = [], []
    for j in range(4):
        aw = np.abs(np.asarray(sd["FC%d.weight" % (j + 1)], np.float64)); ab = np.abs(np.asarray(sd["FC%d.bias" % (j + 1)], np.float64))
        mag = (pooled64[:, j] + pooled_err[:, j]) @ aw.T + ab
        eh.append(pooled_err[:, j] @ aw.T + gamma(257) * mag)
        hm.append(mag)
    eh = np.concatenate(eh, axis=1); hm = np.concatenate(hm, axis=1)
    al = np.abs(np.asarray(sd["linear.weight"], np.float64)[0]); alb = abs(float(np.asarray(sd["linear.bias"])[0]))
    return eh @ al + gamma(513) * ((hm + eh) @ al + alb)


def score_features(sd, feats, levels):
    """feats: per pyramid level a list of per-image [H][W][256] float32 maps; levels: pyramid index per LossNet branch.
    Returns (scores [n] float32, pooled [n][4][256] float32)."""
    n = len(feats[0])
    pooled = np.stack([np.stack([gap(feats[l][i]) for l in levels]) for i in range(n)])
    return lossnet(sd, pooled), pooled


def score_features64(sd, feats, levels):
    """float64 evaluation and the a-priori bound of the float32 one: (scores [n], bound [n])."""
    n = len(feats[0])
    p64 = np.stack([np.stack([gap64(feats[l][i]) for l in levels]) for i in range(n)])
    pe = np.stack([np.stack([gap_bound(feats[l][i]) for l in levels]) for i in range(n)])
    out, _ = lossnet64(sd, p64)
    return out, lossnet_bound(sd, p64, pe)
