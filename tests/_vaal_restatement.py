"""CPU restatement of the VAAL sweep's arithmetic, numpy float32, for tests/test_vaal_sweep.py and tests/test_gpu_vaal_sweep.py, with a
float64 evaluation and an a-priori running-error bound of every stage, and the generator of the test weights.

Written from the stated orders, not from the kernels, and sharing no code with the product:

resize        source index min((dst * in) // 256, in - 1) per axis; the value is the uint8 pixel as a float.
convolution   oracle.conv2d (k-ordered fmaf chain from +0 in the contract's chain order, + bias [, * scale, + shift, ReLU]).
batch norm    train(): per (image, channel) over the N pixels in row-major order, two passes in the pooling order -- chunks of 256 pixels,
              phase q = p mod 4 summed sequentially from +0, chunk sum (s0 + s1) + (s2 + s3), chunks added sequentially from +0;
              mean = sum(x) / N; var = sum(fl(d * d)) / N with d = fl(x - mean); istd = 1 / sqrt(var + 1e-5);
              y = max(0, fl(fl(fl(d * istd) * gamma) + beta)).
              eval(): scale = gamma * (1 / sqrt(running_var + 1e-5)), shift = beta - running_mean * scale in float32, applied by the
              convolution's epilogue: fl(fl(r * scale) + shift), ReLU.
fc_mu         k' = pixel * 1024 + channel; 256 segments of 256 consecutive k', each one k'-ascending fmaf chain from +0; segment sums added
              sequentially in increasing segment index from +0; + bias.
head          three layers of k-ascending fmaf chains from +0, + bias, ReLU after the first two; 1 / (1 + exp(-x)) with the library's
              deterministic float32 exp (DESIGN.md arithmetic contract), restated below.

Bounds.  u = 2^-24, gamma(d) = d u / (1 - d u).  e denotes an elementwise bound on |float32 value - float64 value| of a stage's input.
  conv / linear with a chain of K products and a bias:  |W| e + gamma(K + 1) (|W| |x| + |b|)
  batch statistics (d = 64 + 2 + chunks + 1 roundings on a sum):
      mean   em = mean(e) + gamma(d) mean|x|                         centred  ed = e + em + u |dc|
      square es = (2 |dc| + ed) ed + u dc^2                          variance ev = mean(es) + gamma(d) mean(dc^2) + u (var + eps)
      istd   ei = 0.5 max(var + eps - ev, eps)^-1.5 ev + 3 u istd     (|d/dv (v + eps)^-1/2| at the smallest admissible argument)
      y      |g| (istd ed + (|dc| + ed) ei) + gamma(3) (|dc istd g| + |b|)
  running statistics: the folded scale carries gamma(4) |scale|, the shift |mean| times that + gamma(2) (|beta| + |mean scale|);
      y      |scale| e + |r| e_scale + e_shift + gamma(2) (|r scale| + |shift|)
  ReLU is 1-Lipschitz; sigmoid has slope <= 1/4, and its evaluation (exp to 4 u relative, one add, one division) adds 8 u.
"""
import hashlib

import numpy as np

F32 = np.float32
U = 2.0 ** -24
EPS = 1e-5
WIDTHS = (3, 64, 128, 256, 512, 1024)
MAP_PIX = (16384, 4096, 1024, 256, 64)
SIZES = (1, 2, 255, 256, 257, 333, 500, 1333)


def gamma(d):
    return d * U / (1.0 - d * U)


def fma32(a, b, c):
    """Correctly rounded float32 a * b + c, elementwise: the product of two float32 is exact in float64; the float64 sum is made
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


# ----------------------------------------------------------------------------- weights
def used_keys():
    """(key, shape) of every tensor the sweep reads, in generation order."""
    out = []
    for l in range(5):
        out += [("encoder.%d.weight" % (3 * l), (WIDTHS[l + 1], WIDTHS[l], 4, 4)), ("encoder.%d.bias" % (3 * l), (WIDTHS[l + 1],))]
        out += [("encoder.%d.%s" % (3 * l + 1, p), (WIDTHS[l + 1],)) for p in ("weight", "bias", "running_mean", "running_var")]
    out += [("fc_mu.weight", (256, 65536)), ("fc_mu.bias", (256,))]
    out += [("net.0.weight", (512, 256)), ("net.0.bias", (512,)), ("net.2.weight", (512, 512)), ("net.2.bias", (512,)),
            ("net.4.weight", (1, 512)), ("net.4.bias", (1,))]
    return out


def _grid(a, bits):
    return (np.round(np.asarray(a, np.float64) * 2.0 ** bits) / 2.0 ** bits).astype(F32)


def make_weights(seed):
    """{key: float32 array} of used_keys(), from numpy's RandomState alone, on a coarse binary grid.  Weights scale as 1 / sqrt(fan_in)
    (about 64 grid steps per standard deviation); biases, BatchNorm gamma / beta and running statistics are non-trivial; the first layer's
    running statistics sit where a convolution of raw 0..255 pixels puts them, the others where a convolution of ReLU'd normalised
    maps does."""
    rs = np.random.RandomState(seed)
    sd = {}
    for key, shape in used_keys():
        name = key.rsplit(".", 1)[1]
        bn = key.startswith("encoder.") and int(key.split(".")[1]) % 3 == 1
        first = key.startswith("encoder.1.")
        if bn and name == "weight":
            a = _grid(np.clip(1.0 + 0.2 * rs.randn(*shape), 0.4, 1.6), 6)
        elif bn and name == "bias":
            a = _grid(0.05 + 0.1 * rs.randn(*shape), 8)
        elif name == "running_mean":
            a = _grid(40.0 * rs.randn(*shape), 2) if first else _grid(0.3 * rs.randn(*shape), 8)
        elif name == "running_var":
            a = _grid(2000.0 * rs.uniform(0.5, 1.5, shape), 0) if first else _grid(rs.uniform(0.25, 0.75, shape), 8)
        elif name == "bias":
            a = _grid(0.02 + 0.1 * rs.randn(*shape), 8)
        else:
            fan = int(np.prod(shape[1:]))
            bits = int(np.ceil(np.log2(np.sqrt(fan)))) + 6
            a = _grid(rs.randn(*shape) / np.sqrt(fan), bits)
        sd[key] = np.ascontiguousarray(a, F32)
    return sd


def weights_sha1(sd):
    h = hashlib.sha1()
    for key, _ in used_keys():
        h.update(np.ascontiguousarray(sd[key], F32).tobytes())
    return h.hexdigest()


# ----------------------------------------------------------------------------- stages, float32
def resize_index(n_in):
    """Source index of each of the 256 destination positions along an axis of n_in pixels."""
    return np.minimum((np.arange(256, dtype=np.int64) * n_in) // 256, n_in - 1)


def resize(img):
    """uint8 [H][W][3] -> float32 [256][256][3]: the byte as a float."""
    img = np.asarray(img)
    return img[resize_index(img.shape[0])][:, resize_index(img.shape[1])].astype(F32)


def kmajor(w):
    """torch conv weight [Cout][Cin][KH][KW] -> oracle.conv2d's K-major [(kh, kw, cin)][Cout]"""
    w = np.asarray(w, F32)
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0]))


def ordered_sum(x):
    """x [N][C] float32 -> [C]: the sum over N in the stated chunk / phase order."""
    x = np.ascontiguousarray(x, F32)
    N, C = x.shape
    nch = (N + 255) // 256
    pad = np.zeros((nch * 256, C), F32)          # +0 beyond the last pixel: x + (+0) is x for every x an accumulator started at +0 can hold
    pad[:N] = x
    pad = pad.reshape(nch, 64, 4, C)
    ph = np.zeros((nch, 4, C), F32)
    for i in range(64):
        ph = (ph + pad[:, i]).astype(F32)
    cs = ((ph[:, 0] + ph[:, 1]).astype(F32) + (ph[:, 2] + ph[:, 3]).astype(F32)).astype(F32)
    tot = np.zeros(C, F32)
    for k in range(nch):
        tot = (tot + cs[k]).astype(F32)
    return tot


def bn_stats(x):
    """x [N][C] -> (mean, istd, centred values) in the stated two-pass order."""
    x = np.ascontiguousarray(x, F32)
    N = x.shape[0]
    mean = (ordered_sum(x) / F32(N)).astype(F32)
    dc = (x - mean[None]).astype(F32)
    var = (ordered_sum((dc * dc).astype(F32)) / F32(N)).astype(F32)
    istd = (F32(1.0) / np.sqrt((var + F32(EPS)).astype(F32)).astype(F32)).astype(F32)
    return mean, istd, dc, var


def bn_relu(x, g, b):
    """Batch-statistics BatchNorm + ReLU of one image's map x [N][C]."""
    _, istd, dc, _ = bn_stats(x)
    y = ((((dc * istd[None]).astype(F32) * np.asarray(g, F32)[None]).astype(F32)) + np.asarray(b, F32)[None]).astype(F32)
    return np.where(y > 0, y, F32(0)).astype(F32)


def folded_bn(sd, l):
    p = "encoder.%d." % (3 * l + 1)
    g, b, rm, rv = (np.asarray(sd[p + k], F32) for k in ("weight", "bias", "running_mean", "running_var"))
    scale = (g * (F32(1.0) / np.sqrt((rv + F32(EPS)).astype(F32)).astype(F32)).astype(F32)).astype(F32)
    shift = (b - (rm * scale).astype(F32)).astype(F32)
    return scale, shift


def chains(x, wt):
    """x [n][K], wt [K][D] -> [n][D]: one k-ascending fmaf chain from +0 per output."""
    x = np.ascontiguousarray(x, F32)
    acc = np.zeros((x.shape[0], wt.shape[1]), F32)
    for k in range(x.shape[1]):
        acc = fma32(x[:, k:k + 1], wt[k][None], acc)
    return acc


def fc_weight_kprime(w):
    """fc_mu.weight [256][c * 64 + p] -> [p * 1024 + c][256]"""
    return np.ascontiguousarray(np.asarray(w, F32).reshape(256, 1024, 64).transpose(2, 1, 0).reshape(65536, 256))


def fc_mu(act, wt, bias):
    """act [n][65536] in k' order, wt [65536][256] -> mu [n][256] in the stated two-level order."""
    act = np.ascontiguousarray(act, F32).reshape(-1, 256, 256)          # [n][segment][k]
    w = wt.reshape(256, 256, 256)                                         # [segment][k][j]
    acc = np.zeros((act.shape[0], 256, 256), F32)                         # [n][segment][j]
    for k in range(256):
        acc = fma32(act[:, :, k, None], w[None, :, k, :], acc)
    tot = np.zeros((act.shape[0], 256), F32)
    for s in range(256):
        tot = (tot + acc[:, s]).astype(F32)
    return (tot + np.asarray(bias, F32)[None]).astype(F32)


def det_exp(x):
    """The library's deterministic float32 exp (DESIGN.md arithmetic contract), elementwise."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.rint((x * F32(1.44269504)).astype(F32)).astype(F32)
        r = fma32(n, F32(-0.693145752), x)
        r = fma32(n, F32(-1.42860677e-6), r)
        p = np.full(x.shape, F32(1.9875691500e-4), F32)
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = fma32(p, r, F32(c))
        r2 = (r * r).astype(F32)
        y = (fma32(p, r2, r) + F32(1.0)).astype(F32)
        ni = np.where(np.isfinite(n), n, 0).astype(np.int64)
        n1 = np.where(ni >= 0, ni // 2, -((-ni) // 2))                   # C division truncates toward zero
        n2 = ni - n1
        pow2 = lambda e: np.ldexp(F32(1.0), np.clip(e, -126, 127).astype(np.int32)).astype(F32)
        y = ((y * pow2(n1)).astype(F32) * pow2(n2)).astype(F32)
        y = np.where(x > F32(88.72283), F32(np.inf), np.where(x < F32(-87.0), F32(0.0), y))
    return np.where(np.isnan(x), x, y).astype(F32)


def head_logit(sd, mu):
    h = (chains(mu, np.asarray(sd["net.0.weight"], F32).T) + np.asarray(sd["net.0.bias"], F32)[None]).astype(F32)
    h = np.where(h > 0, h, F32(0)).astype(F32)
    h = (chains(h, np.asarray(sd["net.2.weight"], F32).T) + np.asarray(sd["net.2.bias"], F32)[None]).astype(F32)
    h = np.where(h > 0, h, F32(0)).astype(F32)
    return (chains(h, np.asarray(sd["net.4.weight"], F32).T)[:, 0] + F32(np.asarray(sd["net.4.bias"], F32)[0])).astype(F32)


def sigmoid(x):
    with np.errstate(over="ignore", divide="ignore"):
        return (F32(1.0) / (F32(1.0) + det_exp((-np.asarray(x, F32)).astype(F32))).astype(F32)).astype(F32)


def head(sd, mu):
    """mu [n][256] -> preds [n]"""
    return sigmoid(head_logit(sd, np.ascontiguousarray(mu, F32)))


def encode(orc, sd, img, running, keep=None):
    """One uint8 image -> the encoder's last map [64][1024] float32 (pixel-major).  keep: optional list that receives every stage's
    convolution output and activation."""
    x = resize(img)
    for l in range(5):
        wk, b = kmajor(sd["encoder.%d.weight" % (3 * l)]), np.asarray(sd["encoder.%d.bias" % (3 * l)], F32)
        r = orc.conv2d(x, wk, 4, 4, 2, 1, bias=b)
        C = r.shape[2]
        if running:
            sc, sh = folded_bn(sd, l)
            y = ((r * sc).astype(F32) + sh).astype(F32)
            y = np.where(y > 0, y, F32(0)).astype(F32)
        else:
            y = bn_relu(r.reshape(-1, C), sd["encoder.%d.weight" % (3 * l + 1)], sd["encoder.%d.bias" % (3 * l + 1)]).reshape(r.shape)
        if keep is not None:
            keep.append((r, y))
        x = y
    return x.reshape(64, 1024)


def sweep(orc, sd, images, running, wt=None):
    """(mu [n][256], preds [n]) float32 of uint8 images."""
    wt = fc_weight_kprime(sd["fc_mu.weight"]) if wt is None else wt
    act = np.stack([encode(orc, sd, im, running).reshape(-1) for im in images])
    mu = fc_mu(act, wt, sd["fc_mu.bias"])
    return mu, head(sd, mu)


def select_lowest(preds, budget):
    """Loader positions of the `budget` lowest predictions, lowest first, ties by lower position."""
    preds = np.asarray(preds)
    order = sorted(range(len(preds)), key=lambda i: (preds[i], i))
    return np.array(order[:max(0, min(int(budget), len(preds)))], np.int64)


# ----------------------------------------------------------------------------- float64 evaluation and a-priori bounds
def _conv64(x, w):
    """x [H][W][C] float64, w torch layout -> [Ho][Wo][Cout] float64 (4 x 4, stride 2, padding 1)"""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64).transpose(2, 0, 1)[None]))
    o = F.conv2d(t, torch.from_numpy(np.asarray(w, np.float64)), None, 2, 1)
    return o[0].permute(1, 2, 0).contiguous().numpy()


def conv_bound(w, b, x_abs, e):
    """|W| e + gamma(K + 1) (|W| |x| + |b|) for the 4 x 4 / 2 / 1 convolution; x_abs = |float32 input|, e = its error bound."""
    w = np.abs(np.asarray(w, np.float64))
    K = 16 * w.shape[1]
    return _conv64(e, w) + gamma(K + 1) * (_conv64(x_abs, w) + np.abs(np.asarray(b, np.float64)))


def bn_batch_bound(rh, er, g, be):
    """rh [H][W][C]: the float32 convolution output, er: its error bound -> the bound of the normalised, ReLU'd map."""
    C = rh.shape[2]
    g, be = np.asarray(g, np.float64), np.asarray(be, np.float64)
    _, istd, dc, var = (a.astype(np.float64) for a in bn_stats(rh.reshape(-1, C).astype(F32)))
    er2 = er.reshape(-1, C)
    d = 64 + 2 + (dc.shape[0] + 255) // 256 + 1
    em = er2.mean(axis=0) + gamma(d) * np.abs(rh.reshape(-1, C).astype(np.float64)).mean(axis=0)
    ed = er2 + em[None] + U * np.abs(dc)
    es = (2 * np.abs(dc) + ed) * ed + U * dc * dc
    ev = es.mean(axis=0) + gamma(d) * (dc * dc).mean(axis=0) + U * (var + EPS)
    ei = 0.5 * np.maximum(var + EPS - ev, EPS) ** -1.5 * ev + 3 * U * istd
    return (np.abs(g)[None] * (istd[None] * ed + (np.abs(dc) + ed) * ei[None])
            + gamma(3) * (np.abs(dc * istd[None] * g[None]) + np.abs(be)[None])).reshape(rh.shape)


def bn_running_bound(sd, l, rh, er):
    p = "encoder.%d." % (3 * l + 1)
    g, be, rm, rv = (np.asarray(sd[p + k], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    sc = g / np.sqrt(rv + EPS)
    sch, shh = (a.astype(np.float64) for a in folded_bn(sd, l))
    esc = gamma(4) * np.abs(sc)
    esh = np.abs(rm) * esc + gamma(2) * (np.abs(be) + np.abs(rm * sc))
    rh = np.abs(rh.astype(np.float64))
    return np.abs(sch) * er + rh * esc + esh + gamma(2) * (rh * np.abs(sch) + np.abs(shh))


def bn64(sd, l, r, running):
    p = "encoder.%d." % (3 * l + 1)
    g, be, rm, rv = (np.asarray(sd[p + k], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    if running:
        return np.maximum((r - rm) / np.sqrt(rv + EPS) * g + be, 0.0)
    return np.maximum((r - r.mean(axis=(0, 1))) / np.sqrt(r.var(axis=(0, 1)) + EPS) * g + be, 0.0)


def fc_bound(sd, act_abs, e):
    """act_abs, e: [65536] in NCHW order"""
    fw = np.abs(np.asarray(sd["fc_mu.weight"], np.float64))
    return fw @ e + gamma(513) * (fw @ act_abs + np.abs(np.asarray(sd["fc_mu.bias"], np.float64)))


def head64(sd, mu):
    W1, b1 = np.asarray(sd["net.0.weight"], np.float64), np.asarray(sd["net.0.bias"], np.float64)
    W2, b2 = np.asarray(sd["net.2.weight"], np.float64), np.asarray(sd["net.2.bias"], np.float64)
    W3, b3 = np.asarray(sd["net.4.weight"], np.float64)[0], float(np.asarray(sd["net.4.bias"])[0])
    h2 = np.maximum(W2 @ np.maximum(W1 @ mu + b1, 0.0) + b2, 0.0)
    return 1.0 / (1.0 + np.exp(-(W3 @ h2 + b3)))


def head_bound(sd, mu_abs, emu):
    W1, b1 = np.abs(np.asarray(sd["net.0.weight"], np.float64)), np.abs(np.asarray(sd["net.0.bias"], np.float64))
    W2, b2 = np.abs(np.asarray(sd["net.2.weight"], np.float64)), np.abs(np.asarray(sd["net.2.bias"], np.float64))
    W3, b3 = np.abs(np.asarray(sd["net.4.weight"], np.float64))[0], abs(float(np.asarray(sd["net.4.bias"])[0]))
    m1 = W1 @ (mu_abs + emu) + b1; e1 = W1 @ emu + gamma(257) * m1
    m2 = W2 @ (m1 + e1) + b2; e2 = W2 @ e1 + gamma(513) * m2
    m3 = W3 @ (m2 + e2) + b3; e3 = W3 @ e2 + gamma(513) * m3
    return 0.25 * e3 + 8 * U


def stage_checks(orc, sd, img, running):
    """Every stage of one image on its own: the float32 output against the float64 evaluation of the SAME float32 input, over the stage's
    bound with e = 0.  Returns [(stage, largest |difference| / bound)]; each must be <= 1.  These are the bounds with teeth: carried
    through the whole path (sweep64) a worst-case bound grows by the absolute-weight norm of every layer and ends far above the values."""
    keep, out = [], []
    act = encode(orc, sd, img, running, keep)
    x = resize(img).astype(np.float64)
    for l in range(5):
        w, b = sd["encoder.%d.weight" % (3 * l)], np.asarray(sd["encoder.%d.bias" % (3 * l)], np.float64)
        rh, yh = keep[l]
        r64 = _conv64(x, w) + b
        zero = np.zeros_like(x)
        out.append(("conv%d" % (l + 1), (np.abs(rh - r64) / conv_bound(w, b, np.abs(x), zero)).max()))
        y64 = bn64(sd, l, rh.astype(np.float64), running)
        p = "encoder.%d." % (3 * l + 1)
        bound = bn_running_bound(sd, l, rh, np.zeros(rh.shape)) if running else bn_batch_bound(rh, np.zeros(rh.shape), sd[p + "weight"], sd[p + "bias"])
        out.append(("bn%d" % (l + 1), (np.abs(yh - y64) / bound).max()))
        x = yh.astype(np.float64)
    a = x.transpose(2, 0, 1).reshape(-1)
    mu = fc_mu(act.reshape(1, -1), fc_weight_kprime(sd["fc_mu.weight"]), sd["fc_mu.bias"])[0]
    mu64 = np.asarray(sd["fc_mu.weight"], np.float64) @ a + np.asarray(sd["fc_mu.bias"], np.float64)
    out.append(("fc_mu", (np.abs(mu - mu64) / fc_bound(sd, np.abs(a), np.zeros_like(a))).max()))
    pr = head(sd, mu[None])[0]
    out.append(("head", abs(float(pr) - head64(sd, mu.astype(np.float64))) / head_bound(sd, np.abs(mu.astype(np.float64)), np.zeros(256))))
    return out


def sweep64(sd, images, running, orc=None):
    """The float64 evaluation of the sweep and the a-priori bound of its float32 restatement carried through the whole path:
    (mu64 [n][256], preds64 [n], mu_bound [n][256], preds_bound [n]).  The bound follows the float32 values of the restatement (orc: the
    oracle module); without orc only the float64 values are returned (bounds None).  It is a worst-case bound: every layer multiplies the
    incoming bound by its absolute-weight norm, so at the end of six dense layers it is rigorous and far above the values themselves."""
    mu64, p64, mub, pb = [], [], [], []
    fw = np.asarray(sd["fc_mu.weight"], np.float64)
    for img in images:
        keep = []
        if orc is not None:
            encode(orc, sd, img, running, keep)
        x = resize(img).astype(np.float64)
        e = np.zeros_like(x)
        for l in range(5):
            w = np.asarray(sd["encoder.%d.weight" % (3 * l)], np.float64); b = np.asarray(sd["encoder.%d.bias" % (3 * l)], np.float64)
            p = "encoder.%d." % (3 * l + 1)
            r = _conv64(x, w) + b
            if orc is not None:
                xh = np.abs(keep[l - 1][1].astype(np.float64)) if l else np.abs(x)
                er = conv_bound(w, b, xh, e)
                e = bn_running_bound(sd, l, keep[l][0], er) if running else bn_batch_bound(keep[l][0], er, sd[p + "weight"], sd[p + "bias"])
            x = bn64(sd, l, r, running)
        a64 = x.transpose(2, 0, 1).reshape(-1)                                 # NCHW flattening: k = c * 64 + p
        mu = fw @ a64 + np.asarray(sd["fc_mu.bias"], np.float64)
        mu64.append(mu)
        p64.append(head64(sd, mu))
        if orc is not None:
            ah = np.abs(keep[4][1].astype(np.float64)).transpose(2, 0, 1).reshape(-1)
            emu = fc_bound(sd, ah, e.transpose(2, 0, 1).reshape(-1))
            mub.append(emu)
            pb.append(head_bound(sd, np.abs(mu), emu))
    if orc is None:
        return np.stack(mu64), np.array(p64), None, None
    return np.stack(mu64), np.array(p64), np.stack(mub), np.array(pb)
