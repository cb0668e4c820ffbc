"""Independent restatements of the layer operations of csrc/nn.hip (ORACLE,
test-only): numpy integer arithmetic for the dropout mask, torch float64 for
everything else, written from include/acfe.h's text and the Keras semantics of
the layers -- not from the kernels' indexing.  Activations are NHWC
([rows][C] for the per-channel operations), as the C ABI has them.

Nothing here rounds to a storage type: callers that need the stored value
round the float64 result themselves (to_f32 / to_bf16 below).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.models import avgpool_same, keras_adam, keras_loss, logmeanexp  # noqa: F401  (re-exported)

F64 = torch.float64
BN_EPS, BN_MOMENTUM = 1e-3, 0.99


# ------------------------------------------------------------------ rounding
def to_bf16(t):
    """Round-to-nearest-even to bfloat16, returned in float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def to_f32(t):
    return t.to(torch.float32).to(F64)


# ------------------------------------------------------------------ dropout
def _fmix32(h):
    """murmur3's 32-bit finalizer on uint64 arrays holding 32-bit values."""
    m = np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def pair_hash(seed, pair):
    """The 32-bit hash of element pair `pair` (= idx >> 1) under `seed`: a Weyl
    step of the low words, the high words mixed in, then murmur3's finalizer."""
    m = np.uint64(0xFFFFFFFF)
    pair = np.asarray(pair, dtype=np.uint64)
    seed = np.uint64(seed)
    h = ((pair & m) * np.uint64(0x9E3779B1) + (seed & m)) & m
    h = h ^ ((((pair >> np.uint64(32)) * np.uint64(0x85EBCA77)) & m) ^ (seed >> np.uint64(32)))
    return _fmix32(h)


def dropout_threshold(rate):
    t = np.float32(rate) * np.float32(65536.0)
    return 65536 if t >= 65536.0 else int(t)


def dropout_scale(rate):
    return np.float32(1) / (np.float32(1) - np.float32(rate))


def dropout_keep(seed, idx, rate):
    """Keep mask (bool array) of the flat element indices `idx`: an element is
    kept iff its 16-bit half of its pair's hash (low half for an even index,
    high half for an odd one) is >= rate * 2^16."""
    idx = np.asarray(idx, dtype=np.uint64)
    h = pair_hash(seed, idx >> np.uint64(1))
    half = np.where((idx & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return half >= np.uint64(dropout_threshold(rate))


def dropout(x, seed, rate, bf16):
    """Dropout of the stored tensor x (float64 holding f32 / bf16 values) over
    its flat index: kept values are rnd(fl32(x * scale)), the rest 0."""
    keep = torch.from_numpy(dropout_keep(seed, np.arange(x.numel(), dtype=np.uint64), rate)).view(x.shape)
    v = (x.to(torch.float32) * torch.tensor(dropout_scale(rate))).to(F64)
    if bf16:
        v = to_bf16(v)
    return torch.where(keep, v, torch.zeros_like(v)), keep


# ------------------------------------------------------------------ pools (NHWC)
def windows(x, kh, kw):
    """[N, P, Q, kh*kw, C]: the valid windows of x, row-major inside a window."""
    N, H, W, C = x.shape
    P, Q = H // kh, W // kw
    w = x[:, :P * kh, :Q * kw].reshape(N, P, kh, Q, kw, C).permute(0, 1, 3, 2, 4, 5)
    return w.reshape(N, P, Q, kh * kw, C)


def maxpool(x, kh, kw):
    """MaxPool2D((kh, kw), strides = pool, "valid"): values and the index of the
    first maximum of each window in row-major window order (uint8)."""
    w = windows(x, kh, kw)
    y = w.max(dim=3).values
    first = (w == y.unsqueeze(3)).to(torch.int64).argmax(dim=3)  # argmax of a 0/1 tensor: first 1
    return y, first.to(torch.uint8)


def maxpool_bwd_from_argmax(am, dy, H, W, kh, kw):
    """The gradient goes to the window position `am` names; rows and columns
    past the last whole window get zero."""
    N, P, Q, C = dy.shape
    onehot = F.one_hot(am.to(torch.int64), kh * kw).permute(0, 1, 2, 4, 3).to(dy.dtype)  # [N,P,Q,khkw,C]
    g = (onehot * dy.unsqueeze(3)).reshape(N, P, Q, kh, kw, C).permute(0, 1, 3, 2, 4, 5).reshape(N, P * kh, Q * kw, C)
    dx = torch.zeros((N, H, W, C), dtype=dy.dtype)
    dx[:, :P * kh, :Q * kw] = g
    return dx


def maxpool_bwd(x, dy, kh, kw):
    return maxpool_bwd_from_argmax(maxpool(x, kh, kw)[1], dy, x.shape[1], x.shape[2], kh, kw)


def _same_geometry(n, k):
    """(windows, pad_before) of a "same" pool of stride k over n elements."""
    out = -(-n // k)
    return out, (out * k - n) // 2


def _window_counts(H, W, k):
    """[P, Q]: the in-bounds elements of every window."""
    (P, pt), (Q, pl) = _same_geometry(H, k), _same_geometry(W, k)
    ch = torch.tensor([min(p * k - pt + k, H) - max(p * k - pt, 0) for p in range(P)], dtype=F64)
    cw = torch.tensor([min(q * k - pl + k, W) - max(q * k - pl, 0) for q in range(Q)], dtype=F64)
    return ch[:, None] * cw[None, :]


def avgpool(x, k):
    """AveragePooling2D(k, strides = k, "same"), in-bounds averaging: windows
    start at -pad_before with pad_total = (ceil(n / k) - 1) k + k - n and
    pad_before = pad_total // 2 (TF).  The input is laid into a zero canvas of
    whole windows; each window's sum is divided by its in-bounds count."""
    N, H, W, C = x.shape
    (P, pt), (Q, pl) = _same_geometry(H, k), _same_geometry(W, k)
    canvas = torch.zeros((N, P * k, Q * k, C), dtype=x.dtype)
    canvas[:, pt:pt + H, pl:pl + W] = x
    return canvas.reshape(N, P, k, Q, k, C).sum((2, 4)) / _window_counts(H, W, k)[None, :, :, None]


def avgpool_bwd(dy, H, W, k):
    """Every in-bounds element of a window receives dy / count."""
    N, P, Q, C = dy.shape
    pt, pl = _same_geometry(H, k)[1], _same_geometry(W, k)[1]
    g = dy / _window_counts(H, W, k)[None, :, :, None]
    canvas = g.repeat_interleave(k, 1).repeat_interleave(k, 2)
    return canvas[:, pt:pt + H, pl:pl + W].clone()


def sub_bwd(g, H, W, k):
    """Input gradient of a 1x1 "valid" convolution of stride k as seen at its
    input: g lands on the pixels (k p, k q), zero elsewhere."""
    N, P, Q, C = g.shape
    dx = torch.zeros((N, H, W, C), dtype=g.dtype)
    dx[:, ::k, ::k][:, :P, :Q] = g
    return dx


# ------------------------------------------------------------------ BatchNormalization over [rows][C]
def bn_stats(x):
    """{sum x, sum x^2} per channel: [2][C]."""
    return torch.stack([x.sum(0), (x * x).sum(0)])


def bn_finalize(sums, count, gamma, beta, moving_mean, moving_var, training=True, eps=BN_EPS,
                momentum=BN_MOMENTUM):
    """dict(scale, shift, mean, invstd, moving_mean, moving_var) from the
    per-channel {sum, sum of squares}: biased variance, Keras moving update."""
    if training:
        mean = sums[0] / count
        var = (sums[1] / count - mean * mean).clamp_min(0)
        mm = moving_mean * momentum + mean * (1 - momentum)
        mv = moving_var * momentum + var * (1 - momentum)
    else:
        mean, var, mm, mv = moving_mean, moving_var, moving_mean, moving_var
    invstd = 1 / torch.sqrt(var + eps)
    scale = gamma * invstd
    return dict(scale=scale, shift=beta - mean * scale, mean=mean, invstd=invstd, moving_mean=mm, moving_var=mv)


def bn_apply(x, scale, shift, relu):
    y = x * scale + shift
    return y.clamp_min(0) if relu else y


def bn_masked_grad(dy, x, scale, shift, relu):
    """The gradient at the BN's (pre-ReLU) output: dy where the BN's own ReLU
    let the value through."""
    return torch.where(x * scale + shift > 0, dy, torch.zeros_like(dy)) if relu else dy


def bn_bwd_reduce(dy, x, scale, shift, mean, invstd, relu):
    g = bn_masked_grad(dy, x, scale, shift, relu)
    return torch.stack([g.sum(0), (g * (x - mean) * invstd).sum(0)])


def bn_bwd_finalize(sums, count, scale, mean, invstd):
    """dgamma, dbeta and coef[3][C] = {a, b, c} of dx = a g + b x + c, from
    dx = scale (g - mean(g) - xhat mean(g xhat)), xhat = (x - mean) invstd."""
    mg, mgx = sums[0] / count, sums[1] / count
    coef = torch.stack([scale, -scale * mgx * invstd, -scale * mg + scale * mgx * invstd * mean])
    return sums[1], sums[0], coef


def bn_bwd_apply(dy, x, scale, shift, coef, relu=0, add=None):
    """dx before storage: relu bit 0 masks dy by the BN's ReLU, bit 1 masks the
    result by x > 0 (x is itself a ReLU output) after the residual `add`."""
    g = bn_masked_grad(dy, x, scale, shift, relu & 1)
    v = coef[0] * g + coef[1] * x + coef[2]
    if add is not None:
        v = v + add
    if relu & 2:
        v = torch.where(x > 0, v, torch.zeros_like(v))
    return v


# ------------------------------------------------------------------ head
def axis_pool(x, sharpness, mode):
    """[outer][L][inner] -> [outer][inner]: log-mean-exp (mode 0) or mean."""
    return logmeanexp(x, 1, sharpness) if mode == 0 else x.mean(1)


def axis_pool_bwd(x, dy, sharpness, mode):
    xr = x.clone().requires_grad_(True)
    (axis_pool(xr, sharpness, mode) * dy).sum().backward()
    return xr.grad


def dense(x, w, b):
    return x @ w + b


def dense_bwd(x, w, dz):
    return dz @ w.T, x.T @ dz, dz.sum(0)


def loss(z, y, mode, grad_scale):
    """(mean loss, grad_scale * dloss/dz) of keras_loss; mode 0 BCE, 1 CCE."""
    zr = z.clone().requires_grad_(True)
    l = keras_loss(zr, y, "bce" if mode == 0 else "cce")
    l_sum = l * z.shape[0]  # the per-row losses summed: dz is per row (grad_scale carries the 1 / B)
    l_sum.backward()
    return l.detach(), zr.grad * grad_scale


def adam_alpha(lr, t, b1=0.9, b2=0.999):
    return lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)


def adam(p, g, m, v, grad_scale, t, lr=0.01, b1=0.9, b2=0.999, eps=1e-7):
    ps, ms, vs = keras_adam([p.clone()], [g * grad_scale], [m.clone()], [v.clone()], t, lr, b1, b2, eps)
    return ps[0], ms[0], vs[0]
