"""A plain-torch restatement of badwinner2's eval-mode forward on the CPU, the
independent reference of tests/test_badwinner2_gpu.py and
tests/test_badwinner2_host.py (test infrastructure, no test of its own).

Written from the model's description (MagTransform, a BatchNormalization over
the mel rows without gamma / beta, "valid" convolutions each followed by
LeakyReLU(0.01) and a BatchNormalization on its moving statistics, two max
pools, a class convolution with a bare LeakyReLU, optional log-mean-exp
pooling at sharpness 5 over H then W, a global average, then sigmoid or
softmax), with torch.nn.functional.conv2d / max_pool2d in NCHW.  Modes:

  "f64"   everything in float64
  "f32"   everything in float32
  "bf16"  bf16 storage: the convolution weights and every activation a bf16
          model stores (the normalised input, each convolution output, each
          LeakyReLU + BN output) rounded to bf16, arithmetic in float64

Parameters come from a BadWinner2 module's state (CPU copies); the first
kernel is summed over its input channels in float32 in every mode, as the
model does before it packs it.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

ALPHA, EPS, SHARP = 0.01, 1e-3, 5.0
HOP, SR = 281, 48000


def clip_samples(frames):
    """Samples of a clip whose centred STFT (hop 281) has `frames` frames."""
    return (frames - 1) * HOP


def chirp_clips(b, frames, seed):
    """b seeded clips of chirps over noise (tests/conftest.py synth_clips' recipe
    at the clip length that gives `frames` frames), float32 in [-1, 1]."""
    n = clip_samples(frames)
    out = np.zeros((b, n), np.float32)
    t = np.arange(n) / SR
    dur_all = n / SR
    for i in range(b):
        rng = np.random.default_rng(seed + i)
        x = rng.normal(0, rng.uniform(0.002, 0.02), n)
        for _ in range(rng.integers(1, 4)):
            f0, f1 = rng.uniform(500, 10000, 2)
            amp = rng.uniform(0.05, 0.5)
            on = rng.uniform(0, 0.6 * dur_all)
            dur = rng.uniform(0.1 * dur_all, dur_all - on)
            m = (t >= on) & (t < on + dur)
            tt = t[m] - on
            x[m] += amp * np.sin(2 * np.pi * (f0 * tt + 0.5 * (f1 - f0) / dur * tt * tt))
        out[i] = np.clip(x, -1, 1)
    return out


def cpu_mel(clips, n_mels):
    """The fp32 mel power [B, M, T] of raw clips by the CPU oracle (normalise,
    centred STFT with constant padding, |X|^2, mel): what
    FrontEnd(pcen=False, dtype=float32)(clips, pad_mode="constant") computes."""
    from oracle import frontend as of

    w = of.mel_f(SR, n_mels, 100, 11000, 4096, 1000)
    return torch.from_numpy(of.get_spect(of.normalize(clips), w).astype(np.float32))


def seed_model(model, seed):
    """Seeded parameters at the Keras initialisers' scale (Glorot-uniform
    limits for every kernel; an orthogonal kernel has the same order of
    magnitude), small biases, BN gamma / beta / moving statistics near
    (1, 0, 0, 1) with spread, the input statistics near the transformed mel's,
    a-power in [-2, 1]."""
    g = torch.Generator().manual_seed(seed)

    def rnd(shape, lo, hi):
        return torch.rand(shape, generator=g) * (hi - lo) + lo

    with torch.no_grad():
        model.mag.a.copy_(rnd((1,), -1.5, 0.5))
        model.norm.moving_mean.copy_(rnd(model.norm.moving_mean.shape, 0.05, 0.6))
        model.norm.moving_variance.copy_(rnd(model.norm.moving_variance.shape, 0.02, 0.5))
        for conv in list(model.convs) + [model.class_conv]:
            K, R, S, C = conv.weight.shape
            lim = math.sqrt(6.0 / (R * S * C + R * S * K))
            conv.weight.copy_(rnd(conv.weight.shape, -lim, lim))
            conv.bias.copy_(rnd(conv.bias.shape, -0.05, 0.05))
        for bn in model.bns:
            bn.gamma.copy_(rnd(bn.gamma.shape, 0.7, 1.3))
            bn.beta.copy_(rnd(bn.beta.shape, -0.2, 0.2))
            bn.moving_mean.copy_(rnd(bn.moving_mean.shape, -0.2, 0.2))
            bn.moving_variance.copy_(rnd(bn.moving_variance.shape, 0.6, 1.5))
    return model


def state_of(model):
    return {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def forward(sd, mel, mode, multi_label, lme, taps=None):
    """Probabilities [B, labels] (float64) of the fp32 mel [B, M, T] for the
    state `sd` (state_of); taps receives every stage's output as the model's
    `taps` does, NHWC, float64."""
    dt = torch.float32 if mode == "f32" else torch.float64
    store = _bf if mode == "bf16" else (lambda t: t)

    def tap(t, nchw=True):
        if taps is not None:
            taps.append((t.permute(0, 2, 3, 1) if nchw else t).double().contiguous())

    p = torch.sigmoid(sd["mag.a"].to(dt))
    mean, var = sd["norm.moving_mean"].to(dt), sd["norm.moving_variance"].to(dt)
    x = mel.to(dt)
    x = store((torch.pow(x, p) - mean[None, :, None]) / torch.sqrt(var[None, :, None] + EPS))
    tap(x, nchw=False)
    x = x[:, None]  # NCHW, one channel
    n = sum(1 for k in sd if k.startswith("trunk.") and k.endswith(".weight"))  # trunk: conv, bn, conv, bn, ...
    for i in range(n + 1):
        last = i == n
        pre = "class_conv" if last else f"trunk.{2 * i}"
        w = sd[pre + ".weight"]  # [K, R, S, C] float32
        if i == 0 and w.shape[3] != 1:
            w = w.sum(3, keepdim=True)
        w = store(w.to(dt)).permute(0, 3, 1, 2)
        x = store(F.conv2d(x, w, sd[pre + ".bias"].to(dt)))
        x = torch.where(x > 0, x, ALPHA * x)
        if not last:
            b = f"trunk.{2 * i + 1}."
            scale = sd[b + "gamma"].to(dt) / torch.sqrt(sd[b + "moving_variance"].to(dt) + EPS)
            shift = sd[b + "beta"].to(dt) - sd[b + "moving_mean"].to(dt) * scale
            x = x * scale[None, :, None, None] + shift[None, :, None, None]
        x = store(x)
        tap(x)
        if i == 1:
            x = F.max_pool2d(x, (3, 3))
            tap(x)
        elif i == 4:
            x = F.max_pool2d(x, (5, 3))
            tap(x)
    if lme:
        x = x.to(torch.float32 if mode == "f32" else torch.float64)
        for axis in (2, 3):
            x = torch.logsumexp(x * SHARP, dim=axis, keepdim=True) - math.log(x.shape[axis])
            x = x / SHARP
            tap(x)
    z = x.mean((2, 3))
    tap(z, nchw=False)
    prob = torch.sigmoid(z) if multi_label else torch.softmax(z, 1)
    return prob.double()
