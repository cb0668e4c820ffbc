"""badwinner2 (reference: badwinner2.py:212-324) on the acfe kernels, inference only.

    MagTransform -> BatchNormalization over the mel axis (no gamma / beta)
    -> [Conv2D(64, 3x3) -> LeakyReLU(0.01) -> BatchNormalization] x 2 -> MaxPool2D((3, 3))
    -> [Conv2D(128, 3x3) -> LeakyReLU -> BN] x 2
    -> Conv2D(128, (44, 3)) (n_mels 160; (22, 3) for 96) -> LeakyReLU -> BN -> MaxPool2D((5, 3))
    -> Conv2D(1024, (1, 9)) -> LeakyReLU -> BN -> Conv2D(1024, 1) -> LeakyReLU -> BN
    -> Conv2D(labels, 1) -> LeakyReLU [-> LME over H, then W] -> GlobalAveragePooling2D
    -> sigmoid (multi_label) or softmax

All convolutions are "valid" (acfe_conv2d_fwd); the passes between them are
csrc/bw2.hip (acfe_mag_rownorm, acfe_leaky_bn, acfe_softmax), acfe_maxpool2d
and acfe_axis_pool.  Eval mode only: Dropout is the identity and every
BatchNormalization uses its moving statistics; training badwinner2 is not
implemented.  Input: the fp32 mel power [B, n_mels, T], the output of
acfe.train.FrontEnd(pcen=False, dtype=torch.float32) -- MagTransform is the
compression (the reference feeds mel power straight in, predict.py:874-887).
The mel must not be rounded to bf16 first: it spans more than ten decades.
"""
from __future__ import annotations

import torch
from torch import nn

from acfe import ops
from acfe.layers import BatchNormalization, Conv2D

LEAKY_ALPHA = 0.01  # badwinner2.py:223
LME_SHARPNESS = 5.0  # :312-313
CONDENSE_ROWS = {160: 44, 96: 22}  # :259-262


class MagTransform(nn.Module):
    """badwinner2.MagTransform (:33-49): x ** sigmoid(a), one variable `a-power` [1]."""

    keras_kind = "mag_transform"
    keras_auto = True

    def __init__(self):
        super().__init__()
        self.name = "mag_transform"
        self.a = nn.Parameter(torch.full((1,), -1.0))


class RowNormalization(nn.Module):
    """BatchNormalization(axis=1, scale=False, center=False) (:233) in eval mode:
    the moving statistics of every mel row, no gamma / beta."""

    keras_kind = "batch_normalization"
    keras_auto = True

    def __init__(self, rows, eps=1e-3):
        super().__init__()
        self.name, self.eps = "batch_normalization", eps
        self.register_buffer("moving_mean", torch.zeros(rows))
        self.register_buffer("moving_variance", torch.ones(rows))


def _orthogonal_(w: torch.Tensor, seed: int):
    """tf.keras.initializers.Orthogonal on a KRSC kernel: the Keras kernel
    [R, S, C, K] flattened to [R S C, K] has orthonormal columns (or rows)."""
    K, R, S, C = w.shape
    g = torch.Generator().manual_seed(int(seed))
    rows, cols = R * S * C, K
    a = torch.randn((max(rows, cols), min(rows, cols)), generator=g, dtype=torch.float64)
    q, r = torch.linalg.qr(a)
    q = q * torch.sign(torch.diagonal(r))
    if rows < cols:
        q = q.t()
    with torch.no_grad():
        w.copy_(q.reshape(R, S, C, K).permute(3, 0, 1, 2).to(torch.float32))


def output_hw(n_mels: int, frames: int) -> tuple[int, int]:
    """(H, W) of the class convolution's output, before the class pooling, for
    an n_mels x frames input.  ValueError for n_mels other than 160 / 96 and
    when a dimension falls below 1 (the smallest input is 103 frames)."""
    if n_mels not in CONDENSE_ROWS:
        raise ValueError(f"badwinner2 handles 160 or 96 mel bands, not {n_mels} (badwinner2.py:259-264)")
    h, w = n_mels, int(frames)
    for kh, kw, pool in ((3, 3, 0), (3, 3, 0), (3, 3, 1), (3, 3, 0), (3, 3, 0), (CONDENSE_ROWS[n_mels], 3, 0),
                         (5, 3, 1), (1, 9, 0)):
        h, w = (h // kh, w // kw) if pool else (h - kh + 1, w - kw + 1)
        if h < 1 or w < 1:
            raise ValueError(f"badwinner2: a {n_mels} x {frames} input is too small (103 frames at least)")
    return h, w


class BadWinner2(nn.Module):
    def __init__(self, input_shape, num_labels, multi_label=False, lme=False, dtype=torch.bfloat16, seed=0):
        super().__init__()
        shape = tuple(input_shape)
        n_mels, frames = shape[0], shape[1]
        cin = shape[2] if len(shape) > 2 else 1
        if cin not in (1, 3):
            raise ValueError(f"badwinner2: 1 or 3 input channels, not {cin}")
        output_hw(n_mels, frames)
        self.input_shape, self.classes, self.dtype = (n_mels, frames, cin), int(num_labels), dtype
        self.multi_label, self.lme = bool(multi_label), bool(lme)
        # the reference's layer creation order: Keras auto-names every layer by it
        self.mag = MagTransform()
        self.norm = RowNormalization(n_mels)
        spec = [(cin, 64, (3, 3)), (64, 64, (3, 3)), (64, 128, (3, 3)), (128, 128, (3, 3)),
                (128, 128, (CONDENSE_ROWS[n_mels], 3)), (128, 1024, (1, 9)), (1024, 1024, 1)]
        self.trunk = nn.ModuleList()  # conv, bn, conv, bn, ...: modules() keeps the creation order
        for i, (c, k, ks) in enumerate(spec):
            conv = Conv2D(c, k, ks, 1, "valid", name=f"conv2d_{i}", seed=seed)
            bn = BatchNormalization(k, name=f"batch_normalization_{i + 1}")
            conv.keras_auto = bn.keras_auto = True
            if i >= 5:
                _orthogonal_(conv.weight, seed + 100 + i)
            self.trunk.append(conv)
            self.trunk.append(bn)
        # the first convolution's Cin (3: raw_to_mel repeats the mel, tfdataset.py:2053;
        # 1: stored spectrograms, :1090) follows the checkpoint
        self.convs[0].keras_flex_cin = (1, 3)
        self.class_conv = Conv2D(1024, self.classes, 1, 1, "valid", name="conv2d_7", seed=seed)
        self.class_conv.keras_auto = True
        _orthogonal_(self.class_conv.weight, seed + 107)
        self._folded = (None, None)

    @property
    def convs(self):
        return list(self.trunk)[0::2]

    @property
    def bns(self):
        return list(self.trunk)[1::2]

    def _constants(self):
        """Per-model constants formed on the device from the parameters and kept
        until one of them changes: every BN's (scale, shift) = (gamma /
        sqrt(moving_variance + eps), beta - moving_mean * scale), and the first
        kernel summed over its Cin copies (the input channels are identical,
        as in layers.StemConv2D)."""
        src = [self.convs[0].weight]
        for bn in self.bns:
            src += [bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance]
        key = tuple((t.data_ptr(), t._version) for t in src)
        if self._folded[0] != key:
            with torch.no_grad():
                aff = []
                for bn in self.bns:
                    scale = (bn.gamma.float() * torch.rsqrt(bn.moving_variance.float() + bn.eps)).contiguous()
                    aff.append((scale, (bn.beta.float() - bn.moving_mean.float() * scale).contiguous()))
                w1 = self.convs[0].weight
                if w1.shape[3] != 1:
                    w1 = w1.sum(3, keepdim=True).contiguous()
            self._folded = (key, (w1, aff))
        return self._folded[1]

    def forward(self, mel, taps=None):
        """fp32 mel power [B, n_mels, T] -> fp32 logits [B, labels].  taps: a list
        that receives every stage's output (the normalised input, each conv +
        LeakyReLU + BN, both pools, the class conv + LeakyReLU, the two LME
        poolings, the logits), in order."""
        if self.training:
            raise NotImplementedError("badwinner2 runs in eval mode only (Dropout as identity, BatchNormalization "
                                      "on its moving statistics): call .eval(); training it is not implemented")
        if mel.dim() == 4 and mel.shape[-1] == 1:
            mel = mel[..., 0]
        if mel.dim() != 3 or mel.dtype != torch.float32 or mel.shape[1] != self.input_shape[0]:
            raise ValueError(f"badwinner2 takes the fp32 mel [B, {self.input_shape[0]}, T], got "
                             f"{tuple(mel.shape)} {mel.dtype}")
        output_hw(mel.shape[1], mel.shape[2])
        # the largest activation (the first convolution's output) stays below 2^31 elements per launch
        per_clip = (mel.shape[1] - 2) * (mel.shape[2] - 2) * 64
        nmax = max(1, (2 ** 31 - 1) // per_clip)
        if mel.shape[0] > nmax:
            if taps is not None:
                raise ValueError(f"badwinner2: taps are for batches of at most {nmax} clips")
            return torch.cat([self.forward(mel[i:i + nmax].contiguous()) for i in range(0, mel.shape[0], nmax)])

        def tap(t):
            if taps is not None:
                taps.append(t)
            return t

        with torch.no_grad():
            w1, aff = self._constants()
            x = ops.mag_rownorm(mel, self.mag.a, self.norm.moving_mean, self.norm.moving_variance, self.dtype,
                                self.norm.eps)
            x = tap(x).unsqueeze(-1)  # NHWC with one channel
            for i, (conv, (scale, shift)) in enumerate(zip(self.convs, aff)):
                w = w1 if i == 0 else conv.weight
                y, _ = ops.conv2d(x, w, conv.bias, 1, "valid")
                x = tap(ops.leaky_bn(y, LEAKY_ALPHA, scale, shift, out=y))
                if i == 1:
                    x = tap(ops.max_pool_valid(x, 3, 3))
                elif i == 4:
                    x = tap(ops.max_pool_valid(x, 5, 3))
            y, _ = ops.conv2d(x, self.class_conv.weight, self.class_conv.bias, 1, "valid")
            x = tap(ops.leaky_bn(y, LEAKY_ALPHA, out=y))
            if self.lme:  # LMELayer(axis=1), LMELayer(axis=2), keepdims (:312-313, :343-355)
                x = tap(ops.logmeanexp(x, 1, LME_SHARPNESS).unsqueeze(1))
                x = tap(ops.logmeanexp(x, 2, LME_SHARPNESS).unsqueeze(2))
            return tap(ops.global_avg_pool(x))

    def activation(self, logits):
        """The model's output activation (:316-321): sigmoid for a multi-label
        checkpoint, softmax otherwise."""
        return ops.sigmoid(logits) if self.multi_label else ops.softmax(logits)

    def predict(self, x):
        return self.activation(self.forward(x))


def build_model(input_shape, norm_layer, num_labels, multi_label=False, lme=False, add_dense=True,
                big_condense=True, input_name="input", dtype=torch.bfloat16):
    """badwinner2.build_model (:212-324) with the arguments audiomodel.py:741-749
    passes; norm_layer and input_name are unused, as in the reference."""
    if not (add_dense and big_condense):
        raise ValueError("badwinner2: only big_condense=True and add_dense=True are built")
    return BadWinner2(input_shape, num_labels, multi_label=multi_label, lme=lme, dtype=dtype)
