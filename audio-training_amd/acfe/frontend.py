"""Feature front end on the GPU: normalize, mix_up, STFT->mel, PCEN.

Mirrors the reference operators (tfdataset.normalize :1916-1934,
tfdataset.mix_up :930-955, tfdataset.raw_to_mel :2007-2059,
predict_utils.get_spect :163-239, tfpcen.PCEN :42-99) on torch device tensors,
executing the HIP kernels of csrc/frontend.hip through the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import call, lib
from ._torch import dtype_code, ptr, require_cuda, stream

PAD_MODES = {"end": _lib.PAD_END, "constant": _lib.PAD_CENTER_CONSTANT, "reflect": _lib.PAD_CENTER_REFLECT}


def mel_filterbank(sr, n_mels, fmin, fmax, n_fft, break_freq) -> np.ndarray:
    """custommel.mel_f (custommel.py:18-54), computed by the C restatement in libacfe."""
    out = np.zeros((int(n_mels), 1 + int(n_fft) // 2), dtype=np.float32)
    call("acfe_mel_filterbank", int(sr), int(n_mels), float(fmin), float(fmax), int(n_fft), float(break_freq),
         out.ctypes.data_as(C.c_void_p))
    return out


class MelPlan:
    """Device plan (twiddles, window, banded filterbank) for one feature config.

    Equivalent of the reference's module globals MEL_WEIGHTS / NFFT /
    HOP_LENGTH set by tfdataset.get_dataset (tfdataset.py:430-460)."""

    def __init__(self, sr=48000, n_fft=4096, hop=281, n_mels=128, fmin=100, fmax=11000, break_freq=1000,
                 weights: np.ndarray | None = None, device=None):
        self.sr, self.n_fft, self.hop, self.n_mels = int(sr), int(n_fft), int(hop), int(n_mels)
        self.fmin, self.fmax, self.break_freq = fmin, fmax, break_freq
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if weights is None:
            weights = mel_filterbank(sr, n_mels, fmin, fmax, n_fft, break_freq)
        self.weights = np.ascontiguousarray(weights, dtype=np.float32)
        if self.weights.shape != (self.n_mels, 1 + self.n_fft // 2):
            raise ValueError(f"weights shape {self.weights.shape} does not match n_mels/n_fft")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            call("acfe_plan_create", self.sr, self.n_fft, self.hop, self.n_mels, float(fmin), float(fmax),
                 float(break_freq), self.weights.ctypes.data_as(C.c_void_p), C.byref(h))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        # at interpreter shutdown the module globals may already be gone
        if h is not None and h.value and lib is not None:
            lib.acfe_plan_destroy(h)
            self._h = None

    def num_frames(self, n_samples: int, pad_mode: str = "end") -> int:
        return call("acfe_plan_num_frames", self._h, int(n_samples), PAD_MODES[pad_mode])

    def mel(self, raw: torch.Tensor, stats: torch.Tensor | None = None, pad_mode="end", power=2,
            layout="btm", n: int | None = None, clip_stride: int | None = None, batch: int | None = None,
            out: torch.Tensor | None = None, timer: list | None = None) -> torch.Tensor:
        """raw [B, N] fp32 (or a 1-D recording with explicit n / clip_stride / batch
        for overlapping windows) -> mel [B,T,M] ("btm") or [B,M,T] ("bmt")."""
        require_cuda(raw, stats)
        if raw.dtype != torch.float32:
            raise TypeError("raw audio must be float32")
        if raw.dim() == 2 and n is None:
            batch, n, clip_stride = raw.shape[0], raw.shape[1], raw.shape[1]
        if n is None or clip_stride is None or batch is None:
            raise ValueError("1-D input needs n, clip_stride and batch")
        if raw.numel() < (batch - 1) * clip_stride + n:
            raise ValueError("raw buffer too small for batch/clip_stride/n")
        t = self.num_frames(n, pad_mode)
        shape = (batch, t, self.n_mels) if layout == "btm" else (batch, self.n_mels, t)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=raw.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("bad out tensor")
        e0 = None
        if timer is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        call("acfe_mel_fwd", self._h, ptr(raw), int(clip_stride), int(batch), int(n), ptr(stats),
             PAD_MODES[pad_mode], int(power), ptr(out), _lib.LAYOUT_BTM if layout == "btm" else _lib.LAYOUT_BMT,
             stream())
        if timer is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            timer.append(("mel", e0, e1))
        return out


    def mel_from_spec(self, spec: torch.Tensor, power=1, layout="btm", out: torch.Tensor | None = None,
                      timer: list | None = None) -> torch.Tensor:
        """Stored magnitude spectrograms [B, F, T] fp32 (F = 1 + n_fft/2, the
        record's audio/spectogram reshaped (2049, 513), tfdataset.py:1082) ->
        mel = W . S^power [B,T,M] ("btm") or [B,M,T] ("bmt") (tfdataset.py:1089)."""
        require_cuda(spec)
        if spec.dtype != torch.float32 or spec.dim() != 3 or not spec.is_contiguous():
            raise TypeError("spectrograms must be contiguous float32 [B, F, T]")
        b, f, t = spec.shape
        if f != self.n_fft // 2 + 1:
            raise ValueError(f"expected {self.n_fft // 2 + 1} frequency bins, got {f}")
        shape = (b, t, self.n_mels) if layout == "btm" else (b, self.n_mels, t)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=spec.device)
        e0 = None
        if timer is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        call("acfe_mel_from_spec", self._h, ptr(spec), f * t, b, f, t, int(power), ptr(out),
             _lib.LAYOUT_BTM if layout == "btm" else _lib.LAYOUT_BMT, stream())
        if timer is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            timer.append(("mel", e0, e1))
        return out


def normalize_stats(x: torch.Tensor, n: int | None = None, clip_stride: int | None = None,
                    batch: int | None = None) -> torch.Tensor:
    """Per-clip {min, max(x-min)} (tfdataset.normalize reductions)."""
    require_cuda(x)
    if x.dim() == 2 and n is None:
        batch, n, clip_stride = x.shape[0], x.shape[1], x.shape[1]
    st = torch.empty((batch, 2), dtype=torch.float32, device=x.device)
    call("acfe_normalize_stats", ptr(x), int(clip_stride), int(batch), int(n), ptr(st), stream())
    return st


def normalize_apply(x: torch.Tensor, st: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """(x - min) / max(x - min) per clip with precomputed stats; [B, N] fp32."""
    require_cuda(x, st)
    y = torch.empty_like(x) if out is None else out
    call("acfe_normalize_apply", ptr(x), x.shape[1], x.shape[0], x.shape[1], ptr(st), ptr(y), stream())
    return y


def normalize(x: torch.Tensor) -> torch.Tensor:
    """tfdataset.normalize (tfdataset.py:1916-1934) on [B, N] fp32."""
    return normalize_apply(x, normalize_stats(x))


def normalize_windows(rec: torch.Tensor, plan, n: int, out: torch.Tensor | None = None,
                      stats: torch.Tensor | None = None) -> torch.Tensor:
    """The normalised windows [n_windows, n] that the host table `plan`
    ((src, count, pad) rows, predict.track_window_plan) cuts from the 1-D fp32
    device recording `rec`: tfdataset.normalize of each zero-padded window
    v[i] = rec[src + i - pad] (pad <= i < pad + count, 0 elsewhere),
    bit-identical to normalize() of the windows cut on the host.  The table
    is validated on the host (predict.check_window_plan) before it is
    uploaded.  `stats` [n_windows, 2] receives {min, max - min} per window
    when given."""
    from predict import check_window_plan  # host-only index arithmetic, next to track_window_plan

    require_cuda(rec, out, stats)
    if rec.dtype != torch.float32 or rec.dim() != 1 or not rec.is_contiguous():
        raise TypeError("the recording must be a contiguous 1-D float32 tensor")
    n = int(n)
    if n <= 0:
        raise ValueError("n must be positive")
    plan = check_window_plan(plan, rec.numel(), n)
    batch = plan.shape[0]
    if out is None:
        out = torch.empty((batch, n), dtype=torch.float32, device=rec.device)
    elif tuple(out.shape) != (batch, n) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("bad out tensor")
    if stats is not None and (tuple(stats.shape) != (batch, 2) or stats.dtype != torch.float32
                              or not stats.is_contiguous()):
        raise ValueError("bad stats tensor")
    if batch == 0:
        return out
    dplan = torch.from_numpy(plan).to(rec.device)
    call("acfe_windows_normalize", ptr(rec), rec.numel(), ptr(dplan), batch, n, ptr(out), ptr(stats), stream())
    return out


def sosfilt_segments(rec: torch.Tensor, seg, sos, out: torch.Tensor | None = None) -> torch.Tensor:
    """scipy.signal.sosfilt of segments of the 1-D fp32 device recording
    `rec`, each with its own filter, as one packed float32 device buffer:
    out[dst + i] = float32(sosfilt(sos[k], float64(rec[src : src + len]))[i])
    for the rows (src, len, dst) of the host table `seg` [n_seg, 3] and the
    float64 second-order sections `sos` [n_seg, 2, 6]
    (predict.sos_segment_plan; two identity sections copy the segment bit for
    bit).  Computed in float64 by the chunked scan of csrc/sosfilt.hip, from a
    zero state at each segment's first sample.  Both tables are validated on
    the host (predict.check_sos_segments) before they are uploaded.  `out`
    defaults to a new buffer of max(dst + len) rounded up to 4 floats;
    elements of it that no segment covers are left as they were."""
    from predict import check_sos_segments  # host-only index arithmetic, next to sos_segment_plan

    require_cuda(rec, out)
    if rec.dtype != torch.float32 or rec.dim() != 1 or not rec.is_contiguous():
        raise TypeError("the recording must be a contiguous 1-D float32 tensor")
    if out is not None and (out.dim() != 1 or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError("bad out tensor")
    seg = np.ascontiguousarray(seg, np.int64)
    if seg.ndim != 2 or seg.shape[1] != 3:
        raise ValueError(f"segment table must be [n_seg, 3], got {seg.shape}")
    if out is not None:
        out_len = out.numel()
    elif len(seg):  # clipped so that a bad row reaches check_sos_segments' message, not an overflow here
        out_len = int((np.clip(seg[:, 1], 0, 2**40) + np.clip(seg[:, 2], 0, 2**40)).max() + 3) & ~3
    else:
        out_len = 0
    seg, sos = check_sos_segments(seg, sos, rec.numel(), out_len)
    if out is None:
        out = torch.empty(out_len, dtype=torch.float32, device=rec.device)
    n_seg = seg.shape[0]
    if n_seg == 0 or out_len == 0:
        return out
    nbytes = lib.acfe_sosfilt_workspace(out_len, n_seg)
    _lib.check(nbytes, "acfe_sosfilt_workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=rec.device)
    dseg = torch.from_numpy(seg).to(rec.device)
    dsos = torch.from_numpy(sos).to(rec.device)
    call("acfe_sosfilt_segments", ptr(rec), rec.numel(), ptr(dseg), ptr(dsos), n_seg, ptr(out), out_len, ptr(ws),
         stream())
    return out


_RESAMPLE_TAPS: dict = {}  # (rate, sr, device) -> (ResamplePlan, its taps on the device)


def resample_poly(x: torch.Tensor, rate: int, sr: int = 48000, out: torch.Tensor | None = None) -> torch.Tensor:
    """scipy.signal.resample_poly(x, sr // g, rate // g), g = gcd(rate, sr), of
    the 1-D device recording `x` sampled at `rate` -> float32 [n_out] at `sr`
    (the resampling of predict.load_recording, on the device).  x is float32,
    or int16 PCM, which enters as float32(v) / 32767 -- bit-identical to
    converting on the host first.  The taps and the index arithmetic are
    scipy's (predict.resample_plan; the taps are uploaded once per (rate, sr,
    device)); every output is summed in float64 and rounded to float32 once
    (csrc/resample.hip).  rate == sr returns a float32 x itself and converts
    an int16 x with the same kernel.  ValueError for a rate whose filter has
    more taps than the kernel stages (plan.device is False)."""
    from predict import resample_plan  # host-only filter design and index arithmetic

    require_cuda(x, out)
    if x.dim() != 1 or x.dtype not in (torch.float32, torch.int16):
        raise TypeError("the recording must be a contiguous 1-D float32 or int16 tensor")
    key = (int(rate), int(sr), x.device)
    if key not in _RESAMPLE_TAPS:
        plan = resample_plan(rate, sr)
        _RESAMPLE_TAPS[key] = (plan, torch.from_numpy(plan.h).to(x.device) if plan.device else None)
    plan, taps = _RESAMPLE_TAPS[key]
    if not plan.device:
        raise ValueError(f"{rate} -> {sr} Hz needs {len(plan.h)} filter taps, more than the device resampler's "
                         "16384: resample on the host")
    n_out = plan.n_out(x.numel())
    if out is not None and (tuple(out.shape) != (n_out,) or out.dtype != torch.float32):
        raise ValueError("bad out tensor")
    if plan.up == plan.down and x.dtype == torch.float32 and out is None:
        return x
    if out is None:
        out = torch.empty(n_out, dtype=torch.float32, device=x.device)
    code = _lib.DTYPE_F32 if x.dtype == torch.float32 else _lib.DTYPE_I16
    call("acfe_resample_poly", ptr(x), code, x.numel(), ptr(taps), len(plan.h), plan.up, plan.down, plan.t0,
         ptr(out), n_out, stream())
    return out


def mix_up(x1, x2, lam, stats1=None, stats2=None) -> torch.Tensor:
    """tfdataset.mix_up image blend (tfdataset.py:950); lam [B] fp32 on device."""
    require_cuda(x1, x2, lam, stats1, stats2)
    y = torch.empty_like(x1)
    call("acfe_mixup", ptr(x1), ptr(stats1), ptr(x2), ptr(stats2), ptr(lam), x1.shape[0], x1.shape[1], ptr(y),
         stream())
    return y


def sample_mixup_lambda(batch, alpha=0.5, chance=0.25, device=None) -> torch.Tensor:
    """tfdataset.sample_beta_distribution(batch, alpha, alpha) * 1[U < chance]
    (tfdataset.py:920-946); drawn on the host from torch's global generator."""
    gam = torch.distributions.Gamma(torch.tensor(float(alpha)), torch.tensor(1.0))
    g1, g2 = gam.sample((batch,)), gam.sample((batch,))
    lam = g1 / (g1 + g2)
    aug = (torch.rand(batch) < chance).float()
    return (lam * aug).to(torch.float32).to(device if device is not None else "cpu")


class _PCENFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mel_btm, params, eps, out_dtype, scope_minmax):
        require_cuda(mel_btm, params)
        b, t, m = mel_btm.shape
        dev = mel_btm.device
        npart = lib.acfe_pcen_partials(b, m)
        y = torch.empty((b, m, t), dtype=torch.float32, device=dev)
        part = torch.empty(2 * npart, dtype=torch.float32, device=dev)
        s = stream()
        call("acfe_pcen_fwd", ptr(mel_btm), b, t, m, ptr(params), float(eps), ptr(y), ptr(part), s)
        out = torch.empty((b, m, t), dtype=out_dtype, device=dev)
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        call("acfe_pcen_normalize", ptr(y), y.numel(), ptr(part), npart, ptr(scope_minmax), ptr(out),
             dtype_code(out_dtype), ptr(stats), s)
        ctx.save_for_backward(mel_btm, params, stats)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dout):
        mel_btm, params, stats = ctx.saved_tensors
        b, t, m = mel_btm.shape
        dout = dout.contiguous()
        npart = lib.acfe_pcen_partials(b, m)
        ws = torch.empty(32 * npart, dtype=torch.float32, device=dout.device)
        dparams = torch.empty(4, dtype=torch.float32, device=dout.device)
        call("acfe_pcen_bwd", ptr(mel_btm), b, t, m, ptr(params), float(ctx.eps), ptr(stats), ptr(dout),
             dtype_code(dout.dtype), ptr(ws), ptr(dparams), stream())
        return None, dparams, None, None, None


def check_pcen_segments(seg_start, batch: int) -> np.ndarray:
    """A segment table of acfe_pcen_normalize_segments (predict.pcen_segments'
    form) as contiguous int32, after checking it against a launch of `batch`
    clips: ValueError unless it is 1-D with at least 2 entries, starts at 0,
    never decreases and ends at batch.  Segment s is the clips
    [seg_start[s], seg_start[s + 1]); an empty segment is allowed."""
    seg = np.asarray(seg_start)
    if seg.ndim != 1 or len(seg) < 2:
        raise ValueError(f"segment table must be 1-D with at least 2 offsets, got shape {seg.shape}")
    if not np.issubdtype(seg.dtype, np.integer):
        raise ValueError(f"segment table must hold integers, got {seg.dtype}")
    seg = seg.astype(np.int64)
    if seg[0] != 0 or seg[-1] != batch:
        raise ValueError(f"segment table must run from 0 to the batch of {batch}, got {int(seg[0])} .. {int(seg[-1])}")
    if (np.diff(seg) < 0).any():
        k = int(np.flatnonzero(np.diff(seg) < 0)[0])
        raise ValueError(f"segment table decreases at entry {k + 1}: {int(seg[k])} -> {int(seg[k + 1])}")
    return np.ascontiguousarray(seg, np.int32)


def pcen_normalize_segments(y_bmt: torch.Tensor, segments, out_dtype=torch.float32):
    """normalize_minmax (tfpcen.py:105-110) of acfe_pcen_fwd's un-normalised
    output y [B, M, T] per segment of the host table `segments`
    (check_pcen_segments) -> (out [B, M, T] of out_dtype, seg_minmax
    [n_seg, 2] fp32 {min, max}).  Each segment is normalised by the extrema of
    its own clips, bit-identical to normalising those clips alone
    (csrc/pcen_scope.hip)."""
    require_cuda(y_bmt)
    if y_bmt.dtype != torch.float32 or y_bmt.dim() != 3 or not y_bmt.is_contiguous():
        raise TypeError("y must be a contiguous [B, M, T] float32 tensor")
    b, clip = y_bmt.shape[0], y_bmt.shape[1] * y_bmt.shape[2]
    seg = check_pcen_segments(segments, b)
    n_seg = len(seg) - 1
    if n_seg > b:
        raise ValueError(f"{n_seg} segments for a batch of {b}: drop the empty ones")
    dev = y_bmt.device
    out = torch.empty(y_bmt.shape, dtype=out_dtype, device=dev)
    seg_minmax = torch.empty((n_seg, 2), dtype=torch.float32, device=dev)
    nbytes = lib.acfe_pcen_segments_workspace(b, clip)
    _lib.check(nbytes, "acfe_pcen_segments_workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dseg = torch.from_numpy(seg).to(dev)
    call("acfe_pcen_normalize_segments", ptr(y_bmt), b, clip, ptr(dseg), n_seg, ptr(out), dtype_code(out_dtype),
         ptr(seg_minmax), ptr(ws), stream())
    return out, seg_minmax


def pcen(mel_btm: torch.Tensor, params: torch.Tensor, eps: float = 1e-6, out_dtype=torch.float32,
         scope_minmax: torch.Tensor | None = None, segments=None) -> torch.Tensor:
    """tfpcen.PCEN.call + normalize_minmax: mel [B,T,M] -> normalised [B,M,T].
    The min / max are those of the whole batch, or `scope_minmax` when given.
    With `segments` (a host table of offsets, check_pcen_segments) every
    segment of clips is normalised by its own extrema instead, as if it had
    been a batch of its own; that form is inference only (no backward), and
    excludes scope_minmax."""
    if segments is None:
        return _PCENFunction.apply(mel_btm.contiguous(), params, eps, out_dtype, scope_minmax)
    if scope_minmax is not None:
        raise ValueError("segments and scope_minmax exclude each other")
    if torch.is_grad_enabled() and params.requires_grad:
        raise RuntimeError("PCEN with segments is inference only: run it under torch.no_grad()")
    mel_btm = mel_btm.contiguous()
    require_cuda(mel_btm, params)
    b, t, m = mel_btm.shape
    seg = check_pcen_segments(segments, b)  # before any launch
    npart = lib.acfe_pcen_partials(b, m)
    y = torch.empty((b, m, t), dtype=torch.float32, device=mel_btm.device)
    part = torch.empty(2 * npart, dtype=torch.float32, device=mel_btm.device)
    call("acfe_pcen_fwd", ptr(mel_btm), b, t, m, ptr(params), float(eps), ptr(y), ptr(part), stream())
    return pcen_normalize_segments(y, seg, out_dtype)[0]


class PCEN(torch.nn.Module):
    """Trainable PCEN (tfpcen.py:42-99). Parameters packed as one device vector
    {gain 0.98, bias 2.0, root 2.0, smooth 0.04}; eps = 1e-6.  The unused
    `a-power` weight of the reference (tfpcen.py:78-86) is kept for checkpoint
    compatibility but does not enter the computation, as in the reference."""

    def __init__(self, gain=0.98, bias=2.0, root=2.0, smooth=0.04, eps=1e-6, out_dtype=torch.float32):
        super().__init__()
        self.params = torch.nn.Parameter(torch.tensor([gain, bias, root, smooth], dtype=torch.float32))
        self.a_power = torch.nn.Parameter(torch.tensor([-1.0]), requires_grad=False)
        self.eps = eps
        self.out_dtype = out_dtype

    def forward(self, mel_btm, scope_minmax=None, segments=None):
        return pcen(mel_btm, self.params, self.eps, self.out_dtype, scope_minmax, segments)
