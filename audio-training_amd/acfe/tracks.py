"""Track detection of the predict path on the GPU: the device form of
identifytracks.get_end (reference identifytracks.py:21-48) and signal_noise
(:51-143), executing the kernels of csrc/tracks.hip through the C ABI.

The recording is uploaded once.  |STFT| (n_fft 2048, hop 281), its maximum,
the exact medians along both axes, the threshold map, the four box morphology
passes and the run extraction all stay on the device; only the run list (a few
thousand triples per minute of audio) and get_end's chunk flags come back.
The host then unions the runs into 8-connected components and filters them
with the same code the host detector uses (identifytracks.boxes_from_runs,
signals_from_stats), so for one and the same spectrogram both detectors
return the same signals in the same order.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call, lib
from ._torch import ptr, require_cuda, stream

N_FFT = 2048  # identifytracks.py:55
HOP = 281
ERODE, DILATE = 0, 1


def _image(t: torch.Tensor, dtype) -> tuple[int, int]:
    require_cuda(t)
    if t.dtype != dtype or t.dim() != 2 or t.numel() == 0:
        raise TypeError(f"expected a non-empty 2-D {dtype} device tensor")
    return t.shape


def median(img: torch.Tensor, axis: int, scale: torch.Tensor | None = None) -> torch.Tensor:
    """np.median(img / scale, axis) of a finite, non-negative float32 image,
    exact (acfe_median); scale is a one-element device tensor or None."""
    rows, cols = _image(img, torch.float32)
    require_cuda(scale)
    out = torch.empty(rows if axis == 1 else cols, dtype=torch.float32, device=img.device)
    call("acfe_median", ptr(img), rows, cols, int(axis), ptr(scale), ptr(out), stream())
    return out


def morph_box(src: torch.Tensor, h: int, w: int, op: int, out: torch.Tensor | None = None,
              ws: torch.Tensor | None = None) -> torch.Tensor:
    """cv2.erode (op ERODE) / cv2.dilate (op DILATE) of a 0 / 1 uint8 map with
    an h x w box (acfe_morph_box)."""
    rows, cols = _image(src, torch.uint8)
    if out is None:
        out = torch.empty_like(src)
    if ws is None:
        ws = torch.empty(lib.acfe_morph_box_workspace(rows, cols), dtype=torch.uint8, device=src.device)
    call("acfe_morph_box", ptr(src), rows, cols, int(h), int(w), int(op), ptr(out), ptr(ws), stream())
    return out


def map_runs(m: torch.Tensor, capacity: int | None = None) -> np.ndarray:
    """The horizontal runs (row, first col, last col) of a 0 / 1 uint8 map as
    a host int32 [n, 3] array (acfe_map_runs).  When the first buffer of
    `capacity` runs is too small, the call is repeated once with the count the
    first one reported."""
    rows, cols = _image(m, torch.uint8)
    cap = max(1, 4 * cols) if capacity is None else int(capacity)
    count = torch.empty(1, dtype=torch.int32, device=m.device)
    for _ in range(2):
        runs = torch.empty((cap, 3), dtype=torch.int32, device=m.device)
        call("acfe_map_runs", ptr(m), rows, cols, ptr(runs), cap, ptr(count), stream())
        n = int(count.item())
        if n <= cap:
            return runs[:n].cpu().numpy()
        cap = n
    raise _lib.AcfeError(f"acfe_map_runs: {n} runs after a retry sized for them")


class SignalDetector:
    """get_end and signal_noise of one recording on the device.

    `frames` is a 1-D float32 numpy array or device tensor; upload() moves a
    host array to the device once and every method accepts its result.  With
    `timer` set to a list, each stage appends (name, start event, end event)."""

    def __init__(self, device=None, sr=48000):
        from identifytracks import box_geometry

        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.sr = int(sr)
        self.freqs, self.height, self.width = box_geometry(self.sr, HOP, N_FFT)
        self.timer: list | None = None
        self._mel_plan = None
        self._amax = None  # (spectrogram, its maximum) of the last spectrogram() call

    def _stage(self, name, fn):
        if self.timer is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.timer.append((name, e0, e1))
        return out

    def upload(self, frames) -> torch.Tensor:
        if isinstance(frames, torch.Tensor):
            x = frames.to(self.device, torch.float32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).to(self.device)
        if x.dim() != 1:
            raise ValueError("a recording is one 1-D array of samples")
        return x.contiguous()

    def spectrogram(self, frames) -> torch.Tensor:
        """|librosa.stft(frames, 2048, 281)| -> float32 [1025, 1 + n // 281]."""
        x = self.upload(frames)
        n = x.numel()
        nbytes = lib.acfe_stft_mag_workspace(n, N_FFT, HOP)
        _lib.check(nbytes, "acfe_stft_mag_workspace")
        spec = torch.empty((1 + N_FFT // 2, 1 + n // HOP), dtype=torch.float32, device=self.device)
        amax = torch.empty(1, dtype=torch.float32, device=self.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._stage("stft", lambda: call("acfe_stft_mag", ptr(x), n, N_FFT, HOP, ptr(spec), ptr(amax), ptr(ws),
                                         stream()))
        self._amax = (spec, amax)
        return spec

    def _max_of(self, spec):
        if self._amax is None or self._amax[0] is not spec:
            raise ValueError("signal_map / boxes take the spectrogram of this detector's last spectrogram() call "
                             "(its maximum comes from the STFT kernel)")
        return self._amax[1]

    def signal_map(self, spec: torch.Tensor) -> torch.Tensor:
        """The final binary map of signal_noise (:78-99) as uint8 [1025, T]:
        threshold against the two medians, open 4x4, dilate height x width,
        erode (height // 10) x width.  `spec` is the tensor the last
        spectrogram() call returned."""
        rows, cols = _image(spec, torch.float32)
        amax = self._max_of(spec)
        col_med = self._stage("median_frames", lambda: median(spec, 0, amax))
        row_med = self._stage("median_rows", lambda: median(spec, 1, amax))
        a = torch.empty((rows, cols), dtype=torch.uint8, device=spec.device)
        b = torch.empty_like(a)
        ws = torch.empty(lib.acfe_morph_box_workspace(rows, cols), dtype=torch.uint8, device=spec.device)
        self._stage("signal_map", lambda: call("acfe_signal_map", ptr(spec), rows, cols, ptr(amax), ptr(col_med),
                                               ptr(row_med), ptr(a), stream()))

        def morphology():
            morph_box(a, 4, 4, ERODE, b, ws)  # MORPH_OPEN
            morph_box(b, 4, 4, DILATE, a, ws)
            morph_box(a, self.height, self.width, DILATE, b, ws)
            return morph_box(b, self.height // 10, self.width, ERODE, a, ws)

        return self._stage("morphology", morphology)

    def boxes(self, spec: torch.Tensor, run_capacity: int | None = None):
        """Component stats [(left, top, width, height, area)] of the final map,
        in signal_noise's order (sorted by left)."""
        from identifytracks import boxes_from_runs

        m = self.signal_map(spec)
        runs = self._stage("runs", lambda: map_runs(m, run_capacity))
        return boxes_from_runs(runs)

    def signal_noise(self, frames):
        """identifytracks.signal_noise -> (signals, device |STFT|)."""
        from identifytracks import signals_from_stats

        spec = self.spectrogram(frames)
        return signals_from_stats(self.boxes(spec), self.sr, self.freqs, self.height, self.width), spec

    def get_end(self, frames):
        """identifytracks.get_end: seconds of real data before a digitally
        silent tail, from the 120-band mel image of the front-end kernel."""
        from identifytracks import get_nfft

        from .frontend import MelPlan

        x = self.upload(frames)
        n = x.numel()
        if self._mel_plan is None:
            self._mel_plan = MelPlan(sr=self.sr, n_fft=get_nfft(self.sr), hop=HOP, n_mels=120, fmin=50, fmax=11000,
                                     break_freq=1750, device=self.device)
        chunk = self.sr // HOP
        t = 1 + n // HOP
        n_chunks = (t - 1) // chunk  # the chunks with end < T (:41)
        if n_chunks > 0:
            mel = self._stage("mel", lambda: self._mel_plan.mel(x[None], pad_mode="constant", power=1, layout="bmt"))
            flags = torch.empty(n_chunks, dtype=torch.int32, device=self.device)
            self._stage("chunk_flat", lambda: call("acfe_chunk_flat", ptr(mel), 120, t, chunk, n_chunks, ptr(flags),
                                                   stream()))
            silent = np.flatnonzero(flags.cpu().numpy())
            if len(silent):
                return int(silent[0]) * chunk * HOP // self.sr
        return n / self.sr
