#!/usr/bin/env python3
"""Inference driver of the acfe path (reference predict.py:726-967,
predict_utils.py:9-239).

  python predict.py --file REC.wav CHECKPOINT_DIR [--stride 1] [--batch-size 1024] [--detector gpu]
                    [--windows device] [--filter-freqs | --filter-below HZ] [--resample device]
                    [--pcen-scope {batch,track,window}]

The recording is decoded on the host (WAV via scipy; the reference's ffmpeg /
librosa loader is out of scope) and resampled to 48 kHz: with scipy's
resample_poly on the host (--resample host, the default), or with --resample
device by the HIP kernel of acfe_resample_poly, which applies the same taps at
the same indices to the uploaded samples (an int16 mono file is uploaded as
int16, half the bytes) and sums every output in float64.  The 48 kHz
recording is then a device tensor: with --detector gpu and --windows device
it never passes through host memory, otherwise it is downloaded once.  A rate
whose filter is longer than 16384 taps (44 101 Hz, say) is resampled on the
host with a warning.

--mode tracks (default, the reference's predict.py:735-956): the digitally
silent tail is cut (get_end) and signals are detected -- on the host with
numpy (--detector host, the default) or on the GPU (--detector gpu: the
recording is uploaded once and acfe.tracks runs the STFT, the medians, the
morphology and the run extraction as HIP kernels, returning the same signals
for the same spectrogram) --, the signals are merged into tracks on the host
(identifytracks.py), each track is cut into 3 s windows at a 1 s
stride (predict_utils.load_samples:59-150: short tracks centred in a 3 s
window, partial windows zero padded at a random offset), the windows of all
tracks go to the GPU as one batch (normalize, librosa-style centred STFT with
constant padding, |X|^2, mel, PCEN: predict_utils.get_spect) and the mean
sigmoid output per track is thresholded at 0.7, else the argmax becomes the
raw tag (predict.py:931-956).  With --windows device the host computes only
where each window lies (track_window_plan: source sample, length and left
padding per window, the same arithmetic and the same random offsets) and one
HIP kernel cuts, zero pads and normalises the windows straight out of the
uploaded recording -- with --detector gpu the buffer the detector already
holds -- so no window passes through host memory; the predictions are those
of --windows host, which stays the default.

--filter-freqs runs every track's audio through a second-order Butterworth
band-pass at the track's own [freq_start, freq_end] before its windows are cut
(predict_utils.load_samples:103-113, butter_bandpass :245-262);
--filter-below HZ does so only for tracks with freq_end < HZ.  With --windows
host this is scipy's sosfilt on the host; with --windows device the filter is
the float64 HIP scan of acfe_sosfilt_segments, which writes the filtered tracks
into one packed device buffer that the window kernel then reads, so the audio
still never passes through host memory.  Both are off by default.

--mode windows: the recording is uploaded once and 3 s windows every
`stride` seconds are read in place by the fused front-end kernel; the
per-recording result is the mean of the window probabilities.

--pcen-scope: PCEN (if the model was trained with it) ends in
normalize_minmax, which scales its output by the min / max of everything the
layer is given at once (tfpcen.py:105-110).  Which windows that is:
  batch  (default) each launch of up to --batch-size windows of the recording,
         all tracks together: a track's features depend on --batch-size and on
         what else the recording holds.
  track  each track's own windows, in runs of at most 32: what the reference
         computes, whose model.predict runs once per track (predict.py:887)
         and is cut into batches of 32 by Keras.  Tracks are split at 6 s, so
         in practice this is one min / max per track.  --mode tracks only.
  window each window by itself: a window's features depend on nothing else.
The launches keep their size under every scope (they are cut at segment
boundaries, never inside one); the kernels of acfe_pcen_normalize_segments take
the extrema per segment of a launch and normalise each segment as if it had
been a launch of its own, bit for bit.
"""
from __future__ import annotations

import argparse
import json
import logging
import math
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR = 48000


RESAMPLE_MAX_TAPS = 16384  # what acfe_resample_poly stages in LDS (64 KiB of float32 taps)


class ResamplePlan:
    """The FIR taps and index arithmetic of scipy.signal.resample_poly(x, up,
    down) for a float32 x and its default window and padding (resample_plan).
    With x[j] = 0 outside [0, n_in):
      t = n * down + t0;  p = t % up;  j0 = t // up
      out[n] = sum over k >= 0 with p + k * up < len(h) of h[p + k * up] * x[j0 - k]
    for n < n_out(n_in).  device: whether acfe.frontend.resample_poly takes
    the plan (len(h) <= RESAMPLE_MAX_TAPS)."""

    def __init__(self, rate, sr, up, down, h, t0):
        self.rate, self.sr, self.up, self.down, self.h, self.t0 = rate, sr, up, down, h, t0
        self.terms = -(-len(h) // up)  # the most taps that meet one output (K)
        self.device = len(h) <= RESAMPLE_MAX_TAPS

    def n_out(self, n_in):
        return -(-int(n_in) * self.up // self.down)


def resample_plan(rate, sr=SR):
    """What resample_poly(x, sr // g, rate // g), g = gcd(rate, sr), computes
    with, as a ResamplePlan: scipy's own float32 taps (firwin over
    2 * half_len + 1 points with a Kaiser(5.0) window, times up) bit for bit,
    and the offset t0 that its zero pre-padding of h and the outputs it then
    drops amount to.  rate == sr is the identity: the one tap 1.0, t0 = 0."""
    from scipy.signal import firwin

    rate, sr = int(rate), int(sr)
    if rate < 1 or sr < 1:
        raise ValueError(f"sample rates must be positive, got {rate} -> {sr}")
    g = math.gcd(rate, sr)
    up, down = sr // g, rate // g
    if up == down:
        return ResamplePlan(rate, sr, 1, 1, np.ones(1, np.float32), 0)
    half_len = 10 * max(up, down)
    h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    return ResamplePlan(rate, sr, up, down, h, n_pre_remove * down - n_pre_pad)


def _float_mono(data):
    """Decoded WAV samples as float32 mono: integer PCM over its positive
    full scale, channels averaged."""
    if np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max)
    data = data.astype(np.float32)
    if data.ndim > 1:
        data = data.mean(1)
    return data


def load_recording(path, sr=SR, resample="host", device=None):
    """predict.load_recording (predict.py:59-66) for WAV input -> float32
    samples at `sr`.  resample "host": scipy's resample_poly, a numpy array.
    "device": the decoded samples are uploaded to `device` (default: the
    current one) -- an int16 mono file as int16, anything else as float32
    after the host conversion and channel mean -- and resampled there by
    acfe.frontend.resample_poly; the result is a 1-D float32 device tensor
    (also for a file already at `sr`, which is only uploaded).  A rate whose
    filter the kernel does not take (resample_plan(rate, sr).device is False)
    logs one warning and gives the host result."""
    from scipy.io import wavfile
    from scipy.signal import resample_poly

    if resample not in ("host", "device"):
        raise ValueError(f"resample {resample!r}: expected 'host' or 'device'")
    rate, data = wavfile.read(path)
    if resample == "device":
        if resample_plan(rate, sr).device:
            from acfe import frontend as fe

            device = device or torch.device("cuda", torch.cuda.current_device())
            if data.dtype != np.int16 or data.ndim != 1:
                data = _float_mono(data)
            return fe.resample_poly(torch.from_numpy(np.ascontiguousarray(data)).to(device), rate, sr)
        logging.warning("%s: %d -> %d Hz needs more than %d filter taps, resampling on the host", path, rate, sr,
                        RESAMPLE_MAX_TAPS)
    data = _float_mono(data)
    if rate != sr:
        g = math.gcd(rate, sr)
        data = resample_poly(data, sr // g, rate // g).astype(np.float32)
    return data


class ModelResult:
    """predict.ModelResult (predict.py:1103-1120)."""

    def __init__(self, model):
        self.model = model
        self.labels, self.confidences = [], []
        self.raw_tag = self.raw_confidence = None

    def get_meta(self):
        meta = {"model": self.model, "species": self.labels, "likelihood": self.confidences}
        if self.raw_tag is not None:
            meta["raw_tag"] = self.raw_tag
            meta["raw_confidence"] = self.raw_confidence
        return meta


def butter_bandpass(lowcut, highcut, fs, order=2):
    """The Butterworth filter of one track as float64 second-order sections
    [n_sections, 6], or None for no filter.  For arguments scipy.signal.butter
    accepts this is predict_utils.butter_bandpass (:245-256): lowcut > 0 gives
    a "bandpass" [lowcut, highcut] (2 sections for order 2), otherwise a
    "lowpass" at highcut (1 section).  Signal.extend can push a track's
    freq_end past Nyquist, where that function raises inside scipy; those
    inputs follow the reference's other copy (audiodataset.py:1347-1377):
    highcut >= fs / 2 (or None) with a usable lowcut gives a "highpass" at
    lowcut (1 section); no usable edge (neither 0 < lowcut < fs / 2 nor
    0 < highcut < fs / 2), or highcut <= lowcut, gives None and the track is
    left unfiltered.  Each departure from the plain band-pass / low-pass logs
    one line."""
    from scipy.signal import butter

    nyq = 0.5 * fs
    low = lowcut if lowcut is not None and 0 < lowcut < nyq else None
    if highcut is not None and highcut <= (lowcut or 0):
        logging.warning("No freq to filter: band [%s, %s]", lowcut, highcut)
        return None
    if highcut is not None and highcut < nyq:
        if low is not None:
            return butter(order, [low / nyq, highcut / nyq], analog=False, btype="bandpass", output="sos")
        return butter(order, highcut / nyq, analog=False, btype="lowpass", output="sos")
    if low is None:
        logging.warning("No freq to filter: band [%s, %s] at fs %s", lowcut, highcut, fs)
        return None
    logging.warning("Band [%s, %s] reaches Nyquist (%s): high-pass at %s", lowcut, highcut, nyq, lowcut)
    return butter(order, low / nyq, analog=False, btype="highpass", output="sos")


def butter_bandpass_filter(data, lowcut, highcut, fs, order=2):
    """sosfilt of `data` with butter_bandpass (predict_utils.py:259-262) as
    float64, from a zero initial state; None when there is no filter."""
    from scipy.signal import sosfilt

    sos = butter_bandpass(lowcut, highcut, fs, order=order)
    return None if sos is None else sosfilt(sos, data)


def track_sos(t, sr, filter_freqs=False, filter_below=None):
    """The filter load_samples (:103-113) applies to track t: butter_bandpass of
    its band when filter_freqs is set, or when filter_below is and the track
    ends under it; None for a track that stays unfiltered."""
    if filter_freqs or (filter_below and t.freq_end is not None and t.freq_end < filter_below):
        return butter_bandpass(t.freq_start, t.freq_end, sr)
    return None


def track_windows(frames, sr, tracks, segment_length=3, stride=1, fmin=100, fmax=11000, pad_short_tracks=False,
                  rng=None, filter_freqs=False, filter_below=None):
    """The raw 3 s windows predict_utils.load_samples (:59-150) cuts from each
    track (before its normalize / spectrogram, which run on the GPU) ->
    list of [n_i, sr * segment_length] float32 arrays, one per track (empty
    for tracks wholly outside [fmin, fmax], which are not classified).
    filter_freqs / filter_below (track_sos): the whole clipped slice of the
    track is filtered before the window loop, from a zero state at its first
    sample, and cast back to float32, so the state carries across windows."""
    from scipy.signal import sosfilt

    rng = rng if rng is not None else np.random
    sample_size = int(sr * segment_length)
    frames = np.asarray(frames, np.float32)
    out = []
    for t in tracks:
        wins = []
        if t.freq_start is not None and t.freq_end is not None and (t.freq_start > fmax or t.freq_end < fmin):
            out.append(np.zeros((0, sample_size), np.float32))
            continue
        start, end = 0, segment_length
        sr_end, sr_start = int(t.end * sr), int(sr * t.start)
        if pad_short_tracks:
            end = min(end, t.length)  # predict_utils.py:75-77
            track_frames = frames[sr_start:sr_end]
        else:  # centre short tracks in one window
            missing = sample_size - (sr_end - sr_start)
            if missing > 0:
                offset = missing // 2
                sr_start -= offset
                if sr_start <= 0:
                    sr_start = 0
                    sr_end = min(sample_size, len(frames))
                else:
                    end_offset = sr_end + missing - offset
                    if end_offset > len(frames):
                        end_offset = len(frames)
                        sr_start = max(end_offset - sample_size, 0)
                    sr_end = end_offset
            track_frames = frames[sr_start:sr_end]
        sr_start, sr_end = 0, min(sr_end, sample_size)
        sos = track_sos(t, sr, filter_freqs, filter_below)
        if sos is not None and len(track_frames):
            track_frames = sosfilt(sos, track_frames).astype(np.float32)
        while True:
            data = track_frames[sr_start:sr_end]
            if len(data) != sample_size:
                extra = sample_size - len(data)
                off = int(rng.randint(0, extra))
                data = np.pad(data, (off, extra - off))
            wins.append(data)
            start += stride
            end = start + segment_length
            sr_start = int(start * sr)
            sr_end = min(int(end * sr), sr_start + sample_size)
            if end > t.length:  # always at least one window
                break
        out.append(np.stack(wins).astype(np.float32))
    return out


def track_window_plan(n_frames, sr, tracks, segment_length=3, stride=1, fmin=100, fmax=11000, pad_short_tracks=False,
                      rng=None, segments=False):
    """track_windows as a table instead of copies: the windows it would cut
    from a recording of n_frames samples -> (plan, counts).  plan is int64
    [n_windows, 3] with rows (src, count, pad): window w is
    v[i] = frames[src + i - pad] for pad <= i < pad + count and 0 elsewhere,
    i < n = int(sr * segment_length).  counts[k] is the number of windows of
    track k (0 for tracks outside [fmin, fmax]).  The arithmetic is
    track_windows' own, its numpy slices clipped as numpy clips them, and
    rng.randint is drawn once per partial window in the same order, so that
    applying the plan reproduces track_windows bit for bit.  An empty window
    (count 0) has src 0.  With segments=True the result is (plan, counts,
    segs): segs is int64 [n_tracks, 2] with rows (t0, t_len), the samples
    [t0, t0 + t_len) of the recording that track k's windows are cut from
    (track_windows' track_frames; (0, 0) for a track without windows)."""
    rng = rng if rng is not None else np.random
    sample_size = int(sr * segment_length)
    rows, counts, segs = [], [], []
    for t in tracks:
        if t.freq_start is not None and t.freq_end is not None and (t.freq_start > fmax or t.freq_end < fmin):
            counts.append(0)
            segs.append((0, 0))
            continue
        start, end = 0, segment_length
        sr_end, sr_start = int(t.end * sr), int(sr * t.start)
        if pad_short_tracks:
            end = min(end, t.length)
        else:
            missing = sample_size - (sr_end - sr_start)
            if missing > 0:
                offset = missing // 2
                sr_start -= offset
                if sr_start <= 0:
                    sr_start = 0
                    sr_end = min(sample_size, n_frames)
                else:
                    end_offset = sr_end + missing - offset
                    if end_offset > n_frames:
                        end_offset = n_frames
                        sr_start = max(end_offset - sample_size, 0)
                    sr_end = end_offset
        # track_frames = frames[sr_start:sr_end]: samples [t0, t0 + t_len) of the recording
        t0, t1, _ = slice(sr_start, sr_end).indices(n_frames)
        t_len = max(0, t1 - t0)
        segs.append((t0, t_len))
        sr_start, sr_end = 0, min(sr_end, sample_size)
        n_win = 0
        while True:
            w0, w1, _ = slice(sr_start, sr_end).indices(t_len)  # track_frames[sr_start:sr_end]
            count = max(0, w1 - w0)
            pad = int(rng.randint(0, sample_size - count)) if count != sample_size else 0
            rows.append((t0 + w0 if count else 0, count, pad))
            n_win += 1
            start += stride
            end = start + segment_length
            sr_start = int(start * sr)
            sr_end = min(int(end * sr), sr_start + sample_size)
            if end > t.length:
                break
        counts.append(n_win)
    plan = np.array(rows, np.int64).reshape(-1, 3)
    if segments:
        return plan, counts, np.array(segs, np.int64).reshape(-1, 2)
    return plan, counts


def check_window_plan(plan, rec_len, n):
    """A window table of track_window_plan's form as contiguous int64, after
    checking it against a recording of rec_len samples and windows of n:
    ValueError unless every row has 0 <= count, 0 <= pad, pad + count <= n,
    0 <= src and src + count <= rec_len."""
    plan = np.ascontiguousarray(plan, np.int64)
    if plan.ndim != 2 or plan.shape[1] != 3:
        raise ValueError(f"window plan must be [n_windows, 3], got {plan.shape}")
    src, count, pad = plan[:, 0], plan[:, 1], plan[:, 2]
    # pad + count <= n and src + count <= rec_len, written so that no int64 sum can wrap
    bad = (count < 0) | (count > n) | (pad < 0) | (pad > n - count) | (src < 0) | (src > rec_len - count)
    if bad.any():
        w = int(np.flatnonzero(bad)[0])
        raise ValueError(f"window {w}: (src, count, pad) = {tuple(int(v) for v in plan[w])} does not fit a window "
                         f"of {n} samples in a recording of {rec_len}")
    return plan


SOS_IDENTITY = np.array([[1.0, 0, 0, 1, 0, 0]] * 2)


def sos_segment_plan(tracks, segs, plan, counts, sr, filter_freqs=False, filter_below=None):
    """The device form of track_windows' filtering: from the tracks, their
    segments `segs` and the window table of track_window_plan(segments=True)
    -> (seg, sos, plan2) for acfe.frontend.sosfilt_segments.
    seg: int64 [n_seg, 3] rows (src, len, dst), one per track with windows:
    samples [src, src + len) of the recording are filtered into
    [dst, dst + len) of one packed buffer, dst rounded up to 4 floats so that
    every segment starts 16-B aligned (the buffer holds max(dst + len) rounded
    up likewise).  sos: float64 [n_seg, 2, 6], track_sos of each track with a
    missing section as the identity (1, 0, 0, 1, 0, 0); an unfiltered track
    has two and is a copy.  plan2: `plan` with every non-empty window's src
    rebased into the packed buffer (src - t0 + dst)."""
    plan2 = np.array(plan, np.int64).reshape(-1, 3)
    seg, sos = [], []
    at = dst = 0
    for t, (t0, t_len), c in zip(tracks, np.asarray(segs, np.int64).reshape(-1, 2).tolist(), counts):
        if c == 0:
            continue
        rows = plan2[at:at + c]
        rows[rows[:, 1] > 0, 0] += dst - t0
        at += c
        f = np.array(SOS_IDENTITY)
        s = track_sos(t, sr, filter_freqs, filter_below)
        if s is not None:
            f[:len(s)] = s
        seg.append((t0, t_len, dst))
        sos.append(f)
        dst = (dst + t_len + 3) & ~3
    return np.array(seg, np.int64).reshape(-1, 3), np.array(sos, np.float64).reshape(-1, 2, 6), plan2


def check_sos_segments(seg, sos, rec_len, out_len):
    """A segment table and its filters (sos_segment_plan's form) as contiguous
    int64 / float64, after checking them against a recording of rec_len
    samples and a packed buffer of out_len: ValueError unless every row has
    0 <= src, 0 <= len, src + len <= rec_len, 0 <= dst, dst + len <= out_len,
    the [dst, dst + len) ranges are disjoint, every coefficient is finite and
    every a0 is 1."""
    seg = np.ascontiguousarray(seg, np.int64)
    sos = np.ascontiguousarray(sos, np.float64)
    if seg.ndim != 2 or seg.shape[1] != 3:
        raise ValueError(f"segment table must be [n_seg, 3], got {seg.shape}")
    if sos.shape != (seg.shape[0], 2, 6):
        raise ValueError(f"sos must be [{seg.shape[0]}, 2, 6], got {sos.shape}")
    src, ln, dst = seg[:, 0], seg[:, 1], seg[:, 2]
    # src + len <= rec_len and dst + len <= out_len, written so that no int64 sum can wrap
    bad = (ln < 0) | (src < 0) | (ln > rec_len) | (src > rec_len - ln) | (dst < 0) | (ln > out_len) | \
        (dst > out_len - ln)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"segment {k}: (src, len, dst) = {tuple(int(v) for v in seg[k])} does not fit a recording "
                         f"of {rec_len} samples and a buffer of {out_len}")
    order = np.argsort(dst, kind="stable")
    order = order[ln[order] > 0]
    # consecutive ranges in dst order: len <= next dst - dst (both in [0, out_len], no wrap)
    clash = ln[order[:-1]] > dst[order[1:]] - dst[order[:-1]]
    if clash.any():
        k = int(order[int(np.flatnonzero(clash)[0])])
        raise ValueError(f"segment {k}: (src, len, dst) = {tuple(int(v) for v in seg[k])} overlaps the next "
                         "segment of the buffer")
    if not np.isfinite(sos).all():
        raise ValueError("sos holds a non-finite coefficient")
    if (sos[:, :, 3] != 1.0).any():
        raise ValueError("sos must be normalised: a0 == 1 in every section")
    return seg, sos


PCEN_SCOPES = ("batch", "track", "window")
KERAS_BATCH = 32  # the batch_size default of keras.Model.predict (predict.py:887 passes none)


def pcen_segments(counts, scope, keras_batch=KERAS_BATCH):
    """The clips that share PCEN's min / max (tfpcen.normalize_minmax, :105-110)
    under `scope`, for windows laid out track after track with counts[k]
    windows of track k -> the table of offsets of
    acfe.frontend.check_pcen_segments (int32 [n_seg + 1]: segment s is the
    windows [seg[s], seg[s + 1])), or None.  "batch": None, the extrema of
    each launch.  "window": one segment per window.  "track": for every track
    with windows, consecutive runs of at most keras_batch of them -- the
    batches Keras predict cuts model.predict(one track's windows) into
    (predict.py:887), each of which the layer normalises by its own extrema."""
    if scope not in PCEN_SCOPES:
        raise ValueError(f"pcen scope {scope!r}: expected one of {PCEN_SCOPES}")
    if scope == "batch":
        return None
    counts = [int(c) for c in counts]
    if scope == "window":
        return np.arange(sum(counts) + 1, dtype=np.int32)
    if keras_batch < 1:
        raise ValueError("keras_batch must be positive")
    seg, at = [0], 0
    for c in counts:
        for a in range(0, c, keras_batch):
            at += min(keras_batch, c - a)
            seg.append(at)
    return np.array(seg, np.int32)


def segment_launches(n, batch_size, segments=None):
    """The launches of n windows in order -> list of (a, b, table): windows
    [a, b) with b - a <= batch_size.  Without `segments` they are chunks of
    batch_size and table is None.  With a table of pcen_segments' form over
    the n windows every launch is filled greedily with whole segments, so that
    none is split, and `table` is the launch's own: rebased to start at 0,
    without empty segments.  ValueError for a segment larger than
    batch_size."""
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    if segments is None:
        return [(a, min(a + batch_size, n), None) for a in range(0, n, batch_size)]
    from acfe.frontend import check_pcen_segments

    seg = check_pcen_segments(segments, n).astype(np.int64)
    seg = seg[np.concatenate(([True], np.diff(seg) > 0))]  # empty segments hold no window
    if (np.diff(seg) > batch_size).any():
        raise ValueError(f"a PCEN segment of {int(np.diff(seg).max())} windows does not fit a launch of "
                         f"batch_size {batch_size}")
    out, first = [], 0
    for k in range(1, len(seg)):
        if k + 1 == len(seg) or seg[k + 1] - seg[first] > batch_size:
            out.append((int(seg[first]), int(seg[k]), (seg[first:k + 1] - seg[first]).astype(np.int32)))
            first = k
    return out


def host_frames(frames):
    """A recording as numpy: a 1-D float32 device tensor is downloaded, numpy
    input passes through."""
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 1 or frames.dtype != torch.float32:
            raise TypeError("a recording tensor must be 1-D float32")
        return frames.detach().cpu().numpy()
    return frames


def detect_tracks(frames, sr=SR, detector="host", dev_out=None):
    """predict.main (:735-740): cut the silent tail, detect signals, merge
    them into tracks -> (tracks, frames[:end], end seconds).  detector "host"
    runs identifytracks on numpy; "gpu" (or an acfe.tracks.SignalDetector to
    reuse) uploads the recording once and runs get_end and signal_noise on
    the device, the cut recording being a slice of that one buffer.  The
    merging into tracks is host work on a few hundred boxes either way.
    A device detector appends that slice, the cut recording on the device,
    to the list `dev_out` when one is given.  `frames` may be a 1-D float32
    device tensor (load_recording(resample="device")): a device detector uses
    it where it lies and the returned frames are a slice of it; the host
    detector downloads it first."""
    from identifytracks import get_end, get_tracks_from_signals, signal_noise

    if detector == "host":
        frames = host_frames(frames)
        end = get_end(frames, sr)
        frames = frames[: int(sr * end)]
        signals, _ = signal_noise(frames, sr)
        return get_tracks_from_signals(signals, end), frames, end
    if detector == "gpu":
        from acfe.tracks import SignalDetector

        detector = SignalDetector(sr=sr)
    elif isinstance(detector, str):
        raise ValueError(f"detector {detector!r}: expected 'host' or 'gpu'")
    dev = detector.upload(frames)
    end = detector.get_end(dev)
    cut = int(sr * end)
    signals = detector.signal_noise(dev[:cut])[0] if cut else []
    if dev_out is not None:
        dev_out.append(dev[:cut])
    return get_tracks_from_signals(signals, end), frames[:cut], end


class Predictor:
    def __init__(self, checkpoint_dir, device=None, dtype=None):
        from acfe.train import FrontEnd
        from audiomodel import MODEL_NAMES, build_model

        d = Path(checkpoint_dir)
        self.meta = json.loads((d / "metadata.txt").read_text())
        self.labels = self.meta.get("ebird_labels") or self.meta["labels"]
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        dt = dtype or (torch.bfloat16 if self.meta.get("dtype", "bf16") == "bf16" else torch.float32)
        n_mels = self.meta.get("n_mels", 160)
        name = self.meta.get("name", "wr-resnet")
        bw2 = MODEL_NAMES.get(name) == "badwinner2"
        sd = None
        if (d / "model.pt").exists():
            sd = torch.load(d / "model.pt", map_location="cpu", weights_only=True)
        # badwinner2's first convolution keeps the checkpoint's Cin (a Keras file's is read by its loader)
        cin = sd["1.trunk.0.weight"].shape[-1] if bw2 and sd is not None else 3
        self.model = build_model(name, (n_mels, 513, cin), len(self.labels), dt,
                                 multi_label=self.meta.get("multi_label", True), lme=self.meta.get("lme", False))
        # badwinner2 takes the fp32 mel power itself, whatever the metadata says of
        # PCEN: its MagTransform is the compression (reference predict.py:874-887)
        self.frontend = FrontEnd(n_mels=n_mels, n_fft=self.meta.get("n_fft", 4096), hop=self.meta.get("hop_length", 281),
                                 fmin=self.meta.get("fmin", 100), fmax=self.meta.get("fmax", 11000),
                                 break_freq=self.meta.get("break_freq", 1000),
                                 pcen=False if bw2 else self.meta.get("pcen", True),
                                 dtype=torch.float32 if bw2 else dt, device=self.device,
                                 power=self.meta.get("power", 2))
        holder = torch.nn.ModuleList([self.frontend, self.model])
        if sd is not None:
            holder.load_state_dict(sd)
        else:  # a reference checkpoint dir: {run}.keras / *.weights.h5 (predict.py:746-789)
            from keras_weights import load_keras_weights

            cands = sorted(d.glob("*.keras")) + sorted(d.glob("*.weights.h5"))
            if not cands:
                raise FileNotFoundError(f"{d}: no model.pt, *.keras or *.weights.h5")
            load_keras_weights(self.model, cands[0])
        holder.to(self.device).eval()
        self._detector = None  # acfe.tracks.SignalDetector of predict_tracks(detector="gpu")

    def _probabilities(self, feats):
        """The model's outputs for front-end features: its own activation over
        its logits where it names one (badwinner2: softmax for a single-label
        checkpoint, else sigmoid), ops.sigmoid for the two WRNs."""
        from acfe import ops

        return getattr(self.model, "activation", ops.sigmoid)(self.model(feats))

    @torch.no_grad()
    def predict_windows(self, recording, stride=1.0, batch_size=1024, pad_mode="constant", pcen_scope="batch"):
        """Sigmoid outputs [n_windows, classes] for 3 s windows every `stride` s
        of a numpy recording, or of a 1-D float32 device tensor, which is read
        where it lies.  pcen_scope "batch" normalises PCEN over each launch of
        batch_size windows, "window" over every window by itself, so that a
        window's output depends on nothing else; there are no tracks here, so
        "track" is a ValueError."""
        if pcen_scope not in ("batch", "window"):
            raise ValueError(f"pcen scope {pcen_scope!r}: expected 'batch' or 'window' for windows without tracks")
        n = SR * 3
        if isinstance(recording, torch.Tensor):
            if recording.dim() != 1 or recording.dtype != torch.float32:
                raise TypeError("a recording tensor must be 1-D float32")
            dev_rec = recording.to(self.device).contiguous()
            if dev_rec.numel() < n:  # short recordings are zero padded to one window
                dev_rec = torch.nn.functional.pad(dev_rec, (0, n - dev_rec.numel()))
        else:
            rec = np.asarray(recording, np.float32)
            if len(rec) < n:
                rec = np.pad(rec, (0, n - len(rec)))
            dev_rec = torch.from_numpy(rec).to(self.device)
        hop = int(round(stride * SR))
        n_win = 1 + (dev_rec.numel() - n) // hop
        out = []
        for first in range(0, n_win, batch_size):
            cnt = min(batch_size, n_win - first)
            segs = np.arange(cnt + 1, dtype=np.int32) if pcen_scope == "window" else None
            feats = self.frontend.forward_windows(dev_rec, first, cnt, n=n, hop=hop, pad_mode=pad_mode, segments=segs)
            out.append(self._probabilities(feats))
        return torch.cat(out).float().cpu().numpy()

    @torch.no_grad()
    def predict_clips(self, clips: np.ndarray, batch_size=1024, segments=None):
        """Sigmoid outputs [B, classes] for raw [B, 144000] windows (each
        normalised on the GPU, centred STFT with constant padding).  segments:
        a table of pcen_segments' form over the B windows; PCEN then normalises
        every segment by its own extrema, and the launches are cut at segment
        boundaries (segment_launches).  None: the extrema of each launch."""
        out = []
        for a, b, seg in segment_launches(len(clips), batch_size, segments):
            x = torch.from_numpy(np.ascontiguousarray(clips[a:b], np.float32)).to(self.device)
            out.append(self._probabilities(self.frontend(x, pad_mode="constant", segments=seg)))
        return torch.cat(out).float().cpu().numpy()

    @torch.no_grad()
    def predict_plan(self, rec: torch.Tensor, plan: np.ndarray, batch_size=1024, segments=None):
        """predict_clips for windows that stay on the device: sigmoid outputs
        [n_windows, classes] for the windows the table `plan`
        (track_window_plan) cuts from the 1-D fp32 device recording `rec`,
        cut and normalised by one kernel per launch of up to batch_size
        windows; segments as in predict_clips."""
        from acfe import frontend as fe

        n = SR * 3
        out = []
        for a, b, seg in segment_launches(len(plan), batch_size, segments):
            x = fe.normalize_windows(rec, plan[a:b], n)
            out.append(self._probabilities(self.frontend.features(x, pad_mode="constant", segments=seg)))
        return torch.cat(out).float().cpu().numpy()

    def predict_tracks(self, frames, threshold=None, batch_size=1024, rng=None, detector="host", windows="host",
                       filter_freqs=False, filter_below=None, pcen_scope="batch"):
        """Tracks of one recording with their ModelResult (predict.py:735-956);
        `detector` as in detect_tracks ("gpu" keeps one SignalDetector per Predictor).
        windows "host" cuts every window with numpy and uploads them; "device"
        computes only the window table on the host and cuts the windows out of
        the device recording (the detector's buffer when detector is "gpu",
        else one upload) -- the same windows, so the same predictions.
        filter_freqs / filter_below band-pass the tracks first (track_sos):
        with scipy on the host for windows "host", with
        frontend.sosfilt_segments into one packed device buffer, which the
        window kernel then reads by the rebased table, for "device"; when no
        track is filtered the device path runs as without the options.
        `frames` may be a 1-D float32 device tensor
        (load_recording(resample="device")): with detector "gpu" and windows
        "device" its samples never visit the host; with a host detector or
        host windows it is downloaded once and the call goes on as for numpy.
        pcen_scope: which windows share PCEN's min / max (pcen_segments):
        "batch" every launch of batch_size windows of the recording, "track"
        each track's own windows in runs of 32, as the reference's
        model.predict per track normalises them, "window" each window alone.
        Under "track" and "window" a track's result does not depend on
        batch_size or on the other tracks; "track" needs batch_size >= 32."""
        if windows not in ("host", "device"):
            raise ValueError(f"windows {windows!r}: expected 'host' or 'device'")
        if pcen_scope not in PCEN_SCOPES:
            raise ValueError(f"pcen scope {pcen_scope!r}: expected one of {PCEN_SCOPES}")
        if pcen_scope == "track" and batch_size < KERAS_BATCH:
            raise ValueError(f"pcen scope 'track' normalises runs of up to {KERAS_BATCH} windows together: "
                             f"batch_size {batch_size} is too small")
        if isinstance(frames, torch.Tensor) and (detector == "host" or windows == "host"):
            frames = host_frames(frames)
        if detector == "gpu":
            if self._detector is None:
                from acfe.tracks import SignalDetector

                self._detector = SignalDetector(device=self.device, sr=SR)
            detector = self._detector
        dev = []
        if not isinstance(frames, torch.Tensor):
            frames = np.asarray(frames, np.float32)
        tracks, frames, end = detect_tracks(frames, detector=detector, dev_out=dev)
        thresh = self.meta.get("threshold", 0.7) if threshold is None else threshold
        if windows == "host":
            wins = track_windows(frames, SR, tracks, rng=rng, filter_freqs=filter_freqs, filter_below=filter_below)
            counts = [len(w) for w in wins]
            probs = self.predict_clips(np.concatenate(wins), batch_size,
                                       pcen_segments(counts, pcen_scope)) if sum(counts) else None
        else:
            plan, counts, segs = track_window_plan(len(frames), SR, tracks, rng=rng, segments=True)
            rec = dev[0] if dev else torch.from_numpy(np.ascontiguousarray(frames)).to(self.device)
            if filter_freqs or filter_below:
                from acfe import frontend as fe

                seg, sos, plan2 = sos_segment_plan(tracks, segs, plan, counts, SR, filter_freqs, filter_below)
                if (sos != SOS_IDENTITY).any():
                    rec, plan = fe.sosfilt_segments(rec, seg, sos), plan2
            probs = self.predict_plan(rec, plan, batch_size, pcen_segments(counts, pcen_scope)) if len(plan) else None
        at = 0
        for t, c in zip(tracks, counts):
            if c == 0:
                continue
            prediction = probs[at:at + c].mean(0)
            at += c
            r = ModelResult(self.meta.get("name", "wr-resnet"))
            t.predictions.append(r)
            max_p = None
            for i, p in enumerate(prediction):
                if max_p is None or p > max_p[1]:
                    max_p = (i, p)
                if p >= thresh:
                    r.labels.append(self.labels[i])
                    r.confidences.append(round(float(p) * 100))
            if not r.labels:
                r.raw_tag = self.labels[max_p[0]]
                r.raw_confidence = round(float(max_p[1]) * 100)
        return tracks, end

    def predict_file(self, path, stride=1.0, batch_size=1024, threshold=0.7, resample="host", pcen_scope="batch"):
        probs = self.predict_windows(load_recording(path, resample=resample, device=self.device), stride, batch_size,
                                     pcen_scope=pcen_scope)
        mean = probs.mean(0)
        labels = [(self.labels[i], float(mean[i])) for i in np.argsort(-mean) if mean[i] >= threshold]
        return {"file": str(path), "windows": int(probs.shape[0]), "labels": labels,
                "mean": {l: float(v) for l, v in zip(self.labels, mean)}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", help="checkpoint dir (model.pt + metadata.txt from audiomodel.py)")
    ap.add_argument("--file", required=True, nargs="+")
    ap.add_argument("--stride", type=float, default=1.0)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--mode", choices=("tracks", "windows"), default="tracks")
    ap.add_argument("--detector", choices=("host", "gpu"), default="host",
                    help="track detection (--mode tracks): numpy on the host, or the HIP kernels of acfe.tracks")
    ap.add_argument("--windows", choices=("host", "device"), default="host",
                    help="the 3 s windows of the tracks (--mode tracks): cut with numpy and uploaded, or cut and "
                         "normalised on the GPU from the uploaded recording by the table of window positions")
    ap.add_argument("--filter-freqs", action="store_true",
                    help="band-pass every track at its own frequency band before its windows are cut (--mode tracks)")
    ap.add_argument("--filter-below", type=float, default=None, metavar="HZ",
                    help="band-pass only the tracks whose band ends below HZ (--mode tracks)")
    ap.add_argument("--resample", choices=("host", "device"), default="host",
                    help="resampling of a recording that is not at 48 kHz: scipy's resample_poly on the host, or the "
                         "same filter as a HIP kernel on the uploaded samples (the recording then stays on the GPU)")
    ap.add_argument("--pcen-scope", choices=PCEN_SCOPES, default="batch",
                    help="the windows that share PCEN's min / max: every launch of --batch-size windows, each "
                         "track's own windows in runs of 32 as the reference's model.predict per track "
                         "(--mode tracks only), or each window alone; no effect on a model without PCEN "
                         "(badwinner2, or pcen false in the metadata)")
    a = ap.parse_args(argv)
    if a.mode == "windows" and a.pcen_scope == "track":
        ap.error("--pcen-scope track needs --mode tracks: --mode windows has no tracks")
    p = Predictor(a.model)
    for f in a.file:
        t0 = time.perf_counter()
        if a.mode == "tracks":
            rec = load_recording(f, resample=a.resample, device=p.device)
            tracks, end = p.predict_tracks(rec, a.threshold, a.batch_size, detector=a.detector, windows=a.windows,
                                           filter_freqs=a.filter_freqs, filter_below=a.filter_below,
                                           pcen_scope=a.pcen_scope)
            r = {"file": str(f), "end": end, "tracks": [t.get_meta() for t in tracks]}
        else:
            r = p.predict_file(f, a.stride, a.batch_size, a.threshold, resample=a.resample, pcen_scope=a.pcen_scope)
        r["seconds"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(r, default=float))


if __name__ == "__main__":
    main()
