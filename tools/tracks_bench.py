#!/usr/bin/env python3
"""Track detection, host against device: predict.detect_tracks with
detector="host" (numpy / scipy, wall clock) and with the acfe.tracks
SignalDetector (wall clock of the whole call including the upload, and the
per-stage device times from torch.cuda.Event pairs), on synthetic recordings
with a few chirps per 10 s.  One warm-up call of each, then one timed call;
one JSON line per recording length.

  python tools/tracks_bench.py [--seconds 60 600] [--no-host]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "audio-training_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR = 48000


def synthetic(seconds, seed=0, sr=SR):
    """White noise + three 0.5-1.5 s chirps in every 10 s, float32, sampled at sr."""
    rng = np.random.default_rng(seed)
    n = sr * seconds
    x = rng.normal(0, 0.003, n).astype(np.float32)
    for block in range(0, seconds, 10):
        for _ in range(3):
            dur = rng.uniform(0.5, 1.5)
            on = block + rng.uniform(0, min(10, seconds - block) - dur)
            f0, f1 = rng.uniform(800, 9000, 2)
            a, b = int(on * sr), int((on + dur) * sr)
            tt = np.arange(b - a) / sr
            x[a:b] += (0.3 * np.sin(2 * np.pi * (f0 * tt + 0.5 * (f1 - f0) / dur * tt * tt))).astype(np.float32)
    return x


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--no-host", action="store_true", help="skip the host detector (long recordings)")
    a = ap.parse_args(argv)
    import predict
    from acfe.tracks import SignalDetector
    from identifytracks import get_tracks_from_signals

    det =SignalDetector(sr=SR)
    predict.detect_tracks(synthetic(10), SR, detector=det)  # warm-up: kernels loaded, mel plan made
    if not a.no_host:
        predict.detect_tracks(synthetic(10), SR, detector="host")
    for seconds in a.seconds:
        x = synthetic(seconds)
        r = {"seconds": seconds, "gpu": torch.cuda.get_device_name(0)}
        det.timer = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracks, _, end = predict.detect_tracks(x, SR, detector=det)
        torch.cuda.synchronize()
        r["device_wall_s"] = round(time.perf_counter() - t0, 4)
        stages = {}
        for name, e0, e1 in det.timer:
            stages[name] = round(stages.get(name, 0.0) + e0.elapsed_time(e1), 3)
        det.timer = None
        r["device_stage_ms"] = stages
        r["device_ms"] = round(sum(stages.values()), 3)
        r["device_tracks"], r["end"] = len(tracks), end
        # the part of both wall clocks that is the same host code: merging the signals into tracks
        signals = det.signal_noise(x[: int(SR * end)])[0]
        t0 = time.perf_counter()
        get_tracks_from_signals(signals, end)
        r["merge_wall_s"] = round(time.perf_counter() - t0, 4)
        r["signals"] = len(signals)
        if not a.no_host:
            t0 = time.perf_counter()
            tracks, _, _ = predict.detect_tracks(x, SR, detector="host")
            r["host_wall_s"] = round(time.perf_counter() - t0, 4)
            r["host_tracks"] = len(tracks)
            r["speedup"] = round(r["host_wall_s"] / r["device_wall_s"], 1)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
