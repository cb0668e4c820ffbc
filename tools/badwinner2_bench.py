#!/usr/bin/env python3
"""Throughput of predict.Predictor on a badwinner2 checkpoint (160 mel bands x
513 frames, the production geometry), on one GPU.

  python tools/badwinner2_bench.py [--batch 256] [--launches 20] [--warmup 3] [--dtypes bf16,fp32]
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/badwinner2_bench.py --profile --dtypes bf16

Writes a checkpoint directory with a freshly initialised model to a temporary
directory, then times, with device events around warmed-up launches:
  predict_clips   Predictor.predict_clips on host clips: the upload of
                  batch x 144000 float32 samples, front end, model, download
  device          the front end and the model on clips already on the device
and prints one JSON line per dtype.  `bytes` are what the three bw2.hip
kernels must move per launch (computed from the shapes), for comparing with
their kernel times from a rocprofv3 run; --profile runs two launches per dtype
and no timing, for such a run.
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "audio-training_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_MELS, FRAMES, SAMPLES, LABELS = 160, 513, 144000, 50


def stream_bytes(batch, elem):
    """Bytes each bw2.hip pass reads + writes per launch of `batch` windows
    (activations of `elem` bytes; the mel input is fp32)."""
    shapes = [(158, 511, 64), (156, 509, 64), (50, 167, 128), (48, 165, 128), (5, 163, 128), (1, 46, 1024),
              (1, 46, 1024), (1, 46, LABELS)]
    out = {"mag_rownorm": batch * N_MELS * FRAMES * (4 + elem)}
    for h, w, c in shapes:
        out[f"leaky_bn {h}x{w}x{c}"] = 2 * batch * h * w * c * elem
    return out


def clips(batch, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(SAMPLES) / 48000.0
    x = rng.normal(0, 0.01, (batch, SAMPLES))
    for i in range(batch):
        f0, f1 = rng.uniform(500, 10000, 2)
        x[i] += 0.3 * np.sin(2 * np.pi * (f0 * t + (f1 - f0) / 6.0 * t * t))
    return np.clip(x, -1, 1).astype(np.float32)


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches  # ms per launch


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--profile", action="store_true", help="two launches per dtype, no timing (for rocprofv3)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("badwinner2_bench needs a GPU: nothing is measured without one")
    import badwinner2
    import predict
    from keras_weights import save_keras_weights

    x = clips(a.batch)
    for dt in a.dtypes.split(","):
        with tempfile.TemporaryDirectory() as d:
            meta = {"labels": [f"l{i}" for i in range(LABELS)], "name": "badwinner2", "n_mels": N_MELS, "dtype": dt,
                    "multi_label": True}
            (Path(d) / "metadata.txt").write_text(json.dumps(meta))
            save_keras_weights(badwinner2.build_model((N_MELS, FRAMES, 3), None, LABELS), Path(d) / "m.weights.h5")
            p = predict.Predictor(d)
        xd = torch.from_numpy(x).to(p.device)

        @torch.no_grad()
        def device_only():
            return p._probabilities(p.frontend(xd, pad_mode="constant"))

        if a.profile:
            for _ in range(2):
                p.predict_clips(x, batch_size=a.batch)
            torch.cuda.synchronize()
            continue
        ms_clips = timed(lambda: p.predict_clips(x, batch_size=a.batch), a.launches, a.warmup)
        ms_dev = timed(device_only, a.launches, a.warmup)
        print(json.dumps({"model": "badwinner2", "dtype": dt, "batch": a.batch, "launches": a.launches,
                          "predict_clips_ms": round(ms_clips, 3),
                          "predict_clips_windows_per_s": round(a.batch / ms_clips * 1e3, 1),
                          "device_ms": round(ms_dev, 3), "device_windows_per_s": round(a.batch / ms_dev * 1e3, 1),
                          "bytes": stream_bytes(a.batch, 2 if dt == "bf16" else 4)}))


if __name__ == "__main__":
    main()
