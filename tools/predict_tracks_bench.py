#!/usr/bin/env python3
"""predict_tracks with the windows cut on the host against windows cut on the
device: Predictor.predict_tracks(detector="gpu", windows="host" | "device")
on the synthetic recordings of tools/tracks_bench.py, a random-initialised
wr-resnet-bird checkpoint (128 mels, bf16) and the same seeded rng.  One
warm-up call per setting on a 10 s recording, then timed calls per recording
length; one JSON line per length.

  whole_s   wall clock of the whole predict_tracks call (upload, detection,
            merging into tracks, windows, front end, model, per-track results)
  stage_s   the window stage alone, from the detected tracks to normalised
            windows on the device, perf_counter around it with a device
            synchronise at both ends.  host: track_windows + np.concatenate +
            the upload of every chunk + normalize_stats / normalize_apply, as
            predict_clips and FrontEnd.forward run them; device:
            track_window_plan + normalize_windows on the detector's buffer.
            One untimed run of each, then STAGE_REPS timed ones, host and
            device alternating: every time is listed, the ratio is of the minima.
  The whole call likewise: WHOLE_REPS timed calls per setting, alternating.

  python tools/predict_tracks_bench.py [--seconds 60 600] [--batch-size 1024]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "audio-training_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SR = 48000
N = 3 * SR
STAGE_REPS = 3
WHOLE_REPS = 2


def make_checkpoint(d, device):
    from acfe.train import FrontEnd
    from audiomodel import build_model

    meta = {"labels": ["bird", "noise"], "name": "wr-resnet-bird", "n_mels": 128, "dtype": "bf16"}
    (d / "metadata.txt").write_text(json.dumps(meta))
    torch.manual_seed(0)
    model = build_model("wr-resnet-bird", (128, 513, 3), 2, torch.bfloat16)
    fe = FrontEnd(n_mels=128, dtype=torch.bfloat16, device=device)
    torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([fe, model]).state_dict().items()}, d / "model.pt")


def host_stage(predict, fe, frames, tracks, device, batch_size):
    clips = np.concatenate(predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(0)))
    last = None
    for a in range(0, len(clips), batch_size):
        x = torch.from_numpy(np.ascontiguousarray(clips[a:a + batch_size], np.float32)).to(device)
        last = fe.normalize_apply(x, fe.normalize_stats(x))
    return last


def device_stage(predict, fe, dev, n_frames, tracks, batch_size):
    plan, _ = predict.track_window_plan(n_frames, SR, tracks, rng=np.random.RandomState(0))
    last = None
    for a in range(0, len(plan), batch_size):
        last = fe.normalize_windows(dev, plan[a:a + batch_size], N)
    return last


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round(time.perf_counter() - t0, 5)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--batch-size", type=int, default=1024)
    a = ap.parse_args(argv)
    import identifytracks as it
    import predict
    from acfe import frontend as fe
    from tracks_bench import synthetic

    device = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        make_checkpoint(Path(tmp), device)
        p = predict.Predictor(tmp, device=device)
    for windows in ("host", "device"):  # warm-up: kernels loaded, plans made, allocator filled
        p.predict_tracks(synthetic(10), rng=np.random.RandomState(0), detector="gpu", windows=windows,
                         batch_size=a.batch_size)
    for seconds in a.seconds:
        x = synthetic(seconds)
        r = {"seconds": seconds, "gpu": torch.cuda.get_device_name(0), "batch_size": a.batch_size}
        metas = {}
        whole = {"host": [], "device": []}
        for _ in range(WHOLE_REPS):
            for windows in ("host", "device"):
                it.Signal._next_id = 0  # the ids in get_meta count up over the process
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tracks, end = p.predict_tracks(x, rng=np.random.RandomState(0), detector="gpu", windows=windows,
                                               batch_size=a.batch_size)
                torch.cuda.synchronize()
                whole[windows].append(round(time.perf_counter() - t0, 4))
                metas[windows] = [t.get_meta() for t in tracks]
        r["host_whole_s"], r["device_whole_s"] = whole["host"], whole["device"]
        r["tracks"], r["same_results"] = len(metas["host"]), metas["host"] == metas["device"]
        dev = []
        tracks, frames, end = predict.detect_tracks(x, detector=p._detector, dev_out=dev)
        plan, _ = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(0))
        r["windows"], r["partial_windows"] = len(plan), int((plan[:, 1] < N).sum())
        stages = {"host": lambda: host_stage(predict, fe, frames, tracks, device, a.batch_size),
                  "device": lambda: device_stage(predict, fe, dev[0], len(frames), tracks, a.batch_size)}
        for k in range(STAGE_REPS + 1):
            for name, fn in stages.items():
                dt = timed(fn)
                if k:  # the first run of each is not counted
                    r.setdefault(f"{name}_stage_s", []).append(dt)
        r["stage_speedup"] = round(min(r["host_stage_s"]) / min(r["device_stage_s"]), 1)
        r["whole_speedup"] = round(min(r["host_whole_s"]) / min(r["device_whole_s"]), 2)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
