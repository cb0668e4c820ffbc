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

--filter-freqs measures the Butterworth band-pass of the tracks
(predict_tracks(filter_freqs=True)) instead, one JSON line per length:

  whole_s          the whole call with the option on, windows "host" (scipy
                   sosfilt inside track_windows) against "device"
                   (sosfilt_segments + the window kernel), alternating
  host_filter_s    wall clock of the host filter stage alone: sosfilt + the
                   float32 cast of every track segment (FILTER_REPS runs after
                   one untimed)
  device_filter_ms HIP events around frontend.sosfilt_segments on the
                   detector's buffer (table upload, workspace, four kernels);
                   device_filter_wall_s the same call by wall clock with a
                   device synchronise at both ends
  filter_err       max |device - float32(host)| / max |host| over the segments,
                   in units of 2^-22 (the test bound)
  prob_diff        max |p_device - p_host| over all windows and classes

--rate HZ (other than 48000) measures the resampling to 48 kHz instead
(load_recording(resample="host" | "device")), on the same synthetic recording
generated at HZ and written as an int16 mono WAV; one JSON line per length:

  host_resample_s    wall clock of scipy.signal.resample_poly on the float32
                     samples (RESAMPLE_REPS runs after one untimed)
  upload_s           wall clock of the upload of the decoded samples, int16 (what
                     the device path uploads) and float32 at 48 kHz (what the
                     host path uploads afterwards), a device synchronise at
                     both ends
  device_resample_ms HIP events around frontend.resample_poly on the uploaded
                     int16 samples; device_resample_wall_s the same call by wall
                     clock with a device synchronise at both ends
  whole_s            load_recording + predict_tracks(detector="gpu",
                     windows="device") by wall clock, resample "host" against
                     "device", alternating
  resample_diff      max |device - host| over the 48 kHz samples, and the same
                     as a fraction of the test bound of that sample
                     ((K + 3) 2^-24 sum |h x| + ...), from the first 2^20 outputs
  tracks, same_tracks, prob_diff   of the two whole calls

--pcen-scope measures PCEN's min / max per track (predict_tracks(pcen_scope=
"track")) against per launch ("batch") instead, detector "gpu" and windows
"device"; one JSON line per length:

  whole_s            the whole call under either scope, alternating, after one
                     untimed pair at this length
  tracks_changed     tracks whose ModelResult (labels, confidences, raw tag)
                     differs between the scopes; labels_changed: those whose
                     labels or raw tag differ, not only a confidence
  windows, segments, launches   of the "track" table (segment_launches)
  normalise_ms       HIP events around the normalise stage over the launches'
                     un-normalised PCEN output (y_bytes of float32, computed
                     beforehand): batch = acfe_pcen_normalize (one kernel);
                     track = frontend.pcen_normalize_segments (table upload,
                     workspace, three kernels).  One untimed run of each, then
                     STAGE_REPS timed, alternating; normalise_extra_ms is the
                     difference of the minima

  python tools/predict_tracks_bench.py [--seconds 60 600] [--batch-size 1024] [--filter-freqs] [--rate HZ]
                                       [--pcen-scope]
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
FILTER_REPS = 5
RESAMPLE_REPS = 5


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


def filter_report(p, predict, fe, it, x, seconds, batch_size):
    from scipy.signal import sosfilt

    r = {"seconds": seconds, "gpu": torch.cuda.get_device_name(0), "batch_size": batch_size, "filter_freqs": True}
    whole = {"host": [], "device": []}
    boxes = {}
    for _ in range(WHOLE_REPS):
        for windows in ("host", "device"):
            it.Signal._next_id = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tracks, end = p.predict_tracks(x, rng=np.random.RandomState(0), detector="gpu", windows=windows,
                                           batch_size=batch_size, filter_freqs=True)
            torch.cuda.synchronize()
            whole[windows].append(round(time.perf_counter() - t0, 4))
            boxes[windows] = [(t.start, t.end, t.freq_start, t.freq_end, len(t.predictions)) for t in tracks]
    r["host_whole_s"], r["device_whole_s"] = whole["host"], whole["device"]
    r["tracks"], r["same_tracks"] = len(boxes["host"]), boxes["host"] == boxes["device"]
    dev = []
    tracks, frames, end = predict.detect_tracks(x, detector=p._detector, dev_out=dev)
    plan, counts, segs = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(0),
                                                   segments=True)
    seg, sos, plan2 = predict.sos_segment_plan(tracks, segs, plan, counts, SR, filter_freqs=True)
    r["windows"], r["segments"], r["filtered_samples"] = len(plan), len(seg), int(seg[:, 1].sum())
    r["recording_samples"] = len(frames)

    def host_filter():
        return [sosfilt(f, frames[a:a + n]).astype(np.float32) for (a, n, _), f in zip(seg.tolist(), sos)]

    for k in range(FILTER_REPS + 1):
        t0 = time.perf_counter()
        ref = host_filter()
        dt = round(time.perf_counter() - t0, 5)
        wall = timed(lambda: fe.sosfilt_segments(dev[0], seg, sos))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        filtered = fe.sosfilt_segments(dev[0], seg, sos)
        e1.record()
        torch.cuda.synchronize()
        if k:  # the first run of each is not counted
            r.setdefault("host_filter_s", []).append(dt)
            r.setdefault("device_filter_wall_s", []).append(wall)
            r.setdefault("device_filter_ms", []).append(round(e0.elapsed_time(e1), 4))
    buf = filtered.cpu().numpy()
    err = 0.0
    for (a, n, d), f, h in zip(seg.tolist(), sos, ref):
        m = np.abs(sosfilt(f, frames[a:a + n])).max()
        err = max(err, float(np.abs(buf[d:d + n].astype(np.float64) - h).max() / m) * 2.0 ** 22)
    r["filter_err"] = round(err, 4)
    wins = np.concatenate(predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(0), filter_freqs=True))
    probs = p.predict_plan(filtered, plan2, batch_size), p.predict_clips(wins, batch_size)
    r["prob_diff"] = float(np.abs(probs[0] - probs[1]).max())
    r["filter_speedup_events"] = round(min(r["host_filter_s"]) * 1e3 / min(r["device_filter_ms"]), 1)
    r["filter_speedup_wall"] = round(min(r["host_filter_s"]) / min(r["device_filter_wall_s"]), 1)
    r["whole_speedup"] = round(min(r["host_whole_s"]) / min(r["device_whole_s"]), 2)
    print(json.dumps(r), flush=True)


def resample_report(p, predict, fe, it, seconds, rate, batch_size, tmp):
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    from tracks_bench import synthetic

    device = p.device
    plan = predict.resample_plan(rate)
    pcm = (synthetic(seconds, sr=rate) * 32767).astype(np.int16)
    path = Path(tmp) / f"rec_{rate}_{seconds}.wav"
    wavfile.write(path, rate, pcm)
    xf = pcm.astype(np.float32) / 32767.0
    r = {"seconds": seconds, "rate": rate, "up": plan.up, "down": plan.down, "taps": len(plan.h),
         "gpu": torch.cuda.get_device_name(0), "batch_size": batch_size, "samples_in": len(pcm),
         "samples_out": plan.n_out(len(pcm))}
    dev16 = torch.from_numpy(pcm).to(device)
    for k in range(RESAMPLE_REPS + 1):
        t0 = time.perf_counter()
        host = resample_poly(xf, plan.up, plan.down).astype(np.float32)
        dt = round(time.perf_counter() - t0, 5)
        up16 = timed(lambda: torch.from_numpy(pcm).to(device))
        up32 = timed(lambda: torch.from_numpy(host).to(device))
        wall = timed(lambda: fe.resample_poly(dev16, rate))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        got = fe.resample_poly(dev16, rate)
        e1.record()
        torch.cuda.synchronize()
        if k:  # the first run of each is not counted
            r.setdefault("host_resample_s", []).append(dt)
            r.setdefault("upload_int16_s", []).append(up16)
            r.setdefault("upload_float32_48k_s", []).append(up32)
            r.setdefault("device_resample_wall_s", []).append(wall)
            r.setdefault("device_resample_ms", []).append(round(e0.elapsed_time(e1), 4))
    g = got.cpu().numpy()
    diff = np.abs(g.astype(np.float64) - host.astype(np.float64))
    n = np.arange(min(len(g), 1 << 20), dtype=np.int64)
    t = n * plan.down + plan.t0
    q, j0 = t % plan.up, t // plan.up
    amp, ref = np.zeros(len(n)), np.zeros(len(n))
    for k in range(plan.terms):
        ih, jx = q + k * plan.up, j0 - k
        ok = (ih < len(plan.h)) & (jx >= 0) & (jx < len(xf))
        term = plan.h[ih[ok]].astype(np.float64) * xf[jx[ok]].astype(np.float64)
        ref[ok] += term
        amp[ok] += np.abs(term)
    bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -45 * amp + 2.0 ** -149 + (plan.terms + 2) * 2.0 ** -24 * amp
    r["resample_diff"] = float(diff.max())
    r["resample_diff_of_bound"] = round(float((diff[:len(n)] / bound).max()), 4)
    r["device_of_formula_bound"] = round(float((np.abs(g[:len(n)] - ref) / (bound - (plan.terms + 2) * 2.0 ** -24 * amp)
                                                ).max()), 4)

    probs = {}
    orig = p.predict_plan

    def spy(*a, **k):
        probs[mode] = orig(*a, **k)
        return probs[mode]

    p.predict_plan = spy
    whole = {"host": [], "device": []}
    boxes = {}
    for _ in range(WHOLE_REPS + 1):
        for mode in ("host", "device"):
            it.Signal._next_id = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = predict.load_recording(path, resample=mode, device=device)
            t1 = time.perf_counter()
            tracks, end = p.predict_tracks(rec, rng=np.random.RandomState(0), detector="gpu", windows="device",
                                           batch_size=batch_size)
            torch.cuda.synchronize()
            whole[mode].append((round(time.perf_counter() - t0, 4), round(t1 - t0, 4)))
            boxes[mode] = [(t.start, t.end, t.freq_start, t.freq_end, len(t.predictions)) for t in tracks]
    p.predict_plan = orig
    for mode in whole:  # the first pair is the warm-up of this length
        r[f"{mode}_whole_s"] = [w for w, _ in whole[mode][1:]]
        r[f"{mode}_load_s"] = [l for _, l in whole[mode][1:]]
    r["tracks"] = [len(boxes["host"]), len(boxes["device"])]
    r["same_tracks"] = boxes["host"] == boxes["device"]
    a, b = probs.get("host"), probs.get("device")
    r["prob_diff"] = float(np.abs(a - b).max()) if a is not None and b is not None and a.shape == b.shape else None
    r["resample_speedup_events"] = round(min(r["host_resample_s"]) * 1e3 / min(r["device_resample_ms"]), 1)
    r["resample_speedup_wall"] = round(min(r["host_resample_s"]) / min(r["device_resample_wall_s"]), 1)
    r["whole_speedup"] = round(min(r["host_whole_s"]) / min(r["device_whole_s"]), 2)
    print(json.dumps(r), flush=True)


def scope_report(p, predict, fe, it, x, seconds, batch_size):
    from acfe._lib import call, lib
    from acfe._torch import ptr, stream

    r = {"seconds": seconds, "gpu": torch.cuda.get_device_name(0), "batch_size": batch_size, "pcen_scope": True}
    whole = {"batch": [], "track": []}
    results = {}
    for k in range(WHOLE_REPS + 1):
        for scope in ("batch", "track"):
            it.Signal._next_id = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tracks, end = p.predict_tracks(x, rng=np.random.RandomState(0), detector="gpu", windows="device",
                                           batch_size=batch_size, pcen_scope=scope)
            torch.cuda.synchronize()
            if k:  # the first pair is the warm-up of this length
                whole[scope].append(round(time.perf_counter() - t0, 4))
            results[scope] = [[q.get_meta() for q in t.predictions] for t in tracks]
    r["batch_whole_s"], r["track_whole_s"] = whole["batch"], whole["track"]
    r["tracks"] = len(results["batch"])
    r["tracks_changed"] = sum(a != b for a, b in zip(results["batch"], results["track"]))
    r["labels_changed"] = sum([(q["species"], q.get("raw_tag")) for q in a] != [(q["species"], q.get("raw_tag")) for q in b]
                              for a, b in zip(results["batch"], results["track"]))

    dev = []
    tracks, frames, end = predict.detect_tracks(x, detector=p._detector, dev_out=dev)
    plan, counts = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(0))
    seg = predict.pcen_segments(counts, "track")
    r["windows"], r["segments"] = len(plan), len(seg) - 1
    launches = predict.segment_launches(len(plan), batch_size, seg)
    r["launches"] = [b - a for a, b, _ in launches]
    ys = []
    with torch.no_grad():
        for a, b, table in launches:
            w = fe.normalize_windows(dev[0], plan[a:b], N)
            mel = p.frontend.plan.mel(w, None, pad_mode="constant", power=p.frontend.power, layout="btm")
            bb, t, m = mel.shape
            npart = lib.acfe_pcen_partials(bb, m)
            y = torch.empty((bb, m, t), dtype=torch.float32, device=mel.device)
            part = torch.empty(2 * npart, dtype=torch.float32, device=mel.device)
            call("acfe_pcen_fwd", ptr(mel), bb, t, m, ptr(p.frontend.pcen.params), 1e-6, ptr(y), ptr(part), stream())
            ys.append((y, part, npart, table))
    r["y_bytes"] = sum(y.numel() * 4 for y, _, _, _ in ys)
    dt = p.frontend.dtype

    def norm_batch():
        for y, part, npart, _ in ys:
            out = torch.empty(y.shape, dtype=dt, device=y.device)
            stats = torch.empty(4, dtype=torch.float32, device=y.device)
            call("acfe_pcen_normalize", ptr(y), y.numel(), ptr(part), npart, None, ptr(out), 1, ptr(stats), stream())

    def norm_track():
        for y, _, _, table in ys:
            fe.pcen_normalize_segments(y, table, dt)

    for k in range(STAGE_REPS + 1):
        for name, fn in (("batch", norm_batch), ("track", norm_track)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k:  # the first run of each is not counted
                r.setdefault(f"{name}_normalise_ms", []).append(round(e0.elapsed_time(e1), 4))
    r["normalise_extra_ms"] = round(min(r["track_normalise_ms"]) - min(r["batch_normalise_ms"]), 4)
    r["whole_ratio"] = round(min(r["track_whole_s"]) / min(r["batch_whole_s"]), 3)
    print(json.dumps(r), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=int, nargs="+", default=[60, 600])
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--filter-freqs", action="store_true", help="measure the band-pass of the tracks instead")
    ap.add_argument("--rate", type=int, default=SR, metavar="HZ",
                    help="generate the recording at HZ and measure its resampling to 48 kHz instead")
    ap.add_argument("--pcen-scope", action="store_true",
                    help="measure PCEN's min / max per track (pcen_scope='track') against per launch instead")
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
                         batch_size=a.batch_size, filter_freqs=a.filter_freqs)
    if a.rate != SR:
        fe.resample_poly(torch.zeros(1000, dtype=torch.int16, device=device), a.rate)  # warm-up: kernel loaded, taps up
        with tempfile.TemporaryDirectory() as tmp:
            for seconds in a.seconds:
                resample_report(p, predict, fe, it, seconds, a.rate, a.batch_size, tmp)
        return
    for seconds in a.seconds:
        x = synthetic(seconds)
        if a.filter_freqs:
            filter_report(p, predict, fe, it, x, seconds, a.batch_size)
            continue
        if a.pcen_scope:
            scope_report(p, predict, fe, it, x, seconds, a.batch_size)
            continue
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
