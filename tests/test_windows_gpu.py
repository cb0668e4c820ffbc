"""acfe_windows_normalize (csrc/windows.hip): the classification windows of
predict cut, zero padded and normalised on the device from a table of
(src, count, pad) rows, bit for bit what normalising the host-cut windows
gives; and predict_tracks(windows="device") end to end against
windows="host"."""
import json

import numpy as np
import pytest
import torch

from oracle import frontend as of

pytestmark = pytest.mark.gpu

SR = 48000
GUARD = 12345.0


@pytest.fixture(scope="module")
def fe(cuda):
    from acfe import frontend

    return frontend


def cut(rec, plan, n):
    out = np.zeros((len(plan), n), np.float32)
    for w, (src, count, pad) in enumerate(plan):
        out[w, pad:pad + count] = rec[src:src + count]
    return out


def same_bits(a, b):
    """Equal bit patterns, except that a NaN matches any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def check(fe, cuda, rec, dev, plan, n):
    """normalize_windows of `plan` against numpy and against the two-kernel
    path on the uploaded host-cut windows; guard rows around out."""
    plan = np.asarray(plan, np.int64).reshape(-1, 3)
    b = len(plan)
    buf = torch.full((b + 2, n), GUARD, dtype=torch.float32, device=cuda)
    stats = torch.full((b + 2, 2), GUARD, dtype=torch.float32, device=cuda)
    out = fe.normalize_windows(dev, plan, n, out=buf[1:b + 1], stats=stats[1:b + 1])
    assert b == 0 or out.data_ptr() == buf[1:].data_ptr()
    got, st = buf.cpu().numpy(), stats.cpu().numpy()
    assert (got[0] == GUARD).all() and (got[-1] == GUARD).all()
    assert (st[0] == GUARD).all() and (st[-1] == GUARD).all()
    wins = cut(rec, plan, n)
    if b == 0:
        return wins
    mn, mx = wins.min(1), wins.max(1)
    assert same_bits(st[1:-1, 0], mn) and same_bits(st[1:-1, 1], mx - mn)
    assert same_bits(got[1:-1], of.normalize_f32(wins))
    x = torch.from_numpy(wins).to(cuda)
    assert same_bits(got[1:-1], fe.normalize_apply(x, fe.normalize_stats(x)).cpu().numpy())
    # without the optional arguments: the same rows in a fresh tensor
    assert same_bits(fe.normalize_windows(dev, plan, n).cpu().numpy(), got[1:-1])
    return wins


@pytest.fixture(scope="module")
def small(cuda):
    rec = np.random.default_rng(1).standard_normal(20000).astype(np.float32)
    rec[15000:16000] = np.abs(rec[15000:16000]) + 0.5  # all positive: a padded window's min is the padding
    rec[16000:17100] = -np.abs(rec[16000:17100]) - 0.5  # all negative: its max is the padding
    assert not np.signbit(rec[rec == 0]).any()
    return rec, torch.from_numpy(rec).to(cuda)


@pytest.mark.parametrize("n", [1000, 1027])
def test_windows_normalize_small(fe, cuda, small, n):
    """n = 1000: 16-B aligned output rows; n = 1027: rows at every alignment,
    scalar head and tail.  Rows are (src, count, pad)."""
    rec, dev = small
    L = len(rec)
    plan = [(0, n, 0), (1, n, 0), (4002, n, 0), (7, n, 0),  # full windows, src % 4 = 0, 1, 2, 3
            (L - n, n, 0),  # ends on the recording's last sample
            (13, n - 1, 1), (20, n - 1, 0), (2001, n - 1, 0),  # count n - 1 at either end
            (101, 5, 3), (102, 5, n - 5), (6, 5, 128), (3, 400, 301), (L - 5, 5, 7),  # pad % 4 = 3, *, 0, 1, 3
            (203, 1, 0), (L - 1, 1, 7), (11, 1, n - 1),
            (0, 0, 0), (500, 0, 9), (L, 0, 0),  # empty: 0 / 0
            (15003, 5, 3), (16002, n - 1, 1)]  # extremum supplied by the padding zeros
    wins = check(fe, cuda, rec, dev, plan, n)
    assert np.isnan(of.normalize_f32(wins[16])).all() and wins[19].min() == 0 and wins[20].max() == 0
    check(fe, cuda, rec, dev, plan[:1], n)  # batch 1
    check(fe, cuda, rec, dev, plan[8:9], n)
    check(fe, cuda, rec, dev, [], n)  # batch 0


def test_windows_normalize_abi_arguments(fe, cuda, small):
    from acfe import _lib

    rec, dev = small
    plan = torch.zeros((1, 3), dtype=torch.int64, device=cuda)
    out = torch.empty((1, 8), dtype=torch.float32, device=cuda)
    f = _lib.lib.acfe_windows_normalize
    assert f(dev.data_ptr(), len(rec), plan.data_ptr(), 0, 8, out.data_ptr(), None, None) == 0  # batch 0
    assert f(None, len(rec), plan.data_ptr(), 1, 8, out.data_ptr(), None, None) == _lib.E_INVAL
    assert f(dev.data_ptr(), len(rec), None, 1, 8, out.data_ptr(), None, None) == _lib.E_INVAL
    assert f(dev.data_ptr(), len(rec), plan.data_ptr(), 1, 8, None, None, None) == _lib.E_INVAL
    assert f(dev.data_ptr(), len(rec), plan.data_ptr(), 1, 0, out.data_ptr(), None, None) == _lib.E_INVAL
    assert f(dev.data_ptr(), len(rec), plan.data_ptr(), -1, 8, out.data_ptr(), None, None) == _lib.E_INVAL
    # the host check of the Python layer comes before any launch
    with pytest.raises(ValueError):
        fe.normalize_windows(dev, [(len(rec) - 3, 4, 0)], 8)
    with pytest.raises(TypeError):
        fe.normalize_windows(dev.double(), [(0, 4, 0)], 8)


def test_windows_normalize_real_size(fe, cuda):
    """The predict path's window: n = 144000 out of a 6 s recording."""
    n, L = 3 * SR, 6 * SR
    rec = np.random.default_rng(2).standard_normal(L).astype(np.float32)
    dev = torch.from_numpy(rec).to(cuda)
    plan = [(0, n, 0), (12345, n, 0), (1001, 50000, 30001), (3, n - 1, 1), (L - 100000, 100000, 44000)]
    check(fe, cuda, rec, dev, plan, n)


def test_many_windows(fe, cuda, small):
    """More windows than a grid's y / z extent (65 535): one workgroup each."""
    rec, dev = small
    n, b = 8, 65600
    rng = np.random.default_rng(3)
    count = rng.integers(0, n + 1, b)
    pad = rng.integers(0, n + 1 - count)
    src = rng.integers(0, len(rec) - n, b)
    plan = np.stack([src, count, pad], 1)
    got = fe.normalize_windows(dev, plan, n).cpu().numpy()
    assert same_bits(got, of.normalize_f32(cut(rec, plan, n)))


def _recording(chirps, seconds, noise=0.003, seed=0):
    """The generator of tests/test_identifytracks.py, restated."""
    rng = np.random.default_rng(seed)
    n = SR * seconds
    x = rng.normal(0, noise, n)
    t = np.arange(n) / SR
    for on, dur, f0, f1 in chirps:
        m = (t >= on) & (t < on + dur)
        tt = t[m] - on
        x[m] += 0.3 * np.sin(2 * np.pi * (f0 * tt + 0.5 * (f1 - f0) / dur * tt * tt))
    return x.astype(np.float32)


def test_predict_tracks_device_windows(tmp_path, cuda, capsys, fe):
    """predict_tracks(detector="gpu", windows="device") against
    windows="host" on the checkpoint and 10 s chirp recording of
    test_predict_cli_with_gpu_detector: the same features, the same
    per-window probabilities, the same ModelResult per track; and the CLI."""
    import identifytracks as it
    import predict
    from acfe.train import FrontEnd
    from audiomodel import build_model
    from scipy.io import wavfile

    ck = tmp_path / "ck"
    ck.mkdir()
    meta = {"labels": ["bird", "noise"], "name": "wr-resnet-bird", "n_mels": 128, "dtype": "bf16"}
    (ck / "metadata.txt").write_text(json.dumps(meta))
    torch.manual_seed(0)
    model = build_model("wr-resnet-bird", (128, 513, 3), 2, torch.bfloat16)
    front = FrontEnd(n_mels=128, n_fft=4096, hop=281, fmin=100, fmax=11000, break_freq=1000, pcen=True,
                     dtype=torch.bfloat16, device=cuda, power=2)
    torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([front, model]).state_dict().items()},
               ck / "model.pt")
    rec = _recording([(1.0, 1.0, 3000, 4000), (4.0, 0.8, 6000, 5000), (7.0, 1.5, 1500, 2500)], seconds=10, seed=3)
    wavfile.write(tmp_path / "rec.wav", SR, (rec * 32767).astype(np.int16))
    rec = predict.load_recording(tmp_path / "rec.wav")

    p = predict.Predictor(ck)
    metas = {}
    for windows in ("host", "device"):
        it.Signal._next_id = 0  # the ids in get_meta count up over the process: the same ones for both calls
        tracks, end = p.predict_tracks(rec, rng=np.random.RandomState(0), detector="gpu", windows=windows)
        assert end == 10.0 and len(tracks) == 3
        assert all(len(t.predictions) == 1 for t in tracks)
        metas[windows] = [t.get_meta() for t in tracks]
    assert metas["device"] == metas["host"]

    # the one batch behind those results, stage by stage
    dev = []
    tracks, frames, end = predict.detect_tracks(rec, detector=p._detector, dev_out=dev)
    assert len(dev) == 1 and dev[0].is_cuda and np.array_equal(dev[0].cpu().numpy(), frames)
    wins = np.concatenate(predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(0)))
    plan, counts = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(0))
    assert len(plan) == len(wins) >= 3 and sum(counts) == len(plan)
    with torch.no_grad():
        f_host = p.frontend(torch.from_numpy(wins).to(cuda), pad_mode="constant")
        f_dev = p.frontend.features(fe.normalize_windows(dev[0], plan, 3 * SR), pad_mode="constant")
    assert f_host.shape == f_dev.shape and torch.equal(f_host, f_dev)
    assert np.array_equal(p.predict_plan(dev[0], plan), p.predict_clips(wins))
    with pytest.raises(ValueError):
        p.predict_tracks(rec, detector="gpu", windows="gpu")

    predict.main([str(ck), "--file", str(tmp_path / "rec.wav"), "--detector", "gpu", "--windows", "device"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["end"] == 10.0 and len(out["tracks"]) == 3
    for t in out["tracks"]:
        assert len(t["predictions"]) == 1
    assert [t["predictions"] for t in out["tracks"]] == \
        json.loads(json.dumps([m["predictions"] for m in metas["device"]], default=float))
