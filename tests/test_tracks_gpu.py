"""The device track detector (acfe/tracks.py over csrc/tracks.hip) against the
host detector it replaces (identifytracks.get_end / signal_noise).

Two comparisons carry the parity.  The magnitude STFT is held to a float64
reference within 2e-5 of its maximum (the bound of the mel front end).
Everything after it thresholds on the last bits of the spectrogram, so it is
compared exactly, on the DEVICE's own spectrogram copied to the host: same
final map cell for cell, same signals in the same order, same tracks.  The
ABI stages (medians, box morphology, runs) are also pinned one by one, exact,
against numpy / scipy."""
import ctypes as C
import json

import numpy as np
import pytest
import torch
from scipy.ndimage import find_objects, label

import identifytracks as it

pytestmark = pytest.mark.gpu

SR = 48000
HOP = 281
CHIRPS = [(2.0, 1.0, 3000, 4000), (8.0, 0.6, 6000, 5000), (14.0, 2.5, 1500, 2500)]
# 4 s: a chirp from t = 0, one that ends on the last sample, and one near 0 Hz
# whose box reaches frequency bin 0
EDGE_CHIRPS = [(0.0, 1.0, 3000, 4000), (1.5, 0.8, 40, 160), (2.8, 1.2, 6000, 5000)]


def _recording(chirps, seconds=20, noise=0.003, seed=0):
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


_CACHE = {}


def recording(name):
    """The test recordings, made once: "even" 4 s (T = 684, not a multiple of
    64), "odd" the same minus one hop (T = 683), "tiny" 1500 samples (T = 6,
    shorter than the FFT and than every morphology box), "chirps" the 20 s
    recording of test_identifytracks."""
    if not _CACHE:
        four = _recording(EDGE_CHIRPS, seconds=4, seed=1)
        _CACHE.update(even=four, odd=four[:-HOP].copy(), tiny=four[:1500].copy(), chirps=_recording(CHIRPS))
    return _CACHE[name]


RECORDINGS = ("even", "odd", "tiny", "chirps")
FRAMES = {"even": 684, "odd": 683, "tiny": 6, "chirps": 1 + 20 * SR // HOP}


@pytest.fixture(scope="module")
def det(cuda):
    from acfe.tracks import SignalDetector

    return SignalDetector(device=cuda, sr=SR)


def stft_f64(x, n_fft=2048, hop=HOP):
    """|rfft| of the centred, zero-padded, periodic-Hann frames in float64."""
    xp = np.pad(x.astype(np.float64), n_fft // 2)
    t = 1 + len(x) // hop
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    idx = np.arange(t)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.abs(np.fft.rfft(xp[idx] * win, axis=-1)).T


@pytest.mark.parametrize("name", ["even", "odd", "tiny"])
def test_stft_matches_float64(det, name):
    """max |got - ref| <= 2e-5 max(ref).  Measured on an MI355X: 1.7e-7 for
    the two 4 s recordings, 1.0e-7 for the 1500-sample one."""
    x = recording(name)
    got = det.spectrogram(x).cpu().numpy()
    ref = stft_f64(x)
    assert got.shape == ref.shape == (1025, FRAMES[name]) and got.dtype == np.float32
    err = np.abs(got - ref).max() / ref.max()
    print(f"stft {name}: max |got - ref| / max(ref) = {err:.3e}")
    assert err <= 2e-5


def test_stft_silent_frames_are_exactly_zero(det):
    x = recording("even").copy()
    x[3 * SR:] = 0
    got = det.spectrogram(x).cpu().numpy()
    first = -(-(3 * SR + 1024) // HOP)  # first frame whose window starts at or after the last sample
    assert first < got.shape[1] - 100
    assert np.all(got[:, first:] == 0.0) and not np.signbit(got[:, first:]).any()
    assert np.all(got[:, first - 8:first].max(0) > 0)


def test_stft_rejects_other_sizes(det):
    from acfe import _lib

    assert _lib.lib.acfe_stft_mag_workspace(48000, 1024, HOP) == _lib.E_INVAL
    assert _lib.lib.acfe_stft_mag_workspace(48000, 4096, HOP) == _lib.E_INVAL
    assert _lib.lib.acfe_stft_mag_workspace(0, 2048, HOP) == _lib.E_INVAL
    buf = torch.zeros(1 << 16, device=det.device)
    p = buf.data_ptr()
    assert _lib.lib.acfe_stft_mag(p, 4096, 1024, HOP, p, p, p, None) == _lib.E_INVAL


def host_final_map(spec):
    """signal_noise's binary map after the morphology, on the host."""
    _, height, width = it.box_geometry(SR)
    s = spec / np.amax(spec)
    m = ((s > 2 * np.median(s, axis=0)[None, :]) & (s > 3 * np.median(s, axis=1)[:, None])).astype(np.uint8)
    m = it._box_max(it._box_min(m, 4, 4), 4, 4)
    return it._box_min(it._box_max(m, height, width), height // 10, width)


def fields(signals):
    return [(s.start, s.end, s.freq_start, s.freq_end, s.mass) for s in signals]


@pytest.mark.parametrize("name", RECORDINGS)
def test_detector_matches_host_on_device_spectrogram(det, name):
    x = recording(name)
    got, spec = det.signal_noise(x)
    spec_host = spec.cpu().numpy()
    assert spec_host.shape == (1025, FRAMES[name])
    want, _ = it.signal_noise(x, SR, spectogram=spec_host)
    assert fields(got) == fields(want)
    assert np.array_equal(det.signal_map(spec).cpu().numpy(), host_final_map(spec_host))
    if name == "tiny":
        assert got == []
    else:
        assert len(got) >= 3
    if name in ("even", "odd"):  # boxes on both time edges and on frequency bin 0
        t = FRAMES[name]
        assert any(s.start == 0 for s in got) and any(s.end == t * HOP / SR for s in got)
        assert any(s.freq_start == 0 for s in got)
    end = len(x) / SR
    assert fields(it.get_tracks_from_signals(got, end)) == fields(it.get_tracks_from_signals(want, end))


# ---------------------------------------------------------------------------
# ABI stages


def tie_rows(length, rng):
    """Rows of one length: continuous values, a few distinct values, all
    equal, mostly zero -- finite and non-negative."""
    return np.stack([
        rng.random(length) ** 4 * 1e3,
        rng.integers(0, 4, length) * 0.25,
        np.full(length, 0.7),
        np.where(rng.random(length) < 0.8, 0.0, rng.random(length)),
        np.where(rng.random(length) < 0.5, 0.0, 1e-30 * rng.random(length)),
    ]).astype(np.float32)


@pytest.mark.parametrize("length", [1, 2, 3, 1025, 4096, 4097])
def test_median_matches_numpy(cuda, length):
    from acfe import tracks

    rng = np.random.default_rng(length)
    img = tie_rows(length, rng)  # [5, length]
    got = tracks.median(torch.from_numpy(img).to(cuda), 1).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, np.median(img, axis=1))
    # the other axis: `length` rows, 70 columns (several workgroups, a partial last one)
    tall = np.ascontiguousarray(np.concatenate([tie_rows(length, rng) for _ in range(14)]).T)
    assert tall.shape == (length, 70)
    got = tracks.median(torch.from_numpy(tall).to(cuda), 0).cpu().numpy()
    assert np.array_equal(got, np.median(tall, axis=0))


def test_median_of_scaled_image(cuda):
    """np.median(S / max(S)) along both axes of a [1025, 130] image, from S."""
    from acfe import tracks

    rng = np.random.default_rng(7)
    img = (rng.random((1025, 130)) ** 6 * 37.0).astype(np.float32)
    img[rng.random(img.shape) < 0.1] = 0
    d = torch.from_numpy(img).to(cuda)
    mx = d.amax().reshape(1)
    s = img / np.amax(img)
    assert np.array_equal(tracks.median(d, 1, mx).cpu().numpy(), np.median(s, axis=1))  # 130: even count
    assert np.array_equal(tracks.median(d, 0, mx).cpu().numpy(), np.median(s, axis=0))  # 1025: odd count


BOXES = [(4, 4), (6, 42), (3, 5), (1, 7), (0, 42), (40, 300)]


@pytest.mark.parametrize("shape", [(23, 31), (1025, 130), (5, 200)])
def test_morph_box_matches_host(cuda, shape):
    from acfe import tracks

    rng = np.random.default_rng(shape[0])
    a = (rng.random(shape) < 0.3).astype(np.uint8)
    d = torch.from_numpy(a).to(cuda)
    for h, w in BOXES:
        assert np.array_equal(tracks.morph_box(d, h, w, tracks.DILATE).cpu().numpy(), it._box_max(a, h, w)), (h, w)
        assert np.array_equal(tracks.morph_box(d, h, w, tracks.ERODE).cpu().numpy(), it._box_min(a, h, w)), (h, w)
    # erosion only shows on a dense map
    b = (rng.random(shape) < 0.97).astype(np.uint8)
    db = torch.from_numpy(b).to(cuda)
    for h, w in BOXES[:5]:
        assert np.array_equal(tracks.morph_box(db, h, w, tracks.ERODE).cpu().numpy(), it._box_min(b, h, w)), (h, w)


def label_stats(m):
    lab, n = label(m, structure=np.ones((3, 3), np.uint8))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    stats = []
    for k, sl in enumerate(find_objects(lab), start=1):
        top, left = sl[0].start, sl[1].start
        stats.append((left, top, sl[1].stop - left, sl[0].stop - top, int(area[k])))
    stats.sort(key=lambda s: s[0])
    return stats


def device_boxes(m, cuda, capacity=None):
    from acfe import tracks

    return it.boxes_from_runs(tracks.map_runs(torch.from_numpy(np.ascontiguousarray(m, np.uint8)).to(cuda), capacity))


@pytest.mark.parametrize("shape,density,box", [((23, 31), 0.03, (2, 3)), ((1025, 130), 0.002, (6, 42)),
                                               ((40, 700), 0.01, (2, 9))])
def test_runs_and_union_match_scipy_label(cuda, shape, density, box):
    rng = np.random.default_rng(shape[1])
    m = it._box_max((rng.random(shape) < density).astype(np.uint8), *box)
    want = label_stats(m)
    assert len(want) > 3 and device_boxes(m, cuda) == want


def test_runs_edge_cases(cuda):
    from acfe import _lib, tracks

    assert device_boxes(np.zeros((9, 70), np.uint8), cuda) == []
    assert device_boxes(np.ones((9, 200), np.uint8), cuda) == [(0, 0, 200, 9, 1800)]  # runs across 64-cell steps
    diag = np.eye(70, dtype=np.uint8)
    assert device_boxes(diag, cuda) == [(0, 0, 70, 70, 70)]
    assert device_boxes(diag[:, ::-1], cuda) == [(0, 0, 70, 70, 70)]
    # a first buffer far too small: the call reports the count, one retry holds them all
    rng = np.random.default_rng(5)
    m = (rng.random((64, 300)) < 0.3).astype(np.uint8)
    want = label_stats(m)
    assert device_boxes(m, cuda, capacity=3) == want == device_boxes(m, cuda)
    d = torch.from_numpy(m).to(cuda)
    n_runs = len(tracks.map_runs(d))
    runs = torch.full((3, 3), -1, dtype=torch.int32, device=cuda)
    guard = runs.clone()
    count = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("acfe_map_runs", d.data_ptr(), 64, 300, runs.data_ptr(), 2, count.data_ptr(), None)
    torch.cuda.synchronize()
    assert int(count.item()) == n_runs > 100
    assert torch.equal(runs[2], guard[2]) and (runs[:2] >= 0).all()  # nothing stored past cap


@pytest.mark.parametrize("noise_s,silent_s", [(3, 3), (5, 0)])
def test_get_end_matches_host(det, noise_s, silent_s):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.normal(0, 0.1, SR * noise_s), np.zeros(SR * silent_s)]).astype(np.float32)
    want = it.get_end(x, SR)
    got = det.get_end(x)
    assert got == want and type(got) is type(want)
    assert want == (3 if silent_s else 5.0)


def test_predict_cli_with_gpu_detector(tmp_path, cuda, capsys):
    """predict.main --detector gpu against --detector host on a 10 s recording
    of clean chirps: same `end`, same number of tracks, one prediction each.
    The track boxes themselves are not compared between the two runs: the host
    STFT and the device STFT differ in their last bits and the detector
    thresholds on them (the exact comparison, on one spectrogram, is
    test_detector_matches_host_on_device_spectrogram)."""
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
    fe = FrontEnd(n_mels=128, n_fft=4096, hop=281, fmin=100, fmax=11000, break_freq=1000, pcen=True,
                  dtype=torch.bfloat16, device=cuda, power=2)
    torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([fe, model]).state_dict().items()}, ck / "model.pt")
    rec = _recording([(1.0, 1.0, 3000, 4000), (4.0, 0.8, 6000, 5000), (7.0, 1.5, 1500, 2500)], seconds=10, seed=3)
    wavfile.write(tmp_path / "rec.wav", SR, (rec * 32767).astype(np.int16))
    out = {}
    for detector in ("host", "gpu"):
        predict.main([str(ck), "--file", str(tmp_path / "rec.wav"), "--detector", detector])
        out[detector] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["gpu"]["end"] == out["host"]["end"] == 10.0
    assert len(out["gpu"]["tracks"]) == len(out["host"]["tracks"]) == 3
    for t in out["gpu"]["tracks"]:
        assert len(t["predictions"]) == 1
