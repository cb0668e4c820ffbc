"""acfe_resample_poly (csrc/resample.hip): scipy.signal.resample_poly of a
device recording with float64 accumulation, its Python wrapper
frontend.resample_poly, load_recording(resample="device") and the predict
entry points on a device tensor.

The kernel writes TILE = 256 outputs per workgroup and grid step.

Reference: the float64 formula of tests/resample_ref.py, with taps recomputed
from firwin (not taken from predict.resample_plan).  Bound, per sample:
  |got - ref| <= 2^-24 |ref| + 2^-45 A + 2^-149,    A = sum |h x| in float64
-- the one final rounding to float32; a generous cover of the float64
roundings of at most 81 terms (83 * 2^-53 < 2^-46); a result at the bottom of
the float32 range.  Against scipy's float32 resample_poly the bound is that
plus (K + 2) * 2^-24 * A, scipy's own float32 accumulation error over K terms."""
import json
import logging

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

import resample_ref as rr

pytestmark = pytest.mark.gpu

SR = 48000
TILE = 256
GUARD = 12345.0
# (up, down) -> the source rate
RATIOS = [(3, 1), (6, 1), (3, 2), (1, 2), (3, 4), (1, 4), (160, 147), (320, 147), (640, 147)]
N_OUTS = [0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


def rate_of(up, down):
    assert SR * down % up == 0
    return SR * down // up


@pytest.fixture(scope="module")
def fe(cuda):
    from acfe import frontend

    return frontend


@pytest.fixture(scope="module")
def predict():
    import predict

    return predict


def bound(ref, a):
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -45 * a + 2.0 ** -149


def abi(cuda, x, h, up, down, t0, n_out, x_off=0, out_off=0, n_in=None, n_taps=None):
    """acfe_resample_poly of the numpy samples x (float32 or int16) into the
    middle of a buffer of guard values -> (rc, out[n_out], guards untouched).
    x_off / out_off: floats by which the input / output base is moved off a
    16-B boundary."""
    from acfe import _lib

    pad = np.zeros(x_off, x.dtype)
    xd = torch.from_numpy(np.concatenate([pad, x])).to(cuda)[x_off:]
    hd = torch.from_numpy(np.ascontiguousarray(h, np.float32)).to(cuda)
    buf = torch.full((n_out + 16,), GUARD, dtype=torch.float32, device=cuda)
    o = buf[4 + out_off:]
    assert buf.data_ptr() % 16 == 0 and (x_off == 0 or len(x) == 0 or xd.data_ptr() % 16 != 0)
    code = _lib.DTYPE_I16 if x.dtype == np.int16 else _lib.DTYPE_F32
    rc = _lib.lib.acfe_resample_poly(xd.data_ptr(), code, len(x) if n_in is None else n_in, hd.data_ptr(),
                                     len(h) if n_taps is None else n_taps, up, down, t0, o.data_ptr(), n_out,
                                     torch.cuda.current_stream().cuda_stream)
    got = buf.cpu().numpy()
    lo, hi = 4 + out_off, 4 + out_off + n_out
    return rc, got[lo:hi], bool((got[:lo] == GUARD).all() and (got[hi:] == GUARD).all())


@pytest.mark.parametrize("up,down", RATIOS)
def test_ratios_lengths_alignments(cuda, up, down):
    """Every n_out of N_OUTS from the shortest input that reaches it (the
    outputs past ceil(n_in up / down) see zeros), and n_in in {1, 2, K - 1, K,
    K + 1} with the natural output length, which is also compared with scipy;
    input and output base on and one float off a 16-B boundary."""
    h, t0 = rr.taps(up, down)
    k = rr.terms(h, up)
    rng = np.random.default_rng(100 * up + down)
    cases = [(-(-m * down // up), m) for m in N_OUTS] + [(n, rr.n_out(n, up, down)) for n in (1, 2, k - 1, k, k + 1)]
    for n_in, n_out in cases:
        x = rng.standard_normal(n_in).astype(np.float32)
        ref, a = rr.formula(x, h, up, down, t0, np.arange(n_out))
        for x_off, out_off in ((0, 0), (1, 1)):
            rc, got, guards = abi(cuda, x, h, up, down, t0, n_out, x_off, out_off)
            assert rc == 0 and guards, (n_in, n_out, x_off)
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bound(ref, a)).all(), (n_in, n_out, x_off, float((err / bound(ref, a)).max()))
            if n_in and n_out == rr.n_out(n_in, up, down):
                sp = resample_poly(x, up, down)
                assert sp.dtype == np.float32 and len(sp) == n_out
                err = np.abs(got.astype(np.float64) - sp.astype(np.float64))
                assert (err <= bound(ref, a) + (k + 2) * 2.0 ** -24 * a).all(), (n_in, n_out, x_off)


def test_empty_input_writes_zeros(cuda):
    h, t0 = rr.taps(3, 1)
    rc, got, guards = abi(cuda, np.zeros(0, np.float32), h, 3, 1, t0, TILE + 3)
    assert rc == 0 and guards and (got.view(np.uint32) == 0).all()


@pytest.mark.parametrize("up,down", [(3, 1), (1, 2), (160, 147), (640, 147)])
def test_impulses_pick_single_taps(cuda, up, down):
    """x = delta at sample 0, at n_in - 1 and at the sample whose outputs
    straddle the seam of the second and third tile: every output is one tap
    times 1.0, i.e. float32(h[p + k up]) or 0, bit for bit."""
    h, t0 = rr.taps(up, down)
    n_out = 3 * TILE + 5
    n_in = -(-n_out * down // up)
    seam = (2 * TILE * down + t0) // up - rr.terms(h, up) // 2  # its taps lie on both sides of output 2 TILE
    assert 0 < seam < n_in - 1
    hit = False
    for at in (0, n_in - 1, seam):
        x = np.zeros(n_in, np.float32)
        x[at] = 1.0
        ref, _ = rr.formula(x, h, up, down, t0, np.arange(n_out))
        ref = ref.astype(np.float32)
        assert np.isin(ref[ref != 0], h).all() and (ref != 0).any()
        rc, got, guards = abi(cuda, x, h, up, down, t0, n_out, 1, 1)
        assert rc == 0 and guards
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (at, np.flatnonzero(got != ref)[:8])
        if at == seam:
            hit = (ref[:2 * TILE] != 0).any() and (ref[2 * TILE:] != 0).any()  # taps on both sides of the seam
    assert hit


@pytest.mark.parametrize("up,down", [(3, 1), (160, 147)])
def test_int16_is_the_float32_path_of_the_converted_samples(fe, cuda, up, down):
    rng = np.random.default_rng(7)
    x = rng.integers(-32768, 32768, 3 * TILE + 11).astype(np.int16)
    x[5], x[6], x[-1] = -32768, 32767, -32768
    xf = x.astype(np.float32) / 32767.0
    rate = rate_of(up, down)
    a = fe.resample_poly(torch.from_numpy(x).to(cuda), rate)
    b = fe.resample_poly(torch.from_numpy(xf).to(cuda), rate)
    assert a.dtype == torch.float32 and a.shape == (rr.n_out(len(x), up, down),)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
    h, t0 = rr.taps(up, down)
    ref, amp = rr.formula(xf, h, up, down, t0)
    assert (np.abs(b.cpu().numpy().astype(np.float64) - ref) <= bound(ref, amp)).all()
    # the same through the ABI with the input one sample (2 bytes) off
    rc, got, guards = abi(cuda, x, h, up, down, t0, len(ref), 1, 0)
    assert rc == 0 and guards and np.array_equal(got.view(np.uint32), a.cpu().numpy().view(np.uint32))


def test_same_rate(fe, cuda):
    x = np.random.default_rng(8).integers(-32768, 32768, TILE + 9).astype(np.int16)
    x[0], x[1] = -32768, 32767
    got = fe.resample_poly(torch.from_numpy(x).to(cuda), SR)
    assert got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), (x.astype(np.float32) / 32767.0).view(np.uint32))
    xf = torch.randn(100, device=cuda)
    assert fe.resample_poly(xf, SR) is xf
    out = torch.empty(100, dtype=torch.float32, device=cuda)
    assert fe.resample_poly(xf, 44100, 44100, out=out) is out and torch.equal(out, xf)


def test_wrapper(fe, cuda):
    """n_out, the taps cache, `out`, and the arguments it refuses."""
    x = np.random.default_rng(9).standard_normal(1000).astype(np.float32)
    xd = torch.from_numpy(x).to(cuda)
    got = fe.resample_poly(xd, 44100)
    assert got.shape == (1089,) and got.dtype == torch.float32 and got.device == xd.device
    h, t0 = rr.taps(160, 147)
    ref, a = rr.formula(x, h, 160, 147, t0)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= bound(ref, a)).all()
    taps = fe._RESAMPLE_TAPS[(44100, SR, xd.device)][1]
    assert np.array_equal(taps.cpu().numpy().view(np.uint32), h.view(np.uint32))
    buf = torch.full((1089 + 8,), GUARD, dtype=torch.float32, device=cuda)
    assert fe.resample_poly(xd, 44100, out=buf[3:3 + 1089]).data_ptr() == buf[3:].data_ptr()
    assert fe._RESAMPLE_TAPS[(44100, SR, xd.device)][1] is taps
    assert torch.equal(buf[3:3 + 1089], got) and (buf[:3] == GUARD).all() and (buf[3 + 1089:] == GUARD).all()
    assert fe.resample_poly(xd[:0], 16000).shape == (0,)
    with pytest.raises(ValueError, match="44101"):
        fe.resample_poly(xd, 44101)
    with pytest.raises(ValueError):
        fe.resample_poly(xd, 44100, out=buf[:1000])
    with pytest.raises(ValueError):
        fe.resample_poly(xd, 44100, out=torch.empty(1089, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        fe.resample_poly(xd.cpu(), 44100)
    with pytest.raises((TypeError, ValueError)):
        fe.resample_poly(xd[::2], 44100)
    with pytest.raises(TypeError):
        fe.resample_poly(xd.double(), 44100)
    with pytest.raises(TypeError):
        fe.resample_poly(xd.view(10, 100), 44100)


def test_abi_refuses_bad_arguments(cuda):
    from acfe import _lib

    h, t0 = rr.taps(3, 1)
    x = np.ones(100, np.float32)
    big = np.zeros(16385, np.float32)
    for kw in (dict(n_taps=16385, h=big), dict(up=0), dict(down=0), dict(up=-3), dict(n_in=-1), dict(n_out=-1),
               dict(n_taps=0), dict(t0=-1), dict(code=1), dict(code=3), dict(down=2 ** 31 - 1, n_out=2 ** 33)):
        a = dict(h=h, up=3, down=1, t0=t0, n_out=300, n_in=100, n_taps=None, code=_lib.DTYPE_F32)
        a.update(kw)
        xd = torch.from_numpy(x).to(cuda)
        hd = torch.from_numpy(a["h"]).to(cuda)
        buf = torch.full((316,), GUARD, dtype=torch.float32, device=cuda)
        rc = _lib.lib.acfe_resample_poly(xd.data_ptr(), a["code"], a["n_in"], hd.data_ptr(),
                                         len(a["h"]) if a["n_taps"] is None else a["n_taps"], a["up"], a["down"],
                                         a["t0"], buf[4:].data_ptr(), a["n_out"], None)
        torch.cuda.synchronize()
        assert rc == _lib.E_INVAL, kw
        assert (buf.cpu().numpy() == GUARD).all(), kw  # nothing was launched
    # exactly 16384 taps are taken: a filter of that length whose last tap alone is set
    big = np.zeros(16384, np.float32)
    big[-1] = 2.0
    rc, got, guards = abi(cuda, x, big, 16384, 1, 16383, 50)  # t = n + 16383: p = 16383, j0 = 0 at n = 0 only
    assert rc == 0 and guards and got[0] == 2.0 and (got[1:] == 0).all()


def test_64_bit_sample_indices(fe, cuda):
    """620 s at 44.1 kHz: t = n * 147 + t0 passes 2^31 and 2^32 inside the
    recording.  Four windows of 4096 outputs against the formula."""
    up, down = 160, 147
    n_in = 44100 * 620
    x = np.random.default_rng(10).standard_normal(n_in, dtype=np.float32)
    got = fe.resample_poly(torch.from_numpy(x).to(cuda), 44100)
    n_out = rr.n_out(n_in, up, down)
    assert got.shape == (n_out,) and (n_out - 1) * down > 2 ** 32
    h, t0 = rr.taps(up, down)
    for first in (0, 2 ** 31 // down - 2048, 2 ** 32 // down - 2048, n_out - 4096):
        n = np.arange(first, first + 4096, dtype=np.int64)
        ref, a = rr.formula(x, h, up, down, t0, n)
        err = np.abs(got[first:first + 4096].cpu().numpy().astype(np.float64) - ref)
        assert (err <= bound(ref, a)).all(), (first, float((err / bound(ref, a)).max()))
        assert np.abs(ref).max() > 0.5


def scipy_bound_ok(got, x, up, down, host):
    h, t0 = rr.taps(up, down)
    ref, a = rr.formula(x, h, up, down, t0)
    err = np.abs(got.astype(np.float64) - host.astype(np.float64))
    return len(got) == len(host) and bool((err <= bound(ref, a) + (rr.terms(h, up) + 2) * 2.0 ** -24 * a).all())


def test_load_recording_device(fe, predict, cuda, tmp_path):
    from scipy.io import wavfile

    rng = np.random.default_rng(11)
    mono = (rng.standard_normal(2 * 44100) * 6000).astype(np.int16)
    wavfile.write(tmp_path / "mono.wav", 44100, mono)
    got = predict.load_recording(tmp_path / "mono.wav", resample="device", device=cuda)
    assert isinstance(got, torch.Tensor) and got.device == cuda and got.dtype == torch.float32 and got.dim() == 1
    xf = mono.astype(np.float32) / 32767.0
    assert torch.equal(got, fe.resample_poly(torch.from_numpy(xf).to(cuda), 44100))
    host = predict.load_recording(tmp_path / "mono.wav")
    assert isinstance(host, np.ndarray) and scipy_bound_ok(got.cpu().numpy(), xf, 160, 147, host)

    stereo = (rng.standard_normal((4000, 2)) * 6000).astype(np.int16)
    wavfile.write(tmp_path / "stereo.wav", 44100, stereo)
    got = predict.load_recording(tmp_path / "stereo.wav", resample="device", device=cuda)
    xf = (stereo.astype(np.float32) / 32767.0).mean(1)
    assert torch.equal(got, fe.resample_poly(torch.from_numpy(xf).to(cuda), 44100))
    assert scipy_bound_ok(got.cpu().numpy(), xf, 160, 147, predict.load_recording(tmp_path / "stereo.wav"))

    flt = (rng.standard_normal(4000) * 0.2).astype(np.float32)
    wavfile.write(tmp_path / "float.wav", 16000, flt)
    got = predict.load_recording(tmp_path / "float.wav", resample="device", device=cuda)
    assert got.shape == (12000,)
    assert scipy_bound_ok(got.cpu().numpy(), flt, 3, 1, predict.load_recording(tmp_path / "float.wav"))

    # already at 48 kHz: uploaded, not resampled
    wavfile.write(tmp_path / "same.wav", SR, mono[:5000])
    got = predict.load_recording(tmp_path / "same.wav", resample="device", device=cuda)
    assert isinstance(got, torch.Tensor) and got.device == cuda
    assert np.array_equal(got.cpu().numpy(), predict.load_recording(tmp_path / "same.wav"))


def test_load_recording_falls_back_to_the_host(predict, cuda, tmp_path, caplog):
    from scipy.io import wavfile

    x = (np.random.default_rng(12).standard_normal(300) * 6000).astype(np.int16)
    wavfile.write(tmp_path / "odd.wav", 44101, x)
    with caplog.at_level(logging.WARNING):
        got = predict.load_recording(tmp_path / "odd.wav", resample="device", device=cuda)
    assert len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got, predict.load_recording(tmp_path / "odd.wav"))


def _recording(chirps, seconds, sr, noise=0.003, seed=0):
    """The generator of tests/test_sosfilt_gpu.py at a sample rate of choice."""
    rng = np.random.default_rng(seed)
    n = sr * seconds
    x = rng.normal(0, noise, n)
    t = np.arange(n) / sr
    for on, dur, f0, f1 in chirps:
        m = (t >= on) & (t < on + dur)
        tt = t[m] - on
        x[m] += 0.3 * np.sin(2 * np.pi * (f0 * tt + 0.5 * (f1 - f0) / dur * tt * tt))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def checkpoint(cuda, tmp_path_factory):
    from acfe.train import FrontEnd
    from audiomodel import build_model

    ck = tmp_path_factory.mktemp("ck")
    meta = {"labels": ["bird", "noise"], "name": "wr-resnet-bird", "n_mels": 128, "dtype": "bf16"}
    (ck / "metadata.txt").write_text(json.dumps(meta))
    torch.manual_seed(0)
    model = build_model("wr-resnet-bird", (128, 513, 3), 2, torch.bfloat16)
    front = FrontEnd(n_mels=128, n_fft=4096, hop=281, fmin=100, fmax=11000, break_freq=1000, pcen=True,
                     dtype=torch.bfloat16, device=cuda, power=2)
    torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([front, model]).state_dict().items()},
               ck / "model.pt")
    return ck


@pytest.fixture(scope="module")
def predictor(predict, checkpoint, cuda):
    return predict.Predictor(checkpoint, device=cuda)


@pytest.fixture(scope="module")
def wav_44k(tmp_path_factory):
    from scipy.io import wavfile

    rec = _recording([(1.0, 1.0, 3000, 4000), (4.0, 0.8, 6000, 5000), (7.0, 1.5, 1500, 2500)], 10, 44100, seed=3)
    path = tmp_path_factory.mktemp("rec") / "rec44k.wav"
    wavfile.write(path, 44100, (rec * 32767).astype(np.int16))
    return path


def test_predict_tracks_on_the_device_tensor(predict, predictor, checkpoint, wav_44k, cuda, monkeypatch, capsys):
    """predict_tracks on the tensor of load_recording(resample="device") with
    the GPU detector and device windows -- no download of the samples --
    against the same call on that tensor's numpy copy: the same 48 kHz
    samples, so the same tracks and the same probabilities.  The difference
    to the host-resampled recording is printed, not asserted."""
    import identifytracks as it

    p = predictor
    dev = predict.load_recording(wav_44k, resample="device", device=cuda)
    assert isinstance(dev, torch.Tensor) and dev.shape == (10 * SR,)
    probs = []

    def spy(*a, _f=p.predict_plan, **k):
        probs.append(_f(*a, **k))
        return probs[-1]

    monkeypatch.setattr(p, "predict_plan", spy)

    def tracks_of(frames, **kw):
        it.Signal._next_id = 0
        tracks, end = p.predict_tracks(frames, rng=np.random.RandomState(0), **kw)
        return [t.get_meta() for t in tracks], end

    with monkeypatch.context() as m:
        m.setattr(predict, "host_frames", None)  # downloading the recording would raise
        on_dev, end = tracks_of(dev, detector="gpu", windows="device")
    as_numpy, end2 = tracks_of(dev.cpu().numpy(), detector="gpu", windows="device")
    # how the detector groups the chirps of a band-limited recording is its own business: at least one track
    assert end == end2 == 10.0 and len(on_dev) >= 1 and all(len(t["predictions"]) == 1 for t in on_dev)
    assert on_dev == as_numpy and len(probs) == 2 and np.array_equal(probs[0], probs[1])
    # host windows need host samples: the tensor is downloaded once and gives what numpy input gives
    assert tracks_of(dev, detector="gpu", windows="host") == tracks_of(dev.cpu().numpy(), detector="gpu",
                                                                       windows="host")
    host, _ = tracks_of(predict.load_recording(wav_44k), detector="gpu", windows="device")
    with capsys.disabled():
        same = [{k: v for k, v in t.items() if k != "predictions"} for t in host] == \
            [{k: v for k, v in t.items() if k != "predictions"} for t in on_dev]
        diff = np.abs(probs[-1] - probs[0]).max() if probs[-1].shape == probs[0].shape else None
        print("\nhost against device resampling: same tracks:", same, "; max |p_device - p_host|:", diff)

    capsys.readouterr()
    predict.main([str(checkpoint), "--file", str(wav_44k), "--resample", "device", "--windows", "device",
                  "--detector", "gpu"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["end"] == 10.0 and len(out["tracks"]) == len(on_dev)


def test_predict_windows_on_the_device_tensor(predict, predictor, wav_44k, cuda):
    dev = predict.load_recording(wav_44k, resample="device", device=cuda)
    a = predictor.predict_windows(dev, stride=2.0)
    b = predictor.predict_windows(dev.cpu().numpy(), stride=2.0)
    assert a.shape == (4, 2) and np.array_equal(a, b)
    short = dev[:SR]  # zero padded to one window on either path
    assert np.array_equal(predictor.predict_windows(short), predictor.predict_windows(short.cpu().numpy()))
    with pytest.raises(TypeError):
        predictor.predict_windows(dev.double())
