"""predict.resample_plan: the taps, the output length and the index arithmetic
of scipy.signal.resample_poly(x, up, down) for a float32 x, as the device
resampler (acfe_resample_poly) is given them.  No GPU.

Bound of the formula against scipy's float32 output, per sample:
(K + 2) * 2^-24 * sum |h x| with K the number of terms (21 when up-sampling,
ceil(taps / up) otherwise: 41 for 96 kHz, 81 for 192 kHz): scipy accumulates K float32 products in
float32, each step rounding by at most 2^-24 of the running magnitude, which
sum |h x| bounds; the float64 formula's own error is far below that."""
import numpy as np
import pytest
from scipy.signal import resample_poly

import resample_ref as rr

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 64000, 96000, 192000]
LENGTHS = [1, 2, 7, 1000, 5003]


@pytest.fixture(scope="module")
def predict():
    import predict

    return predict


@pytest.mark.parametrize("rate", RATES)
def test_plan_is_scipys(predict, rate):
    up, down = rr.ratio(rate)
    plan = predict.resample_plan(rate)
    h, t0 = rr.taps(up, down)
    assert (plan.up, plan.down, plan.t0) == (up, down, t0)
    assert plan.h.dtype == np.float32 and np.array_equal(plan.h.view(np.uint32), h.view(np.uint32))
    assert plan.device and len(plan.h) == 20 * max(up, down) + 1
    k = rr.terms(h, up)
    assert plan.terms == k and k == (21 if up > down else -(-(20 * down + 1) // up))
    rng = np.random.default_rng(rate)
    for n_in in LENGTHS:
        x = rng.standard_normal(n_in).astype(np.float32)
        ref = resample_poly(x, up, down)
        assert ref.dtype == np.float32
        assert plan.n_out(n_in) == len(ref) == rr.n_out(n_in, up, down)
        got, a = rr.formula(x, plan.h, plan.up, plan.down, plan.t0)
        err = np.abs(got - ref.astype(np.float64))
        assert (err <= (k + 2) * 2.0 ** -24 * a).all(), (rate, n_in, float((err / np.maximum(a, 1e-300)).max()))


def test_device_capable_up_to_16384_taps(predict):
    assert predict.RESAMPLE_MAX_TAPS == 16384
    p = predict.resample_plan(11025)
    assert len(p.h) == 12801 and p.device
    p = predict.resample_plan(44101)
    assert (p.up, p.down, len(p.h)) == (48000, 44101, 960001) and not p.device
    p = predict.resample_plan(16000, 22050)  # up 441, down 320: 8821 taps
    assert (p.up, p.down, len(p.h)) == (441, 320, 8821) and p.device
    p = predict.resample_plan(48000, 44100 * 6)  # up 441, down 80
    assert len(p.h) == 8821 and p.device
    p = predict.resample_plan(1000, 819)  # 20001 taps
    assert len(p.h) == 20001 and not p.device


def test_same_rate_is_the_identity(predict):
    for rate, sr in [(48000, 48000), (44100, 44100)]:
        p = predict.resample_plan(rate, sr)
        assert (p.up, p.down, p.t0, p.terms) == (1, 1, 0, 1) and p.device
        assert p.h.dtype == np.float32 and p.h.tolist() == [1.0]
        x = np.random.default_rng(1).standard_normal(50).astype(np.float32)
        assert p.n_out(len(x)) == 50
        got, _ = rr.formula(x, p.h, 1, 1, 0)
        assert np.array_equal(got, x.astype(np.float64))
    with pytest.raises(ValueError):
        predict.resample_plan(0)


def test_load_recording_host_default_unchanged(predict, tmp_path):
    from scipy.io import wavfile

    x = (np.random.default_rng(2).standard_normal(4410) * 8000).astype(np.int16)
    wavfile.write(tmp_path / "a.wav", 44100, x)
    got = predict.load_recording(tmp_path / "a.wav")
    ref = resample_poly(x.astype(np.float32) / 32767.0, 160, 147).astype(np.float32)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref)
    assert np.array_equal(got, predict.load_recording(tmp_path / "a.wav", resample="host"))
    with pytest.raises(ValueError):
        predict.load_recording(tmp_path / "a.wav", resample="gpu")
