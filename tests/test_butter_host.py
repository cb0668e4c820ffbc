"""The Butterworth band-pass of predict's track path on the host (reference
predict_utils.load_samples :103-113, butter_bandpass :245-262): the filter
design and its rules past Nyquist, track_windows(filter_freqs / filter_below)
against an independent restatement, and the tables of the device path
(sos_segment_plan, check_sos_segments) applied with numpy."""
import logging

import numpy as np
import pytest
from scipy.signal import butter, sosfilt

import identifytracks as it
import predict

SR = 48000
N = 3 * SR


def test_butter_bandpass_equals_scipy():
    for lo, hi in [(1000, 3000), (20, 24), (100, 110), (2500.5, 11000), (1, 23999)]:
        sos = predict.butter_bandpass(lo, hi, SR)
        ref = butter(2, [lo / (0.5 * SR), hi / (0.5 * SR)], analog=False, btype="bandpass", output="sos")
        assert sos.dtype == np.float64 and sos.shape == (2, 6) and np.array_equal(sos, ref)
    for lo, hi in [(0, 3000), (0, 150), (-5, 9000), (None, 4000)]:
        sos = predict.butter_bandpass(lo, hi, SR)
        ref = butter(2, [hi / (0.5 * SR)], analog=False, btype="lowpass", output="sos")
        assert sos.dtype == np.float64 and sos.shape == (1, 6) and np.array_equal(sos, ref)
    assert np.array_equal(predict.butter_bandpass(500, 900, 16000, order=3),
                          butter(3, [500 / 8000, 900 / 8000], btype="bandpass", output="sos"))
    x = np.random.default_rng(0).standard_normal(5000).astype(np.float32)
    got = predict.butter_bandpass_filter(x, 1000, 3000, SR)
    assert got.dtype == np.float64 and np.array_equal(got, sosfilt(predict.butter_bandpass(1000, 3000, SR), x))


def test_butter_bandpass_nyquist_and_inverted_bands(caplog):
    nyq = SR / 2
    with caplog.at_level(logging.WARNING):
        for hi in (nyq, nyq + 1, 30000, None):  # highcut at or past Nyquist: high-pass at lowcut
            caplog.clear()
            sos = predict.butter_bandpass(2000, hi, SR)
            assert np.array_equal(sos, butter(2, [2000 / nyq], btype="highpass", output="sos")) and sos.shape == (1, 6)
            assert len(caplog.records) == 1
        for lo, hi in [(0, nyq), (0, 40000), (None, None), (0, None), (30000, 40000),  # no usable edge
                       (3000, 3000), (3000, 1000), (0, 0), (25000, 1000)]:  # empty or inverted band
            caplog.clear()
            assert predict.butter_bandpass(lo, hi, SR) is None
            assert len(caplog.records) == 1
            assert predict.butter_bandpass_filter(np.ones(8), lo, hi, SR) is None
        caplog.clear()
        predict.butter_bandpass(1000, 3000, SR)
        predict.butter_bandpass(0, 3000, SR)
        assert not caplog.records


def load_samples_restated(frames, tracks, filter_freqs, filter_below, rng, fmin=100, fmax=11000):
    """load_samples (:59-150) for stride 1, 3 s windows, tracks not padded:
    slice, sosfilt, cast, cut -- written from the reference, not from
    predict.track_windows: the window starts are enumerated, not iterated."""
    out = []
    for t in tracks:
        if t.freq_start > fmax or t.freq_end < fmin:
            out.append(np.zeros((0, N), np.float32))
            continue
        a, b = int(SR * t.start), int(t.end * SR)
        if b - a < N:
            missing = N - (b - a)
            a -= missing // 2
            if a <= 0:
                a, b = 0, min(N, len(frames))
            else:
                b = b + missing - missing // 2
                if b > len(frames):
                    b = len(frames)
                    a = max(b - N, 0)
        x = frames[a:b]
        if filter_freqs or (filter_below and t.freq_end < filter_below):
            lo, hi = t.freq_start / (SR / 2), t.freq_end / (SR / 2)
            if hi >= 1:
                sos = butter(2, [lo], btype="highpass", output="sos")
            elif lo > 0:
                sos = butter(2, [lo, hi], btype="bandpass", output="sos")
            else:
                sos = butter(2, [hi], btype="lowpass", output="sos")
            x = sosfilt(sos, x).astype(np.float32)
        n_win = 1 + max(0, int(np.floor(t.length - 3)))  # window s >= 1 exists while s + 3 <= length
        wins = []
        for s in range(n_win):
            w = x[s * SR:s * SR + N] if s else x[:min(b, N)]
            if len(w) != N:
                off = int(rng.randint(0, N - len(w)))
                w = np.pad(w, (off, N - len(w) - off))
            wins.append(w)
        out.append(np.stack(wins).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def scene():
    frames = np.random.default_rng(5).standard_normal(12 * SR).astype(np.float32)
    tracks = [it.Signal(2.0, 7.5, 1000, 3000, 1),  # multi-window: 5.5 s -> windows at +0, +1, +2 s
              it.Signal(5.0, 6.2, 0, 800, 1),  # short, centred; low-pass
              it.Signal(11.3, 12.0, 4000, 9000, 1),  # at the recording's end
              it.Signal(3.0, 4.0, 12000, 15000, 1),  # outside [fmin, fmax]: not classified
              it.Signal(0.2, 1.0, 6000, 25000, 1),  # near the start, band past Nyquist: high-pass
              it.Signal(8.0, 9.0, 200, 450, 1)]
    return frames, tracks


@pytest.mark.parametrize("kw", [dict(filter_freqs=True), dict(filter_below=1000), dict(filter_below=500),
                                dict(filter_freqs=True, filter_below=1000)])
def test_track_windows_filtered(scene, kw):
    frames, tracks = scene
    got = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(4), **kw)
    ref = load_samples_restated(frames, tracks, kw.get("filter_freqs", False), kw.get("filter_below"),
                                np.random.RandomState(4))
    plain = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(4))
    assert [len(g) for g in got] == [3, 1, 1, 0, 1, 1]
    for k, (g, r, p) in enumerate(zip(got, ref, plain)):
        assert g.dtype == np.float32 and g.shape == r.shape and np.array_equal(g, r), k
        filtered = kw.get("filter_freqs") or tracks[k].freq_end < kw["filter_below"]
        assert len(g) == 0 or np.array_equal(g, p) != bool(filtered), k


def test_track_windows_defaults_unchanged(scene):
    frames, tracks = scene
    a = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(1))
    b = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(1), filter_freqs=False, filter_below=None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the state carries from window to window: window 1 of the long track is not the filter restarted at 3 s
    w = predict.track_windows(frames, SR, tracks[:1], rng=np.random.RandomState(1), filter_freqs=True)[0]
    sos = predict.butter_bandpass(1000, 3000, SR)
    whole = sosfilt(sos, frames[2 * SR:int(7.5 * SR)]).astype(np.float32)
    assert np.array_equal(w[1], whole[SR:SR + N])
    assert not np.array_equal(w[1], sosfilt(sos, frames[3 * SR:6 * SR]).astype(np.float32))


def test_window_plan_default_return_unchanged(scene):
    frames, tracks = scene
    r = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(2))
    assert isinstance(r, tuple) and len(r) == 2
    plan, counts, segs = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(2),
                                                   segments=True)
    assert np.array_equal(plan, r[0]) and counts == r[1]
    assert segs.dtype == np.int64 and segs.shape == (6, 2)
    assert segs[0].tolist() == [2 * SR, int(7.5 * SR) - 2 * SR] and segs[2].tolist() == [len(frames) - N, N]
    assert segs[3].tolist() == [0, 0] and segs[4].tolist() == [0, N] and segs[5].tolist() == [7 * SR, N]
    assert segs[1, 1] == N and segs[1, 0] + N // 2 == (int(5.0 * SR) + int(6.2 * SR)) // 2  # centred


@pytest.mark.parametrize("kw", [dict(filter_freqs=True), dict(filter_below=1000)])
def test_rebased_plan_on_host_filtered_segments(scene, kw):
    """sos_segment_plan applied with numpy -- every segment filtered with
    sosfilt into the packed buffer, the rebased plan cut from it --
    reproduces track_windows(filter...) bit for bit with the same RandomState."""
    frames, tracks = scene
    wins = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(7), **kw)
    plan, counts, segs = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(7),
                                                   segments=True)
    seg, sos, plan2 = predict.sos_segment_plan(tracks, segs, plan, counts, SR, **kw)
    assert seg.dtype == np.int64 and seg.shape == (5, 3) and sos.dtype == np.float64 and sos.shape == (5, 2, 6)
    assert (seg[:, 2] % 4 == 0).all() and seg[0, 2] == 0
    assert np.array_equal(seg[:, :2], segs[[0, 1, 2, 4, 5]])
    total = int((seg[:, 1] + seg[:, 2]).max() + 3) & ~3
    predict.check_sos_segments(seg, sos, len(frames), total)
    ident = [1, 0, 0, 1, 0, 0]
    if "filter_freqs" in kw:
        assert sos[1, 1].tolist() == ident and sos[3, 1].tolist() == ident  # low-pass, high-pass: one section
        assert np.array_equal(sos[0], butter(2, [1000 / 24000, 3000 / 24000], btype="bandpass", output="sos"))
    else:
        assert [s.tolist() == [ident, ident] for s in sos] == [True, False, True, True, False]
    buf = np.full(total, np.nan, np.float32)
    for (src, ln, dst), f in zip(seg.tolist(), sos):
        buf[dst:dst + ln] = sosfilt(f, frames[src:src + ln]).astype(np.float32)
    got = np.zeros((len(plan2), N), np.float32)
    for w, (src, count, pad) in enumerate(plan2.tolist()):
        got[w, pad:pad + count] = buf[src:src + count]
    assert np.array_equal(plan2[:, 1:], plan[:, 1:]) and len(plan2) == 7
    assert np.array_equal(got, np.concatenate(wins))
    assert np.array_equal(plan, predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(7))[0])


def test_check_sos_segments_rejects_bad_rows():
    good_seg = np.array([[0, 100, 0], [50, 30, 100], [999, 1, 132], [10, 0, 50]], np.int64)
    good_sos = np.tile(predict.SOS_IDENTITY, (4, 1, 1))
    seg, sos = predict.check_sos_segments(good_seg.tolist(), good_sos.tolist(), 1000, 136)
    assert seg.dtype == np.int64 and sos.dtype == np.float64 and seg.flags.c_contiguous and sos.flags.c_contiguous
    for row in [(0, 2, 130), (998, 2, 133), (0, 0, 136), (1000, 0, 0)]:  # touching its neighbours / the ends
        ok = good_seg.copy()
        ok[3] = row
        predict.check_sos_segments(ok, good_sos, 1000, 136)
    big = np.iinfo(np.int64).max
    for row in [(-1, 5, 0), (0, -1, 0), (996, 5, 0), (1001, 0, 0), (0, 5, -4), (0, 5, 132), (0, 5, 137),
                (big, 5, 0), (5, big, 0), (0, 5, big), (big, big, big),  # sums that would wrap
                (0, 5, 98), (0, 60, 96), (0, 5, 110)]:  # overlap segment 0's end, segment 1's start, inside 1
        bad = good_seg.copy()
        bad[3] = row
        with pytest.raises(ValueError):
            predict.check_sos_segments(bad, good_sos, 1000, 136)
    for idx, v in [((1, 0, 3), 2.0), ((2, 1, 3), 0.0), ((0, 0, 1), np.nan), ((3, 1, 5), np.inf)]:
        bad = good_sos.copy()
        bad[idx] = v
        with pytest.raises(ValueError):
            predict.check_sos_segments(good_seg, bad, 1000, 136)
    for seg_, sos_ in [(good_seg[:, :2], good_sos), (good_seg, good_sos[:3]), (good_seg, good_sos[:, :1]),
                       (good_seg.ravel(), good_sos)]:
        with pytest.raises(ValueError):
            predict.check_sos_segments(seg_, sos_, 1000, 136)
    seg, sos = predict.check_sos_segments(np.zeros((0, 3)), np.zeros((0, 2, 6)), 1000, 0)
    assert seg.shape == (0, 3) and sos.shape == (0, 2, 6)
