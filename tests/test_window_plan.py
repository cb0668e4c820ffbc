"""predict.track_window_plan: the windows of predict.track_windows (reference
predict_utils.load_samples :59-150) as a table of (src, count, pad) rows, and
predict.check_window_plan, the host-side validation of such a table.  Host
only: no kernel runs here."""
import numpy as np
import pytest

from conftest import GOLDEN

import identifytracks as it
import predict

SR = 48000
N = 3 * SR


def apply_plan(frames, plan, n):
    """The windows a plan describes, materialised with numpy."""
    out = np.zeros((len(plan), n), np.float32)
    for w, (src, count, pad) in enumerate(plan):
        out[w, pad:pad + count] = frames[src:src + count]
    return out


def _tracks(rows):
    return [it.Signal(float(a), float(b), float(c), float(d), 1) for a, b, c, d in rows]


def test_plan_matches_reference_load_samples_rows():
    """Every ls_* case of tracks_golden.npz (made by the reference's
    load_samples over a ramp recording): the plan's rows as (track, pad, src,
    count) are the fixture's, exactly."""
    z = np.load(GOLDEN / "tracks_golden.npz")
    meta, rows, case = z["ls_meta"], z["ls_rows"], z["ls_case"]
    n_rows = n_partial = 0
    for k, (secs, pad, seed, stride, ntr) in enumerate(meta):
        plan, counts = predict.track_window_plan(SR * int(secs), SR, _tracks(z[f"ls_tracks{k}"]), stride=int(stride),
                                                 pad_short_tracks=bool(pad), rng=np.random.RandomState(int(seed)))
        assert plan.dtype == np.int64 and plan.shape == (sum(counts), 3) and len(counts) == int(ntr)
        track = np.repeat(np.arange(len(counts)), counts)
        got = [(int(t), int(p), int(s), int(c)) for t, (s, c, p) in zip(track, plan)]
        ref = [tuple(int(v) for v in r) for r, c in zip(rows, case) if c == k]
        assert got == ref, (k, got, ref)
        predict.check_window_plan(plan, SR * int(secs), N)
        n_rows += len(plan)
        n_partial += int((plan[:, 1] < N).sum())
    assert n_rows == len(rows) and n_partial > 0  # the fixture has padded windows


TRACKS = [(0.2, 0.9, 3000, 4000),  # short, near the start: centring clips at 0
          (4.0, 5.5, 500, 900),  # short, centred
          (6.0, 13.4, 2000, 5000),  # long: full windows and a partial last one
          (7.0, 8.0, 20, 60),  # below fmin: not classified
          (18.3, 19.9, 1000, 9000),  # short, at the end: centring clips at the end
          (15.0, 18.0, 12000, 13000),  # above fmax
          (10.0, 13.0, 100, 11000)]  # exactly one window long


@pytest.mark.parametrize("pad_short,stride", [(False, 1), (True, 1), (False, 2), (True, 2)])
def test_applied_plan_equals_track_windows(pad_short, stride):
    """Applying the plan to a random recording == track_windows with the same
    RandomState seed, bit for bit, window for window."""
    frames = np.random.default_rng(5).standard_normal(20 * SR).astype(np.float32)
    tracks = _tracks(TRACKS)
    wins = predict.track_windows(frames, SR, tracks, stride=stride, pad_short_tracks=pad_short,
                                 rng=np.random.RandomState(7))
    plan, counts = predict.track_window_plan(len(frames), SR, tracks, stride=stride, pad_short_tracks=pad_short,
                                             rng=np.random.RandomState(7))
    assert counts == [len(w) for w in wins]
    assert counts[3] == counts[5] == 0 and min(c for i, c in enumerate(counts) if i not in (3, 5)) >= 1
    predict.check_window_plan(plan, len(frames), N)
    assert np.array_equal(apply_plan(frames, plan, N), np.concatenate(wins))
    if pad_short:
        assert (plan[:, 1] < N).any() and (plan[:, 2] > 0).any()  # partial windows at random offsets


def test_recording_shorter_than_a_window():
    """A 2 s recording: one partial window, the whole recording, at the offset
    track_windows draws."""
    frames = np.random.default_rng(9).standard_normal(2 * SR).astype(np.float32)
    tracks = _tracks([(0.5, 1.5, 1000, 2000)])
    plan, counts = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(3))
    assert counts == [1] and plan.shape == (1, 3)
    src, count, pad = (int(v) for v in plan[0])
    assert (src, count) == (0, 2 * SR)
    assert pad == np.random.RandomState(3).randint(0, N - count)
    wins = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(3))
    assert np.array_equal(apply_plan(frames, plan, N), wins[0])


def test_no_tracks_gives_an_empty_plan():
    plan, counts = predict.track_window_plan(10 * SR, SR, [])
    assert plan.shape == (0, 3) and plan.dtype == np.int64 and counts == []
    predict.check_window_plan(plan, 10 * SR, N)


@pytest.mark.parametrize("row", [(-1, 10, 0),  # negative src
                                 (95, 10, 0),  # src + count > rec_len
                                 (0, 40, 20),  # pad + count > n
                                 (0, -1, 0),  # negative count
                                 (0, 10, -1)],  # negative pad
                         ids=["src<0", "src+count>len", "pad+count>n", "count<0", "pad<0"])
def test_check_window_plan_rejects(row):
    good = [(0, 50, 0), (90, 10, 40), (100, 0, 50), (0, 0, 0)]
    out = predict.check_window_plan(good, 100, 50)
    assert out.dtype == np.int64 and out.flags.c_contiguous and out.tolist() == [list(r) for r in good]
    with pytest.raises(ValueError):
        predict.check_window_plan(good + [row], 100, 50)
    with pytest.raises(ValueError):
        predict.check_window_plan(np.zeros((4, 2), np.int64), 100, 50)
