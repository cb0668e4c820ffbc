"""Host pieces the device track detector (acfe/tracks.py) shares with
identifytracks.signal_noise: the stats -> Signal filter factored out of
signal_noise, and the union of horizontal runs into 8-connected components
(identifytracks.boxes_from_runs), which replaces scipy.ndimage.label on the
device path.  No GPU involved: the runs are extracted with numpy here."""
import numpy as np
import pytest
from scipy.ndimage import find_objects, label

import identifytracks as it

SR = 48000
CHIRPS = [(2.0, 1.0, 3000, 4000), (8.0, 0.6, 6000, 5000), (14.0, 2.5, 1500, 2500)]


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


def label_stats(m):
    """signal_noise's component stats: scipy label (8-connectivity) in label
    order, then the stable sort by left."""
    lab, n = label(m, structure=np.ones((3, 3), np.uint8))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    stats = []
    for k, sl in enumerate(find_objects(lab), start=1):
        top, left = sl[0].start, sl[1].start
        stats.append((left, top, sl[1].stop - left, sl[0].stop - top, int(area[k])))
    stats.sort(key=lambda s: s[0])
    return stats


def numpy_runs(m):
    """(row, first col, last col) of every horizontal run of a 0 / 1 map."""
    p = np.pad(m.astype(np.int8), ((0, 0), (1, 1)))
    d = np.diff(p, axis=1)
    r0, c0 = np.nonzero(d == 1)
    r1, c1 = np.nonzero(d == -1)
    assert np.array_equal(r0, r1)
    return np.stack([r0, c0, c1 - 1], 1)


def test_signal_filter_helper_keeps_signal_noise_output():
    """signal_noise through signals_from_stats == the filter as it stood
    inline (size thresholds, 281 / sr scaling, bin frequencies), on the 20 s
    chirp recording of test_identifytracks."""
    x = _recording(CHIRPS)
    signals, spec = it.signal_noise(x, SR)
    freqs = np.fft.rfftfreq(2048, 1.0 / SR)
    height = next(i + 1 for i, f in enumerate(freqs) if f > 100)
    width = int(0.25 * SR / 281)
    assert (height, width) == (6, 42) and it.box_geometry(SR)[1:] == (6, 42)
    s = spec / np.amax(spec)
    m = ((s > 2 * np.median(s, axis=0)[None, :]) & (s > 3 * np.median(s, axis=1)[:, None])).astype(np.uint8)
    m = it._box_min(it._box_max(it._box_max(it._box_min(m, 4, 4), 4, 4), height, width), height // 10, width)
    want = []
    for left, top, w, h, area in label_stats(m):
        if w > 0.65 * width and h > height - height // 10:
            want.append((left * 281 / SR, (left + w) * 281 / SR, freqs[top], freqs[min(len(freqs) - 1, top + h)], area))
    got = [(g.start, g.end, g.freq_start, g.freq_end, g.mass) for g in signals]
    assert len(got) >= 3 and got == want
    # explicit thresholds still override the defaults
    loose, _ = it.signal_noise(x, SR, min_width=0, min_height=0, spectogram=spec)
    assert len(loose) == len(label_stats(m))


@pytest.mark.parametrize("shape,density,seed", [((23, 31), 0.3, 0), ((64, 200), 0.05, 1), ((5, 200), 0.5, 2),
                                                ((120, 130), 0.02, 3)])
def test_run_union_matches_scipy_label(shape, density, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random(shape) < density).astype(np.uint8)
    for mm in (m, it._box_max(m, 3, 5)):
        runs = numpy_runs(mm)
        assert it.boxes_from_runs(runs) == label_stats(mm)
        assert it.boxes_from_runs(runs[rng.permutation(len(runs))]) == label_stats(mm)  # any run order


def test_run_union_edge_cases():
    assert it.boxes_from_runs(np.zeros((0, 3), np.int32)) == []
    full = np.ones((7, 9), np.uint8)
    assert it.boxes_from_runs(numpy_runs(full)) == [(0, 0, 9, 7, 63)]
    # cells that touch only diagonally are one component; a gap of one cell is two
    diag = np.eye(6, dtype=np.uint8)
    assert it.boxes_from_runs(numpy_runs(diag)) == [(0, 0, 6, 6, 6)]
    anti = diag[:, ::-1].copy()
    assert it.boxes_from_runs(numpy_runs(anti)) == [(0, 0, 6, 6, 6)]
    gap = np.zeros((3, 8), np.uint8)
    gap[0, 0:3] = gap[1, 4:6] = gap[2, 7] = 1  # 3 | gap | 2 | gap | 1: the first two do not touch
    assert it.boxes_from_runs(numpy_runs(gap)) == label_stats(gap)
    # ties in `left` keep the raster order of the components' first cells
    tie = np.zeros((9, 4), np.uint8)
    tie[7, 0] = tie[1, 0:2] = tie[4, 0] = 1
    assert it.boxes_from_runs(numpy_runs(tie)) == label_stats(tie) == [(0, 1, 2, 1, 2), (0, 4, 1, 1, 1), (0, 7, 1, 1, 1)]
    # a U whose arms join only at the bottom: one component, two roots merged late
    u = np.zeros((5, 7), np.uint8)
    u[:, 0] = u[:, 6] = u[4, :] = 1
    assert it.boxes_from_runs(numpy_runs(u)) == [(0, 0, 7, 5, 15)]
