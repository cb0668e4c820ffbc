"""Host side of --use-weighting / --label-smoothing: tfdataset.get_weighting
(reference tfdataset.py:1737-1758) on a count vector, AudioDataset.label_counts
(the examples per label, from the same decode pass as count()) and the two
options of audiomodel.parse_args (reference audiomodel.py:2299)."""
import numpy as np

import tfrecord as tfr

N = 144000
LABELS = ["bird", "noise", "human"]


def _weighting_f32(dist):
    """The reference's arithmetic, written out in float32."""
    dist = [np.float32(d) for d in dist]
    total = np.float32(0)
    for d in dist:
        total = np.float32(total + d)
    nz = np.float32(sum(1 for d in dist if d > 0))
    out = []
    for d in dist:
        if d == 0:
            out.append(np.float32(0))
            continue
        w = np.float32(np.float32(np.float32(1) / d) * np.float32(total / nz))
        out.append(min(max(w, np.float32(0.25)), np.float32(4)))
    return np.array(out, np.float32)


def test_get_weighting_values():
    import tfdataset

    dist = [1000, 10, 0, 100, 3]
    w = tfdataset.get_weighting(dist)
    ref = _weighting_f32(dist)
    assert w.dtype == np.float32 and w.shape == (5,)
    assert np.array_equal(w, ref), (w, ref)
    # total 1113 over 4 labels with examples = 278.25 per label
    assert abs(w[0] - 0.27825) < 1e-6           # uncapped: 278.25 / 1000, just above the floor
    assert w[1] == 4 and w[4] == 4              # 27.8 and 92.75: capped at 4
    assert w[2] == 0                            # no examples
    assert abs(w[3] - 2.7825) < 1e-5            # uncapped
    assert np.array_equal(tfdataset.get_weighting(np.array([7, 0, 7], np.int64)), np.array([1, 0, 1], np.float32))


def test_get_weighting_floor():
    """A label that far outnumbers the rest is held at 0.25 (with the counts
    above the largest label's raw weight is 0.278, which the floor leaves)."""
    import tfdataset

    dist = [1000, 1, 0, 1, 1, 1]  # 1004 over 5 labels with examples: 200.8 / 1000 = 0.2008 -> 0.25
    w = tfdataset.get_weighting(dist)
    assert np.array_equal(w, _weighting_f32(dist))
    assert w[0] == np.float32(0.25) and w[2] == 0 and (w[[1, 3, 4, 5]] == 4).all()


def test_get_weighting_all_zero():
    import tfdataset

    w = tfdataset.get_weighting([0, 0, 0])
    assert w.dtype == np.float32 and np.array_equal(w, np.zeros(3, np.float32))


def _write(path, labs, k0):
    with tfr.TFRecordWriter(path) as w:
        for k, lab in enumerate(labs, k0):
            w.write(tfr.audio_example(np.full(N, 0.001 * (k + 1), np.float32), f"r{k}", k, lab, lab))


def test_label_counts(tmp_path):
    import tfdataset

    d = tmp_path / "train"
    d.mkdir()
    # 10 records over 3 labels and one with a label the dataset does not keep
    a = ["bird", "bird", "noise", "bird", "human", "other"]
    b = ["noise", "bird", "bird", "human", "bird"]
    _write(d / "00000.tfrecord", a, 0)
    _write(d / "00001.tfrecord", b, len(a))
    want = np.array([sum(x == lab for x in a + b) for lab in LABELS], np.int64)
    assert want.tolist() == [6, 2, 2]
    files = tfdataset._files(d)
    ds = tfdataset.AudioDataset(files, LABELS, batch_size=4, device="cpu", threads=2)
    c = ds.label_counts()
    assert c.dtype == np.int64 and c.shape == (3,)
    assert np.array_equal(c, want)
    assert ds.count() == int(want.sum()) == 10
    # the two results come from one decode pass
    calls = []
    ds2 = tfdataset.AudioDataset(files, LABELS, batch_size=4, device="cpu", threads=2)
    orig = ds2._count_file
    ds2._count_file = lambda i, p: (calls.append(p), orig(i, p))[1]
    assert ds2.count() == 10 and np.array_equal(ds2.label_counts(), want)
    assert sorted(calls) == sorted(files)
    # a caller's epoch_size: the pass runs on first use of label_counts
    ds3 = tfdataset.AudioDataset(files, LABELS, batch_size=4, device="cpu", threads=2, epoch_size=10)
    assert ds3.count() == 10 and ds3._label_counts is None
    assert np.array_equal(ds3.label_counts(), want)
    # record shards of two ranks add up to the whole
    parts = [tfdataset.AudioDataset(files, LABELS, batch_size=4, device="cpu", threads=2,
                                    record_shard=(r, 2)) for r in range(2)]
    pc = [p.label_counts() for p in parts]
    assert np.array_equal(pc[0] + pc[1], want)
    assert [p.count() for p in parts] == [int(x.sum()) for x in pc]
    assert all(x.sum() > 0 for x in pc)


def test_cli_options():
    import audiomodel

    a = audiomodel.parse_args(["run", "-d", "data"])
    assert not a.use_weighting and a.label_smoothing == 0
    a = audiomodel.parse_args(["run", "-d", "data", "--use-weighting", "--label-smoothing", "0.1"])
    assert a.use_weighting == 1 and a.label_smoothing == 0.1
