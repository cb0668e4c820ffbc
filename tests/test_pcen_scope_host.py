"""The host side of --pcen-scope: predict.pcen_segments (which windows share
PCEN's min / max), acfe.frontend.check_pcen_segments (the table's validation),
predict.segment_launches (launches cut at segment boundaries) and the CLI's
argument check."""
import numpy as np
import pytest

COUNTS = [0, 1, 33, 64, 0, 3]
SIZES = [1, 32, 1, 32, 32, 3]  # Keras predict batches of 32, track after track


def test_pcen_segments():
    import predict

    seg = predict.pcen_segments(COUNTS, "track", keras_batch=32)
    assert seg.dtype == np.int32 and seg.ndim == 1
    assert seg[0] == 0 and seg[-1] == sum(COUNTS)
    assert np.diff(seg).tolist() == SIZES
    assert np.array_equal(seg, predict.pcen_segments(COUNTS, "track"))  # 32 is the default
    assert np.diff(predict.pcen_segments(COUNTS, "track", keras_batch=40)).tolist() == [1, 33, 40, 24, 3]
    win = predict.pcen_segments(COUNTS, "window")
    assert win.dtype == np.int32 and np.array_equal(win, np.arange(sum(COUNTS) + 1))
    assert predict.pcen_segments(COUNTS, "batch") is None
    assert np.array_equal(predict.pcen_segments([], "track"), [0])
    with pytest.raises(ValueError):
        predict.pcen_segments(COUNTS, "recording")


def test_check_pcen_segments():
    from acfe.frontend import check_pcen_segments

    seg = check_pcen_segments([0, 2, 2, 3, 7], 7)
    assert seg.dtype == np.int32 and seg.flags["C_CONTIGUOUS"] and seg.tolist() == [0, 2, 2, 3, 7]
    assert check_pcen_segments(np.array([0, 7], np.int64), 7).dtype == np.int32
    for bad in ([1, 3, 7],  # wrong start
                [0, 4, 3, 7],  # decreasing
                [0, 3, 6],  # wrong end
                [0, 3, 8],
                [[0, 3], [3, 7]],  # 2-D
                [7],  # length 1
                []):
        with pytest.raises(ValueError):
            check_pcen_segments(bad, 7)
    with pytest.raises(ValueError):
        check_pcen_segments([0.0, 7.0], 7)


@pytest.mark.parametrize("batch_size", [32, 40, 1024])
def test_segment_launches(batch_size):
    import predict

    seg = predict.pcen_segments(COUNTS, "track", keras_batch=32)
    n = int(seg[-1])
    launches = predict.segment_launches(n, batch_size, seg)
    bounds = set(seg.tolist())
    at, pieces = 0, []
    for a, b, table in launches:
        assert a == at and a < b <= n  # in order, nothing skipped or repeated
        assert b - a <= batch_size
        assert a in bounds and b in bounds  # whole segments only
        assert table.dtype == np.int32 and table[0] == 0 and table[-1] == b - a
        assert (np.diff(table) > 0).all()
        assert set((table + a).tolist()) <= bounds
        pieces += np.diff(table).tolist()
        at = b
    assert at == n and pieces == SIZES  # every segment once, unsplit, in order
    # greedy: the segment that follows a launch would not have fitted into it
    for (a, b, _), (_, b2, t2) in zip(launches, launches[1:]):
        assert b - a + t2[1] > batch_size
    if batch_size == 32:
        assert [(a, b) for a, b, _ in launches] == [(0, 1), (1, 33), (33, 34), (34, 66), (66, 98), (98, 101)]
    if batch_size == 40:
        assert [(a, b) for a, b, _ in launches] == [(0, 34), (34, 66), (66, 101)]
    if batch_size == 1024:
        assert len(launches) == 1 and np.array_equal(launches[0][2], seg)


def test_segment_launches_edges():
    import predict

    seg = predict.pcen_segments(COUNTS, "track", keras_batch=32)
    with pytest.raises(ValueError):
        predict.segment_launches(int(seg[-1]), 16, seg)  # a segment of 32 cannot be split
    with pytest.raises(ValueError):
        predict.segment_launches(int(seg[-1]) + 1, 1024, seg)  # the table does not cover the windows
    # without a table: plain chunks, as before
    assert predict.segment_launches(70, 32) == [(0, 32, None), (32, 64, None), (64, 70, None)]
    assert predict.segment_launches(0, 32) == []
    # empty segments vanish from a launch's table
    (a, b, table), = predict.segment_launches(7, 1024, [0, 2, 2, 3, 7])
    assert (a, b) == (0, 7) and table.tolist() == [0, 2, 3, 7]
    # one window per segment
    launches = predict.segment_launches(5, 2, predict.pcen_segments([5], "window"))
    assert [(a, b, t.tolist()) for a, b, t in launches] == [(0, 2, [0, 1, 2]), (2, 4, [0, 1, 2]), (4, 5, [0, 1])]


def test_cli_rejects_track_scope_without_tracks(capsys):
    import predict

    with pytest.raises(SystemExit) as e:
        predict.main(["no_such_checkpoint", "--file", "x.wav", "--mode", "windows", "--pcen-scope", "track"])
    assert e.value.code == 2
    assert "--pcen-scope track" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        predict.main(["no_such_checkpoint", "--file", "x.wav", "--pcen-scope", "recording"])
    assert e.value.code == 2
