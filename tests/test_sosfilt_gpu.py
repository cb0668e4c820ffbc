"""acfe_sosfilt_segments (csrc/sosfilt.hip): scipy.signal.sosfilt of segments
of a device recording, each with its own Butterworth filter, as a float64
chunked scan stored float32 -- against scipy in float64 cast to float32; and
predict_tracks(filter_freqs=True) on the device against the host filter.

The kernel's chunk is L = 32 samples per lane and its workgroup tile 256
chunks = 8192 samples; the lengths below sit on either side of both.

Bound, per segment: |got - float32(ref)| <= 2^-22 max|ref|.  Two float64
values much closer than a float32 ulp round at most one ulp apart, one ulp is
at most 2^-23 max|ref|, and the bound is twice that."""
import json

import numpy as np
import pytest
import torch
from scipy.signal import butter, sosfilt

pytestmark = pytest.mark.gpu

SR = 48000
L, TILE = 32, 8192
GUARD = 12345.0
IDENT = np.array([[1.0, 0, 0, 1, 0, 0]] * 2)


@pytest.fixture(scope="module")
def fe(cuda):
    from acfe import frontend

    return frontend


def sos2(sos):
    out = IDENT.copy()
    if sos is not None:
        out[:len(sos)] = sos
    return out


FILTERS = {"band": butter(2, [1000 / 24000, 3000 / 24000], btype="bandpass", output="sos"),  # 2 sections
           "low": butter(2, 800 / 24000, btype="lowpass", output="sos"),  # 1 section
           "high": butter(2, 2000 / 24000, btype="highpass", output="sos"),  # 1 section
           "narrow": butter(2, [100 / 24000, 110 / 24000], btype="bandpass", output="sos"),  # pole radius 0.9998
           "sub": butter(2, [20 / 24000, 24 / 24000], btype="bandpass", output="sos"),
           "ident": None}


def within_bound(got, ref64):
    ref = ref64.astype(np.float32)
    if len(ref) == 0:
        return True
    return bool((np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2.0 ** -22 * np.abs(ref64).max()).all())


def run(fe, cuda, rec, dev, rows, filters, gap=0):
    """sosfilt_segments of the (src, len) rows into a guarded buffer, dst
    rounded up to 4 floats (with gap: plus 1, 2, 3, 0, ... floats, so that
    dst takes every alignment); checks the guards in front, in the gaps
    and behind, every segment against scipy, identity segments bit for bit."""
    seg, at = [], 0
    for i, (src, ln) in enumerate(rows):
        seg.append((src, ln, at))
        at = ((at + ln + 3) & ~3) + gap * (i + 1) % 4
    total = (at + 3) & ~3
    buf = torch.full((total + 8,), GUARD, dtype=torch.float32, device=cuda)
    sos = np.stack([sos2(FILTERS[f]) for f in filters]) if rows else np.zeros((0, 2, 6))
    out = fe.sosfilt_segments(dev, np.array(seg, np.int64).reshape(-1, 3), sos, out=buf[4:4 + total])
    assert out.numel() == total and (total == 0 or out.data_ptr() == buf[4:].data_ptr())
    got = buf.cpu().numpy()
    covered = np.zeros(total + 8, bool)
    for (src, ln, dst), f in zip(seg, filters):
        g = got[4 + dst:4 + dst + ln]
        covered[4 + dst:4 + dst + ln] = True
        if FILTERS[f] is None:
            assert np.array_equal(g.view(np.uint32), rec[src:src + ln].view(np.uint32)), (src, ln, f)
        elif ln:  # scipy's sosfilt does not take an empty signal
            assert within_bound(g, sosfilt(FILTERS[f], rec[src:src + ln].astype(np.float64))), (src, ln, f)
    assert (got[~covered] == GUARD).all()
    return got[4:4 + total], seg


LENGTHS = [0, 1, L - 1, L, L + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]


@pytest.mark.parametrize("kind,rec_off", [("noise", 0), ("noise", 1), ("impulse0", 0), ("impulse_chunk_end", 2)])
def test_lengths_alignments_filters(fe, cuda, kind, rec_off):
    """Every length at every filter kind in one call per filter rotation; src
    at 0, 1, 2, 3 mod 4 (on top of a recording whose base is rec_off floats
    off a 16-B line).  impulse0: everything after the first chunk is carried
    state only; impulse_chunk_end: the impulse is a chunk's last sample."""
    rng = np.random.default_rng(11)
    parts, rows, pos = [], [], 0
    for i, ln in enumerate(LENGTHS):
        lead = (i % 4 - pos) % 4 + 4  # src = pos + lead is i mod 4
        if kind == "noise":
            x = rng.standard_normal(lead + ln).astype(np.float32)
        else:
            x = np.zeros(lead + ln, np.float32)
            at = 0 if kind == "impulse0" else min(L - 1, ln - 1)
            if ln:
                x[lead + at] = 1.0
        parts.append(x)
        rows.append((pos + lead, ln))
        pos += lead + ln
    parts.append(rng.standard_normal(7).astype(np.float32))
    rec = np.concatenate(parts)
    assert [s % 4 for s, _ in rows] == [i % 4 for i in range(len(rows))]
    base = torch.from_numpy(np.concatenate([np.zeros(rec_off, np.float32), rec])).to(cuda)
    dev = base[rec_off:]
    names = list(FILTERS)
    for rot in range(len(names)):
        run(fe, cuda, rec, dev, rows, [names[(i + rot) % len(names)] for i in range(len(rows))])
    run(fe, cuda, rec, dev, rows[-1:], ["band"])  # one segment
    run(fe, cuda, rec, dev, rows[:1], ["band"])  # only an empty one
    run(fe, cuda, rec, dev, [], [])  # n_seg 0
    # dst % 4 = 0, 1, 2, 3
    run(fe, cuda, rec, dev, rows[2:8], ["narrow", "low", "ident", "high", "band", "ident"], gap=1)


def test_narrow_band_long_segment(fe, cuda):
    """100-110 Hz over 480 000 samples (59 tiles: the tile carry of one
    segment), with a 20-24 Hz neighbour and overlapping sources."""
    rec = np.random.default_rng(12).standard_normal(480000 + 3).astype(np.float32)
    dev = torch.from_numpy(rec).to(cuda)
    run(fe, cuda, rec, dev, [(3, 480000), (1, 200001), (100000, 150000)], ["narrow", "sub", "band"])


def test_abi_arguments_and_clamping(fe, cuda):
    from acfe import _lib

    f, wsz = _lib.lib.acfe_sosfilt_segments, _lib.lib.acfe_sosfilt_workspace
    assert wsz(-1, 1) == _lib.E_INVAL and wsz(10, -1) == _lib.E_INVAL and wsz(0, 0) >= 0
    assert wsz(1 << 20, 3) >= (1 << 20)
    rec = np.random.default_rng(13).standard_normal(1000).astype(np.float32)
    dev = torch.from_numpy(rec).to(cuda)
    out_len = 400
    rows = [(990, 50, 0),  # runs 40 samples past rec_len: those read as zero
            (-5, 20, 52),  # starts 5 samples in front of the recording
            (0, 100, out_len - 20),  # dst + len past out_len: only 20 samples are written
            (2 ** 62, 8, 80), (0, -3, 90), (0, 8, -40), (0, 8, out_len + 7), (10, 2 ** 62, 2 ** 62)]
    sos = np.stack([sos2(FILTERS["band"])] * len(rows))
    dseg = torch.tensor(rows, dtype=torch.int64, device=cuda)
    dsos = torch.from_numpy(sos).to(cuda)
    ws = torch.empty(wsz(out_len, len(rows)), dtype=torch.uint8, device=cuda)
    buf = torch.full((out_len + 8,), GUARD, dtype=torch.float32, device=cuda)
    o = buf[4:]
    args = (dev.data_ptr(), len(rec), dseg.data_ptr(), dsos.data_ptr(), len(rows), o.data_ptr(), out_len,
            ws.data_ptr(), None)
    for i, bad in [(0, None), (2, None), (3, None), (5, None), (7, None), (1, -1), (4, -1), (6, -1)]:
        a = list(args)
        a[i] = bad
        assert f(*a) == _lib.E_INVAL
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all()  # nothing was launched
    assert f(dev.data_ptr(), len(rec), None, None, 0, o.data_ptr(), out_len, None, None) == 0  # n_seg 0
    assert f(*args) == 0
    got = buf.cpu().numpy()
    assert (got[:4] == GUARD).all() and (got[4 + out_len:] == GUARD).all()
    band = FILTERS["band"]
    x = rec.astype(np.float64)
    assert within_bound(got[4:54], sosfilt(band, np.concatenate([x[990:], np.zeros(40)])))
    assert within_bound(got[4 + 52:4 + 72], sosfilt(band, np.concatenate([np.zeros(5), x[:15]])))
    assert within_bound(got[4 + 380:4 + 400], sosfilt(band, x[:20]))
    # (2^62, 8, 80): eight zeros filtered; the other rows clamp to nothing (len <= 0 or dst outside out)
    assert (got[4 + 80:4 + 88] == 0).all()
    rest = np.ones(out_len + 8, bool)
    for a, b in [(0, 50), (52, 72), (80, 88), (380, 400)]:
        rest[4 + a:4 + b] = False
    assert (got[rest] == GUARD).all()


def test_binding_rejects_bad_arguments(fe, cuda):
    rec = torch.zeros(1000, dtype=torch.float32, device=cuda)
    one = IDENT[None]
    with pytest.raises(TypeError):
        fe.sosfilt_segments(rec.double(), [(0, 4, 0)], one)
    with pytest.raises((TypeError, ValueError)):
        fe.sosfilt_segments(rec[::2], [(0, 4, 0)], one)
    with pytest.raises(TypeError):
        fe.sosfilt_segments(rec.view(10, 100), [(0, 4, 0)], one)
    for seg in ([(998, 4, 0)], [(-1, 4, 0)], [(0, -4, 0)], [(0, 4, -4)], [(0, 4, 0, 0)]):
        with pytest.raises(ValueError):
            fe.sosfilt_segments(rec, seg, one)
    with pytest.raises(ValueError):  # overlapping destinations
        fe.sosfilt_segments(rec, [(0, 8, 0), (0, 8, 4)], np.stack([IDENT, IDENT]))
    with pytest.raises(ValueError):  # does not fit the given buffer
        fe.sosfilt_segments(rec, [(0, 8, 0)], one, out=torch.empty(4, dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        fe.sosfilt_segments(rec, [(0, 8, 0)], one, out=torch.empty(8, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):  # a0 != 1
        fe.sosfilt_segments(rec, [(0, 8, 0)], 2 * one)
    with pytest.raises(ValueError):
        fe.sosfilt_segments(rec, [(0, 8, 0)], IDENT[None, :1])
    with pytest.raises(ValueError):
        fe.sosfilt_segments(rec, [(0, 8, 0)], one, out=rec.cpu())  # out must be on the device
    assert fe.sosfilt_segments(rec, np.zeros((0, 3), np.int64), np.zeros((0, 2, 6))).numel() == 0
    assert fe.sosfilt_segments(rec, [(4, 9, 4)], one).shape == (16,)


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


def test_predict_tracks_filter_freqs(tmp_path, cuda, capsys, fe, monkeypatch):
    """predict_tracks(filter_freqs=True): windows="device" (sosfilt_segments +
    the window kernel on the rebased plan) against windows="host" (scipy) on a
    10 s recording of three chirps in different bands.  The two filters agree
    within the bound; from the same filtered buffer the window stage is exact.
    The probabilities of the two paths are not compared: a one-ulp input
    difference through a bf16 model has no derivable bound (the observed
    difference is in profiles/predict_filter_device.md)."""
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
    n_windows = []
    for name in ("predict_clips", "predict_plan"):
        def spy(*a, _f=getattr(p, name), **k):
            r = _f(*a, **k)
            n_windows.append(len(r))
            return r
        monkeypatch.setattr(p, name, spy)

    def tracks_of(**kw):
        it.Signal._next_id = 0  # the ids in get_meta count up over the process: the same ones for every call
        tracks, end = p.predict_tracks(rec, rng=np.random.RandomState(0), detector="gpu", **kw)
        assert end == 10.0 and len(tracks) == 3 and all(len(t.predictions) == 1 for t in tracks)
        return [t.get_meta() for t in tracks]

    def boxes(metas):
        return [{k: v for k, v in m.items() if k != "predictions"} for m in metas]

    host = tracks_of(windows="host", filter_freqs=True)
    device = tracks_of(windows="device", filter_freqs=True)
    assert boxes(host) == boxes(device) and n_windows[0] == n_windows[1] >= 3

    # both options off: today's output, and no filter launch when no track qualifies
    plain = tracks_of(windows="device")
    assert plain == tracks_of(windows="device", filter_freqs=False, filter_below=None)
    assert plain == tracks_of(windows="host")
    with monkeypatch.context() as m:
        m.setattr(fe, "sosfilt_segments", None)  # calling it would raise
        assert plain == tracks_of(windows="device", filter_below=50)
    below = tracks_of(windows="device", filter_below=3000)  # some tracks filtered, the others copied
    assert boxes(below) == boxes(plain)

    # stage by stage
    dev = []
    tracks, frames, end = predict.detect_tracks(rec, detector=p._detector, dev_out=dev)
    n = 3 * SR
    wins = np.concatenate(predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(0), filter_freqs=True))
    plan, counts, segs = predict.track_window_plan(len(frames), SR, tracks, rng=np.random.RandomState(0),
                                                   segments=True)
    seg, sos, plan2 = predict.sos_segment_plan(tracks, segs, plan, counts, SR, filter_freqs=True)
    assert len(seg) == 3 and not (sos == IDENT).all(axis=(1, 2)).any()
    filtered = fe.sosfilt_segments(dev[0], seg, sos)
    buf = filtered.cpu().numpy()
    for (src, ln, dst), f in zip(seg.tolist(), sos):
        assert within_bound(buf[dst:dst + ln], sosfilt(f, frames[src:src + ln].astype(np.float64)))
    cut = np.zeros((len(plan2), n), np.float32)
    for w, (src, count, pad) in enumerate(plan2.tolist()):
        cut[w, pad:pad + count] = buf[src:src + count]
    with torch.no_grad():
        f_host = p.frontend(torch.from_numpy(cut).to(cuda), pad_mode="constant")
        f_dev = p.frontend.features(fe.normalize_windows(filtered, plan2, n), pad_mode="constant")
    assert f_host.shape == f_dev.shape and torch.equal(f_host, f_dev)
    assert np.array_equal(p.predict_plan(filtered, plan2), p.predict_clips(cut))
    with capsys.disabled():
        print("\nmax |p_device - p_host| over the windows:", np.abs(p.predict_clips(cut) - p.predict_clips(wins)).max(),
              "; samples differing after the filter:", int((cut != wins).sum()), "of", wins.size)

    capsys.readouterr()
    predict.main([str(ck), "--file", str(tmp_path / "rec.wav"), "--filter-freqs", "--windows", "device",
                  "--detector", "gpu"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["end"] == 10.0 and len(out["tracks"]) == 3
    assert all(len(t["predictions"]) == 1 for t in out["tracks"])
