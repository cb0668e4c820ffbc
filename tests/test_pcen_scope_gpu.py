"""acfe_pcen_normalize_segments (csrc/pcen_scope.hip): PCEN's normalize_minmax
per segment of a launch, bit for bit what acfe_pcen_normalize gives on each
segment's clips alone and within the forward tolerance of the float64 oracle;
and predict's --pcen-scope end to end: under "track" / "window" the features
of a track / window are those of that track / window run alone."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SR = 48000
GUARD = 12345.0
PARAMS = (0.98, 2.0, 2.0, 0.04)
TOL = {torch.float32: 5e-5, torch.bfloat16: 8e-3}  # test_frontend_gpu.test_pcen_forward's, against float64

# (B, M, T) -> (index of the all-zero clip, segment tables)
CASES = {
    (7, 160, 33): (2, ([0, 7], [0, 1, 2, 3, 4, 5, 6, 7], [0, 2, 2, 3, 7])),  # 64-row PCEN blocks straddle clips
    (5, 40, 513): (2, ([0, 5], [0, 1, 2, 3, 4, 5], [0, 2, 2, 3, 5])),
    (3, 128, 513): (0, ([0, 1, 3], [0, 3])),  # the real size
}


@pytest.fixture(scope="module")
def fe(cuda):
    from acfe import frontend

    return frontend


def f32(t):
    return t.float().cpu().numpy()


def same_bits(a, b):
    """Equal bit patterns, except that a NaN matches any NaN (bf16 widened to
    float32, which keeps distinct values distinct)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def make_mel(shape, zero_clip, cuda):
    """Random positive mel [B, T, M] with a per-clip scale from 1e-3 to 1e3 and
    one all-zero clip."""
    b, m, t = shape
    rng = np.random.default_rng(b * 1000 + m)
    mel = rng.uniform(0.05, 1.0, (b, t, m)) ** 3 * np.geomspace(1e-3, 1e3, b)[:, None, None]
    mel[zero_clip] = 0
    return torch.from_numpy(mel.astype(np.float32)).to(cuda)


def pcen_y(mel, p):
    """acfe_pcen_fwd alone: the un-normalised y [B, M, T] and its partials."""
    from acfe._lib import call, lib
    from acfe._torch import ptr, stream

    b, t, m = mel.shape
    npart = lib.acfe_pcen_partials(b, m)
    y = torch.empty((b, m, t), dtype=torch.float32, device=mel.device)
    part = torch.empty(2 * npart, dtype=torch.float32, device=mel.device)
    call("acfe_pcen_fwd", ptr(mel), b, t, m, ptr(p), 1e-6, ptr(y), ptr(part), stream())
    return y, part


def existing_stats(mel, p):
    """stats[0:2] = {mn, mx} of the existing path on `mel`."""
    from acfe._lib import call
    from acfe._torch import ptr, stream

    y, part = pcen_y(mel, p)
    out, stats = torch.empty_like(y), torch.empty(4, dtype=torch.float32, device=mel.device)
    call("acfe_pcen_normalize", ptr(y), y.numel(), ptr(part), part.numel() // 2, None, ptr(out), 0, ptr(stats),
         stream())
    return stats[:2].cpu().numpy()


_ORACLE = {}


def oracle(shape, mel, a, b):
    """oracle.torch_ref.pcen_torch in float64 on clips [a, b), computed once."""
    from oracle.torch_ref import pcen_torch

    if (shape, a, b) not in _ORACLE:
        _ORACLE[shape, a, b] = pcen_torch(mel[a:b].cpu().double(), torch.tensor(PARAMS, dtype=torch.float64)).numpy()
    return _ORACLE[shape, a, b]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(CASES), ids=lambda s: "x".join(map(str, s)))
def test_pcen_normalize_segments(fe, cuda, shape, dtype):
    zero_clip, tables = CASES[shape]
    mel = make_mel(shape, zero_clip, cuda)
    p = torch.tensor(PARAMS, device=cuda)
    y, _ = pcen_y(mel, p)
    whole = fe.pcen(mel, p, out_dtype=dtype)
    whole_mm = existing_stats(mel, p)
    for table in tables:
        out, mm = fe.pcen_normalize_segments(y, table, dtype)
        assert out.dtype == dtype and out.shape == y.shape and mm.shape == (len(table) - 1, 2)
        got, mm = f32(out), mm.cpu().numpy()
        assert same_bits(f32(fe.pcen(mel, p, out_dtype=dtype, segments=table)), got)
        seen = []
        for s, (a, b) in enumerate(zip(table, table[1:])):
            if a == b:
                assert mm[s, 0] == np.inf and mm[s, 1] == -np.inf
                continue
            ref_mm = existing_stats(mel[a:b], p)
            seen.append(tuple(ref_mm))
            assert same_bits(mm[s], ref_mm)
            assert same_bits(got[a:b], f32(fe.pcen(mel[a:b], p, out_dtype=dtype)))
            ref = oracle(shape, mel, a, b)
            if a <= zero_clip < b and b - a == 1:
                assert np.isnan(ref).all() and np.isnan(got[a:b]).all()  # 0 / 0
            else:
                assert np.isfinite(ref).all()
            err = np.abs(got[a:b] - ref)
            assert np.array_equal(np.isnan(got[a:b]), np.isnan(ref)) and not (err > TOL[dtype]).any()
        if len(seen) > 1:
            # the segments' extrema really differ, from one another and from the launch's:
            # the launch-wide pair cannot reproduce any segment's output
            assert len(set(seen)) == len(seen) and tuple(whole_mm) not in seen
        else:
            assert same_bits(got, f32(whole)) and same_bits(mm[0], whole_mm)  # one segment == the unsegmented call


def test_pcen_segments_arguments(fe, cuda):
    from acfe import _lib

    b, ce = 7, 40
    y = torch.rand((b, ce), device=cuda)
    seg = torch.tensor([0, 3, 7], dtype=torch.int32, device=cuda)
    out = torch.empty((b, ce), device=cuda)
    mm = torch.empty((2, 2), device=cuda)
    w = _lib.lib.acfe_pcen_segments_workspace
    assert w(b, ce) >= 4 * 2 * (b + b) and w(b, 3 * 16384 + 1) >= 4 * 2 * (4 * b + b)
    assert w(0, ce) == _lib.E_INVAL and w(-1, ce) == _lib.E_INVAL
    assert w(b, 0) == _lib.E_INVAL and w(b, -5) == _lib.E_INVAL
    ws = torch.empty(w(b, ce), dtype=torch.uint8, device=cuda)
    f = _lib.lib.acfe_pcen_normalize_segments
    Y, S, O, M, W = y.data_ptr(), seg.data_ptr(), out.data_ptr(), mm.data_ptr(), ws.data_ptr()
    assert f(Y, b, ce, S, 2, O, 0, M, W, None) == 0
    assert f(Y, b, ce, S, 2, O, 1, M, W, None) == 0
    torch.cuda.synchronize()
    for args in ((None, b, ce, S, 2, O, 0, M, W), (Y, b, ce, None, 2, O, 0, M, W), (Y, b, ce, S, 2, None, 0, M, W),
                 (Y, b, ce, S, 2, O, 0, None, W), (Y, b, ce, S, 2, O, 0, M, None),  # a null pointer
                 (Y, 0, ce, S, 2, O, 0, M, W), (Y, -1, ce, S, 2, O, 0, M, W),  # batch
                 (Y, b, 0, S, 2, O, 0, M, W), (Y, b, -1, S, 2, O, 0, M, W),  # clip_elems
                 (Y, b, ce, S, 0, O, 0, M, W), (Y, b, ce, S, -1, O, 0, M, W), (Y, b, ce, S, b + 1, O, 0, M, W),  # n_seg
                 (Y, b, ce, S, 2, O, 2, M, W), (Y, b, ce, S, 2, O, -1, M, W)):  # dtype
        assert f(*args, None) == _lib.E_INVAL
    # the Python layer checks before any launch
    mel = torch.rand((b, 8, 5), device=cuda)
    p = torch.tensor(PARAMS, device=cuda)
    with pytest.raises(ValueError):
        fe.pcen(mel, p, segments=[0, 3, 6])
    with pytest.raises(ValueError):
        fe.pcen(mel, p, segments=[0, 7], scope_minmax=torch.tensor([0.0, 1.0], device=cuda))
    pg = torch.tensor(PARAMS, device=cuda, requires_grad=True)
    with pytest.raises(RuntimeError):
        fe.pcen(mel, pg, segments=[0, 7])
    with torch.no_grad():
        assert same_bits(f32(fe.pcen(mel, pg, segments=[0, 7])), f32(fe.pcen(mel, p)))
    assert same_bits(f32(fe.PCEN().to(cuda).requires_grad_(False)(mel, segments=[0, 3, 7])[:3]),
                     f32(fe.pcen(mel[:3], p)))


def test_pcen_segments_malformed_table(fe, cuda):
    """A table the host check would refuse, passed straight to the C call:
    offsets past the batch and running backwards are clamped, nothing outside
    out is written."""
    from acfe import _lib

    b, ce = 7, 1027
    y = torch.rand((b, ce), device=cuda)
    seg = torch.tensor([0, 9, 3, 100], dtype=torch.int32, device=cuda)
    for code, dtype in ((0, torch.float32), (1, torch.bfloat16)):
        buf = torch.full(((b + 2) * ce,), GUARD, dtype=dtype, device=cuda)
        mm = torch.full((5, 2), GUARD, device=cuda)
        ws = torch.empty(_lib.lib.acfe_pcen_segments_workspace(b, ce), dtype=torch.uint8, device=cuda)
        rc = _lib.lib.acfe_pcen_normalize_segments(y.data_ptr(), b, ce, seg.data_ptr(), 3, buf[ce:].data_ptr(), code,
                                                   mm[1:].data_ptr(), ws.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        got, guard = f32(buf), f32(torch.tensor(GUARD, dtype=dtype))
        assert (got[:ce] == guard).all() and (got[(b + 1) * ce:] == guard).all()
        m = mm.cpu().numpy()
        assert (m[0] == GUARD).all() and (m[4] == GUARD).all()
        assert m[2, 0] == np.inf and m[2, 1] == -np.inf  # [9, 3) is empty
        yh = y.cpu().numpy()
        assert m[1, 0] == yh.min() and m[1, 1] == yh.max()  # [0, 9) -> the whole batch
        assert m[3, 0] == yh[3:].min() and m[3, 1] == yh[3:].max()  # [3, 100) -> [3, 7)
        assert np.isfinite(got[ce:(b + 1) * ce]).all()


# ---------------------------------------------------------------- predict

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


class Run:
    """The checkpoint and 10 s chirp recording of
    test_predict_tracks_device_windows, its Predictor with the model's inputs
    recorded, and each track's windows."""

    def __init__(self, tmp, cuda):
        import predict
        from acfe.train import FrontEnd
        from audiomodel import build_model
        from scipy.io import wavfile

        self.ck = tmp / "ck"
        self.ck.mkdir()
        meta = {"labels": ["bird", "noise"], "name": "wr-resnet-bird", "n_mels": 128, "dtype": "bf16"}
        (self.ck / "metadata.txt").write_text(json.dumps(meta))
        torch.manual_seed(0)
        model = build_model("wr-resnet-bird", (128, 513, 3), 2, torch.bfloat16)
        front = FrontEnd(n_mels=128, n_fft=4096, hop=281, fmin=100, fmax=11000, break_freq=1000, pcen=True,
                         dtype=torch.bfloat16, device=cuda, power=2)
        torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([front, model]).state_dict().items()},
                   self.ck / "model.pt")
        rec = _recording([(1.0, 1.0, 3000, 4000), (4.0, 0.8, 6000, 5000), (7.0, 1.5, 1500, 2500)], seconds=10, seed=3)
        self.wav = tmp / "rec.wav"
        wavfile.write(self.wav, SR, (rec * 32767).astype(np.int16))
        self.rec = predict.load_recording(self.wav)
        self.p = predict.Predictor(self.ck)
        self.fed = []  # every batch the model is given
        self.p.model.register_forward_pre_hook(lambda mod, args: self.fed.append(args[0].detach().clone()))
        tracks, frames, _ = predict.detect_tracks(self.rec, detector="gpu")
        self.det_tracks, self.frames = tracks, frames
        self.wins = predict.track_windows(frames, SR, tracks, rng=np.random.RandomState(0))
        self.counts = [len(w) for w in self.wins]
        assert len(tracks) == 3 and min(self.counts) >= 1 and max(self.counts) <= 32
        self._alone = {}

    def tracks(self, rec=None, **kw):
        """predict_tracks -> (the tracks' metadata, the features the model saw)."""
        import identifytracks as it

        it.Signal._next_id = 0  # the ids in get_meta count up over the process
        del self.fed[:]
        tracks, end = self.p.predict_tracks(self.rec if rec is None else rec, rng=np.random.RandomState(0),
                                            detector="gpu", **kw)
        assert end == 10.0 and len(tracks) == 3 and all(len(t.predictions) == 1 for t in tracks)
        return [t.get_meta() for t in tracks], torch.cat(self.fed)

    def alone(self, clips):
        """frontend features of `clips` run as a batch of their own (the existing path)."""
        with torch.no_grad():
            return self.p.frontend(torch.from_numpy(np.ascontiguousarray(clips)).to(self.p.device),
                                   pad_mode="constant")


@pytest.fixture(scope="module")
def run(tmp_path_factory, cuda):
    return Run(tmp_path_factory.mktemp("pcen_scope"), cuda)


def test_predict_tracks_scope_features(run):
    """Under "track" the model sees, for each track, the features of that
    track's windows run alone (host and device windows, batch_size 32 and
    1024); under "window" those of each window alone; "batch" is the call
    without the argument."""
    import predict

    at = np.concatenate(([0], np.cumsum(run.counts)))
    per_track = torch.cat([run.alone(w) for w in run.wins])
    per_window = torch.cat([run.alone(w[i:i + 1]) for w in run.wins for i in range(len(w))])
    together = run.alone(np.concatenate(run.wins))
    # the scopes differ on this recording, so the equalities below tell them apart
    assert not torch.equal(per_track, together)
    assert torch.equal(per_window, per_track) == (max(run.counts) == 1)
    assert sum(torch.equal(per_track[a:b], together[a:b]) for a, b in zip(at, at[1:])) <= 1

    meta_default, f_default = run.tracks()
    meta_batch, f_batch = run.tracks(pcen_scope="batch")
    assert meta_batch == meta_default and torch.equal(f_batch, f_default) and torch.equal(f_batch, together)
    for windows in ("host", "device"):
        for batch_size in (32, 1024):
            _, f = run.tracks(pcen_scope="track", windows=windows, batch_size=batch_size)
            assert f.shape == per_track.shape and torch.equal(f, per_track), (windows, batch_size)
        _, f = run.tracks(pcen_scope="window", windows=windows)
        assert torch.equal(f, per_window), windows
    _, f = run.tracks(pcen_scope="window", batch_size=2)  # launches of 2 windows
    assert torch.equal(f, per_window)
    # together with the other options: the recording as a device tensor, the band-pass of the tracks
    dev_rec = torch.from_numpy(run.rec).to(run.p.device)
    _, f = run.tracks(dev_rec, pcen_scope="track", windows="device")
    assert torch.equal(f, per_track)
    filtered = predict.track_windows(run.frames, SR, run.det_tracks, rng=np.random.RandomState(0), filter_freqs=True)
    _, f = run.tracks(pcen_scope="track", filter_freqs=True)
    assert torch.equal(f, torch.cat([run.alone(w) for w in filtered])) and not torch.equal(f, per_track)
    _, f = run.tracks(dev_rec, pcen_scope="track", windows="device", filter_freqs=True)  # within an ulp of the host's
    assert f.shape == per_track.shape and bool(torch.isfinite(f.float()).all())
    # the same windows as two longer "tracks": runs of several windows share their extrema
    wins = np.concatenate(run.wins)
    counts = [2, len(wins) - 2]
    del run.fed[:]
    run.p.predict_clips(wins, 1024, segments=predict.pcen_segments(counts, "track"))
    grouped = torch.cat([run.alone(wins[:2]), run.alone(wins[2:])])
    assert torch.equal(torch.cat(run.fed), grouped) and not torch.equal(grouped, per_window)
    del run.fed[:]
    run.p.predict_clips(wins, 2, segments=predict.pcen_segments(counts, "track", keras_batch=1))
    assert torch.equal(torch.cat(run.fed), per_window)
    with pytest.raises(ValueError):
        run.p.predict_tracks(run.rec, detector="gpu", pcen_scope="track", batch_size=16)
    with pytest.raises(ValueError):
        run.p.predict_tracks(run.rec, detector="gpu", pcen_scope="recording")
    with pytest.raises(ValueError):
        run.p.predict_windows(run.rec, pcen_scope="track")


def test_predict_windows_and_cli(run, capsys):
    """predict_windows(pcen_scope="window") is one window at a time; the CLI
    with --pcen-scope track prints the predictions of the API call."""
    import predict

    rec = run.rec[:5 * SR]
    assert run.p.predict_windows(rec, pcen_scope="window").shape[0] == 3
    del run.fed[:]
    run.p.predict_windows(rec, pcen_scope="window", batch_size=2)
    f_window = torch.cat(run.fed)
    del run.fed[:]
    for i in range(3):
        run.p.predict_windows(rec[i * SR:(i + 3) * SR])
    assert torch.equal(f_window, torch.cat(run.fed))
    assert np.array_equal(run.p.predict_windows(rec, pcen_scope="batch"), run.p.predict_windows(rec))

    meta, _ = run.tracks(pcen_scope="track", windows="device")
    capsys.readouterr()
    predict.main([str(run.ck), "--file", str(run.wav), "--pcen-scope", "track", "--detector", "gpu", "--windows",
                  "device"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["end"] == 10.0 and len(out["tracks"]) == 3
    assert [t["predictions"] for t in out["tracks"]] == \
        json.loads(json.dumps([m["predictions"] for m in meta], default=float))


def test_predict_tracks_scope_probabilities(run):
    """Per-track mean probabilities under "track" against predict_clips of that
    track's windows alone.  The features are identical
    (test_predict_tracks_scope_features), so a difference can only come from
    the model running at another batch size.  That effect, measured with the
    parent commit's entry points alone (the model and the batch-scope front
    end) for this checkpoint and recording (3 tracks of one window each) as
    sigmoid(model(f))[a:b] against sigmoid(model(f[a:b])) on the batch-scope
    features f, on an MI355X: 0 per window and 0 per track mean
    (profiles/predict_pcen_scope.md), so the comparison here is exact."""
    import predict

    seg = predict.pcen_segments(run.counts, "track")
    probs = run.p.predict_clips(np.concatenate(run.wins), 1024, segments=seg)
    at = np.concatenate(([0], np.cumsum(run.counts)))
    for k, (a, b) in enumerate(zip(at, at[1:])):
        alone = run.p.predict_clips(run.wins[k])
        diff = float(np.abs(probs[a:b].mean(0) - alone.mean(0)).max())
        print(f"track {k}: per-track mean probability, batched against alone: max |diff| = {diff:.3e}")
        assert np.array_equal(probs[a:b].mean(0), alone.mean(0))
    # and these are the probabilities behind predict_tracks' results
    meta, _ = run.tracks(pcen_scope="track")
    for k, (a, b) in enumerate(zip(at, at[1:])):
        r = meta[k]["predictions"][0]
        mean = probs[a:b].mean(0)
        assert r["species"] == [l for l, v in zip(run.p.labels, mean) if v >= 0.7]
        if not r["species"]:
            assert r["raw_tag"] == run.p.labels[int(mean.argmax())] and \
                r["raw_confidence"] == round(float(mean.max()) * 100)
