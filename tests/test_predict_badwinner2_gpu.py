"""predict.py on a badwinner2 checkpoint directory (metadata.txt + a Keras 3
model.weights.h5 written by save_keras_weights, n_mels 96 to keep it small):
Predictor builds the model and the PCEN-less fp32 front end from the metadata,
predict_clips equals the model applied to the front end's features, a
single-label checkpoint's rows are softmax rows, the CLI runs in both modes;
and the two WRNs still get ops.sigmoid of the same logits, bit for bit.
"""
import json

import numpy as np
import pytest
import torch

import bw2_reference as R
from conftest import synth_clips

pytestmark = pytest.mark.gpu

SR = 48000
LABELS = ["bird", "frog", "insect", "noise", "rain"]


def _checkpoint(path, cin, multi_label, dtype="bf16", lme=False):
    import badwinner2
    from keras_weights import save_keras_weights

    path.mkdir()
    meta = {"labels": LABELS, "name": "badwinner2", "n_mels": 96, "dtype": dtype, "multi_label": multi_label,
            "lme": lme, "pcen": True}  # (pcen: the WRN default; this family must ignore it)
    (path / "metadata.txt").write_text(json.dumps(meta))
    model = R.seed_model(badwinner2.build_model((96, 513, cin), None, len(LABELS)), 7 + cin)
    save_keras_weights(model, path / "model.weights.h5", auto_offset={"conv2d": 3})
    return model


@pytest.mark.parametrize("cin,multi_label,dtype", [(3, True, "bf16"), (1, False, "fp32")])
def test_predictor_equals_model_on_features(tmp_path, cuda, cin, multi_label, dtype):
    import predict

    src = _checkpoint(tmp_path / "ck", cin, multi_label, dtype)
    p = predict.Predictor(tmp_path / "ck")
    assert type(p.model).__name__ == "BadWinner2" and p.model.multi_label == multi_label and not p.model.training
    assert p.model.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float32)
    assert p.model.convs[0].weight.shape[3] == cin  # the file's Cin, whatever the model was built with
    assert p.frontend.pcen is None and p.frontend.dtype == torch.float32
    for k, v in src.state_dict().items():
        assert torch.equal(v, p.model.state_dict()[k].cpu()), k
    clips = synth_clips(2, seed=77)
    probs = p.predict_clips(clips)
    with torch.no_grad():
        feats = p.frontend(torch.from_numpy(clips).to(cuda), pad_mode="constant")
        assert feats.dtype == torch.float32 and feats.shape == (2, 96, 513)
        want = p.model.predict(feats)
    assert probs.shape == (2, len(LABELS)) and np.array_equal(probs, want.float().cpu().numpy())
    assert np.isfinite(probs).all() and (probs > 0).all() and (probs < 1).all()
    if multi_label:
        from acfe import ops

        assert torch.equal(want, ops.sigmoid(p.model(feats)))
    else:
        assert np.abs(probs.sum(1) - 1).max() < 1e-5
    # batch_size cuts the launches, not the result (no PCEN: no batch statistics)
    assert np.array_equal(p.predict_clips(clips, batch_size=1), probs)


def test_model_pt_checkpoint(tmp_path, cuda):
    """A model.pt directory: the first convolution's Cin comes from the state."""
    import predict
    from acfe.train import FrontEnd

    src = _checkpoint(tmp_path / "ck", 1, True)
    (tmp_path / "ck" / "model.weights.h5").unlink()
    front = FrontEnd(n_mels=96, pcen=False, dtype=torch.float32, device=cuda)
    torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([front, src]).state_dict().items()},
               tmp_path / "ck" / "model.pt")
    p = predict.Predictor(tmp_path / "ck")
    assert p.model.convs[0].weight.shape[3] == 1
    assert torch.equal(p.model.class_conv.weight.cpu(), src.class_conv.weight)


def test_cli_both_modes(tmp_path, cuda, capsys):
    import predict
    from scipy.io import wavfile

    _checkpoint(tmp_path / "ck", 3, False)
    t = np.arange(5 * SR) / SR
    rng = np.random.default_rng(5)
    rec = rng.normal(0, 0.005, t.size)
    for on, dur, f0, f1 in ((0.5, 1.0, 3000, 4000), (2.5, 1.5, 6000, 5000)):
        m = (t >= on) & (t < on + dur)
        tt = t[m] - on
        rec[m] += 0.3 * np.sin(2 * np.pi * (f0 * tt + 0.5 * (f1 - f0) / dur * tt * tt))
    wavfile.write(tmp_path / "rec.wav", SR, (np.clip(rec, -1, 1) * 32767).astype(np.int16))
    predict.main([str(tmp_path / "ck"), "--file", str(tmp_path / "rec.wav"), "--mode", "windows"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["windows"] == 3 and sorted(out["mean"]) == sorted(LABELS)
    assert abs(sum(out["mean"].values()) - 1) < 1e-4  # the mean of softmax rows
    predict.main([str(tmp_path / "ck"), "--file", str(tmp_path / "rec.wav"), "--mode", "tracks", "--detector", "gpu",
                  "--windows", "device"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["end"] > 4.0 and len(out["tracks"]) >= 1
    for tr in out["tracks"]:
        assert len(tr["predictions"]) == 1 and tr["predictions"][0]["model"] == "badwinner2"


@pytest.mark.parametrize("name", ["wr-resnet", "wr-resnet-bird"])
def test_wrn_probabilities_unchanged(tmp_path, cuda, name):
    """The refactored Predictor gives a WRN ops.sigmoid of the same logits."""
    import predict
    from acfe import ops
    from acfe.train import FrontEnd
    from audiomodel import build_model

    ck = tmp_path / "ck"
    ck.mkdir()
    (ck / "metadata.txt").write_text(json.dumps({"labels": ["a", "b", "c"], "name": name, "n_mels": 128,
                                                 "dtype": "bf16"}))
    torch.manual_seed(0)
    model = build_model(name, (128, 513, 3), 3, torch.bfloat16)
    front = FrontEnd(n_mels=128, pcen=True, dtype=torch.bfloat16, device=cuda)
    torch.save({k: v.detach().cpu() for k, v in torch.nn.ModuleList([front, model]).state_dict().items()},
               ck / "model.pt")
    p = predict.Predictor(ck)
    assert not hasattr(p.model, "activation")
    clips = synth_clips(2, seed=78)
    with torch.no_grad():
        want = ops.sigmoid(p.model(p.frontend(torch.from_numpy(clips).to(cuda), pad_mode="constant")))
    assert np.array_equal(p.predict_clips(clips), want.float().cpu().numpy())
