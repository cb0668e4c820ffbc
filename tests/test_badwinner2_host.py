"""badwinner2 without a GPU: geometry, the Keras weight layout and round trip,
the model name in audiomodel.py, and the three modes of the CPU restatement
(tests/bw2_reference.py) against each other.

Keras parity is unpinned, as for the WRNs (tests/test_keras_weights.py): the
reference ships no checkpoint and h5py is absent, so the reader is exercised
on files the writer produces in the Keras 3 layout.
"""
import zipfile

import numpy as np
import pytest
import torch

import bw2_reference as R


def _model(cin=1, n_mels=96, labels=7, seed=0, **kw):
    import badwinner2

    return badwinner2.build_model((n_mels, 513, cin), None, labels, **kw)


def test_output_hw():
    from badwinner2 import output_hw

    assert output_hw(160, 513) == (1, 46)
    assert output_hw(96, 513) == (1, 46)
    assert output_hw(96, 103) == (1, 1)
    assert output_hw(96, 131) == (1, 4)
    with pytest.raises(ValueError):
        output_hw(128, 513)
    with pytest.raises(ValueError):
        output_hw(96, 102)


def test_build_model_arguments():
    import badwinner2

    m = badwinner2.build_model((160, 513, 3), None, 50, multi_label=True, lme=True)
    assert (m.classes, m.multi_label, m.lme, m.dtype) == (50, True, True, torch.bfloat16)
    assert m.training  # a fresh module; only a forward in training mode is refused
    with pytest.raises(ValueError):
        badwinner2.build_model((128, 513, 3), None, 5)
    with pytest.raises(ValueError):
        badwinner2.build_model((160, 513, 3), None, 5, big_condense=False)
    with pytest.raises(ValueError):
        badwinner2.build_model((160, 513, 3), None, 5, add_dense=False)
    with pytest.raises(NotImplementedError, match="eval mode only"):
        m(torch.zeros(1, 160, 513))


@pytest.mark.parametrize("n_mels,rows", [(160, 44), (96, 22)])
def test_keras_layers_order_and_shapes(n_mels, rows):
    from keras_weights import keras_layers, keras_weights_tree

    m = _model(cin=3, n_mels=n_mels, labels=50)
    kinds = [k for k, _, _ in keras_layers(m)]
    assert kinds == ["mag_transform", "batch_normalization"] + ["conv2d", "batch_normalization"] * 7 + ["conv2d"]
    assert all(name is None for _, name, _ in keras_layers(m))  # every layer is auto-named
    tree = keras_weights_tree(m)["layers"]
    shapes = {k: [v.shape for _, v in sorted(d["vars"].items())] for k, d in tree.items()}
    assert shapes["mag_transform"] == [(1,)]
    assert shapes["batch_normalization"] == [(n_mels,), (n_mels,)]  # moving mean, moving variance only
    kernels = [(3, 3, 3, 64), (3, 3, 64, 64), (3, 3, 64, 128), (3, 3, 128, 128), (rows, 3, 128, 128),
               (1, 9, 128, 1024), (1, 1, 1024, 1024), (1, 1, 1024, 50)]
    for i, ks in enumerate(kernels):
        name = "conv2d" if i == 0 else f"conv2d_{i}"
        assert shapes[name] == [ks, (ks[3],)], name
        if i < 7:
            assert shapes[f"batch_normalization_{i + 1}"] == [(ks[3],)] * 4
    assert len(tree) == 17


def _randomise(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in list(m.parameters()) + list(m.buffers()):
            t.copy_(torch.randn(t.shape, generator=g))
    return m


@pytest.mark.parametrize("offset", [None, {"conv2d": 4, "batch_normalization": 9, "mag_transform": 2}],
                         ids=["fresh", "offset"])
@pytest.mark.parametrize("cin", [1, 3])
def test_weights_round_trip(tmp_path, cin, offset):
    """.weights.h5 and .keras, bit for bit, whatever the session's auto-name
    offset; a model built with the other Cin takes the file's."""
    from keras_weights import load_keras_weights, save_keras_weights

    a = _randomise(_model(cin=cin), 1)
    f = save_keras_weights(a, tmp_path / "model.weights.h5", auto_offset=offset)
    z = tmp_path / "run.keras"
    with zipfile.ZipFile(z, "w") as zf:
        zf.writestr("config.json", "{}")
        zf.writestr("model.weights.h5", f.read_bytes())
    for path in (f, z):
        for build_cin in (cin, 4 - cin):
            b = _randomise(_model(cin=build_cin), 2)
            rep = load_keras_weights(b, path)
            assert rep["skipped"] == [] and rep["loaded"] == 17
            sa, sb = a.state_dict(), b.state_dict()
            assert sorted(sa) == sorted(sb)
            for k in sa:
                assert torch.equal(sa[k], sb[k]), (k, path.name, build_cin)
            assert b.convs[0].weight.shape[3] == cin


def test_malformed_files_name_the_layer(tmp_path):
    import h5lite
    from keras_weights import keras_weights_tree, load_keras_weights

    a = _model()
    tree = keras_weights_tree(a)
    # an input BatchNormalization with gamma / beta
    bad = {"layers": dict(tree["layers"]), "vars": {}}
    two = tree["layers"]["batch_normalization"]["vars"]
    bad["layers"]["batch_normalization"] = {"vars": {"0": two["0"], "1": two["0"], "2": two["0"], "3": two["1"]}}
    f = tmp_path / "four.weights.h5"
    f.write_bytes(h5lite.write_h5(bad))
    with pytest.raises(ValueError, match="batch_normalization: 4 variables"):
        load_keras_weights(_model(), f)
    # no MagTransform
    bad = {"layers": {k: v for k, v in tree["layers"].items() if k != "mag_transform"}, "vars": {}}
    g = tmp_path / "nomag.weights.h5"
    g.write_bytes(h5lite.write_h5(bad))
    with pytest.raises(ValueError, match="mag_transform"):
        load_keras_weights(_model(), g)
    # a first convolution with two input channels is not a checkpoint of this model
    bad = {"layers": dict(tree["layers"]), "vars": {}}
    k = tree["layers"]["conv2d"]["vars"]
    bad["layers"]["conv2d"] = {"vars": {"0": np.zeros((3, 3, 2, 64), np.float32), "1": k["1"]}}
    h = tmp_path / "cin2.weights.h5"
    h.write_bytes(h5lite.write_h5(bad))
    with pytest.raises(ValueError, match="conv2d"):
        load_keras_weights(_model(), h)


def test_audiomodel_knows_the_name_and_refuses_training(tmp_path):
    import audiomodel

    args = audiomodel.parse_args(["run", "-d", str(tmp_path / "no-such-dataset"), "--model-name", "badwinner2"])
    assert args.model_name == "badwinner2"
    with pytest.raises(SystemExit, match="inference only"):
        audiomodel.train_model(args)  # before the (missing) dataset directory is looked at
    m = audiomodel.build_model("badwinner2", (96, 513, 3), 7, torch.float32, multi_label=False, lme=True)
    assert type(m).__name__ == "BadWinner2" and (m.multi_label, m.lme, m.dtype) == (False, True, torch.float32)


@pytest.mark.parametrize("cin", [1, 3])
def test_restatement_modes_agree(cin):
    """float64, float32 and bf16-storage restatements of one seeded model on
    the CPU oracle's mel: the caps tests/test_badwinner2_gpu.py asserts."""
    M, T, B = 96, 103, 3
    mel = R.cpu_mel(R.chirp_clips(B, T, 1000 + M + T), M)
    assert mel.shape == (B, M, T)
    sd = R.state_of(R.seed_model(_model(cin=cin, dtype=torch.float32), 50 + M + T + cin))
    for ml in (True, False):
        for lme in (False, True):
            taps = []
            p64 = R.forward(sd, mel, "f64", ml, lme, taps)
            assert len(taps) == (14 if lme else 12)
            assert p64.shape == (B, 7) and bool(torch.isfinite(p64).all())
            e32 = float((R.forward(sd, mel, "f32", ml, lme) - p64).abs().max())
            ebf = float((R.forward(sd, mel, "bf16", ml, lme) - p64).abs().max())
            assert 0 < e32 <= 1e-4 and e32 < ebf <= 0.1, (e32, ebf)
            if not ml:
                assert float(p64.max()) < 0.99 and float((p64.sum(1) - 1).abs().max()) < 1e-12
