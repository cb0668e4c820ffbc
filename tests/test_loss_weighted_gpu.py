"""acfe_loss_weighted (csrc/loss_weighted.hip): Keras fit(class_weight=...) on
one-hot targets and the loss object's label_smoothing inside the loss kernel
(reference audiomodel.py:523-562, :1206-1223), through the C ABI, acfe.ops
.loss_and_grad and acfe.train.Trainer.

The reference is float64 torch: oracle.models.keras_loss per row on the
smoothed target y' = y (1 - s) + (BCE: s / 2, CCE: s / L), times the weight of
the row's argmax class (lowest index on ties, class 0 for an all-zero row),
summed and divided by B; autograd gives dz.

Bounds: loss error 1e-5 and dz rel-L2 1e-5, those acfe_loss itself is held to
(test_nn_variants_gpu.test_loss); the new kernel adds one multiply and one fused
multiply-add per element to it.  The weight lookup, the zero-weight rows and the
identity with acfe_loss at weights 1 / smoothing 0 are exact.

Shapes: L = 1, 2, 50 (one partial wave), 255 / 256 / 257 and 300 (around the
256-thread stride), 513 (three strides).  Over rows, modes and smoothings the hot
index of a row is at 0, 63 / 64 (a wave boundary), 255 / 256 (a stride
boundary) and L - 1.
"""
import numpy as np
import pytest
import torch

from oracle.models import keras_loss
from test_nn_variants_gpu import out_buf, put, rel_l2

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SHAPES = [(1, 1), (3, 2), (7, 50), (2, 255), (2, 256), (3, 257), (5, 300), (2, 513)]
SMOOTH = [0.0, 0.1]
GRAD_SCALE = 0.25
MODES = {0: "bce", 1: "cce"}
TOL = 1e-5


@pytest.fixture(scope="module")
def env(cuda):
    from acfe._lib import E_INVAL, call, lib
    from acfe._torch import ptr, stream

    return call, lib, ptr, stream, E_INVAL


# ------------------------------------------------------------------ reference
def ref_row_weight(y, cw):
    if cw is None:
        return torch.ones(y.shape[0], dtype=F64)
    idx = np.argmax(y.numpy(), axis=1)  # first occurrence of the maximum
    return cw[torch.from_numpy(idx)]


def reference(z, y, mode, cw, s, grad_scale):
    """float64 (loss, dz, row_loss, row_weight); z, y, cw are float64 CPU tensors."""
    B, L = z.shape
    w = ref_row_weight(y, cw)
    ys = y * (1 - s) + (0.5 * s if mode == 0 else s / L)
    zr = z.clone().requires_grad_(True)
    rows = torch.stack([keras_loss(zr[b:b + 1], ys[b:b + 1], MODES[mode]) for b in range(B)]) * w
    (rows.sum() * grad_scale).backward()
    return rows.sum().detach() / B, zr.grad, rows.detach(), w


def hot_indices(B, L, shift):
    spots = sorted({c for c in (0, 63, 64, 255, 256, L - 1) if c < L})
    return [spots[(b + shift) % len(spots)] for b in range(B)]


def one_hot_case(B, L, mode, si):
    """Inputs of a parametrised case: logits, one-hot targets with the hot
    index walking over the boundary spots, weights in [0, 4] with an exact 0."""
    g = torch.Generator().manual_seed(1000 * B + L)
    z = (torch.randn((B, L), generator=g) * 2).to(F32).to(F64)
    hot = hot_indices(B, L, 2 * (2 * mode + si))
    y = torch.zeros((B, L), dtype=F64)
    y[torch.arange(B), torch.tensor(hot)] = 1
    cw = (torch.rand(L, generator=g) * 4).to(F32).to(F64)
    # the exact zero: the class of row 0 when there is another row to carry a
    # loss, else a class no row has (L = 1 has only the row's own class: it is
    # zeroed for s = 0 and kept for s > 0)
    if B > 1 or (L == 1 and si == 0):
        cw[hot[0]] = 0
    elif L > 1:
        cw[(hot[0] + 1) % L] = 0
    return z, y, cw, hot


def run(env, cuda, z, y, mode, cw, s, grad_scale=GRAD_SCALE, with_row_weight=True):
    call, lib, ptr, stream, _ = env
    B, L = z.shape
    zb, yb = put(z, F32, cuda), put(y, F32, cuda)
    cwb = put(cw, F32, cuda) if cw is not None else None
    loss, dz = out_buf((1,), F32, cuda), out_buf((B, L), F32, cuda)
    rl, rw = out_buf((B,), F32, cuda), out_buf((B,), F32, cuda)
    call("acfe_loss_weighted", ptr(zb.t), ptr(yb.t), B, L, mode, grad_scale, ptr(cwb.t) if cwb else None, s,
         ptr(loss.t), ptr(dz.t), ptr(rl.t), ptr(rw.t) if with_row_weight else None, stream())
    torch.cuda.synchronize()
    return loss, dz, rl, rw


def run_plain(env, cuda, z, y, mode, grad_scale=GRAD_SCALE):
    call, lib, ptr, stream, _ = env
    B, L = z.shape
    zb, yb = put(z, F32, cuda), put(y, F32, cuda)
    loss, dz, ws = out_buf((1,), F32, cuda), out_buf((B, L), F32, cuda), out_buf((B,), F32, cuda)
    call("acfe_loss", ptr(zb.t), ptr(yb.t), B, L, mode, grad_scale, ptr(loss.t), ptr(dz.t), ptr(ws.t), stream())
    torch.cuda.synchronize()
    return loss, dz, ws


def loss_err(got, ref):
    return abs(got - ref) / max(1.0, abs(ref))


# ------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("si", [0, 1], ids=["s0", "s0.1"])
@pytest.mark.parametrize("mode", [0, 1], ids=["bce", "cce"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weighted_loss(env, cuda, shape, mode, si):
    B, L = shape
    s = SMOOTH[si]
    z, y, cw, hot = one_hot_case(B, L, mode, si)
    loss, dz, rl, rw = run(env, cuda, z, y, mode, cw, s)
    assert loss.intact() and dz.intact() and rl.intact() and rw.intact()
    lr, dzr, rlr, wr = reference(z, y, mode, cw, s, GRAD_SCALE)
    # the lookup is exact
    assert torch.equal(rw.t.cpu(), cw[torch.tensor(hot)].to(F32)), (hot, rw.t, cw[torch.tensor(hot)])
    assert torch.equal(rw.t.cpu(), wr.to(F32))
    el, eg = loss_err(loss.t.item(), lr.item()), rel_l2(dz.t, dzr)
    er = ((rl.t.double().cpu() - rlr).abs() / rlr.abs().clamp_min(1)).max().item()  # per row, as the loss
    print(f"loss_weighted {B}x{L} {MODES[mode]} s={s} hot={hot}: loss err {el:.2e} (1e-5), dz rel-L2 {eg:.2e} "
          f"(1e-5), row_loss err {er:.2e} (1e-5)")
    assert el <= TOL and eg <= TOL and er <= TOL
    # rows of a zero-weight class: exactly nothing
    zero = (wr == 0).nonzero().flatten().tolist()
    assert zero or (B == 1 and (L > 1 or si == 1))
    for b in zero:
        assert (dz.t[b] == 0).all() and rl.t[b].item() == 0, (b, dz.t[b], rl.t[b])
    if B > len(zero) and L > 1:  # (at L = 1 the CCE's q = 1 is clipped: no gradient)
        assert dz.t.abs().sum().item() > 0 and loss.t.item() > 0


def tie_rows(L):
    """(targets [R][L], expected argmax) of rows with equal maxima and more."""
    rows = []

    def row(pairs, want):
        if all(i < L for i, _ in pairs):
            r = torch.zeros(L, dtype=F64)
            for i, v in pairs:
                r[i] = v
            rows.append((r, want))

    row([(40, 1), (2, 1)], 2)            # two lanes of one wave
    row([(5, 1), (70, 1)], 5)            # waves 0 and 1 of one stride
    row([(70, 1), (200, 1)], 70)         # waves 1 and 3
    row([(200, 1), (63, 1), (64, 1)], 63)
    row([(300, 1), (100, 1)], 100)       # stride 1 in wave 0 against stride 0 in wave 1
    row([(7, 1), (263, 1)], 7)           # one lane, two strides
    row([(L - 1, 1), (263, 1)], 263)     # stride 1 against the row's last element
    row([(256, 1), (511, 1), (512, 1)], 256)
    row([(3, 0.5), (400, 0.5)], 3)       # a tie of mixed-up labels (lambda = 0.5)
    row([(10, 0.4), (300, 0.6)], 300)    # no tie: the larger value, not the lower index
    row([(L - 1, 0.25), (L - 2, 0.25)], L - 2)
    row([], 0)                           # an all-zero row: class 0
    row([(0, -1.0), (L - 1, -0.5)], 1 if L > 2 else L - 1)  # zeros beat negatives
    return torch.stack([r for r, _ in rows]), [w for _, w in rows]


@pytest.mark.parametrize("mode", [0, 1], ids=["bce", "cce"])
@pytest.mark.parametrize("L", [50, 300, 513])
def test_weight_lookup_ties(env, cuda, L, mode):
    y, want = tie_rows(L)
    B = y.shape[0]
    g = torch.Generator().manual_seed(L)
    z = (torch.randn((B, L), generator=g) * 2).to(F32).to(F64)
    cw = (torch.rand(L, generator=g) * 3.5 + 0.5).to(F32).to(F64)  # distinct with probability 1
    assert len(set(cw.tolist())) == L
    assert np.argmax(y.numpy(), axis=1).tolist() == want
    loss, dz, rl, rw = run(env, cuda, z, y, mode, cw, 0.1)
    assert loss.intact() and dz.intact() and rl.intact() and rw.intact()
    got = rw.t.cpu()
    assert torch.equal(got, cw[torch.tensor(want)].to(F32)), (want, got.tolist(), cw[torch.tensor(want)].tolist())
    lr, dzr, _, _ = reference(z, y, mode, cw, 0.1, GRAD_SCALE)
    el, eg = loss_err(loss.t.item(), lr.item()), rel_l2(dz.t, dzr)
    print(f"loss_weighted ties L={L} {MODES[mode]}: {B} rows, loss err {el:.2e} (1e-5), dz rel-L2 {eg:.2e} (1e-5)")
    assert el <= TOL and eg <= TOL


@pytest.mark.parametrize("mode", [0, 1], ids=["bce", "cce"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_identical_to_acfe_loss(env, cuda, shape, mode):
    """NULL weights, and all-ones weights, at s = 0: loss and dz are acfe_loss's,
    bit for bit -- on one-hot targets and on mixed (multi-hot, fractional) ones."""
    B, L = shape
    z, y1, _, _ = one_hot_case(B, L, mode, 0)
    g = torch.Generator().manual_seed(B + L)
    y2 = (torch.rand((B, L), generator=g) < 0.1).to(F64) * 0.75
    y2[:, 0] = 0.25
    ones = torch.ones(L, dtype=F64)
    for y in (y1, y2):
        l0, d0, w0 = run_plain(env, cuda, z, y, mode)
        for cw in (None, ones):
            l1, d1, r1, rw = run(env, cuda, z, y, mode, cw, 0.0, with_row_weight=cw is not None)
            assert l1.intact() and d1.intact() and r1.intact() and rw.intact()
            assert torch.equal(l1.t, l0.t), (cw is None, l1.t.item(), l0.t.item())
            assert torch.equal(d1.t, d0.t), (cw is None, (d1.t - d0.t).abs().max().item())
            assert torch.equal(r1.t, w0.t)
            if cw is None:
                assert torch.isnan(rw.t).all()  # NULL row_weight: nothing written
            else:
                assert (rw.t == 1).all()


def test_invalid_arguments_launch_nothing(env, cuda):
    call, lib, ptr, stream, E_INVAL = env
    B, L = 3, 50
    z, y, cw, _ = one_hot_case(B, L, 1, 0)
    zb, yb, cwb = put(z, F32, cuda), put(y, F32, cuda), put(cw, F32, cuda)
    outs = [out_buf((1,), F32, cuda), out_buf((B, L), F32, cuda), out_buf((B,), F32, cuda), out_buf((B,), F32, cuda)]
    loss, dz, rl, rw = (ptr(o.t) for o in outs)
    good = dict(z=ptr(zb.t), y=ptr(yb.t), B=B, L=L, mode=1, s=0.1, loss=loss, dz=dz, rl=rl)
    bad = [dict(s=1.0), dict(s=-0.1), dict(s=float("nan")), dict(mode=2), dict(mode=-1), dict(B=0), dict(B=-1),
           dict(L=0), dict(z=None), dict(y=None), dict(loss=None), dict(dz=None), dict(rl=None)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.acfe_loss_weighted(a["z"], a["y"], a["B"], a["L"], a["mode"], GRAD_SCALE, ptr(cwb.t), a["s"],
                                    a["loss"], a["dz"], a["rl"], rw, stream())
        assert rc == E_INVAL, (change, rc)
    torch.cuda.synchronize()
    for o in outs:
        assert o.intact() and torch.isnan(o.t).all()
    # and the same buffers with the valid arguments
    rc = lib.acfe_loss_weighted(good["z"], good["y"], B, L, 1, GRAD_SCALE, ptr(cwb.t), 0.1, loss, dz, rl, rw, stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(o.intact() and torch.isfinite(o.t).all() for o in outs)


# ------------------------------------------------------------------ acfe.ops
def test_ops_loss_and_grad(env, cuda):
    from acfe import ops

    B, L = 7, 50
    for mode in (0, 1):
        z, y, cw, _ = one_hot_case(B, L, mode, 1)
        zd, yd, cwd = z.to(F32).to(cuda), y.to(F32).to(cuda), cw.to(F32).to(cuda)
        # the keyword path, default grad_scale = 1 / B
        loss, dz = ops.loss_and_grad(zd, yd, MODES[mode], class_weights=cwd, label_smoothing=0.1)
        lr, dzr, _, _ = reference(z, y, mode, cw, 0.1, 1.0 / B)
        el, eg = loss_err(loss.item(), lr.item()), rel_l2(dz, dzr)
        print(f"ops.loss_and_grad {MODES[mode]} weights + s=0.1: loss err {el:.2e} (1e-5), dz rel-L2 {eg:.2e} (1e-5)")
        assert el <= TOL and eg <= TOL
        # smoothing alone
        loss, dz = ops.loss_and_grad(zd, yd, MODES[mode], label_smoothing=0.1)
        lr, dzr, _, _ = reference(z, y, mode, None, 0.1, 1.0 / B)
        assert loss_err(loss.item(), lr.item()) <= TOL and rel_l2(dz, dzr) <= TOL
        # the defaults still go to acfe_loss: bit-equal to the direct call
        loss, dz = ops.loss_and_grad(zd, yd, MODES[mode])
        l0, d0, _ = run_plain(env, cuda, z, y, mode, 1.0 / B)
        assert torch.equal(loss, l0.t) and torch.equal(dz, d0.t)
        loss, dz = ops.loss_and_grad(zd, yd, MODES[mode], class_weights=None, label_smoothing=0.0)
        assert torch.equal(loss, l0.t) and torch.equal(dz, d0.t)
    with pytest.raises(ValueError):
        ops.loss_and_grad(zd, yd, "cce", class_weights=cwd[:-1])
    with pytest.raises(ValueError):
        ops.loss_and_grad(zd, yd, "cce", class_weights=cwd.cpu())
    with pytest.raises(TypeError):
        ops.loss_and_grad(zd, yd, "cce", class_weights=cwd.double())
    with pytest.raises(TypeError):
        ops.loss_and_grad(zd, yd, "cce", class_weights=cw.tolist())
    with pytest.raises(ValueError):
        ops.loss_and_grad(zd, yd, "cce", label_smoothing=1.0)


# ------------------------------------------------------------------ Trainer
CLASSES = 10


def _trainer(cuda, class_weights=None, label_smoothing=0.0):
    from acfe.train import FrontEnd, Trainer
    from resnet.wr_resnet_bird import WRResNet

    torch.manual_seed(0)
    model = WRResNet(input_shape=(128, 64, 3), classes=CLASSES, dtype=torch.bfloat16, dropout=0.0).to(cuda)
    fe = FrontEnd(n_mels=128, dtype=torch.bfloat16, device=cuda).to(cuda)
    return Trainer(model, fe, lr=0.01, device=cuda, class_weights=class_weights, label_smoothing=label_smoothing)


def _batch(cuda):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn((4, 64 * 281), generator=g) * 0.1).clamp(-1, 1).to(cuda)
    y = torch.zeros(4, CLASSES, device=cuda)
    y[torch.arange(4), torch.tensor([1, 7, 3, 1])] = 1
    return x, y


def test_trainer_ones_is_unweighted(cuda):
    """class_weights = ones, label_smoothing = 0 is the unweighted step, bit for
    bit: loss, logits and the parameter arena after one step."""
    x, y = _batch(cuda)
    a = _trainer(cuda)
    b = _trainer(cuda, class_weights=np.ones(CLASSES, np.float32), label_smoothing=0.0)
    assert a.class_weights is None and b.class_weights is not None
    assert torch.equal(a.arena.flat, b.arena.flat)
    la, za = a.step(x, y)
    lb, zb = b.step(x, y)
    torch.cuda.synchronize()
    assert torch.isfinite(la).all()
    assert torch.equal(la, lb), (la.item(), lb.item())
    assert torch.equal(za, zb)
    assert torch.equal(a.arena.flat, b.arena.flat)


def test_trainer_weighted_step(cuda):
    from acfe import ops

    x, y = _batch(cuda)
    cw = np.array([1.0, 4.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.25, 1.0, 2.5], np.float32)
    tr = _trainer(cuda, class_weights=cw, label_smoothing=0.1)
    before = tr.arena.flat.clone()
    loss, z = tr.step(x, y)
    torch.cuda.synchronize()
    assert not torch.equal(before, tr.arena.flat)
    z64, y64 = z.detach().double().cpu(), y.double().cpu()
    lr, _, _, w = reference(z64, y64, 1, torch.from_numpy(cw).double(), 0.1, 0.25)
    assert w.tolist() == [4.0, 0.25, 0.0, 4.0]
    e = abs(loss.item() - lr.item()) / abs(lr.item())
    # evaluate(): the trainer's smoothing, never its class weights
    lv, _ = ops.loss_and_grad(z.detach(), y, tr.loss_mode, label_smoothing=tr.label_smoothing)
    lvr, _, _, _ = reference(z64, y64, 1, None, 0.1, 0.25)
    ev = abs(lv.item() - lvr.item()) / abs(lvr.item())
    print(f"Trainer weighted step: loss {loss.item():.6f} ref {lr.item():.6f} rel err {e:.2e} (1e-5); "
          f"unweighted smoothed loss {lv.item():.6f} ref {lvr.item():.6f} rel err {ev:.2e} (1e-5)")
    assert e <= TOL and ev <= TOL
    assert abs(lr.item() - lvr.item()) > 1e-3 * abs(lvr.item())  # the weights do change the loss here


def test_cli_use_weighting(tmp_path, cuda):
    """audiomodel.py --use-weighting --label-smoothing 0.1, one epoch on a
    dozen synthetic raw clips: the weights are get_weighting of the training
    split's examples per label and are recorded in metadata.txt."""
    import json

    import audiomodel
    import build
    import tfdataset

    assert build.main([str(tmp_path / "ds"), "--synthetic", "16", "--labels", "bird,noise", "--shards", "2",
                       "--no-spectrogram"]) == 0
    td = tmp_path / "ds" / "training-data"
    meta = json.loads((td / "training-meta.json").read_text())
    counts = [meta["counts"]["train"]["sample_counts"].get(lab, 0) for lab in meta["labels"]]
    args = audiomodel.parse_args(["w", "-d", str(td), "--epochs", "1", "--batch-size", "4", "--model-name",
                                  "wr-resnet-bird", "--n_mels", "128", "--load-raw", "--use-weighting",
                                  "--label-smoothing", "0.1", "--checkpoint-dir", str(tmp_path / "ck")])
    hist = audiomodel.train_model(args)
    assert np.isfinite(hist["loss"][0])
    out = json.loads((tmp_path / "ck" / "w" / "metadata.txt").read_text())
    want = tfdataset.get_weighting(counts)
    assert out["use_weighting"] is True and out["label_smoothing"] == 0.1
    assert out["class_weights"] == [float(w) for w in want], (out["class_weights"], want, counts)
    assert sum(counts) > 0 and min(want) >= 0.25


def test_trainer_rejects_bad_weights(cuda):
    for bad in (np.ones(CLASSES - 1), [1.0] * (CLASSES - 1) + [float("nan")], [-1.0] + [1.0] * (CLASSES - 1)):
        with pytest.raises(ValueError):
            _trainer(cuda, class_weights=bad)
    with pytest.raises(ValueError):
        _trainer(cuda, label_smoothing=1.0)
