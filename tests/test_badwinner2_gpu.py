"""badwinner2's whole forward on the GPU against the float64 restatement of
tests/bw2_reference.py.

Inputs: the fp32 mel of seeded chirp clips through FrontEnd(pcen=False,
dtype=float32), as predict.py feeds the model; weights seeded at the Keras
initialisers' scale, moving statistics near (0, 1) with spread
(bw2_reference.seed_model).

fp32: |p - p64| <= 4 e32 + 1e-6, e32 the float32 CPU restatement's own error
against float64: a factor 2 for another summation order over dot products of
up to 16 896 terms, a factor 2 for the hardware log2 / exp2 of the input
transform, which the restatement does not have.  bf16: |p - p64| <= 2 e_bf16 +
0.02, e_bf16 the error of the bf16-storage restatement (weights and every
stored activation rounded to bf16, arithmetic in float64): the rule of DESIGN
row a12.  The same rules hold for every stage's output (the model's `taps`),
each error taken relative to the stage's max |ref|, so a failure names the
layer.  To keep the bounds meaningful the restatements alone must give finite
outputs, e32 <= 1e-4, e_bf16 <= 0.1 and, for softmax, a largest probability
below 0.99.

Measured on an MI355X: probabilities fp32 <= 5.3e-7 (e32 <= 3.8e-7), bf16
<= 2.2e-3 (e_bf16 <= 2.2e-3).  The longest dot products, the (44, 3) / (22, 3)
128 -> 128 convolution's 16 896 / 8 448 terms, are summed in two levels by the
fp32 kernel (k_conv_fwd_g's LONGK variant, csrc/conv.hip): that stage is at
<= 1.2e-6 of its maximum against 1.3e-6 - 2.5e-6 for the float32 restatement.
As one accumulation chain it was at 4.4e-6 - 5.1e-6, and the 160 x 513
single-label case missed this file's rule at the pool behind it (5.11e-6
against 5.01e-6).
"""
import pytest
import torch

import bw2_reference as R

pytestmark = pytest.mark.gpu

LABELS = 7
SMALL = (96, 103, 3)
# (n_mels, frames, batch, cin, multi_label, lme)
CASES = [SMALL + (cin, ml, lme) for cin in (1, 3) for ml in (True, False) for lme in (False, True)]
CASES += [(96, 131, 2, 3, True, False), (96, 131, 2, 1, False, True),
          (160, 513, 1, 3, True, False), (160, 513, 1, 1, False, False)]
STAGES = ["mag_rownorm", "conv0", "conv1", "pool3x3", "conv2", "conv3", "condense", "pool5x3", "conv1x9", "conv1x1",
          "class"]

_cache = {}


def _case(cuda, M, T, B, cin, dtype):
    """The model on the device, its CPU state and the device mel (also on the CPU), shared by the cases of a geometry."""
    import badwinner2
    from acfe.train import FrontEnd

    key = ("model", M, T, B, cin, dtype)
    if key not in _cache:
        mkey = ("mel", M, T, B)
        if mkey not in _cache:
            clips = torch.from_numpy(R.chirp_clips(B, T, 1000 + M + T)).to(cuda)
            mel = FrontEnd(n_mels=M, pcen=False, dtype=torch.float32, device=cuda)(clips, pad_mode="constant")
            assert mel.shape == (B, M, T) and mel.dtype == torch.float32
            _cache[mkey] = (mel, mel.cpu())
        model = R.seed_model(badwinner2.build_model((M, T, cin), None, LABELS, dtype=dtype), 50 + M + T + cin).eval()
        _cache[key] = (model.to(cuda), R.state_of(model)) + _cache[mkey]
    return _cache[key]


def _reference(sd, mel_cpu, key, mode, ml, lme):
    k = ("ref", key, mode, ml, lme)
    if k not in _cache:
        taps = []
        p = R.forward(sd, mel_cpu, mode, ml, lme, taps)
        _cache[k] = (p, taps)
    return _cache[k]


def _stage_names(lme):
    return STAGES + (["lme_h", "lme_w"] if lme else []) + ["logits"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=["{}x{}-b{}-cin{}-ml{:d}-lme{:d}".format(*c) for c in CASES])
def test_forward(cuda, case, dtype):
    M, T, B, cin, ml, lme = case
    model, sd, mel, mel_cpu = _case(cuda, M, T, B, cin, dtype)
    model.multi_label, model.lme = ml, lme
    key = (M, T, B, cin)
    p64, t64 = _reference(sd, mel_cpu, key, "f64", ml, lme)
    mode = "f32" if dtype == torch.float32 else "bf16"
    pm, tm = _reference(sd, mel_cpu, key, mode, ml, lme)

    # the reference alone: the bounds must mean something
    assert bool(torch.isfinite(p64).all()) and bool(torch.isfinite(pm).all())
    e_ref = float((pm - p64).abs().max())
    assert e_ref <= (1e-4 if mode == "f32" else 0.1), e_ref
    if not ml:
        assert float(p64.max()) < 0.99
        assert float((p64.sum(1) - 1).abs().max()) < 1e-12

    def bound(e):
        return 4 * e + 1e-6 if mode == "f32" else 2 * e + 0.02

    taps = []
    p = model.activation(model(mel, taps=taps))
    torch.cuda.synchronize()
    names = _stage_names(lme)
    assert len(taps) == len(t64) == len(tm) == len(names)
    lines = []
    for name, t, r64, rm in zip(names, taps, t64, tm):
        got = t.double().cpu()
        assert got.shape == r64.shape, (name, got.shape, r64.shape)
        assert bool(torch.isfinite(got).all()), name
        mx = float(r64.abs().max())
        e_stage, e_got = float((rm - r64).abs().max()) / mx, float((got - r64).abs().max()) / mx
        lines.append(f"{name} {e_got:.2e}/{e_stage:.2e}")
        assert e_got <= bound(e_stage), (name, e_got, e_stage, bound(e_stage))
    err = float((p.double().cpu() - p64).abs().max())
    print(f"{mode} {case}: probabilities {err:.2e} (restatement {e_ref:.2e}); stages got/restatement: " + ", ".join(lines))
    assert p.shape == (B, LABELS) and p.dtype == torch.float32
    assert err <= bound(e_ref), (err, e_ref, bound(e_ref))
    if not ml:
        assert float((p.sum(1) - 1).abs().max()) < 1e-5


def test_eval_only_and_input_checks(cuda):
    model, sd, mel, _ = _case(cuda, *SMALL, 1, torch.bfloat16)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="eval mode only"):
            model(mel)
    finally:
        model.eval()
    with pytest.raises(ValueError):
        model(mel[:, :, :102].contiguous())
    with pytest.raises(ValueError):
        model(mel.to(torch.bfloat16))
    # the cached BN affines follow a parameter change
    a = model(mel)
    keep = model.bns[6].beta.detach().clone()
    with torch.no_grad():
        model.bns[6].beta.add_(0.5)
    b = model(mel)
    with torch.no_grad():
        model.bns[6].beta.copy_(keep)
    assert not torch.equal(a, b)
    assert torch.equal(model(mel), a)
