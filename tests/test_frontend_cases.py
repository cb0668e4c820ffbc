"""CPU checks of oracle/frontend_cases.py, the case table that
tests/test_frontend_edges_gpu.py runs the HIP front end against: what the PCEN
input recipe promises (tie counts, the gap under the maximum), that every
gradient probe is live and that float32 noise of the reference stays under
half the GPU bound -- all on the reference alone -- plus the TF clamp-edge rule
of oracle.torch_ref.pcen_torch and a float64 restatement of the kernel's
one-pass backward, which must pass the per-probe bound and must fail it on
the matching probe once a defect is planted.

Measured: gap >= 2.2e-4 (the T == 1 shape and the gain 1.0 sets are the
smallest), s >= 1.25e-3 (the corner one-hot of (2, 33, 64)), float32 noise
<= 6.1e-4 * s (T == 1)."""
import numpy as np
import pytest
import torch

from oracle import frontend as of
from oracle import frontend_cases as fc
from oracle.torch_ref import pcen_torch

CASES = [(s, p) for s in fc.PCEN_SHAPES for p in fc.PCEN_PARAMS]
_id = lambda c: f"{c[0][0]}x{c[0][1]}x{c[0][2]}-{c[1]}"  # noqa: E731


def test_table_is_the_one_specified():
    assert fc.PCEN_SHAPES == [(3, 70, 40), (2, 33, 64), (1, 32, 64), (1, 31, 65), (2, 96, 13), (1, 1, 5),
                              (1, 513, 128)]
    assert sorted(fc.PCEN_PARAMS.values()) == sorted([
        (0.98, 2, 2, 0.04), (0.5, 1.5, 3, 0.2), (1.0, 2, 2, 0.04), (0.98, 2, 1.0, 0.04), (0.98, 2, 2, 1.0),
        (0.98, 2, 2, 0.0), (1.3, 2, 2, 0.04), (0.98, 2, 0.5, 0.04), (0.98, 2, 2, -0.1), (0.98, 2, 2, 1.5)])
    for shape in fc.PCEN_SHAPES:
        B, T, M = shape
        names = set(fc.pcen_douts(shape))
        want = {f"t{t}" for t in (0, 1, 7, 8, 31, 32, 33, 63, 64, T - 1) if t < T}
        want |= {f"row{r}" for r in (0, M - 1, M, 63, 64, B * M - 1) if r < B * M}
        assert names == want | {"corner", "full"}, shape


@pytest.mark.parametrize("shape", fc.PCEN_SHAPES, ids=str)
def test_input_recipe(shape):
    B, T, M = shape
    x = fc.pcen_input(shape)
    assert x.dtype == np.float32 and x.shape == shape and np.isfinite(x).all() and (x >= 0).all()
    big = np.sort(x.ravel())[::-1]
    t5 = min(5, T - 1)
    assert x[0, t5, 1] == big[0]
    if B > 1:
        assert np.array_equal(x[B - 1], x[0]) and big[1] == big[0] and big[2] * 64 <= big[0]
    else:
        assert big[1] * 64 <= big[0]
    if T == 1:
        assert (x > 0).all()
        return
    z = slice(T // 2, T // 2 + T // 8)
    assert (x[:, z] == 0).all()
    mz = fc.zero_row_mel(shape)
    assert (x[0, :, mz] == 0).all() and mz not in fc.probe_rows(shape)
    zf = fc.ZERO_FIRST_MEL
    assert x[0, 0, zf] == 0 and (x[0, 1:T // 2, zf] > 0).all() and zf != B * M - 1 and zf != mz
    # nothing else is zero
    live = np.ones(shape, bool)
    live[:, z] = False
    for b in {0, B - 1}:
        live[b, :, mz] = False
        live[b, 0, zf] = False
    assert (x[live] > 0).all()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_reference_conditions(case):
    shape, pname = case
    B, T, M = shape
    x = fc.pcen_input(shape)
    r64 = fc.pcen_reference(shape, pname)
    r32 = fc.pcen_reference(shape, pname, torch.float32)
    # tie counts as planted, in float64 and in float32
    nzero = max(int((x == 0).sum()), 1)
    y64 = r64["y"]
    y32 = pcen_y32(x, fc.PCEN_PARAMS[pname])
    for y in (y64, y32):
        assert (y == y.max()).sum() == (2 if B > 1 else 1)
        assert (y == y.min()).sum() == nzero
        if T > 1:
            assert y.min() == 0
    assert np.unravel_index(y64.argmax(), y64.shape) == np.unravel_index(y32.argmax(), y32.shape)
    ys = np.unique(y64)
    gap = (ys[-1] - ys[-2]) / (ys[-1] - ys[0])
    assert gap >= 1e-4, gap
    # every probe is live
    S, s = fc.probe_scales(r64["grads"])
    assert min(s.values()) >= 1e-3, s
    # float32 noise of the reference itself: at most half the GPU bound
    for k, (e, sk) in fc.probe_errors(r32["grads"], r64["grads"]).items():
        assert e <= 0.5 * fc.DPCEN_BOUND * sk, (k, e, sk)
    # a clamped parameter has no gradient at all; gain / root at 1.0 have
    assert np.abs(r64["out"] - of.pcen(x.astype(np.float64), **dict(zip(("gain", "bias", "root", "smooth"),
                                                                     fc.PCEN_PARAMS[pname]))).transpose(0, 2, 1)).max() < 1e-12
    if pname in fc.PCEN_CLAMPED:
        assert all(g[fc.PCEN_CLAMPED[pname]] == 0 for g in r64["grads"].values())
    if pname in ("gain=1", "root=1"):
        assert r64["grads"]["full"][0 if pname == "gain=1" else 2] != 0


def pcen_y32(x, params):
    """The un-normalised y in float32 (pcen_torch's own operations)."""
    g, b, r, w = (np.float32(v) for v in params)
    g, r, w = min(g, np.float32(1)), max(r, np.float32(1)), min(max(w, np.float32(0)), np.float32(1))
    x = np.asarray(x, np.float32)
    a = x[:, 0]
    out = np.empty_like(x)
    for t in range(x.shape[1]):
        a = w * x[:, t] + (np.float32(1) - w) * a
        out[:, t] = (x[:, t] / (np.float32(1e-6) + a) ** g + b) ** (np.float32(1) / r) - b ** (np.float32(1) / r)
    assert out.dtype == np.float32
    return out.transpose(0, 2, 1)


@pytest.mark.parametrize("shape", [(3, 70, 40), (1, 1, 5)], ids=str)
@pytest.mark.parametrize("pname", ["default", "gain=1", "smooth=0", "root<1"])
def test_forward_mode_equals_backward(shape, pname):
    """The Jacobian contraction the references use == loss.backward()."""
    x = torch.from_numpy(fc.pcen_input(shape)).double()
    ref = fc.pcen_reference(shape, pname)["grads"]
    for k, d in fc.pcen_douts(shape).items():
        p = torch.tensor(fc.PCEN_PARAMS[pname], dtype=torch.float64, requires_grad=True)
        (pcen_torch(x, p) * d).sum().backward()
        S = np.maximum(np.abs(ref[k]).max(), 1e-300)
        assert np.abs(p.grad.numpy() - ref[k]).max() <= 1e-9 * S, k


def _grad(params, x, d, **kw):
    p = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    (pcen_torch(x, p, **kw) * d).sum().backward()
    return p.grad.numpy()


def test_clamp_edges_follow_tf():
    """tf.minimum(gain, 1) / tf.maximum(root, 1): the whole gradient to the
    parameter at the tie (continuous from the inside), none beyond;
    clip_by_value(smooth, 0, 1) likewise on its closed interval."""
    # a plain positive input: with the recipe's zero-first-sample row the EMA
    # is ~smooth * x next to eps = 1e-6 and d/dsmooth bends within 1e-11 of 0
    rng = np.random.default_rng(3)
    x = torch.from_numpy(np.exp(rng.normal(0, 1, (2, 9, 4))))
    d = torch.from_numpy(rng.normal(0, 1, (2, 4, 9)))
    h = 1e-9
    base = [0.98, 2.0, 2.0, 0.04]
    for k, edge, inside, outside in ((0, 1.0, -h, 0.3), (2, 1.0, h, -0.5), (3, 1.0, -h, 0.5), (3, 0.0, h, -0.1)):
        at, near, out = list(base), list(base), list(base)
        at[k], near[k], out[k] = edge, edge + inside, edge + outside
        g_at, g_near, g_out = _grad(at, x, d)[k], _grad(near, x, d)[k], _grad(out, x, d)[k]
        assert g_at != 0 and abs(g_at - g_near) <= 1e-4 * abs(g_at), (k, edge, g_at, g_near)
        assert g_out == 0, (k, edge, g_out)
        # the other three gradients do not see the edge either
        o = [i for i in range(4) if i != k]
        ga = _grad(at, x, d)
        np.testing.assert_allclose(ga[o], _grad(near, x, d)[o], rtol=1e-4, atol=1e-6 * np.abs(ga).max())
    # torch.minimum would have halved it: minimum(p, 1) * 3 at p == 1 gives 1.5
    p = torch.ones((), dtype=torch.float64, requires_grad=True)
    (torch.minimum(p, torch.ones((), dtype=torch.float64)) * 3).backward()
    assert p.grad.item() == 1.5


def test_scope_means_constants():
    """scope_minmax replaces the extrema by constants: same output when it is
    the batch's own {mn, mx}, but no gradient through them."""
    shape = (2, 96, 13)
    x = torch.from_numpy(fc.pcen_input(shape)).double()
    p = torch.tensor(fc.PCEN_PARAMS["default"], dtype=torch.float64)
    y = fc.pcen_reference(shape, "default")["y"]
    a = pcen_torch(x, p)
    b = pcen_torch(x, p, scope_minmax=(float(y.min()), float(y.max())))
    assert (a - b).abs().max() < 1e-12
    d = fc.pcen_douts(shape)["full"]
    ga = _grad(fc.PCEN_PARAMS["default"], x, d)
    gb = _grad(fc.PCEN_PARAMS["default"], x, d, scope_minmax=(float(y.min()), float(y.max())))
    assert np.abs(ga - gb).max() > 1e-3 * np.abs(ga).max()


def _restated(shape, pname, defect=None):
    x = fc.pcen_input(shape)
    return {k: fc.pcen_bwd_restated(x, fc.PCEN_PARAMS[pname], d.numpy(), defect=defect)
            for k, d in fc.pcen_douts(shape).items()}


def _failing(shape, pname, defect):
    errs = fc.probe_errors(_restated(shape, pname, defect), fc.pcen_reference(shape, pname)["grads"])
    return {k for k, (e, s) in errs.items() if not e <= fc.DPCEN_BOUND * s}


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != (1, 513, 128)] + [((1, 513, 128), "default")], ids=_id)
def test_kernel_restatement_passes(case):
    """The kernel's formulation (forward-mode dEMA/dw, 14 accumulators, the
    finaliser's tie and clamp rules) is the gradient of pcen_torch."""
    assert _failing(*case, None) == set()


def test_planted_defects_are_caught():
    """Each defect fails on the probe that was put there for it."""
    # the last step of a partial chunk: the t = T - 1 column
    for shape in [(3, 70, 40), (2, 33, 64), (1, 31, 65), (1, 513, 128)]:
        bad = _failing(shape, "default", "last_step")
        assert f"t{shape[1] - 1}" in bad and "corner" in bad, (shape, bad)
    assert _failing((1, 32, 64), "default", "last_step") == set()  # no partial chunk there
    # the last row of a partial workgroup: the row B * M - 1 probe
    for shape in [(3, 70, 40), (1, 31, 65), (2, 96, 13)]:
        B, T, M = shape
        bad = _failing(shape, "default", "last_row")
        assert f"row{B * M - 1}" in bad and "corner" in bad, (shape, bad)
    assert _failing((2, 33, 64), "default", "last_row") == set()
    # half the gain gradient at 1.0: every probe of the boundary case
    for shape in fc.PCEN_SHAPES:
        assert "full" in _failing(shape, "gain=1", "half_gain"), shape
        assert _failing(shape, "default", "half_gain") == set()


# ---------------------------------------------------------------- mel tables

def test_mel_tables():
    w = fc.default_bank(32, 4096)
    assert fc.band_lengths(w).max() > 40
    assert fc.band_lengths(fc.default_bank(128, 4096)).max() <= 40  # why the production plan never got there
    c = fc.custom_bank_4096()
    st, ln, _ = of.mel_bands(c)
    assert (st[0], ln[0]) == (0, 1) and (st[127], ln[127]) == (2048, 1) and ln[5] == 0 and (st[64], ln[64]) == (0, 2049)
    # in the reference, the DC and the Nyquist row reach 1e-2 of the clip
    # maximum: a dropped bin cannot hide under the 2e-5 bound
    raw = fc.mel_clips().astype(np.float64)
    for power in (1, 2):
        for pad in ("end", "constant", "reflect"):
            ref = fc.mel_reference(raw, c, 4096, fc.HOP, power, pad)
            mx = ref.max((1, 2))
            assert (ref[:, 0].max(1) >= 1e-2 * mx).all() and (ref[:, 127].max(1) >= 1e-2 * mx).all(), (power, pad)
    # k_mel<NC>: at least one case per size with T % 4 != 0 (a partial last workgroup)
    for n_fft in (2048, 512, 256):
        ts = [of.num_frames_pad_end(n, hop) for f, _, n, hop in fc.small_fft_cases() if f == n_fft]
        ts += [1 + n // hop for f, _, n, hop in fc.small_fft_cases() if f == n_fft]
        assert any(t % 4 for t in ts), n_fft
        e = fc.small_bank(n_fft, "edge")
        st, ln, _ = of.mel_bands(e)
        assert (st[0], ln[0]) == (0, 1) and (st[-1], ln[-1]) == (n_fft // 2, 1) and ln[2] == 0
        for n in (n_fft // 2 + 1, 3 * n_fft + 7):
            ref = fc.mel_reference(fc.mel_clips(n).astype(np.float64), e, n_fft, fc.HOP, 2, "end")
            mx = ref.max((1, 2))
            assert (ref[:, 0].max(1) >= 1e-2 * mx).all() and (ref[:, -1].max(1) >= 1e-2 * mx).all(), (n_fft, n)
