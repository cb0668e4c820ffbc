"""Every leaf of the conv2d forward dispatch and every path of the weight
gradient (csrc/conv.hip), per element against float64.

The cases are oracle/conv_paths_cases.py's (shared with the host half,
tests/test_conv_paths_ref.py, which shows on the CPU that the bounds below
leave room for a correct kernel).  The C ABI is called directly
(acfe_conv2d_fwd, _fwd_dropout, _dgrad, _wgrad on ops.pack_weights packings),
not ops.conv2d, whose fused nodes route differently.

Every case first asserts, through the host-only queries acfe_conv2d_fwd_info /
acfe_conv2d_wgrad_info -- the launcher's own decision function --, that its
shape runs on the kernel it is there for: a dispatch change that moves a case
onto another kernel fails it instead of leaving it green on the wrong kernel.
No case skips.

Forward and stride-1 dgrad cases:
  * y lies in a buffer pre-filled with a sentinel byte, 256 guard bytes past
    its end: every element must have been written, the guard must be intact.
  * bf16: every element within 1 bf16 ulp of the exact value + 1e-4 (the
    project's bound, tests/test_production_gpu.py) of the float64 convolution
    of the same bf16 operands.  fp32: within (R S C + 2) 2^-24 (conv(|x|, |w|)
    + |b|), the worst case of fp32 accumulation.
  * x lies between two NaN regions of 4096 elements, so a read outside the
    tensor that reaches an output shows as NaN.
  * the statistics slab (acfe_conv2d_stats_rows rows, pre-filled with NaN, 4
    sentinel rows after it): every row finite (= written), the padded channels
    K .. Kp exactly zero in every row, the column sums equal to the float64
    sums and sums of squares of the STORED output to 1e-6, sentinel rows
    untouched.
  * acfe_conv2d_fwd_dropout (rate 0.1) with a slab and with stats = NULL:
    bit-equal to acfe_dropout of the plain output; the slab holds the sums of
    the dropped-out values.

Weight-gradient cases: dW pre-filled with NaN inside a guarded buffer, against
torch.nn.grad.conv2d_weight in float64 on the same operands: rel-L2 <= 5e-5,
max-relative <= 5e-4 (tests/test_wgrad_branches_gpu.py's bounds) and per
element (M + splits + 2) 2^-24 sum |x dy|; a second call with beta = 1 on top
of the first result equals dW + dW exactly.
"""
import math

import pytest
import torch

from oracle import conv_paths_cases as cc

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL, TAIL, XGUARD, SROWS = 0xA5, 256, 4096, 4
SLAB_SENTINEL = -12345.678
RATE, SEED = 0.1, 4242


@pytest.fixture(scope="module")
def env(cuda):
    from acfe import ops
    from acfe._lib import call, conv2d_fwd_info, conv2d_wgrad_info, lib
    from acfe._torch import ptr, stream

    return ops, call, lib, ptr, stream, conv2d_fwd_info, conv2d_wgrad_info


def _guarded(shape, dtype, device):
    """A tensor of `shape` whose storage carries TAIL sentinel bytes past its
    end (and sentinels inside, so an element never written shows too)."""
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + TAIL,), SENTINEL, dtype=torch.uint8, device=device)
    return raw, raw[:n].view(dtype).view(shape)


def _tail_intact(raw):
    return bool((raw[-TAIL:] == SENTINEL).all())


def _all_written(t):
    """No element of t still holds the sentinel fill."""
    it = torch.int16 if t.element_size() == 2 else torch.int32
    pat = torch.full((1,), SENTINEL, dtype=torch.uint8).repeat(t.element_size()).view(it).item()
    return int((t.view(it) == pat).sum()) == 0


def _between_nans(t, device):
    """t on the device with XGUARD NaN elements before and after it."""
    buf = torch.full((t.numel() + 2 * XGUARD,), float("nan"), dtype=t.dtype, device=device)
    view = buf[XGUARD:XGUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _slab(rows, Kp, device):
    st = torch.full((rows + SROWS, 2, Kp), float("nan"), dtype=F64, device=device)
    st[rows:] = SLAB_SENTINEL
    return st


def _assert_slab(st, rows, K, y, what):
    """The slab rows against the stored output y [..., K]."""
    s = st.cpu()
    assert bool((s[rows:] == SLAB_SENTINEL).all()), (what, "a row past the slab was written")
    assert bool(torch.isfinite(s[:rows]).all()), (what, "a slab row was not written")
    assert bool((s[:rows, :, K:] == 0).all()), (what, "padded channels of the slab not zero")
    t = y.detach().to(F64).cpu().reshape(-1, K)
    want = torch.stack([t.sum(0), (t * t).sum(0)])
    torch.testing.assert_close(s[:rows].sum(0)[:, :K], want, rtol=1e-6, atol=1e-6, msg=lambda m: f"{what}: {m}")


def _assert_values(c, y, exact, bound, what):
    g = y.detach().to(F64).cpu()
    assert bool(torch.isfinite(g).all()), (what, "not finite: a read outside x reached the output")
    err = (g - exact).abs()
    worst = float((err / bound).max())
    print(f"{what}: worst element error / bound {worst:.3f}")
    nbad = int((err > bound).sum())
    assert nbad == 0, (what, nbad, float(err.max()), worst)


@pytest.mark.parametrize("c", cc.FWD_CASES, ids=[c.id for c in cc.FWD_CASES])
def test_forward_path(env, cuda, c):
    ops, call, lib, ptr, stream, fwd_info, _ = env
    dt, code = cc.torch_dtype(c), 1 if c.dtype == "bf16" else 0
    geo = cc.call_geometry(c)
    N, H, W, C, K, R, S, st, pt, pl, P, Q = geo
    fwd = c.kind == "fwd"

    # the leaf, before anything is launched
    info = fwd_info(*geo, dtype=code, dropout=False, stats=fwd)
    want = dict(leaf=c.leaf, a=c.a, b=c.b, **c.expect)
    assert {k: info[k] for k in want} == want, (info, want)
    if fwd:
        for slab in (True, False):
            d = fwd_info(*geo, dtype=code, dropout=True, stats=slab)
            assert (d["leaf"], d["a"], d["b"]) == (c.leaf, c.a, c.b), (d, slab)

    inp, w, b = cc.fwd_operands(c)
    exact = cc.fwd_result(c, inp, w, b)
    bound = cc.bf16_bound(exact) if c.dtype == "bf16" else cc.f32_bound(c, inp, w, b)
    xbuf, x = _between_nans(inp, cuda)
    wd = w.to(cuda)
    wp = ops.pack_weights(wd, dt, not fwd)
    out_shape = (N, P, Q, K)
    raw, y = _guarded(out_shape, dt, cuda)

    if not fwd:
        call("acfe_conv2d_dgrad", ptr(x), c.N, c.P, c.Q, c.K, ptr(wp), c.C, c.R, c.S, 1, c.pt, c.pl, c.H, c.W,
             ptr(y), code, None, stream())
        torch.cuda.synchronize()
        assert _tail_intact(raw), (c.id, "wrote past the end of dx")
        assert _all_written(y), (c.id, "an element of dx was not written")
        _assert_values(c, y, exact, bound, c.id)
        return

    bd = b.to(cuda)
    rows, Kp = lib.acfe_conv2d_stats_rows(N * P * Q, K), wp.shape[0]
    assert Kp >= K and rows >= 1
    slab = _slab(rows, Kp, cuda)
    args = (ptr(x), N, H, W, C, ptr(wp), K, R, S, st, pt, pl, P, Q, ptr(bd))
    call("acfe_conv2d_fwd", *args, ptr(y), code, ptr(slab), stream())
    torch.cuda.synchronize()
    assert _tail_intact(raw), (c.id, "wrote past the end of y")
    assert _all_written(y), (c.id, "an element of y was not written")
    _assert_values(c, y, exact, bound, c.id)
    _assert_slab(slab, rows, K, y, c.id)

    # the fused Dropout: acfe_dropout's mask on the plain output, with and without a slab
    ref = torch.empty_like(y)
    call("acfe_dropout", ptr(y), y.numel(), RATE, SEED, ptr(ref), code, stream())
    for with_slab in (True, False):
        what = f"{c.id} dropout {'slab' if with_slab else 'no slab'}"
        rawd, yd = _guarded(out_shape, dt, cuda)
        slabd = _slab(rows, Kp, cuda)
        call("acfe_conv2d_fwd_dropout", *args, ptr(yd), code, ptr(slabd) if with_slab else None, RATE, SEED,
             stream())
        torch.cuda.synchronize()
        assert _tail_intact(rawd), (what, "wrote past the end of y")
        it = torch.int16 if code else torch.int32
        assert torch.equal(yd.view(it), ref.view(it)), (what, int((yd.view(it) != ref.view(it)).sum()))
        if with_slab:
            _assert_slab(slabd, rows, K, yd, what)
        else:
            s = slabd.cpu()
            assert bool(torch.isnan(s[:rows]).all()) and bool((s[rows:] == SLAB_SENTINEL).all()), what


@pytest.mark.parametrize("c", cc.WGRAD_CASES, ids=[c.id for c in cc.WGRAD_CASES])
def test_wgrad_path(env, cuda, c):
    ops, call, lib, ptr, stream, _, wgrad_info = env
    code = 1 if c.dtype == "bf16" else 0
    info = wgrad_info(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.st, c.P, c.Q, dtype=code)
    assert {k: info[k] for k in c.want} == c.want, (info, c.want)

    x, dy = cc.wgrad_operands(c)
    exact, mag = cc.wgrad_exact(c, x, dy)
    kd = c.R * c.S * c.C
    nws = lib.acfe_conv2d_wgrad_workspace(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.P, c.Q)
    splits = nws // (c.K * kd)  # the planned split count: no launch sums more partials
    if info["path"] == 0:
        assert splits == info["splits"]
    xbuf, xd = _between_nans(x, cuda)
    dbuf, dd = _between_nans(dy, cuda)
    ws = torch.full((nws,), float("nan"), device=cuda)
    raw, dw = _guarded((c.K, c.R, c.S, c.C), torch.float32, cuda)
    dw.fill_(float("nan"))
    args = (ptr(xd), c.N, c.H, c.W, c.C, ptr(dd), c.K, c.R, c.S, c.st, c.pt, c.pl, c.P, c.Q)
    call("acfe_conv2d_wgrad", *args, ptr(dw), 0.0, code, ptr(ws), stream())
    torch.cuda.synchronize()
    assert _tail_intact(raw), (c.id, "wrote past the end of dw")
    cc.assert_dw(dw, exact, mag, c.N * c.P * c.Q, splits, c.id)
    # beta = 1: a second call adds exactly the same gradient
    raw2, dw2 = _guarded((c.K, c.R, c.S, c.C), torch.float32, cuda)
    dw2.copy_(dw)
    call("acfe_conv2d_wgrad", *args, ptr(dw2), 1.0, code, ptr(ws), stream())
    torch.cuda.synchronize()
    assert _tail_intact(raw2), (c.id, "beta = 1 wrote past the end of dw")
    assert torch.equal(dw2, dw + dw), c.id
