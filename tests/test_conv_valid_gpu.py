"""acfe_conv2d_fwd at the "valid" (pad 0, stride 1) geometries of badwinner2
(badwinner2.py:235-302), per element against the float64 convolution of the
rounded operands, bf16 and fp32.

The shapes are the model's layers shrunk to the smallest size that keeps their
tiling edges: partial 4-row and 64-pixel tiles of the row-tile family, the 22-
and 44-row condensing filters, the (1, 9) filter at Q = 1, the 1x1 convolutions
at one pixel, the one- and three-channel first convolution.  Operands, the
float64 reference and both bounds are those of tests/test_conv_paths_gpu.py
(oracle/conv_paths_cases.py): bf16 within 1 bf16 ulp of the exact value + 1e-4,
fp32 within (R S C + 2) 2^-24 (conv(|x|, |w|) + |b|).  As the model does, the
call passes no statistics slab.  y is sentinel-guarded, x lies between NaNs.

The bf16 3x3 cases with C % 64 == 0 must be on the `rows` leaf
(acfe_conv2d_fwd_info), the leaf the model runs them on.
"""
import math

import pytest
import torch

from oracle import conv_paths_cases as cc

pytestmark = pytest.mark.gpu

SENTINEL, TAIL, XGUARD = 0xA5, 256, 4096

# (id, H, W, C, K, R, S)
_SHAPES = [
    ("3x3-64to64-20x70", 20, 70, 64, 64, 3, 3),
    ("3x3-64to128-11x70", 11, 70, 64, 128, 3, 3),
    ("3x3-128to128-11x70", 11, 70, 128, 128, 3, 3),
    ("22x3-128to128-26x29", 26, 29, 128, 128, 22, 3),
    ("44x3-128to128-48x9", 48, 9, 128, 128, 44, 3),
    ("1x9-128to1024-1x9", 1, 9, 128, 1024, 1, 9),
    ("1x9-128to1024-1x54", 1, 54, 128, 1024, 1, 9),
    ("1x1-1024to1024-1x1", 1, 1, 1024, 1024, 1, 1),
    ("1x1-1024to1024-1x46", 1, 46, 1024, 1024, 1, 1),
    ("1x1-1024to7-1x1", 1, 1, 1024, 7, 1, 1),
    ("1x1-1024to7-1x46", 1, 46, 1024, 7, 1, 1),
    ("3x3-1to64-12x37", 12, 37, 1, 64, 3, 3),
    ("3x3-3to64-12x37", 12, 37, 3, 64, 3, 3),
]
CASES = [cc._fwd(f"{i}-{dt}", 2, H, W, C, K, None, 0, R=R, S=S, pad="valid", dtype=dt)
         for i, H, W, C, K, R, S in _SHAPES for dt in ("bf16", "f32")]


def _guarded(shape, dtype, device):
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + TAIL,), SENTINEL, dtype=torch.uint8, device=device)
    return raw, raw[:n].view(dtype).view(shape)


def _all_written(t):
    it = torch.int16 if t.element_size() == 2 else torch.int32
    pat = torch.full((1,), SENTINEL, dtype=torch.uint8).repeat(t.element_size()).view(it).item()
    return int((t.view(it) == pat).sum()) == 0


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_valid_forward(cuda, c):
    from acfe import ops
    from acfe._lib import call, conv2d_fwd_info
    from acfe._torch import ptr, stream

    dt, code = cc.torch_dtype(c), 1 if c.dtype == "bf16" else 0
    geo = cc.call_geometry(c)
    N, H, W, C, K, R, S, st, pt, pl, P, Q = geo
    assert (pt, pl, st, P, Q) == (0, 0, 1, H - R + 1, W - S + 1)
    info = conv2d_fwd_info(*geo, dtype=code, dropout=False, stats=False)
    assert info is not None, "the dispatch refuses the geometry"
    print(f"{c.id}: leaf {info['leaf']} a {info['a']} b {info['b']}")
    if c.dtype == "bf16" and (R, S) == (3, 3) and C % 64 == 0:
        assert (info["leaf"], info["a"]) == ("rows", K), info

    inp, w, b = cc.fwd_operands(c)
    exact = cc.fwd_result(c, inp, w, b)
    bound = cc.bf16_bound(exact) if c.dtype == "bf16" else cc.f32_bound(c, inp, w, b)
    buf = torch.full((inp.numel() + 2 * XGUARD,), float("nan"), dtype=dt, device=cuda)
    x = buf[XGUARD:XGUARD + inp.numel()].view(inp.shape)
    x.copy_(inp)
    wp = ops.pack_weights(w.to(cuda), dt, False)
    bd = b.to(cuda)
    raw, y = _guarded((N, P, Q, K), dt, cuda)
    call("acfe_conv2d_fwd", ptr(x), N, H, W, C, ptr(wp), K, R, S, st, pt, pl, P, Q, ptr(bd), ptr(y), code, None,
         stream())
    torch.cuda.synchronize()
    assert bool((raw[-TAIL:] == SENTINEL).all()), (c.id, "wrote past the end of y")
    assert _all_written(y), (c.id, "an element of y was not written")
    g = y.to(torch.float64).cpu()
    assert bool(torch.isfinite(g).all()), (c.id, "not finite: a read outside x reached the output")
    err = (g - exact).abs()
    worst = float((err / bound).max())
    print(f"{c.id}: worst element error / bound {worst:.3f}")
    nbad = int((err > bound).sum())
    assert nbad == 0, (c.id, nbad, float(err.max()), worst)
