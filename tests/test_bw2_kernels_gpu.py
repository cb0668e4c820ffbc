"""The three kernels of csrc/bw2.hip against float64, at their path edges.

acfe_mag_rownorm: y = (x^sigmoid(a) - mean[m]) / sqrt(var[m] + eps) over
[B][M][T].  fp32 bound: 5e-5 of the per-clip maximum of |y|, the bound DESIGN
row a9 gives PCEN's forward, which forms its powers the same way (hardware
log2 / exp2); bf16: that plus one bf16 rounding (2^-8 |y|).  A zero input gives
exactly the rounded -mean * inv, inv = 1 / sqrt(var + eps) rounded to float32.  Rows
of 103, 131, 1, 64 and 65 floats and a base pointer off the 16-B grid put
groups of four across row ends and exercise the scalar head and tail.

acfe_leaky_bn: y = scale[c] * leaky(x) + shift[c].  Bound per element:
2^-23 (|scale l| + |shift|) for the fp32 arithmetic plus one rounding of the
output dtype (2^-24 |y| fp32, 2^-8 |y| bf16).  C = 64 and 1024 take the 16-B
path, C = 3, 7, 50 and any base pointer off by one element the scalar one.

acfe_softmax: error against float64 at most 4 x the error of torch.softmax in
float32 on the CPU, plus 1e-7 (the kernel sums in another order and takes its
exponentials from the hardware); rows sum to 1 within that bound times L.

Every output lies in a sentinel-filled buffer with guard bytes after it.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL, TAIL = 0xA5, 256
EPS = 1e-3


def _guarded(numel, dtype, device, offset=0):
    """A flat tensor of numel elements starting `offset` elements into a
    sentinel-filled buffer, TAIL guard bytes behind it -> (raw bytes, tensor)."""
    sz = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((offset + numel) * sz + TAIL,), SENTINEL, dtype=torch.uint8, device=device)
    return raw, raw[offset * sz:(offset + numel) * sz].view(dtype)


def _guards_intact(raw, numel, dtype, offset=0):
    sz = torch.empty((), dtype=dtype).element_size()
    return bool((raw[:offset * sz] == SENTINEL).all()) and bool((raw[(offset + numel) * sz:] == SENTINEL).all())


def _offset_copy(t, device, offset):
    """t on the device, `offset` elements past a 16-B aligned address."""
    buf = torch.empty(t.numel() + offset + 8, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def _round_rel(dtype):
    return 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -8


# ---------------------------------------------------------------- mag_rownorm
MAG_SHAPES = [(1, 96, 103), (2, 160, 131), (3, 5, 1), (2, 96, 64), (2, 96, 65)]


def _mag_inputs(B, M, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.pow(10.0, torch.rand((B, M, T), generator=g, dtype=F64) * 16 - 12).float()
    x[torch.rand((B, M, T), generator=g) < 0.05] = 0.0
    x.view(-1)[0] = 0.0
    mean = torch.rand(M, generator=g) * 0.8 + 0.05
    var = torch.rand(M, generator=g) * 0.5 + 0.01
    return x, mean, var


# (x, y) element offsets from a 16-B aligned address: head + groups of four + tail when both
# agree, everything scalar when y's groups would not be aligned
@pytest.mark.parametrize("offset", [(0, 0), (1, 1), (3, 3), (0, 1)], ids=["aligned", "off1", "off3", "y-off1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", MAG_SHAPES, ids=["x".join(map(str, s)) for s in MAG_SHAPES])
def test_mag_rownorm(cuda, shape, dtype, offset):
    from acfe._lib import call
    from acfe._torch import dtype_code, ptr, stream

    B, M, T = shape
    x, mean, var = _mag_inputs(B, M, T, 7 * B + M + T)
    xoff, yoff = offset
    xbuf, xd = _offset_copy(x, cuda, xoff)
    md, vd = mean.to(cuda), var.to(cuda)
    # 1 / sqrt(var + eps) in float64 (eps the float32 the call passes), rounded once to float32
    inv32 = (1.0 / torch.sqrt(var.to(F64) + torch.tensor(EPS, dtype=torch.float32).to(F64))).float()
    zero_want = ((0.0 - mean) * inv32).to(dtype)
    worst = 0.0
    for a in (-2.0, -1.0, 0.0, 1.0):
        ad = torch.tensor([a], device=cuda)
        raw, y = _guarded(x.numel(), dtype, cuda, offset=yoff)
        call("acfe_mag_rownorm", ptr(xd), B, M, T, ptr(ad), ptr(md), ptr(vd), EPS, ptr(y), dtype_code(dtype),
             stream())
        torch.cuda.synchronize()
        assert _guards_intact(raw, x.numel(), dtype, yoff), (shape, a, "wrote outside y")
        got = y.view(B, M, T).cpu()
        p = 1.0 / (1.0 + math.exp(-a))
        ref = (x.to(F64) ** p - mean.to(F64)[None, :, None]) / torch.sqrt(var.to(F64)[None, :, None] + EPS)
        assert bool(torch.isfinite(got.float()).all())
        clipmax = ref.abs().amax((1, 2), keepdim=True)
        bound = 5e-5 * clipmax + (ref.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
        err = (got.to(F64) - ref).abs()
        worst = max(worst, float((err / clipmax).max()))
        assert int((err > bound).sum()) == 0, (shape, a, float((err / bound).max()))
        # 0^p = 0: exactly the rounded -mean * (1 / sqrt(var + eps))
        zm = x == 0
        want = zero_want[None, :, None].expand(B, M, T)
        assert torch.equal(got[zm].float(), want[zm].float()), (shape, a, "zero input")
    print(f"mag_rownorm {shape} {dtype} offset {offset}: worst error / clip max {worst:.3e}")


def test_mag_rownorm_negative_and_invalid(cuda):
    """A negative input does not fault (its value is unspecified); bad
    arguments are ACFE_E_INVAL."""
    from acfe._lib import E_INVAL, lib
    from acfe._torch import ptr, stream

    x = torch.tensor([[[-1.0, 2.0, 0.0, 4.0, -0.5]]], device=cuda)
    a, m, v = torch.zeros(1, device=cuda), torch.zeros(1, device=cuda), torch.ones(1, device=cuda)
    y = torch.empty_like(x)
    args = (ptr(a), ptr(m), ptr(v), EPS, ptr(y), 0, stream())
    assert lib.acfe_mag_rownorm(ptr(x), 1, 1, 5, *args) == 0
    torch.cuda.synchronize()
    got = y.cpu().view(-1)
    inv = 1.0 / math.sqrt(1.0 + EPS)
    assert abs(float(got[1]) - math.sqrt(2.0) * inv) < 1e-5 and abs(float(got[3]) - 2.0 * inv) < 1e-5
    assert lib.acfe_mag_rownorm(None, 1, 1, 5, *args) == E_INVAL
    assert lib.acfe_mag_rownorm(ptr(x), 1, 0, 5, *args) == E_INVAL
    assert lib.acfe_mag_rownorm(ptr(x), 1, 1, 0, *args) == E_INVAL
    assert lib.acfe_mag_rownorm(ptr(x), 1, 1, 5, ptr(a), ptr(m), ptr(v), EPS, ptr(y), 7, stream()) == E_INVAL


# ---------------------------------------------------------------- leaky_bn
ALPHA = 0.01


def _leaky_case(rows, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((rows, C), generator=g) * 3).to(dtype)
    scale = torch.rand(C, generator=g) * 2 + 0.2
    scale[::3] *= -1
    shift = torch.randn(C, generator=g)
    return x, scale, shift


def _leaky_check(got, x, scale, shift, dtype, what):
    xd = x.to(F64)
    a32 = torch.tensor(ALPHA, dtype=torch.float32).to(F64)
    l = torch.where(xd > 0, xd, a32 * xd)
    if scale is None:
        ref, mag = l, l.abs()
    else:
        ref = scale.to(F64) * l + shift.to(F64)
        mag = (scale.to(F64) * l).abs() + shift.to(F64).abs()
    bound = 2.0 ** -23 * mag + _round_rel(dtype) * ref.abs()
    err = (got.cpu().to(F64) - ref).abs()
    nbad = int((err > bound).sum())
    assert nbad == 0, (what, nbad, float((err / bound.clamp_min(1e-300)).max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 1000])
@pytest.mark.parametrize("C", [3, 7, 50, 64, 1024])
def test_leaky_bn(cuda, C, rows, dtype):
    from acfe._lib import call
    from acfe._torch import dtype_code, ptr, stream

    x, scale, shift = _leaky_case(rows, C, dtype, 31 * C + rows)
    sd, hd = scale.to(cuda), shift.to(cuda)
    code, n = dtype_code(dtype), rows * C
    for offset in (0, 1):  # one element off the 16-B grid forces the scalar kernel
        for affine in (True, False):
            what = (C, rows, str(dtype), offset, affine)
            xbuf, xd = _offset_copy(x, cuda, offset)
            raw, y = _guarded(n, dtype, cuda, offset=offset)
            call("acfe_leaky_bn", ptr(xd), rows, C, ALPHA, ptr(sd) if affine else None, ptr(hd) if affine else None,
                 ptr(y), code, stream())
            torch.cuda.synchronize()
            assert _guards_intact(raw, n, dtype, offset), (what, "wrote outside y")
            _leaky_check(y.view(rows, C), x, scale if affine else None, shift if affine else None, dtype, what)
            # in place: the same bits
            raw2, y2 = _guarded(n, dtype, cuda, offset=offset)
            y2.copy_(xd.view(-1))
            call("acfe_leaky_bn", ptr(y2), rows, C, ALPHA, ptr(sd) if affine else None,
                 ptr(hd) if affine else None, ptr(y2), code, stream())
            torch.cuda.synchronize()
            assert _guards_intact(raw2, n, dtype, offset), (what, "in place wrote outside y")
            it = torch.int16 if dtype == torch.bfloat16 else torch.int32
            assert torch.equal(y2.view(it), y.view(it)), (what, "in place differs")


def test_leaky_bn_invalid(cuda):
    from acfe._lib import E_INVAL, lib
    from acfe._torch import ptr, stream

    x = torch.zeros(8, device=cuda)
    s = torch.ones(8, device=cuda)
    assert lib.acfe_leaky_bn(None, 1, 8, ALPHA, None, None, ptr(x), 0, stream()) == E_INVAL
    assert lib.acfe_leaky_bn(ptr(x), 1, 8, ALPHA, ptr(s), None, ptr(x), 0, stream()) == E_INVAL
    assert lib.acfe_leaky_bn(ptr(x), 1, 0, ALPHA, None, None, ptr(x), 0, stream()) == E_INVAL
    assert lib.acfe_leaky_bn(ptr(x), 1, 8, ALPHA, None, None, ptr(x), 5, stream()) == E_INVAL
    assert lib.acfe_leaky_bn(ptr(x), 0, 8, ALPHA, None, None, ptr(x), 0, stream()) == 0


# ---------------------------------------------------------------- softmax
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 50, 257, 4096])
def test_softmax(cuda, L, B):
    from acfe import ops

    g = torch.Generator().manual_seed(100 * L + B)
    z = (torch.rand((B, L), generator=g) * 160 - 80).float()
    z[0, 0] = 80.0
    z[-1, -1] = -80.0
    if L > 2:
        z[0, 1] = 79.5  # two large terms share the mass
    ref = torch.softmax(z.to(F64), 1)
    e_torch = float((torch.softmax(z, 1).to(F64) - ref).abs().max())
    bound = 4 * e_torch + 1e-7
    raw, p = _guarded(B * L, torch.float32, cuda)
    zd = z.to(cuda)
    from acfe._lib import call
    from acfe._torch import ptr, stream

    call("acfe_softmax", ptr(zd), B, L, ptr(p), stream())
    torch.cuda.synchronize()
    assert _guards_intact(raw, B * L, torch.float32), "wrote outside p"
    got = p.view(B, L).cpu().to(F64)
    assert bool(torch.isfinite(got).all()) and bool((got >= 0).all())
    err = float((got - ref).abs().max())
    print(f"softmax L {L} B {B}: error {err:.3e}, torch float32 {e_torch:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    assert float((got.sum(1) - 1).abs().max()) <= bound * L
    assert torch.equal(ops.softmax(zd).cpu(), p.view(B, L).cpu())
