"""Case tables of the per-element convolution path tests
(tests/test_conv_paths_gpu.py on the GPU, tests/test_conv_paths_ref.py on the
host): one entry per leaf of the forward dispatch (fwd_pick in csrc/conv.hip,
asked through acfe_conv2d_fwd_info) and per path of acfe_conv2d_wgrad
(acfe_conv2d_wgrad_info), with the float64 references and the bounds both
files share.

Test infrastructure only (see oracle/__init__.py).

A forward case is a convolution x[N, H, W, C] -> y[N, P, Q, K] with an R x S
filter, a stride and top / left pads; kind "dgrad" is the stride-1
acfe_conv2d_dgrad of such a convolution: dY[N, P, Q, K] -> dX[N, H, W, C],
which the library runs as the forward call (N, P, Q, K -> C, R, S, 1,
R-1-pad_top, S-1-pad_left, H, W) on the flipped weights -- `call_geometry`
gives the geometry the dispatch sees.  `leaf`, `a`, `b` (and `expect`: further
fields of the query that name the edge the case is there for) are what the
case must reach; they were checked by hand against the launcher's code.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

F64 = torch.float64
BF = torch.bfloat16

Fwd = namedtuple("Fwd", "id kind dtype N H W C K R S st pt pl P Q leaf a b expect")
Wg = namedtuple("Wg", "id dtype N H W C K R S st pt pl P Q want")


def same_geometry(H, W, R, S, st):
    """TF "same": P = ceil(H / st), pad_total = max((P - 1) st + R - H, 0), top = total // 2."""
    P, Q = -(-H // st), -(-W // st)
    return max((P - 1) * st + R - H, 0) // 2, max((Q - 1) * st + S - W, 0) // 2, P, Q


def valid_geometry(H, W, R, S, st):
    return 0, 0, (H - R) // st + 1, (W - S) // st + 1


def _fwd(id_, N, H, W, C, K, leaf, a, b=0, R=3, S=3, st=1, pad="same", dtype="bf16", kind="fwd", expect=None):
    pt, pl, P, Q = (same_geometry if pad == "same" else valid_geometry)(H, W, R, S, st)
    return Fwd(id_, kind, dtype, N, H, W, C, K, R, S, st, pt, pl, P, Q, leaf, a, b, expect or {})


def _one(id_, N, H, W, C, K, ncs, nkb, **kw):
    return _fwd(id_, N, H, W, C, K, "1x1_reg", ncs, nkb, R=1, S=1, **kw)


FWD_CASES = [
    # ---- k_conv1x1_reg<NCS, NKB>: all eight instantiations
    _one("1x1-11-k4-quadmask", 3, 5, 7, 8, 4, 1, 1),
    # 263169 px > 2048 workgroups x 128 px: a second round of the grid-stride loop, partial last block
    _one("1x1-11-513-round2", 1, 513, 513, 16, 16, 1, 1, expect=dict(grid_x=2048, tiles=16449)),
    _one("1x1-12-k20", 2, 9, 13, 16, 20, 1, 2),
    # M = 15: one partial block, three waves of the workgroup without a block
    _one("1x1-14-m15", 1, 3, 5, 16, 64, 1, 4, expect=dict(grid_x=1, tiles=1)),
    _one("1x1-14-513-round2", 1, 513, 513, 16, 64, 1, 4, expect=dict(grid_x=2048, tiles=16449)),
    _one("1x1-18-m126", 2, 7, 9, 32, 128, 1, 8, expect=dict(tiles=8)),
    _one("1x1-21", 3, 5, 7, 64, 16, 2, 1),
    _one("1x1-22-c40", 2, 9, 13, 40, 24, 2, 2),
    _one("1x1-41-c104", 2, 9, 13, 104, 8, 4, 1),
    _one("1x1-42", 3, 5, 7, 128, 32, 4, 2),
    # ---- its fall-through neighbours: shapes that look like k_conv1x1_reg's
    _fwd("1x1-fall-32to96-nkb6", 2, 9, 13, 32, 96, "g", 128, R=1, S=1),
    _fwd("1x1-fall-16to100-ragged-wide", 2, 9, 13, 16, 100, "g", 128, R=1, S=1),
    _fwd("1x1-fall-96to16-ncs3", 2, 9, 13, 96, 16, "g", 32, R=1, S=1),
    _fwd("1x1-fall-32to48-nkb3", 2, 9, 13, 32, 48, "g", 64, R=1, S=1),
    # ---- k_conv3x3_c16 (16 -> 64, 8 x 64 tiles)
    _fwd("c16-ragged-row-and-pixel", 3, 9, 65, 16, 64, "c16", 0, expect=dict(tiles=12)),
    _fwd("c16-exact-tile", 1, 8, 64, 16, 64, "c16", 0, expect=dict(tiles=1, grid_x=1)),
    # 260 tiles against 46 slab rows: several tiles per workgroup, the grid capped at the slab
    _fwd("c16-260tiles-46rows", 130, 9, 5, 16, 64, "c16", 0, expect=dict(tiles=260, grid_x=46)),
    # ---- k_conv_fwd_p<BN> (256-pixel M tiles, 3-stage pipeline over K tiles of 64)
    _fwd("p-1x1-nkt1-3images", 3, 5, 7, 64, 64, "p", 64, R=1, S=1, expect=dict(tiles=1, grid_x=1, grid_y=1)),
    _fwd("p-1x1-nkt2-2ntiles", 2, 9, 31, 128, 256, "p", 128, R=1, S=1, expect=dict(tiles=3, grid_x=3, grid_y=2)),
    _fwd("p-1x1-130tiles-128wgs", 1, 129, 257, 64, 256, "p", 128, R=1, S=1,
         expect=dict(tiles=130, grid_x=128, grid_y=2)),
    _fwd("p-3x3-k256", 2, 6, 37, 64, 256, "p", 128, expect=dict(grid_y=2)),
    _fwd("p-3x3-s2-same-pt1-pl0", 2, 9, 12, 64, 128, "p", 128, st=2),
    _fwd("p-3x3-s3-valid", 2, 11, 13, 128, 256, "p", 128, st=3, pad="valid"),
    _fwd("p-1x1-s2-valid", 2, 9, 12, 64, 128, "p", 128, R=1, S=1, st=2, pad="valid"),
    _fwd("p-4x10-40taps", 2, 5, 12, 64, 128, "p", 128, R=4, S=10),
    _fwd("p-4x10-c256", 1, 16, 32, 256, 128, "p", 128, R=4, S=10, expect=dict(tiles=2)),
    _fwd("p-4x10-dgrad-128to256-pt2-pl5", 2, 5, 12, 256, 128, "p", 128, R=4, S=10, kind="dgrad"),
    # ---- k_conv_fwd_g<T, 128, BN>
    _fwd("g-24to32-kdp256", 2, 7, 9, 24, 32, "g", 32),
    _fwd("g-24to64", 2, 7, 9, 24, 64, "g", 64),
    _fwd("g-64to96-padded-k", 2, 7, 9, 64, 96, "g", 128),
    _fwd("g-64to192-two-ntiles", 2, 7, 9, 64, 192, "g", 128, expect=dict(grid_y=2)),
    _fwd("g-cw-shape-valid", 2, 9, 12, 32, 128, "g", 128, pad="valid"),
    _fwd("g-narrow-shape-ck8192", 2, 7, 9, 256, 32, "g", 32),
    # 8255 px = 65 tiles on a 64-workgroup XCD-chunked walk
    _fwd("g-65tiles-64wgs", 1, 65, 127, 8, 32, "g", 32, expect=dict(tiles=65, grid_x=64)),
    _fwd("g-f32-32to20-chunk-major", 2, 7, 9, 32, 20, "g", 32, dtype="f32"),
    _fwd("g-f32-20to64-tap-major", 2, 7, 9, 20, 64, "g", 64, dtype="f32"),
    _fwd("g-f32-64to128-chunk-major", 2, 7, 9, 64, 128, "g", 128, dtype="f32"),
    _fwd("g-f32-s2-same", 2, 9, 12, 64, 128, "g", 128, st=2, dtype="f32"),
    _fwd("g-f32-4x10", 1, 5, 12, 64, 128, "g", 128, R=4, S=10, dtype="f32"),
    # ---- k_conv_fwd<T, 128, BN, false>: a load granule straddles filter taps
    _fwd("generic-4to32", 2, 7, 9, 4, 32, "generic", 32),
    _fwd("generic-50to64", 2, 7, 9, 50, 64, "generic", 64),
    _fwd("generic-5x5-valid-1to16", 2, 9, 11, 1, 16, "generic", 32, R=5, S=5, pad="valid"),
    _fwd("generic-f32-3to16", 2, 7, 9, 3, 16, "generic", 32, dtype="f32"),
    _fwd("generic-f32-50to64", 2, 7, 9, 50, 64, "generic", 64, dtype="f32"),
    _fwd("generic-f32-1x1-50to50", 2, 7, 9, 50, 50, "generic", 64, R=1, S=1, dtype="f32"),
]


def _rows_cases():
    """The 3x3 row-tile family at pads 0 ("valid" forward) and 2 (its dgrad):
    the dispatch takes any 3x3 stride-1 conv with C % 64 == 0 and K = 64 / 128
    without looking at the pads.  The dgrad of 192 -> 64 has 192 output
    channels, which no row-tile kernel serves: the dispatch gives it to
    k_conv_fwd_g (K % 128 != 0 rules k_conv_fwd_p out)."""
    out = []
    for N, H, W in ((3, 10, 70), (2, 6, 20)):
        for C, K in ((64, 64), (128, 64), (128, 128), (64, 128), (192, 64)):
            tag = f"{N}x{H}x{W}-{C}to{K}"
            out.append(_fwd(f"rows-valid-{tag}", N, H, W, C, K, "rows", K, pad="valid"))
            if C == 192:
                out.append(_fwd(f"rows-valid-dgrad-{tag}-is-g", N, H, W, C, K, "g", 128, pad="valid", kind="dgrad"))
            else:
                out.append(_fwd(f"rows-valid-dgrad-{tag}", N, H, W, C, K, "rows", C, pad="valid", kind="dgrad"))
    return out


FWD_CASES += _rows_cases()


def _wg(id_, N, H, W, C, K, want, R=3, S=3, st=1, pad="same", dtype="bf16"):
    pt, pl, P, Q = (same_geometry if pad == "same" else valid_geometry)(H, W, R, S, st)
    return Wg(id_, dtype, N, H, W, C, K, R, S, st, pt, pl, P, Q, want)


def _p0(bmw, fd, fx, **kw):
    return dict(path=0, bmw=bmw, fast_d=fd, fast_x=fx, **kw)


WGRAD_CASES = [
    # ---- path 0: k_conv_wgrad<T, BMW, FAST_D, FAST_X> + k_wgrad_reduce[_g]
    # M = 126: one live split, seven empty ones that must contribute zeros
    _wg("w0-4to32-fd1-fx0-7empty", 2, 7, 9, 4, 32, _p0(32, 1, 0, splits=8, chunk=512, reduce=0)),
    _wg("w0-50to50-fd0-fx0-bmw64", 2, 7, 9, 50, 50, _p0(64, 0, 0)),
    _wg("w0-24to20-fd0-fx1-bmw32", 2, 7, 9, 24, 20, _p0(32, 0, 1)),
    _wg("w0-s2-same-64to128", 2, 17, 30, 64, 128, _p0(128, 1, 1), st=2),
    _wg("w0-s3-valid-128to256", 2, 22, 31, 128, 256, _p0(128, 1, 1), st=3, pad="valid"),
    _wg("w0-1x1-s2-valid-64to128", 2, 17, 30, 64, 128, _p0(128, 1, 1), R=1, S=1, st=2, pad="valid"),
    # 7700 px: 16 splits of 512, chunk boundaries inside image rows, split-parallel reduce
    _wg("w0-7700px-16splits-reduce-g", 1, 70, 110, 8, 32, _p0(32, 1, 1, splits=16, chunk=512, reduce=1)),
    _wg("w0-6to3-scalar-reduce-16splits", 1, 70, 110, 6, 3, _p0(32, 0, 0, splits=16, chunk=512, reduce=0)),
    _wg("w0-q1-rows-wrap", 4, 300, 1, 8, 32, _p0(32, 1, 1, splits=8)),
    _wg("w0-f32-3to16", 2, 7, 9, 3, 16, _p0(32, 1, 0), dtype="f32"),
    _wg("w0-f32-20to50", 2, 7, 9, 20, 50, _p0(64, 0, 1), dtype="f32"),
    _wg("w0-f32-s2-same-64to128", 2, 9, 12, 64, 128, _p0(128, 1, 1), st=2, dtype="f32"),
    # ---- path 2: k_wgrad_row_halo (the (4, 10) head conv), partial 32-pixel segments
    _wg("w2-4x10-64to128", 2, 5, 12, 64, 128, dict(path=2), R=4, S=10),
    _wg("w2-4x10-128to128-q33", 1, 7, 33, 128, 128, dict(path=2), R=4, S=10),
]
# ---- path 1 at pad 0: the halo kernel takes any 3x3 stride-1 shape without looking at the pads
for _N, _H, _W in ((3, 10, 70), (2, 18, 130)):
    for _C, _K in ((64, 64), (128, 128), (128, 64)):
        WGRAD_CASES.append(_wg(f"w1-valid-{_N}x{_H}x{_W}-{_C}to{_K}", _N, _H, _W, _C, _K, dict(path=1), pad="valid"))


def call_geometry(c):
    """(N, H, W, C, K, R, S, st, pt, pl, P, Q) of the forward call the case makes."""
    if c.kind == "dgrad":
        return (c.N, c.P, c.Q, c.K, c.C, c.R, c.S, 1, c.R - 1 - c.pt, c.S - 1 - c.pl, c.H, c.W)
    return (c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.st, c.pt, c.pl, c.P, c.Q)


def torch_dtype(c):
    return BF if c.dtype == "bf16" else torch.float32


def _seed(c):
    return (c.N * 1000003 + c.H * 10007 + c.W * 101 + c.C * 13 + c.K * 7 + c.R * 3 + c.st) % (2 ** 31)


def fwd_operands(c):
    """CPU operands of a forward case: the input of the call (x, or dY for a
    dgrad) in the case's dtype, fp32 KRSC master weights already rounded to the
    dtype (what the packing stores), fp32 bias (None for a dgrad)."""
    g = torch.Generator(device="cpu").manual_seed(_seed(c))
    dt = torch_dtype(c)
    w = (torch.randn((c.K, c.R, c.S, c.C), generator=g) / (c.R * c.S * c.C) ** 0.5).to(dt).float()
    if c.kind == "dgrad":
        return (torch.randn((c.N, c.P, c.Q, c.K), generator=g) * 0.5).to(dt), w, None
    x = torch.randn((c.N, c.H, c.W, c.C), generator=g).to(dt)
    return x, w, torch.randn((c.K,), generator=g) * 0.1


def _conv(x_nhwc, w_krsc, b, c, dt):
    """The case's convolution of NHWC x with KRSC w in dtype dt -> NPQK."""
    x = x_nhwc.to(dt).permute(0, 3, 1, 2)
    pb = max((c.P - 1) * c.st + c.R - c.H - c.pt, 0)
    pr = max((c.Q - 1) * c.st + c.S - c.W - c.pl, 0)
    x = F.pad(x, (c.pl, pr, c.pt, pb))
    y = F.conv2d(x, w_krsc.to(dt).permute(0, 3, 1, 2), None if b is None else b.to(dt), stride=c.st)
    assert y.shape[2] >= c.P and y.shape[3] >= c.Q
    return y[:, :, :c.P, :c.Q].permute(0, 2, 3, 1).contiguous()


def _conv_t(dy_npqk, w_krsc, c, dt):
    """The transposed convolution dY -> dX[N, H, W, C] of the case's conv in dtype dt."""
    x = torch.zeros((c.N, c.H, c.W, c.C), dtype=dt, requires_grad=True)
    y = _conv(x, w_krsc, None, c, dt)
    (dx,) = torch.autograd.grad(y, x, dy_npqk.to(dt))
    return dx.contiguous()


def fwd_result(c, inp, w, b, dt=F64):
    """The output of the case's call (y, or dX for a dgrad) computed in dt."""
    return _conv_t(inp, w, c, dt) if c.kind == "dgrad" else _conv(inp, w, b, c, dt)


def f32_bound(c, inp, w, b):
    """Worst case of fp32 accumulation of the R S C products (+ bias, + the
    final rounding), per element: (R S C + 2) 2^-24 (conv(|x|, |w|) + |b|)."""
    mag = fwd_result(c, inp.abs(), w.abs(), None if b is None else b.abs())
    n = c.R * c.S * (c.K if c.kind == "dgrad" else c.C)
    return (n + 2) * 2.0 ** -24 * mag


def bf16_ulp(t):
    """bf16 unit in the last place of each element of t (float64)."""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -120)))
    return torch.pow(2.0, e - 7)


def bf16_bound(exact, atol=1e-4):
    """The project's bound of a bf16 output: 1 bf16 ulp of the exact value + 1e-4."""
    return bf16_ulp(exact) + atol


def wgrad_operands(c):
    g = torch.Generator(device="cpu").manual_seed(_seed(c) + 1)
    dt = BF if c.dtype == "bf16" else torch.float32
    x = torch.randn((c.N, c.H, c.W, c.C), generator=g).to(dt)
    dy = (torch.randn((c.N, c.P, c.Q, c.K), generator=g) * 0.5).to(dt)
    return x, dy


def wgrad_exact(c, x, dy, dt=F64):
    """dW [K, R, S, C] of the operands computed in dt (float64: the reference),
    and sum |x dy| per element."""
    out = []
    pb = max((c.P - 1) * c.st + c.R - c.H - c.pt, 0)
    pr = max((c.Q - 1) * c.st + c.S - c.W - c.pl, 0)
    for f in (lambda t: t, torch.abs):
        xp = F.pad(f(x.to(dt)).permute(0, 3, 1, 2), (c.pl, pr, c.pt, pb))
        d = f(dy.to(dt)).permute(0, 3, 1, 2)
        # (rows / columns of the padded input past the last strided window take no part)
        dw = torch.nn.grad.conv2d_weight(xp, (c.K, c.C, c.R, c.S), d, stride=c.st, padding=0)
        out.append(dw.permute(0, 2, 3, 1).contiguous())
    return out[0], out[1]


def assert_dw(dw, exact, mag, M, splits, what):
    """dW against the float64 one: the project's norm bounds (rel-L2 5e-5,
    max-relative 5e-4: tests/test_wgrad_branches_gpu.py, valid up to 262144
    summed pixels) and, per element, the worst case of fp32 accumulation of M
    exact products in `splits` partial sums: (M + splits + 2) 2^-24 sum |x dy|."""
    assert M <= 262144
    d = dw.detach().cpu().to(F64)
    assert bool(torch.isfinite(d).all()), (what, "dW not finite: an element was not written")
    err = (d - exact).abs()
    en = ((d - exact).norm() / exact.norm()).item()
    em = (err.max() / exact.abs().max()).item()
    bound = (M + splits + 2) * 2.0 ** -24 * mag
    # (an element no pixel reaches -- a tap that lies in the padding everywhere -- is exactly 0)
    ee = float((err / bound.clamp_min(1e-30)).max())
    print(f"{what}: dW rel-L2 {en:.3e} max-rel {em:.3e} worst element / bound {ee:.3e}")
    assert en <= 5e-5, (what, en)
    assert em <= 5e-4, (what, em)
    assert ee <= 1.0, (what, ee)
