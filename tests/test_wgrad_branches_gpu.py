"""Every launch branch of the halo weight gradient (k_wgrad3x3_halo,
csrc/conv.hip: halo_plan / wgrad_halo_launch) against float64, per shape.

Which instantiation runs depends on C, K, P % 2, P % 8 and Q % 64 together,
so every case first asserts the plan the launcher's own functions give for its
shape (acfe_conv2d_wgrad_halo_info: cw, nr, wp, nchunk, sp, edge, qs, qse) --
a dispatch change that moves a case to another branch fails it -- and then
runs the kernel.  The shapes are the smallest that reach each branch:

  8 x 65        one remainder column with one live pixel (the 513-wide stage-1
                case, small): edge 1, qs 1, qse 1
  16 x 100      three remainder columns, the last one 4 pixels: qse 3
  8 x 144 N 1   the remainder is exactly one full 16-pixel segment after two
                whole 64-pixel columns: qs 2, qse 1
  24 x 81 N 2   two remainder columns, the last one 1 pixel: qse 2
  14 x 100      control, P % 8 != 0: no remainder launch, masked columns
                (edge 0, qs 2)

at N = 3 unless noted (segment ranges cross image boundaries), K = 64 and C in
{64, 128, 16}.  C = 16 -> K = 64 runs on the halo kernel only from 16 splits
on (halo_ok), that is N H W > 4096: there the same H x W run at the smallest
N past that (8 x 65: N 8, 8 x 144: N 4, 24 x 81: N 3), and
test_plain_c16_small_is_generic runs the literal small-N shapes, asserting
that they are NOT the halo kernel's (the generic split-K kernel takes them).

Bounds.  dW (fp32, fp32 accumulation of bf16 products over at most 5832
pixels) against torch.nn.grad.conv2d_weight in float64 on the same bf16
operands: norm-relative 5e-5, max-relative 5e-4 -- the bounds of
test_production_gpu.test_wgrad_halo_narrow at 32 clips, which hold a fortiori
for fewer summed pixels.  The fold's channel sums: within 1e-6 of the float64
column sums of the stored dY relative to sum |dY| (test_conv_wgrad_bnbwd_fused's
bound).  Everything else is bit-for-bit.

Guard bytes: the keep bits, the fold's dY and its sums slab are allocated with
256 sentinel bytes past their logical end, which must stay unchanged (the
remainder launch builds its offsets from wofs and partial segments).

Empty ranges: the N = 1 cases (8 x 65 and 16 x 100; at C = 16, where the halo
kernel needs more than 4096 pixels, 8 x 577 and 16 x 292 -- the same one and
three remainder columns) have sp * nchunk > N * ceil(P / 8) * qse, asserted
from the plan in the plain, fold and keep tests alike, so some workgroups of
the remainder launch have no segment and must add nothing to the slabs and the
channel sums the first launch wrote.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
K64 = 64
SENTINEL, TAIL = 0xA5, 256

# id, N, H, W, the plan fields the case must reach
SHAPES = [
    ("8x65-1col-1px", 3, 8, 65, dict(nr=2, edge=1, qs=1, qse=1)),
    ("16x100-3cols-last4", 3, 16, 100, dict(nr=2, edge=1, qs=1, qse=3)),
    ("8x144-full16-2whole", 1, 8, 144, dict(nr=2, edge=1, qs=2, qse=1)),
    ("24x81-2cols-last1", 2, 24, 81, dict(nr=2, edge=1, qs=1, qse=2)),
    ("14x100-control-masked", 3, 14, 100, dict(nr=2, edge=0, qs=2, qse=0)),
]
# N = 1: remainder-launch workgroups without a segment (sp * nchunk > N * ceil(P / 8) * qse)
EMPTY = [
    ("8x65-n1-empty", 1, 8, 65, dict(nr=2, edge=1, qs=1, qse=1)),
    ("16x100-n1-empty", 1, 16, 100, dict(nr=2, edge=1, qs=1, qse=3)),
]
# the same at C = 16 -> K = 64, whose halo kernel needs N H W > 4096
EMPTY_C16 = [
    ("8x577-n1-empty", 1, 8, 577, dict(nr=2, edge=1, qs=9, qse=1)),
    ("16x292-n1-empty", 1, 16, 292, dict(nr=2, edge=1, qs=4, qse=3)),
]


def _clips(C, N, H, W):
    """N, or for C = 16 -> K = 64 the smallest N at which the halo kernel takes
    H x W (16 splits: N H W > 4096, halo_ok)."""
    if C == 16 and N * H * W <= 4096:
        return 4096 // (H * W) + 1
    return N


def _cases(channels):
    """(C, N, H, W, want, empty) of every shape at every C of `channels`."""
    out = []
    for C in channels:
        for name, N, H, W, want in SHAPES:
            out.append(pytest.param(C, _clips(C, N, H, W), H, W, want, False, id=f"c{C}-{name}"))
        for name, N, H, W, want in (EMPTY_C16 if C == 16 else EMPTY):
            out.append(pytest.param(C, N, H, W, want, True, id=f"c{C}-{name}"))
    return out


@pytest.fixture(scope="module")
def env(cuda):
    from acfe import ops
    from acfe._lib import call, lib, wgrad_halo_info
    from acfe._torch import ptr, stream

    return ops, call, lib, ptr, stream, wgrad_halo_info


def _assert_plan(info, N, H, W, C, K, want, fold=False, empty=False):
    """The plan of the shape has the fields of `want`; empty: some workgroups
    of its remainder launch have no segment."""
    plan = info(N, H, W, C, K, fold=fold)
    assert plan is not None, ("not the halo kernel's shape", N, H, W, C, K, fold)
    cw = {(64, 16): 16, (256, 64): 32}.get((K, C), 64)
    want = dict(want, cw=cw, nchunk=C // cw, wp=2 if (C, K) == (16, 64) else 1)
    got = {k: plan[k] for k in want}
    assert got == want, (plan, want)
    if empty:
        assert plan["sp"] * plan["nchunk"] > N * ((H + 7) // 8) * plan["qse"], plan
    return plan


def _guarded(shape, dtype, device):
    """A tensor of `shape` whose storage carries TAIL sentinel bytes past its
    end (and sentinels inside, so an element never written shows too)."""
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((n + TAIL,), SENTINEL, dtype=torch.uint8, device=device)
    return raw, raw[:n].view(dtype).view(shape)


def _tail_intact(raw):
    return bool((raw[-TAIL:] == SENTINEL).all())


def _dw_exact(x, dy):
    """float64 weight gradient [K, 3, 3, C] of the bf16 operands."""
    K, C = dy.shape[-1], x.shape[-1]
    return torch.nn.grad.conv2d_weight(x.cpu().to(F64).permute(0, 3, 1, 2), (K, C, 3, 3),
                                       dy.cpu().to(F64).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)


def _assert_dw(dw, exact, what):
    d = dw.cpu().to(F64)
    en = ((d - exact).norm() / exact.norm()).item()
    em = ((d - exact).abs().max() / exact.abs().max()).item()
    print(f"{what}: dW rel-L2 {en:.3e} max-rel {em:.3e}")
    assert en < 5e-5, (what, en)
    assert em < 5e-4, (what, em)


def _assert_sums(call, lib, ptr, stream, sums, srows, dy, what):
    """acfe_channel_sum_finalize(sums) against the float64 column sums of the
    stored dY, relative to sum |dY|."""
    K = dy.shape[-1]
    db = torch.empty((K,), device=dy.device)
    call("acfe_channel_sum_finalize", ptr(sums), srows, K, 0.0, ptr(db), stream())
    torch.cuda.synchronize()
    d = dy.cpu().to(F64).reshape(-1, K)
    scale = d.abs().sum(0).clamp_min(1.0)
    err = ((db.cpu().to(F64) - d.sum(0)).abs() / scale).max().item()
    print(f"{what}: channel sums rel err {err:.3e}")
    assert err < 1e-6, (what, err)


def _operands(N, H, W, C, K, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn((N, H, W, C), generator=g).to(BF).to(device)
    dy = (torch.randn((N, H, W, K), generator=g) * 0.5).to(BF).to(device)
    return x, dy, g


def _plain(env, cuda, N, H, W, C, K, what):
    ops, call, lib, ptr, stream, info = env
    x, dy, _ = _operands(N, H, W, C, K, 1000 * C + 10 * H + W + N, cuda)
    ws = torch.empty((lib.acfe_conv2d_wgrad_workspace(N, H, W, C, K, 3, 3, H, W),), device=cuda)
    dw = torch.full((K, 3, 3, C), float("nan"), device=cuda)
    args = (ptr(x), N, H, W, C, ptr(dy), K, 3, 3, 1, 1, 1, H, W)
    call("acfe_conv2d_wgrad", *args, ptr(dw), 0.0, 1, ptr(ws), stream())
    torch.cuda.synchronize()
    _assert_dw(dw, _dw_exact(x, dy), what)
    # beta = 1: a second call adds exactly the same gradient
    dw2 = dw.clone()
    call("acfe_conv2d_wgrad", *args, ptr(dw2), 1.0, 1, ptr(ws), stream())
    torch.cuda.synchronize()
    assert torch.equal(dw2, dw + dw), what


@pytest.mark.parametrize("C,N,H,W,want,empty", _cases([64, 128, 16]))
def test_plain_k64(env, cuda, C, N, H, W, want, empty):
    """acfe_conv2d_wgrad at K = 64: k_wgrad3x3_halo<64, false, 64 | 16, 2> and
    its 16-pixel remainder launch, dW against float64 and beta = 1."""
    _assert_plan(env[5], N, H, W, C, K64, want, empty=empty)
    _plain(env, cuda, N, H, W, C, K64, f"plain c{C} {N}x{H}x{W}")


_SMALL = [c[:4] for c in SHAPES + EMPTY if c[1] * c[2] * c[3] <= 4096]


@pytest.mark.parametrize("name,N,H,W", _SMALL, ids=[c[0] for c in _SMALL])
def test_plain_c16_small_is_generic(env, cuda, name, N, H, W):
    """C = 16 -> K = 64 at the literal small shapes: fewer than 16 splits, so
    NOT the halo kernel's (the plan query says so) -- the generic split-K
    kernel, held to the same float64 bounds."""
    assert env[5](N, H, W, 16, K64) is None
    _plain(env, cuda, N, H, W, 16, K64, f"plain c16 generic {name}")


@pytest.mark.parametrize("C,K,want", [(128, 128, dict(cw=64, nr=1, nchunk=2, edge=1, qs=1, qse=2)),
                                      (64, 256, dict(cw=32, nr=1, nchunk=2, edge=1, qs=1, qse=2))],
                         ids=["k128", "k256"])
def test_plain_k128_k256_remainder(env, cuda, C, K, want):
    """The K = 128 / K = 256 remainder kernels (k_wgrad3x3_halo<128, false, 64,
    1, false, false, 16> / <256, false, 32, 1, false, false, 16>) on two
    chunks of C at 6 x 81: a partial 8-row group (rows 6, 7 load zeros) and two
    remainder columns, the last one 1 pixel."""
    N, H, W = 3, 6, 81
    _assert_plan(env[5], N, H, W, C, K, want)
    _plain(env, cuda, N, H, W, C, K, f"plain c{C} k{K}")


def test_plain_k32_odd_rows(env, cuda):
    """K = 32 at an odd row count: one row per step (k_wgrad3x3_halo<32, false,
    64, 1>; an even P takes the two-row kernel) on two chunks of C at 7 x 70,
    the partial last 64-pixel column masked (K = 32 has no remainder kernel)."""
    N, H, W, C, K = 3, 7, 70, 128, 32
    _assert_plan(env[5], N, H, W, C, K, dict(nr=1, edge=0, qs=2, qse=0))
    _plain(env, cuda, N, H, W, C, K, "plain c128 k32 odd rows")


FORMS = ["drop-relu", "nodrop", "norelu", "add-f1", "add-f3"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,N,H,W,want,empty", _cases([64, 128, 16]))
def test_fold_k64(env, cuda, C, form, N, H, W, want, empty):
    """acfe_conv2d_wgrad_bnbwd at K = 64 (k_wgrad3x3_halo<64, false, 64 | 16,
    2, true, false> and its remainder launch) in every form of the C ABI:
    dropout 0.1 with ReLU, no dropout, no ReLU, and the residual form (`add`,
    flags 1 and 3).  The stored dY bit-identical to acfe_bn_bwd_apply_ex, dW
    bit-identical to acfe_conv2d_wgrad on that dY AND within the plain bounds of
    the float64 weight gradient of (x, stored dY), the channel sums against
    float64 (at C = 128 only chunk 0 stores and sums: a double count shows in
    both; in the N = 1 cases a remainder workgroup without segments that
    overwrote its sums row instead of adding to it shows here), guard bytes
    past dY and the sums intact."""
    ops, call, lib, ptr, stream, info = env
    K = K64
    _assert_plan(info, N, H, W, C, K, want, fold=True, empty=empty)
    _assert_plan(info, N, H, W, C, K, want, empty=empty)  # (the plain kernel splits as the fold does)
    srows = lib.acfe_conv2d_wgrad_bnbwd_rows(N, H, W, C, K)
    assert srows > 0
    what = f"fold c{C} {form} {N}x{H}x{W}"
    g = torch.Generator().manual_seed(7 * C + H + W + FORMS.index(form))
    x = torch.randn((N, H, W, C), generator=g).to(BF).to(cuda)
    gy = torch.randn((N, H, W, K), generator=g).to(BF).to(cuda)
    u = torch.randn((N, H, W, K), generator=g) * 1.5
    addt = torch.randn((N, H, W, K), generator=g).to(BF).to(cuda)
    sc = ((torch.rand(K, generator=g) + 0.5) * torch.where(torch.rand(K, generator=g) < 0.2, -1.0, 1.0)).to(cuda)
    sh = (torch.randn(K, generator=g) * 0.3).to(cuda)
    coef = (torch.randn(3 * K, generator=g) * 0.5).to(cuda)
    rate, seed, flags, add = {"drop-relu": (0.1, 12345, 1, None), "nodrop": (0.0, 0, 1, None),
                              "norelu": (0.1, 777, 0, None), "add-f1": (0.0, 0, 1, addt),
                              "add-f3": (0.0, 0, 3, addt)}[form]
    u = (u.clamp_min(0) if flags & 2 else u).to(BF).to(cuda)
    rows = N * H * W
    addp = ptr(add) if add is not None else None
    # the unfused chain
    dy0 = torch.full((N, H, W, K), float("nan"), dtype=BF, device=cuda)
    nrb = lib.acfe_reduce_blocks(rows)
    sums0 = torch.empty((nrb, 2, K), dtype=F64, device=cuda)
    call("acfe_bn_bwd_apply_ex", ptr(gy), 1, ptr(u), 1, rows, K, ptr(sc), ptr(sh), flags, ptr(coef), addp, rate,
         seed, ptr(dy0), 1, ptr(sums0), stream())
    ws = torch.empty((lib.acfe_conv2d_wgrad_workspace(N, H, W, C, K, 3, 3, H, W),), device=cuda)
    dw0 = torch.empty((K, 3, 3, C), device=cuda)
    call("acfe_conv2d_wgrad", ptr(x), N, H, W, C, ptr(dy0), K, 3, 3, 1, 1, 1, H, W, ptr(dw0), 0.0, 1, ptr(ws),
         stream())
    # the fold
    dyraw, dy1 = _guarded((N, H, W, K), BF, cuda)
    sraw, sums1 = _guarded((srows, 2, K), F64, cuda)
    dw1 = torch.full((K, 3, 3, C), float("nan"), device=cuda)
    ws1 = torch.empty_like(ws)
    call("acfe_conv2d_wgrad_bnbwd", ptr(x), N, H, W, C, ptr(gy), ptr(u), K, ptr(sc), ptr(sh), flags, ptr(coef), addp,
         rate, seed, ptr(dy1), ptr(dw1), 0.0, ptr(ws1), ptr(sums1), stream())
    torch.cuda.synchronize()
    assert _tail_intact(dyraw) and _tail_intact(sraw), what
    assert torch.equal(dy1.view(torch.int16), dy0.view(torch.int16)), what
    assert torch.equal(dw1, dw0), (what, (dw1 - dw0).abs().max().item())
    _assert_dw(dw1, _dw_exact(x, dy1), what)
    _assert_sums(call, lib, ptr, stream, sums1, srows, dy1, what)
    assert _tail_intact(sraw), what


@pytest.mark.parametrize("C,N,H,W,want,empty", _cases([64, 128, 256]))
def test_keep_k64(env, cuda, C, N, H, W, want, empty):
    """The dropout keep bits through the remainder launches: forward
    (acfe_conv2d_fwd_dropout_keep and acfe_conv2d_fwd_bn_keep) y and statistics
    bit-identical to the forward without keep, the keep bytes the packed mask
    of acfe_dropout, and the fold reading them (acfe_conv2d_wgrad_bnbwd_keep,
    k_wgrad3x3_halo<64, false, 64, 2, true, true> + its remainder launch) dY,
    dW and sums bit-identical to the hash-regenerating fold, its dW within the
    float64 bounds and its sums against float64; guard bytes past keep, dY and
    the sums intact.  C = 256: four chunks.  N = 1: remainder workgroups
    without segments."""
    ops, call, lib, ptr, stream, info = env
    K = K64
    _assert_plan(info, N, H, W, C, K, want, fold=True, empty=empty)
    assert lib.acfe_conv2d_dropout_keep_supported(N, H, W, C, K, 1) == 1
    assert lib.acfe_conv2d_bn_prologue_supported(N, H, W, C, K, 1) == 1
    what = f"keep c{C} {N}x{H}x{W}"
    g = torch.Generator(device="cpu").manual_seed(3 * C + H + W)
    x = torch.randn((N, H, W, C), generator=g).to(BF).to(cuda)
    w = (torch.randn((K, 3, 3, C), generator=g) * (1.0 / (3 * C ** 0.5))).to(cuda)
    b = (torch.randn((K,), generator=g) * 0.1).to(cuda)
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(cuda), (torch.randn(C, generator=g) * 0.3).to(cuda)
    wp = ops.pack_weights(w, BF, False)
    rows = lib.acfe_conv2d_stats_rows(N * H * W, K)
    rate, seed = 0.1, 4242

    def fwd(pro, keep):
        y = torch.full((N, H, W, K), float("nan"), dtype=BF, device=cuda)
        st = torch.zeros((rows, 2, wp.shape[0]), dtype=F64, device=cuda)
        xb = torch.empty_like(x)
        if pro and keep is None:
            call("acfe_conv2d_fwd_bn", ptr(x), N, H, W, C, ptr(wp), K, 1, 1, ptr(b), ptr(y), ptr(st), rate, seed,
                 ptr(sc), ptr(sh), 1, ptr(xb), 1, stream())
        elif pro:
            call("acfe_conv2d_fwd_bn_keep", ptr(x), N, H, W, C, ptr(wp), K, 1, 1, ptr(b), ptr(y), ptr(st), rate,
                 seed, ptr(sc), ptr(sh), 1, ptr(xb), ptr(keep), 1, stream())
        elif keep is None:
            call("acfe_conv2d_fwd_dropout", ptr(x), N, H, W, C, ptr(wp), K, 3, 3, 1, 1, 1, H, W, ptr(b), ptr(y), 1,
                 ptr(st), rate, seed, stream())
        else:
            call("acfe_conv2d_fwd_dropout_keep", ptr(x), N, H, W, C, ptr(wp), K, 1, 1, ptr(b), ptr(y), ptr(st), rate,
                 seed, ptr(keep), stream())
        torch.cuda.synchronize()
        return y, st

    ones = torch.ones((N, H, W, K), dtype=BF, device=cuda)
    m = torch.empty_like(ones)
    call("acfe_dropout", ptr(ones), ones.numel(), rate, seed, ptr(m), 1, stream())
    torch.cuda.synchronize()
    mask = (m != 0).reshape(N, H, W, K // 8, 8).to(torch.int32)
    bits = sum(mask[..., j] << j for j in range(8)).to(torch.uint8)
    keep = None
    for pro in (True, False):
        kraw, keep = _guarded((N, H, W, K // 8), torch.uint8, cuda)
        y0, st0 = fwd(pro, None)
        y1, st1 = fwd(pro, keep)
        assert _tail_intact(kraw), (what, pro)
        assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)), (what, pro)
        assert torch.equal(st1, st0), (what, pro)
        assert torch.equal(keep, bits), (what, pro)
    # the fold: BN backward apply (+ReLU mask) -> dropout backward while staging
    dy = torch.randn((N, H, W, K), generator=g).to(BF).to(cuda)
    bsc, bsh = (torch.rand(K, generator=g) + 0.5).to(cuda), (torch.randn(K, generator=g) * 0.2).to(cuda)
    coef = (torch.randn(3 * K, generator=g) * 0.3).to(cuda)
    brows = lib.acfe_conv2d_wgrad_bnbwd_rows(N, H, W, C, K)
    assert brows > 0
    ws = torch.empty((lib.acfe_conv2d_wgrad_workspace(N, H, W, C, K, 3, 3, H, W),), device=cuda)

    def fold(kp):
        graw, gout = _guarded((N, H, W, K), BF, cuda)
        sraw, sums = _guarded((brows, 2, K), F64, cuda)
        dw = torch.full((K, 3, 3, C), float("nan"), device=cuda)
        if kp is None:
            call("acfe_conv2d_wgrad_bnbwd", ptr(x), N, H, W, C, ptr(dy), ptr(y1), K, ptr(bsc), ptr(bsh), 1, ptr(coef),
                 None, rate, seed, ptr(gout), ptr(dw), 0.0, ptr(ws), ptr(sums), stream())
        else:
            call("acfe_conv2d_wgrad_bnbwd_keep", ptr(x), N, H, W, C, ptr(dy), ptr(y1), K, ptr(bsc), ptr(bsh), 1,
                 ptr(coef), rate, seed, ptr(kp), ptr(gout), ptr(dw), 0.0, ptr(ws), ptr(sums), stream())
        torch.cuda.synchronize()
        assert _tail_intact(graw) and _tail_intact(sraw), (what, kp is None)
        return gout, dw, sums

    a, k = fold(None), fold(keep)
    assert torch.equal(a[0].view(torch.int16), k[0].view(torch.int16)), what
    assert torch.equal(a[1], k[1]) and torch.equal(a[2], k[2]), what
    _assert_dw(k[1], _dw_exact(x, k[0]), what)
    _assert_sums(call, lib, ptr, stream, k[2], brows, k[0], what)


def test_keep_supported_agrees_with_launch(env, cuda):
    """acfe_conv2d_dropout_keep_supported against the keep forward itself on
    small images (few statistics slab rows for the two launches to share):
    where it says 1 the forward runs and matches the forward without keep bit
    for bit (y, statistics), where it says 0 the keep forward refuses."""
    ops, call, lib, ptr, stream, info = env
    from acfe._lib import E_INVAL

    C = K = 64
    g = torch.Generator(device="cpu").manual_seed(99)
    w = (torch.randn((K, 3, 3, C), generator=g) * (1.0 / 24)).to(cuda)
    b = (torch.randn((K,), generator=g) * 0.1).to(cuda)
    wp = ops.pack_weights(w, BF, False)
    rate, seed = 0.1, 31
    seen = set()
    for N in (1, 2):
        for H in (1, 2, 3, 9):
            for W in (64, 65, 100, 127, 130):
                x = torch.randn((N, H, W, C), generator=g).to(BF).to(cuda)
                rows = lib.acfe_conv2d_stats_rows(N * H * W, K)
                y1 = torch.full((N, H, W, K), float("nan"), dtype=BF, device=cuda)
                st1 = torch.zeros((rows, 2, wp.shape[0]), dtype=F64, device=cuda)
                kraw, keep = _guarded((N, H, W, K // 8), torch.uint8, cuda)
                ok = lib.acfe_conv2d_dropout_keep_supported(N, H, W, C, K, 1)
                seen.add(ok)
                rc = lib.acfe_conv2d_fwd_dropout_keep(ptr(x), N, H, W, C, ptr(wp), K, 1, 1, ptr(b), ptr(y1),
                                                      ptr(st1), rate, seed, ptr(keep), stream())
                if not ok:
                    assert rc == E_INVAL, (N, H, W, rc)
                    continue
                assert rc == 0, (N, H, W, rc)
                y0 = torch.full_like(y1, float("nan"))
                st0 = torch.zeros_like(st1)
                call("acfe_conv2d_fwd_dropout", ptr(x), N, H, W, C, ptr(wp), K, 3, 3, 1, 1, 1, H, W, ptr(b), ptr(y0),
                     1, ptr(st0), rate, seed, stream())
                torch.cuda.synchronize()
                assert _tail_intact(kraw), (N, H, W)
                assert torch.equal(y1.view(torch.int16), y0.view(torch.int16)), (N, H, W)
                assert torch.equal(st1, st0), (N, H, W)
    assert seen == {0, 1}  # (1, 1, 100): one slab row, none left for the remainder launch


def test_ops_conv_dropout_small_slab(env, cuda):
    """(1, 1, 100) at C = K = 64: the keep forward does not take it (one
    statistics slab row), so the node must not choose the keep path.  What
    this checks is that ops.keep_bits_ok says no and that the training-mode
    Conv2D -> Dropout -> BN node, forward and backward, still runs with finite
    results; with keep_bits_ok false both settings of ops.KEEP_BITS take the
    same path, so their equality only confirms that."""
    ops, call, lib, ptr, stream, info = env
    N, H, W, C, K = 1, 1, 100, 64, 64
    assert lib.acfe_conv2d_dropout_keep_supported(N, H, W, C, K, 1) == 0
    g = torch.Generator(device="cpu").manual_seed(5)
    x0 = torch.randn((N, H, W, C), generator=g).to(BF).to(cuda)
    w0 = (torch.randn((K, 3, 3, C), generator=g) * (1.0 / 24)).to(cuda)
    b0 = (torch.randn((K,), generator=g) * 0.1).to(cuda)
    gout = torch.randn((N, H, W, K), generator=g).to(BF).to(cuda)
    assert not ops.keep_bits_ok(x0, w0, 1, 1, 1, H, W, (0.1, 9), True)
    outs = []
    old = ops.KEEP_BITS
    try:
        for kb in (True, False):
            ops.KEEP_BITS = kb
            x = x0.clone().requires_grad_(True)
            w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            gamma, beta = torch.ones(K, device=cuda, requires_grad=True), torch.zeros(K, device=cuda, requires_grad=True)
            y = ops.conv_dropout_bn(x, w, b, gamma, beta, torch.zeros(K, device=cuda), torch.ones(K, device=cuda),
                                    True, rate=0.1, seed=9)
            y.backward(gout)
            torch.cuda.synchronize()
            outs.append([t.detach().float() for t in (y, x.grad, w.grad, b.grad, gamma.grad, beta.grad)])
    finally:
        ops.KEEP_BITS = old
    for a, c in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, c)
