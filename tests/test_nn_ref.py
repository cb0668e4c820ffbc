"""oracle/nn_ref.py (the float64 / integer restatements the GPU variant tests of
csrc/nn.hip compare against) checked on the CPU against torch's own operators
and autograd, and acfe_nn_launch_info against values worked out by hand from
the constants acfe.h documents: 256-thread workgroups, grid caps 8192 (scalar),
16384 (eight-wide), 4096 (Adam), slab rows min(ceil(rows / 256), 1024)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nn_ref as R
from oracle.models import avgpool_same

F64 = torch.float64


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------ pools
@pytest.mark.parametrize("kh,kw", [(1, 2), (2, 2), (3, 3), (2, 3)])
@pytest.mark.parametrize("H,W", [(13, 35), (12, 36), (14, 37)])
def test_maxpool_matches_torch_without_ties(kh, kw, H, W):
    x = _randn((2, H, W, 5), 1).requires_grad_(True)
    y, _ = R.maxpool(x.detach(), kh, kw)
    yt = F.max_pool2d(x.permute(0, 3, 1, 2), (kh, kw), (kh, kw)).permute(0, 2, 3, 1)
    assert torch.equal(y, yt.detach())
    dy = _randn(tuple(y.shape), 2)
    (yt * dy).sum().backward()
    assert torch.equal(R.maxpool_bwd(x.detach(), dy, kh, kw), x.grad)


def test_maxpool_ties_go_to_the_first_maximum():
    # one 2x3 window per pixel pair; the maximum 2.0 sits at window positions 1, 4 and 5
    x = torch.tensor([[0.0, 2.0, 1.0], [1.0, 2.0, 2.0]], dtype=F64).view(1, 2, 3, 1)
    y, am = R.maxpool(x, 2, 3)
    assert y.item() == 2.0 and am.item() == 1
    dx = R.maxpool_bwd(x, torch.full((1, 1, 1, 1), 7.0, dtype=F64), 2, 3)
    assert dx.flatten().tolist() == [0, 7, 0, 0, 0, 0]
    # an all-equal window: position 0; leftover row and column: zero gradient
    x = torch.zeros((1, 3, 3, 2), dtype=F64)
    y, am = R.maxpool(x, 2, 2)
    assert am.flatten().tolist() == [0, 0]
    dx = R.maxpool_bwd(x, torch.ones((1, 1, 1, 2), dtype=F64), 2, 2)
    assert dx[0, 0, 0].tolist() == [1, 1] and dx.sum().item() == 2


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("H,W", [(13, 35), (12, 36), (14, 37)])
def test_avgpool_matches_oracle_models(k, H, W):
    x = _randn((2, H, W, 3), 3).requires_grad_(True)
    ref = avgpool_same(x.permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)
    y = R.avgpool(x.detach(), k)
    assert (y - ref.detach()).abs().max().item() <= 1e-14
    dy = _randn(tuple(y.shape), 4)
    (ref * dy).sum().backward()
    assert (R.avgpool_bwd(dy, H, W, k) - x.grad).abs().max().item() <= 1e-14


def test_sub_bwd_is_the_strided_1x1_input_gradient():
    x = _randn((2, 7, 9, 3), 5).requires_grad_(True)
    y = x[:, ::2, ::2]
    g = _randn(tuple(y.shape), 6)
    (y * g).sum().backward()
    assert torch.equal(R.sub_bwd(g, 7, 9, 2), x.grad)


# ------------------------------------------------------------------ BatchNormalization
@pytest.mark.parametrize("relu", [0, 1])
def test_bn_backward_matches_autograd(relu):
    rows, C = 203, 6
    x = _randn((rows, C), 7)
    x[:, 2] = 0.75  # a constant channel: variance 0
    gamma, beta = _randn((C,), 8), _randn((C,), 9) * 0.3
    dy = _randn((rows, C), 10)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    mean, var = xr.mean(0), xr.var(0, unbiased=False)
    y = (xr - mean) / torch.sqrt(var + 1e-3) * gr + br
    if relu:
        y = F.relu(y)
    (y * dy).sum().backward()

    fin = R.bn_finalize(R.bn_stats(x), rows, gamma, beta, torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64))
    assert torch.allclose(fin["mean"], mean.detach(), rtol=0, atol=1e-14)
    assert torch.allclose(fin["invstd"], 1 / torch.sqrt(var.detach() + 1e-3), rtol=1e-10)
    assert abs(fin["invstd"][2].item() - 1 / np.sqrt(1e-3)) < 1e-9
    assert torch.allclose(fin["moving_mean"], 0.01 * mean.detach(), rtol=1e-12, atol=1e-16)
    assert torch.allclose(fin["moving_var"], 0.99 + 0.01 * var.detach(), rtol=1e-12)
    assert torch.allclose(R.bn_apply(x, fin["scale"], fin["shift"], relu), y.detach(), rtol=0, atol=1e-11)
    sums = R.bn_bwd_reduce(dy, x, fin["scale"], fin["shift"], fin["mean"], fin["invstd"], relu)
    dgamma, dbeta, coef = R.bn_bwd_finalize(sums, rows, fin["scale"], fin["mean"], fin["invstd"])
    assert torch.allclose(dgamma, gr.grad, rtol=1e-9, atol=1e-11)
    assert torch.allclose(dbeta, br.grad, rtol=1e-9, atol=1e-11)
    dx = R.bn_bwd_apply(dy, x, fin["scale"], fin["shift"], coef, relu)
    assert torch.allclose(dx, xr.grad, rtol=1e-9, atol=1e-9)


def test_bn_bwd_apply_add_and_upstream_relu():
    x, dy, add = _randn((50, 4), 11), _randn((50, 4), 12), _randn((50, 4), 13)
    scale, shift, coef = _randn((4,), 14), _randn((4,), 15), _randn((3, 4), 16)
    base = R.bn_bwd_apply(dy, x, scale, shift, coef, 1)
    full = R.bn_bwd_apply(dy, x, scale, shift, coef, 3, add)
    assert torch.equal(full, torch.where(x > 0, base + add, torch.zeros_like(base)))


def test_eval_mode_finalize_uses_the_moving_statistics():
    mm, mv = _randn((5,), 17), _randn((5,), 18).abs()
    fin = R.bn_finalize(None, 0, torch.ones(5, dtype=F64), torch.zeros(5, dtype=F64), mm, mv, training=False)
    assert torch.equal(fin["mean"], mm) and torch.allclose(fin["invstd"], 1 / torch.sqrt(mv + 1e-3))


# ------------------------------------------------------------------ dropout mask
SEED = (7 << 32) | 12345


def test_dropout_keep_rate():
    n = 1 << 20
    keep = R.dropout_keep(SEED, np.arange(n, dtype=np.uint64), 0.1)
    sd = np.sqrt(0.1 * 0.9 / n)  # binomial: 5 sd = 1.46e-3
    assert abs(keep.mean() - 0.9) <= 5 * sd, keep.mean()
    assert 5 * sd <= 1.5e-3
    assert R.dropout_keep(SEED, np.arange(n, dtype=np.uint64), 0.0).all()


def test_dropout_pair_shares_one_hash_by_halves():
    idx = np.arange(0, 1 << 16, 2, dtype=np.uint64)
    h = R.pair_hash(SEED, idx >> np.uint64(1))
    thr = R.dropout_threshold(0.1)
    assert thr == 6553
    assert np.array_equal(R.dropout_keep(SEED, idx, 0.1), (h & np.uint64(0xFFFF)) >= thr)
    assert np.array_equal(R.dropout_keep(SEED, idx ^ np.uint64(1), 0.1), (h >> np.uint64(16)) >= thr)
    # the halves are not copies of each other, and the seed's upper word takes part
    assert (R.dropout_keep(SEED, idx, 0.1) != R.dropout_keep(SEED, idx ^ np.uint64(1), 0.1)).mean() > 0.1
    assert (R.dropout_keep(SEED, idx, 0.1) != R.dropout_keep(SEED & 0xFFFFFFFF, idx, 0.1)).mean() > 0.1
    # indices past 2^32 use their upper word
    hi = idx + np.uint64(1 << 33)
    assert (R.dropout_keep(SEED, hi, 0.5) != R.dropout_keep(SEED, idx, 0.5)).mean() > 0.3


def test_dropout_values():
    x = R.to_bf16(_randn((4096,), 19))
    y, keep = R.dropout(x, SEED, 0.1, bf16=True)
    assert R.dropout_scale(0.1) == np.float32(1) / np.float32(0.9)
    assert (y[~keep] == 0).all() and torch.equal(y, R.to_bf16(y))
    assert torch.allclose(y[keep], x[keep] / 0.9, rtol=2 ** -8)


# ------------------------------------------------------------------ head
def test_head_restatements():
    x = _randn((3, 5, 4), 20)
    assert torch.allclose(R.axis_pool(x, 5.0, 0), torch.log(torch.exp(5 * x).mean(1)) / 5)
    assert torch.allclose(R.axis_pool_bwd(x, torch.ones(3, 4, dtype=F64), 5.0, 0).sum(1), torch.ones(3, 4, dtype=F64))
    assert torch.allclose(R.axis_pool_bwd(x, torch.ones(3, 4, dtype=F64), 5.0, 1), torch.full((3, 5, 4), 0.2, dtype=F64))
    z, y = _randn((6, 7), 21), (_randn((6, 7), 22) > 0.5).to(F64)
    l, dz = R.loss(z, y, 0, 0.25)
    assert torch.allclose(dz, (torch.sigmoid(z) - y) / 7 * 0.25)
    p, g = _randn((9,), 23), _randn((9,), 24)
    p1, m1, v1 = R.adam(p, g, torch.zeros(9, dtype=F64), torch.zeros(9, dtype=F64), 0.5, 1)
    assert torch.allclose(m1, 0.05 * g) and torch.allclose(v1, 0.00025 * g * g)
    assert torch.allclose(p - p1, 0.01 * torch.sign(g), rtol=1e-4)  # first Adam step: lr * sign(g)


# ------------------------------------------------------------------ launch plans
PLAN_TABLE = [
    # op, rows, C, aligned, slab, geo (H, W, kh, kw), expected (variant, grid, block, passes) or None
    ("bn_stats", 1003, 16, 1, 0, None, (1, 4, 256, 2)),      # 251 rows per workgroup, 128 side by side
    ("bn_stats", 1003, 48, 1, 0, None, (1, 4, 256, 6)),      # 42 side by side
    ("bn_stats", 1003, 50, 1, 0, None, (0, 4, 256, 51)),     # C % 8: scalar, 5 side by side
    ("bn_stats", 1003, 64, 1, 0, None, (1, 4, 256, 8)),
    ("bn_stats", 1003, 256, 1, 0, None, (1, 4, 256, 32)),
    ("bn_stats", 1003, 16, 0, 0, None, (0, 4, 256, 16)),     # misaligned: scalar
    ("bn_stats", 262143, 16, 1, 0, None, (1, 1024, 256, 2)),
    ("bn_stats", 262145, 16, 1, 0, None, (1, 1024, 256, 3)),  # slab rows capped at 1024
    ("bn_stats", 524288 + 560, 256, 1, 0, None, (1, 1024, 256, 65)),   # one flush (64) and one row more
    ("bn_stats", 1310720 + 50, 50, 1, 0, None, (0, 1024, 256, 257)),   # one flush (256) and one row more
    ("bn_stats", 0, 16, 1, 0, None, None),
    ("bn_stats", 1003, 2056, 1, 0, None, None),
    ("bn_bwd_reduce", 1003, 64, 1, 0, None, (1, 4, 256, 8)),
    ("channel_sum", 1003, 50, 1, 0, None, (0, 4, 256, 51)),
    ("bn_finalize", 1024, 50, 1, 0, None, (0, 7, 1024, 8)),  # 8 channels per workgroup, 128 row groups
    ("bn_finalize", 129, 64, 1, 0, None, (0, 8, 1024, 2)),
    ("bn_bwd_finalize", 1, 16, 1, 0, None, (0, 2, 1024, 1)),
    ("channel_sum_finalize", 897, 256, 1, 0, None, (0, 32, 1024, 8)),
    ("bn_apply", 1003, 16, 1, 0, None, (1, 8, 256, 1)),
    ("bn_apply", 1003, 50, 1, 0, None, (0, 196, 256, 1)),
    ("bn_apply", 1003, 16, 0, 0, None, (0, 63, 256, 1)),
    ("bn_bwd_apply", 1003, 64, 1, 0, None, (1, 32, 256, 1)),
    ("bn_bwd_apply", 1003, 64, 1, 1, None, (2, 4, 256, 8)),
    ("bn_bwd_apply", 1003, 48, 1, 0, None, (1, 24, 256, 1)),
    ("bn_bwd_apply", 1003, 48, 1, 1, None, None),            # 256 % 6: no slab form
    ("bn_bwd_apply", 1003, 50, 1, 0, None, (0, 196, 256, 1)),
    ("bn_bwd_apply", 1003, 50, 1, 1, None, None),
    ("bn_bwd_apply", 1003, 64, 0, 1, None, None),
    ("bn_bwd_apply", 262143, 16, 1, 1, None, (2, 1024, 256, 2)),
    ("bn_bwd_apply", 262145, 16, 1, 1, None, (2, 1024, 256, 3)),
    ("bn_bwd_apply", 262144 + 256 + 5, 16, 1, 1, None, (2, 1024, 256, 3)),
    ("bn_bwd_apply", 262144 + 256 + 5, 16, 1, 0, None, (1, 2051, 256, 1)),
    ("bn_bwd_apply", (4194304 + 300) // 2, 16, 1, 0, None, (1, 16384, 256, 2)),
    ("bn_bwd_apply_pool", 1003, 50, 1, 0, None, None),
    ("bn_bwd_apply_pool", 1003, 64, 0, 0, None, None),
    ("bn_bwd_apply_pool", 1003, 64, 1, 1, None, (2, 4, 256, 8)),
    ("add", 2097152 - 3, 8, 1, 0, None, (0, 8192, 256, 1)),
    ("add", 2097152, 8, 1, 0, None, (1, 1024, 256, 1)),
    ("add", 2097152 + 77, 8, 1, 0, None, (0, 8192, 256, 2)),  # grid_for's cap
    ("add", 8 * (4194304 - 300), 8, 1, 0, None, (1, 16383, 256, 1)),
    ("add", 8 * (4194304 + 300), 8, 1, 0, None, (1, 16384, 256, 2)),  # vgrid's cap
    ("add", 8 * (4194304 + 300), 8, 0, 0, None, (0, 8192, 256, 17)),
    ("relu_bwd", 8 * 1003, 8, 1, 0, None, (1, 4, 256, 1)),
    ("dropout", 8 * 1003, 8, 0, 0, None, (0, 32, 256, 1)),
    ("cast", 8 * 1003 + 3, 8, 1, 0, None, (0, 32, 256, 1)),
    ("sigmoid", 2097152 + 77, 8, 1, 0, None, (0, 8192, 256, 2)),
    ("adam", 1048576 - 5, 8, 1, 0, None, (0, 4096, 256, 1)),
    ("adam", 1048576 + 77, 8, 1, 0, None, (0, 4096, 256, 2)),  # Adam's cap
    ("add_stats", 1003, 64, 1, 1, None, (2, 4, 256, 8)),
    ("add_stats", 1003, 48, 1, 1, None, None),
    ("add_stats", 1003, 64, 0, 1, None, None),
    ("relu_bwd_sum", 262144 + 256 + 5, 16, 1, 1, None, (2, 1024, 256, 3)),
    ("maxpool", 2, 16, 1, 0, (13, 35, 2, 2), (1, 2, 256, 1)),
    ("maxpool", 2, 16, 1, 0, (13, 35, 2, 3), (0, 9, 256, 1)),  # no 8-wide (2, 3) kernel
    ("maxpool", 2, 50, 1, 0, (13, 35, 2, 2), (0, 40, 256, 1)),
    ("maxpool", 2, 16, 1, 0, (1, 35, 2, 2), None),
    ("maxpool_bwd", 2, 64, 1, 0, (12, 36, 3, 3), (1, 3, 256, 1)),
    ("maxpool_bwd", 2, 64, 0, 0, (12, 36, 3, 3), (0, 216, 256, 1)),
    ("maxpool_fused", 2, 16, 1, 1, (14, 37, 1, 2), (2, 2, 256, 2)),
    ("maxpool_fused", 2, 16, 1, 0, (14, 37, 1, 2), (1, 4, 256, 1)),
    ("maxpool_fused", 2, 16, 1, 0, (14, 37, 2, 3), None),
    ("maxpool_fused", 2, 50, 1, 0, (14, 37, 2, 2), None),
    ("maxpool_bwd_argmax", 2, 16, 1, 0, (14, 37, 1, 2), (1, 4, 256, 1)),
    ("maxpool_bwd_argmax_bn", 2, 16, 1, 1, (13, 35, 1, 2), (2, 4, 256, 7)),  # 26 pooled rows over 4 workgroups
    ("avgpool", 2, 16, 1, 0, (13, 35, 2, 0), (1, 2, 256, 1)),
    ("avgpool", 2, 50, 1, 0, (13, 35, 2, 0), (0, 50, 256, 1)),
    ("avgpool_bwd", 2, 16, 0, 0, (13, 35, 2, 0), (0, 57, 256, 1)),
    ("axis_pool", 7, 50, 1, 0, None, (0, 2, 256, 1)),
    ("dense_fwd", 7, 50, 1, 0, None, (0, 2, 256, 1)),
    ("dense_bwd_w", 65, 50, 1, 0, None, (0, 813, 256, 1)),   # one wave per output, 4 per workgroup
    ("loss", 7, 50, 1, 0, None, (0, 7, 256, 1)),
]


@pytest.mark.parametrize("row", PLAN_TABLE, ids=lambda r: f"{r[0]}-{r[1]}x{r[2]}-a{r[3]}s{r[4]}" + ("-" + "x".join(map(str, r[5])) if r[5] else ""))
def test_nn_launch_info_table(row):
    from acfe._lib import NN_FIELDS, nn_launch_info

    op, rows, C, aligned, slab, geo, want = row
    got = nn_launch_info(op, rows, C, aligned, slab, geo)
    assert got == (None if want is None else dict(zip(NN_FIELDS, want))), (row, got)


def test_nn_launch_info_rejects_unknown_op():
    from acfe import _lib

    out = (_lib.I32 * 4)()
    assert _lib.lib.acfe_nn_launch_info(len(_lib.NN_OPS), 8, 8, 1, 0, out) == _lib.E_INVAL
    assert _lib.lib.acfe_nn_launch_info(0, 8, 8, 1, 0, None) == _lib.E_INVAL


# ------------------------------------------------------------------ the GPU variant tests' case table
import test_nn_variants_gpu as V  # noqa: E402  (imports no GPU state)

# every variant an entry point can launch
VARIANTS = {
    "bn_stats": {0, 1}, "channel_sum": {0, 1}, "bn_bwd_reduce": {0, 1}, "bn_finalize": {0}, "bn_bwd_finalize": {0},
    "channel_sum_finalize": {0}, "bn_apply": {0, 1}, "bn_bwd_apply": {0, 1, 2}, "bn_bwd_apply_pool": {1, 2},
    "add": {0, 1}, "relu_bwd": {0, 1}, "dropout": {0, 1}, "cast": {0, 1}, "add_stats": {2}, "relu_bwd_sum": {2},
    "maxpool": {0, 1}, "maxpool_bwd": {0, 1}, "maxpool_fused": {1, 2}, "maxpool_bwd_argmax": {1},
    "maxpool_bwd_argmax_bn": {2}, "avgpool": {0, 1}, "avgpool_bwd": {0, 1}, "axis_pool": {0}, "axis_pool_bwd": {0},
    "dense_fwd": {0}, "dense_bwd": {0}, "dense_bwd_w": {0}, "loss": {0}, "sigmoid": {0}, "adam": {0},
}
# (op, variant) whose grid cap a case must pass (>= 2 passes at the capped grid).  Left out: vgrid's
# cap on the eight-wide pools, which needs more than 33.5 M outputs -- a 67 M element input at (1, 2).
CAPPED = {("bn_apply", 0), ("bn_apply", 1), ("bn_bwd_apply", 0), ("bn_bwd_apply", 1), ("bn_bwd_apply", 2),
          ("bn_bwd_apply_pool", 2), ("maxpool", 0), ("maxpool_bwd", 0), ("avgpool", 0), ("avgpool_bwd", 0),
          ("maxpool_bwd_argmax_bn", 2),
          ("add", 0), ("add", 1), ("relu_bwd", 0), ("relu_bwd", 1), ("dropout", 0), ("dropout", 1), ("cast", 0),
          ("cast", 1), ("add_stats", 2), ("relu_bwd_sum", 2), ("maxpool_fused", 2), ("axis_pool", 0),
          ("axis_pool_bwd", 0), ("dense_fwd", 0), ("dense_bwd", 0), ("dense_bwd_w", 0), ("sigmoid", 0), ("adam", 0)}


def _plans(c):
    from acfe._lib import nn_launch_info

    return [(op, V.check_plan(c, nn_launch_info, op)) for op in [c["op"]] + V.COMPANIONS.get(c["op"], [])]


@pytest.mark.parametrize("c", V.ALL_CASES, ids=[f"{c['op']}-{c['id']}" for c in V.ALL_CASES])
def test_variant_case_reaches_its_branch(c):
    """Every case of tests/test_nn_variants_gpu.py has the launch plan it is
    named for (the GPU test asserts the same before it runs the kernel)."""
    _plans(c)


def test_variant_cases_cover_every_variant_and_cap():
    from acfe._lib import NN_OPS

    assert set(VARIANTS) == set(NN_OPS)
    seen, capped, flushed = set(), set(), set()
    for c in V.ALL_CASES:
        for op, plan in _plans(c):
            seen.add((op, plan["variant"]))
            if plan["how"] == "many":
                capped.add((op, plan["variant"]))
            if plan["how"] == "flush":
                flushed.add((op, plan["variant"]))
    want = {(op, v) for op, vs in VARIANTS.items() for v in vs}
    assert seen == want, (want - seen, seen - want)
    assert CAPPED <= capped, CAPPED - capped
    assert flushed == {("bn_stats", 0), ("bn_stats", 1)}
    assert len({(c["op"], c["id"]) for c in V.ALL_CASES}) == len(V.ALL_CASES)


@pytest.mark.parametrize("fn,c", V.sign_cases(), ids=[f"{c['op']}-{c['id']}" for _, c in V.sign_cases()])
def test_variant_case_sign_ambiguous_share(fn, c):
    """The elements whose sign test x scale + shift > 0 a contracted fma may
    decide either way are at most 1e-4 of every case's input (the GPU tests
    leave them out of the comparison)."""
    x, sc, sh = fn(c)
    share = V.ambiguous(x, sc, sh).double().mean().item()
    assert share <= 1e-4, share
