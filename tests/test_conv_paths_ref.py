"""Host half of tests/test_conv_paths_gpu.py (no GPU).

1. The host-only launch queries (acfe_conv2d_fwd_info, acfe_conv2d_wgrad_info)
   answer, for every case of oracle/conv_paths_cases.py, the leaf / path the
   case table names: the tables and the dispatch agree before any GPU run.
2. The bounds the GPU test holds the kernels to leave room for a correct
   kernel: a CPU model of the kernel's arithmetic (float32 accumulation of the
   same operands, F.conv2d, rounded to bf16 for the bf16 cases) stays within
   them of the float64 reference, per element.
"""
import pytest
import torch

from oracle import conv_paths_cases as cc

BF16, F32 = 1, 0


def _dt(c):
    return BF16 if c.dtype == "bf16" else F32


@pytest.mark.parametrize("c", cc.FWD_CASES, ids=[c.id for c in cc.FWD_CASES])
def test_fwd_query_names_the_leaf(c):
    from acfe._lib import conv2d_fwd_info

    geo = cc.call_geometry(c)
    stats = c.kind == "fwd"
    info = conv2d_fwd_info(*geo, dtype=_dt(c), dropout=False, stats=stats)
    want = dict(leaf=c.leaf, a=c.a, b=c.b, **c.expect)
    assert {k: info[k] for k in want} == want, (info, want)
    if c.leaf == "rows":
        assert (info["grid_x"], info["grid_y"], info["tiles"]) == (0, 0, 0)
    else:
        assert info["grid_x"] >= 1 and info["grid_y"] >= 1 and info["tiles"] >= 1
    if c.kind == "fwd":
        # the fused Dropout runs on the same leaf, with or without a slab
        for st in (True, False):
            d = conv2d_fwd_info(*geo, dtype=_dt(c), dropout=True, stats=st)
            assert (d["leaf"], d["a"], d["b"]) == (c.leaf, c.a, c.b), (d, st)


def test_every_1x1_reg_instantiation_has_a_case():
    got = {(c.a, c.b) for c in cc.FWD_CASES if c.leaf == "1x1_reg"}
    assert got == {(1, 1), (1, 2), (1, 4), (1, 8), (2, 1), (2, 2), (4, 1), (4, 2)}


def test_fwd_query_rejects_invalid_arguments():
    from acfe._lib import I32, lib

    out = (I32 * 6)(*[7] * 6)
    assert lib.acfe_conv2d_fwd_info(1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 8, 8, 2, 0, 0, out) == 0
    assert list(out) == [0] * 6
    assert lib.acfe_conv2d_fwd_info(1, 8, 8, 0, 16, 3, 3, 1, 1, 1, 8, 8, 1, 0, 0, out) == 0
    assert lib.acfe_conv2d_fwd_info(1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 8, 8, 1, 0, 0, None) == 0
    out8 = (I32 * 8)(*[7] * 8)
    assert lib.acfe_conv2d_wgrad_info(1, 8, 8, 16, 16, 3, 3, 0, 8, 8, 1, out8) == 0
    assert list(out8) == [0] * 8
    assert lib.acfe_conv2d_wgrad_info(1, 8, 8, 16, 16, 3, 3, 1, 8, 8, 1, None) == 0


@pytest.mark.parametrize("c", cc.WGRAD_CASES, ids=[c.id for c in cc.WGRAD_CASES])
def test_wgrad_query_names_the_path(c):
    from acfe._lib import conv2d_wgrad_info, lib, wgrad_halo_info

    info = conv2d_wgrad_info(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.st, c.P, c.Q, dtype=_dt(c))
    assert {k: info[k] for k in c.want} == c.want, (info, c.want)
    if info["path"] == 0:
        # the plan is the workspace's: splits slabs of K x R S C floats
        assert lib.acfe_conv2d_wgrad_workspace(c.N, c.H, c.W, c.C, c.K, c.R, c.S, c.P, c.Q) == \
            info["splits"] * c.K * c.R * c.S * c.C
        assert info["splits"] % 8 == 0 and info["chunk"] % 64 == 0
        assert info["splits"] * info["chunk"] >= c.N * c.P * c.Q
    else:
        assert [info[k] for k in ("bmw", "fast_d", "fast_x", "splits", "chunk", "tiles", "reduce")] == [0] * 7
    if info["path"] == 1:
        # the halo query answers for "same" shapes; it agrees at the same P x Q
        assert wgrad_halo_info(c.N, c.P, c.Q, c.C, c.K) is not None


def test_wgrad_query_agrees_with_the_halo_query():
    """Over a grid of 3x3 stride-1 "same" bf16 shapes: path 1 exactly where
    acfe_conv2d_wgrad_halo_info takes the shape."""
    from acfe._lib import conv2d_wgrad_info, wgrad_halo_info

    for N in (1, 4):
        for H, W in ((8, 16), (15, 100), (128, 64)):
            for C in (8, 16, 24, 32, 64, 128, 192, 256):
                for K in (16, 20, 32, 64, 128, 256):
                    p = conv2d_wgrad_info(N, H, W, C, K, 3, 3, 1, H, W)["path"]
                    assert (p == 1) == (wgrad_halo_info(N, H, W, C, K) is not None), (N, H, W, C, K, p)


@pytest.fixture(scope="module")
def threads():
    old = torch.get_num_threads()
    torch.set_num_threads(min(old, 16))
    yield
    torch.set_num_threads(old)


@pytest.mark.parametrize("c", cc.FWD_CASES, ids=[c.id for c in cc.FWD_CASES])
def test_fwd_bound_leaves_room_for_f32_accumulation(c, threads):
    inp, w, b = cc.fwd_operands(c)
    exact = cc.fwd_result(c, inp, w, b)
    model = cc.fwd_result(c, inp, w, b, dt=torch.float32)
    if c.dtype == "bf16":
        model = model.to(cc.BF)
        bound = cc.bf16_bound(exact)
    else:
        bound = cc.f32_bound(c, inp, w, b)
    err = (model.to(cc.F64) - exact).abs()
    worst = float((err / bound).max())
    assert worst <= 1.0, (c.id, worst)


@pytest.mark.parametrize("c", cc.WGRAD_CASES, ids=[c.id for c in cc.WGRAD_CASES])
def test_wgrad_bounds_leave_room_for_f32_accumulation(c, threads):
    """A float32 weight gradient of the same operands (conv2d_weight in
    float32) within the GPU test's three bounds of the float64 one."""
    x, dy = cc.wgrad_operands(c)
    exact, mag = cc.wgrad_exact(c, x, dy)
    model, _ = cc.wgrad_exact(c, x.float(), dy.float(), dt=torch.float32)
    cc.assert_dw(model, exact, mag, c.N * c.P * c.Q, 8, c.id)
