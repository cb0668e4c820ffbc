"""Host-only dispatch queries of the convolution launchers (no GPU call):
the halo weight-gradient plan of the production layers
(acfe_conv2d_wgrad_halo_info), acfe_conv2d_dropout_keep_supported against the
launch it answers for, and ops.keep_bits_ok."""
import torch


def _pick(plan, *keys):
    return {k: plan[k] for k in keys}


def test_halo_plan_production_layers():
    """The plans of the layers the training step runs at 128 mels x 513 frames,
    4 clips: wr_resnet stage 1 (64 -> 64 and the block-0 16 -> 64 fold, one
    16-pixel remainder column for the 513th pixel), wr_resnet_bird's pooled
    128 -> 128 at 128 x 256 and its stage-2 128 -> 32 fold."""
    from acfe._lib import wgrad_halo_info as info

    p = info(4, 128, 513, 64, 64, fold=True)
    assert _pick(p, "cw", "nr", "edge", "qs", "qse") == dict(cw=64, nr=2, edge=1, qs=8, qse=1), p
    p = info(4, 128, 513, 16, 64, fold=True)
    assert _pick(p, "wp", "edge") == dict(wp=2, edge=1), p
    p = info(4, 128, 256, 128, 128, unpool=True)
    assert _pick(p, "edge") == dict(edge=0), p
    p = info(4, 64, 128, 128, 32, fold=True)
    assert _pick(p, "nr", "edge") == dict(nr=2, edge=0), p


def test_halo_plan_agrees_with_fold_rows():
    """fold = 1 says yes exactly where acfe_conv2d_wgrad_bnbwd_rows > 0, and
    rows = nchunk * sp; shapes the halo kernel does not take give None."""
    from acfe._lib import lib, wgrad_halo_info as info

    for shape in [(4, 128, 513, 64, 64), (3, 14, 100, 64, 64), (3, 15, 100, 64, 64), (3, 16, 100, 128, 64),
                  (3, 16, 100, 16, 64), (1, 16, 100, 16, 64), (3, 16, 100, 128, 128), (4, 32, 64, 128, 32),
                  (2, 16, 64, 192, 64), (2, 16, 64, 24, 64)]:
        rows = lib.acfe_conv2d_wgrad_bnbwd_rows(*shape)
        p = info(*shape, fold=True)
        assert (p is not None) == (rows > 0), (shape, rows, p)
        if p is not None:
            assert p["nchunk"] * p["sp"] == rows, (shape, rows, p)
    assert info(2, 16, 64, 24, 64) is None  # C = 24: the generic split-K kernel
    assert info(1, 16, 100, 16, 64) is None  # C = 16 -> K = 64 under 16 splits
    assert info(3, 16, 100, 128, 128) is not None and info(3, 16, 100, 128, 128, fold=True) is None


def test_keep_supported_agrees_with_launch_grid():
    """One statistics slab row (N H W <= 128) leaves none for the remainder-
    column launch of a W % 64 != 0 image: the keep forward would return
    ACFE_E_INVAL, so _supported says 0; two rows are enough."""
    from acfe._lib import lib

    assert lib.acfe_conv2d_dropout_keep_supported(1, 1, 100, 64, 64, 1) == 0
    assert lib.acfe_conv2d_dropout_keep_supported(1, 2, 100, 64, 64, 1) == 1
    assert lib.acfe_conv2d_dropout_keep_supported(1, 1, 64, 64, 64, 1) == 1  # no remainder columns
    assert lib.acfe_conv2d_dropout_keep_supported(4, 128, 513, 64, 64, 1) == 1


def test_keep_bits_ok_needs_the_fold(monkeypatch):
    """The keep bits' only reader is the BN-fold weight gradient, which takes
    row pairs: an odd H writes none."""
    from acfe import ops

    monkeypatch.setattr(ops, "KEEP_BITS", True)
    monkeypatch.setattr(ops, "FUSE_BN_BWD", True)
    w = torch.zeros((64, 3, 3, 64))
    for H, want in ((15, False), (16, True)):
        x = torch.zeros((2, H, 100, 64), dtype=torch.bfloat16)
        assert ops.keep_bits_ok(x, w, 1, 1, 1, H, 100, (0.1, 1), True) is want, H
        assert not ops.keep_bits_ok(x, w, 1, 1, 1, H, 100, None, True)
