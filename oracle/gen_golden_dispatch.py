"""Record the answers of libacfe's host-only dispatch queries (no GPU call)
over a fixed shape grid: tests/golden/conv_dispatch_plan.json.

Test infrastructure only (see oracle/__init__.py).  The fixture pins which
kernel variant, grid and workspace every convolution launcher picks per shape,
so that a change of the host dispatch code that is meant to keep behaviour can
be checked exactly (tests/test_dispatch_plan.py).  Generate it from the build
whose behaviour is the reference -- the commit BEFORE such a change -- in the
default configuration (no ACFE_* dispatch switch in the environment):

  ACFE_LIB=/path/to/that/libacfe.so python oracle/gen_golden_dispatch.py

The 3x3 stride-1 "same" bf16 convolution of every (N, H, W, C, K) of the grid
is asked of each query; acfe_stem_blocks per image size and
acfe_conv2d_packed_shape per channel pair (both dtypes, both packings).
"""
import argparse
import ctypes
import itertools
import json
import os
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BF16 = 1

NS, HS, WS = (1, 4), (1, 8, 15, 16, 128), (16, 64, 100, 513)
CS, KS = (16, 24, 32, 64, 128, 192, 256), (16, 32, 64, 128, 256)
SHAPES = list(itertools.product(NS, HS, WS, CS, KS))  # (N, H, W, C, K)
IMAGES = list(itertools.product(NS, HS, WS))
CHANNELS = list(itertools.product(CS, KS))

SHAPE_QUERIES = ("halo_info", "halo_info_fold", "halo_info_unpool", "wgrad_bnbwd_rows", "wgrad_workspace",
                 "stats_rows", "dropout_keep_supported", "pool_supported", "rows_supported", "fwd_add_supported",
                 "bn_prologue_supported", "dgrad_bn_rows", "fwd_leaf")


def dispatch_switches():
    """The ACFE_* environment variables the library reads (csrc getenv calls)."""
    names = set()
    for f in (ROOT / "audio-training_amd" / "csrc").glob("*.hip"):
        names.update(re.findall(r'getenv\("(ACFE_[A-Z0-9_]+)"\)', f.read_text()))
    return sorted(names)


def _halo(lib, N, H, W, C, K, fold, unpool):
    out = (ctypes.c_int * 8)()
    return list(out) if lib.acfe_conv2d_wgrad_halo_info(N, H, W, C, K, fold, unpool, out) else 0


def _fwd_leaf(lib, N, H, W, C, K):
    """{leaf, a, b} of acfe_conv2d_fwd_info: no dropout, with a statistics slab."""
    out = (ctypes.c_int * 6)()
    return list(out)[:3] if lib.acfe_conv2d_fwd_info(N, H, W, C, K, 3, 3, 1, 1, 1, H, W, BF16, 0, 1, out) else 0


def shape_answers(lib, N, H, W, C, K):
    """One value per SHAPE_QUERIES entry (a halo plan is its 8 fields, the
    forward leaf its first 3, or 0)."""
    return [
        _halo(lib, N, H, W, C, K, 0, 0),
        _halo(lib, N, H, W, C, K, 1, 0),
        _halo(lib, N, H, W, C, K, 0, 1),
        lib.acfe_conv2d_wgrad_bnbwd_rows(N, H, W, C, K),
        lib.acfe_conv2d_wgrad_workspace(N, H, W, C, K, 3, 3, H, W),
        lib.acfe_conv2d_stats_rows(N * H * W, K),
        lib.acfe_conv2d_dropout_keep_supported(N, H, W, C, K, BF16),
        lib.acfe_conv2d_pool_supported(N, H, W, C, K, 3, 3, BF16),
        lib.acfe_conv2d_rows_supported(N, H, W, C, K, 3, 3, BF16),
        lib.acfe_conv2d_fwd_add_supported(N, H, W, C, K, BF16),
        lib.acfe_conv2d_bn_prologue_supported(N, H, W, C, K, BF16),
        lib.acfe_conv2d_dgrad_bn_rows(N, H, W, C, K, 3, 3, 1, BF16),
        _fwd_leaf(lib, N, H, W, C, K),
    ]


def image_answer(lib, N, H, W):
    return lib.acfe_stem_blocks(N, H, W)


def channel_answer(lib, C, K):
    """acfe_conv2d_packed_shape of the 3x3 weights: [rc, rows, cols] per (dtype, flip)."""
    out = []
    for dtype, flip in itertools.product((0, 1), (0, 1)):
        r, c = ctypes.c_int(0), ctypes.c_int(0)
        rc = lib.acfe_conv2d_packed_shape(K, 3, 3, C, dtype, flip, ctypes.byref(r), ctypes.byref(c))
        out.append([rc, r.value, c.value])
    return out


def record(lib):
    return {
        "shape_queries": list(SHAPE_QUERIES),
        "shapes": [list(s) + shape_answers(lib, *s) for s in SHAPES],
        "stem_blocks": [list(i) + [image_answer(lib, *i)] for i in IMAGES],
        "packed_shape": [list(ck) + channel_answer(lib, *ck) for ck in CHANNELS],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "conv_dispatch_plan.json"))
    a = ap.parse_args()
    set_ = [n for n in dispatch_switches() if n in os.environ]
    if set_:
        sys.exit(f"unset {set_}: the fixture is the default configuration's")
    sys.path.insert(0, str(ROOT / "audio-training_amd"))
    from acfe._lib import LIB_PATH, lib

    Path(a.out).write_text(json.dumps(record(lib), separators=(",", ":")) + "\n")
    print(f"{LIB_PATH}: {len(SHAPES)} shapes -> {a.out} ({Path(a.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
