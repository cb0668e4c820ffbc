"""Every kernel variant of csrc/nn.hip against the float64 / integer
restatements of oracle/nn_ref.py, through the C ABI on raw pointers.

Which kernel an entry point launches is decided by host predicates the caller
never sees, so every case first asserts acfe_nn_launch_info (the launchers'
own plan function): the `variant` the case is named for (0 scalar, 1 eight-
wide, 2 eight-wide on the slab grid) and its `passes` regime, then runs it.
tests/test_nn_ref.py checks the same table without a GPU and that every
variant of every op, and every grid cap, has a case.

Shapes and the branch each reaches
  rows 1003 (odd, 4 workgroups) at C 16 / 64 / 256   eight-wide, one pass; with
        a slab: 4 slab rows, grid below its cap.  C 48: eight-wide but
        256 % 6 != 0, no slab form, bn_apply's LDS path.  C 50 (the head's class
        count): C % 8 != 0 -> scalar.  C 64 viewed one element into its buffer:
        al16 fails -> scalar, and for the pointwise kernels bit-identical to
        the eight-wide output.
  rows 262144 + 256 + 5 at C 16   the slab grid (cap 1024) walks three times.
  n = 8 (4194304 + 300)           vgrid's cap 16384: two passes (flat bf16, or
                                  rows = n / 16 at C 16; 699101 rows at C 48,
                                  where the grid stride 2^22 is no multiple of
                                  C / 8 = 6 and a thread's channels change
                                  from pass to pass).
  n = 2097152 + 77 (41945 x 50 for [rows][C])   grid_for's cap 8192: two passes.
  n = 1048576 + 77                Adam's cap 4096.
  rows 524288 + 560 at C 256      a k_bn_stats8 thread sums 65 rows: one flush
                                  of its f32 partials into doubles (every 64).
  rows 1310720 + 50 at C 50       a k_bn_stats thread sums 257 rows (every 256).
  pools N 2, H x W 13 x 35, 12 x 36, 14 x 37 (0, 1, 2 leftover rows / columns
        over the windows), windows (1,2) (2,2) (3,3) eight-wide and (2,3) on the
        generic kernel, C 16 / 64 / 50; 2 x 260 x 1030 (1,2) at C 16 for the
        capped slab grid; 2 x 360 x 365 for acfe_bn_bwd_apply_pool / _sub on the
        capped slab grid; 2 x 301 x 303 at C 50 for grid_for's cap on the scalar
        max / average pools and their backwards; 2 x 1000 x 4 for the 16-row
        flush of k_maxpool_bwd8i_bn.  Only vgrid's cap on the eight-wide pools
        (a 67 M element input) is not run.
Indices >= 2^32 (the 64-bit hash path, i32 == false) need 8.6 GB tensors and
are out of scope.

Bounds (u = 2^-24; each derived, the measured value is printed beside it)
  exact     max-pool values, argmax bytes, ReLU / max-pool backward, cast,
            dropout's zeros, mask and kept values rnd(fl32(x scl)): the
            restatement evaluated in float32 with RNE to bf16, bit for bit.
  pointwise BN apply / backward apply, Add, average pool: f32 output
            |got - ref| <= 8 u sum|terms| (at most four f32 operations of half
            an ulp of the largest partial each = 2 u of the magnitude sum, times
            four); bf16 output: plus one bf16 ulp of ref.  After a dropout:
            scl x that bound, plus u |ref scl| for the multiply and one bf16
            ulp of ref scl for the second rounding.
  sign tests (x scale + shift > 0, x > 0, a + b > 0): elements whose float64
            pre-activation has |pre| <= 2^-22 (|x scale| + |shift|) may be
            decided either way by a contracted fma and are left out; their
            share, from the reference alone, must be <= 1e-4.  Sums over such
            elements widen a slab's bound by their |v|.  The dyadic cases (x on
            multiples of 1/8, scale a power of two, shift a multiple of 1/8)
            are exact in f32: nothing is left out and pre == 0 is not positive.
  slabs     per channel |sum_rows(slab) - ref| <= L u sum|v|, L the f32 run
            before the double accumulation: 64 k_bn_stats8 / k_bn_bwd_reduce8,
            256 the scalar forms, 16 pooled rows x kh kw window positions
            x ceil(Q C / 8 / 256) vectors of a row per thread for
            k_maxpool_bwd8i_bn; kernels that add doubles
            directly (k_bn_bwd_apply8, k_add8s, k_relu_bwd8s, k_maxpool8x):
            1e-12 sum|v|.  acfe_bn_bwd_apply_ex's second slab row is zero.
  finalizers against float64 of the same slab read back: 1e-6 relative (f64
            sums and a handful of f32 roundings); invstd at variance 0 is
            1 / sqrt(1e-3).  The inputs are chosen so that no output (shift =
            beta - mean scale, moving_mean = 0.99 m + 0.01 mean, coef c) is a
            difference of near-equal terms, which no f32 result holds relatively.
  head      rel-L2 1e-6 dense, 1e-5 loss and log-mean-exp gradients, 1e-6 Adam
            (test_ops_gpu.py's), at the capped sizes too.

Outputs, slabs and argmax bytes carry 256 sentinel bytes behind them (and the
one-element offset in front), intact after every call; outputs are NaN (or
sentinel) filled first, so an element never written shows.
"""
import math

import numpy as np
import pytest
import torch

from oracle import nn_ref as R

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
SENTINEL, TAIL = 0xA5, 256
SEED = (7 << 32) | 12345
ROWS = 1003
SLAB_ROWS = 262144 + 256 + 5
N_VCAP = 8 * (4194304 + 300)
N_GCAP = 2097152 + 77
ROWS_GCAP50 = 41945  # x 50 = 2097250 > 2097152
ROWS_VCAP48 = (4194304 + 300) // 6 + 1  # x 6 vectors = 4194606 > 4194304
N_ADAM = 1048576 + 77
HW = [(13, 35), (12, 36), (14, 37)]
WINDOWS = [(1, 2), (2, 2), (3, 3), (2, 3)]
CAPS = {"scalar": 8192, "vec": 16384, "slab": 1024, "adam": 4096}


def case(id, op, variant, passes, rows, C=8, aligned=True, slab=False, geo=None, **kw):
    """passes: "one" (a single pass), "uncapped" (grid below its cap),
    "many" (grid at its cap, >= 2 passes), "noflush" / "flush" (reductions:
    rows per thread within / past the f32 run)."""
    return dict(id=id, op=op, variant=variant, passes=passes, rows=rows, C=C, aligned=aligned, slab=slab, geo=geo, **kw)


def _rowsC(op, slab_variants=True, big_scalar=True, big_vec=True):
    """The [rows][C] cases of a pointwise op: small at every C, the misaligned
    view, and the capped grids."""
    out = [case(f"c{C}", op, 1, "one", ROWS, C) for C in (16, 64, 256, 48)]
    out += [case("c50-scalar", op, 0, "one", ROWS, 50), case("c64-misaligned", op, 0, "one", ROWS, 64, aligned=False)]
    if slab_variants:
        out += [case(f"c{C}-slab", op, 2, "uncapped", ROWS, C, slab=True) for C in (16, 64, 256)]
        out += [case("c16-slab-capped", op, 2, "many", SLAB_ROWS, 16, slab=True)]
    if big_scalar:
        out += [case("c50-scalar-capped", op, 0, "many", ROWS_GCAP50, 50)]
    if big_vec:
        out += [case("c16-vec-capped", op, 1, "many", N_VCAP // 16, 16),
                # the capped grid's stride, 2^22 vectors, is no multiple of C / 8 = 6: a thread's channels change per pass
                case("c48-vec-capped", op, 1, "many", ROWS_VCAP48, 48)]
    return out


def _reduce(op):
    return ([case(f"c{C}", op, 1, "noflush", ROWS, C) for C in (16, 64, 256, 48)] +
            [case("c50-scalar", op, 0, "noflush", ROWS, 50),
             case("c64-misaligned", op, 0, "noflush", ROWS, 64, aligned=False),
             case("c16-slab-capped", op, 1, "noflush", SLAB_ROWS, 16, grid=1024)])


def _flat(op):
    return [case("vec", op, 1, "one", 8 * ROWS), case("tail", op, 0, "one", 8 * ROWS + 3),
            case("misaligned", op, 0, "one", 8 * ROWS, aligned=False),
            case("vec-capped", op, 1, "many", N_VCAP), case("scalar-capped", op, 0, "many", N_GCAP)]


def _slab_only(op):
    return ([case(f"c{C}-slab", op, 2, "uncapped", ROWS, C, slab=True) for C in (16, 64, 256)] +
            [case("c16-slab-capped", op, 2, "many", SLAB_ROWS, 16, slab=True)])


def _pool_variant(C, kh, kw, aligned=True):
    return 1 if C % 8 == 0 and aligned and (kh, kw) != (2, 3) else 0


def _maxpool_cases(op):
    out = []
    for kh, kw in WINDOWS:
        for H, W in HW:
            for C, al in ((16, True), (64, True), (50, True), (16, False)):
                out.append(case(f"{kh}x{kw}-{H}x{W}-c{C}" + ("" if al else "-misaligned"), op, _pool_variant(C, kh, kw, al),
                                "one", 2, C, aligned=al, geo=(H, W, kh, kw)))
    return out


def _fused_cases(op, slabs):
    out = []
    for kh, kw in WINDOWS[:3]:
        for H, W in HW:
            for C in (16, 64):
                for sl in slabs:
                    out.append(case(f"{kh}x{kw}-{H}x{W}-c{C}" + ("-slab" if sl else ""), op, 2 if sl else 1,
                                    "uncapped" if sl else "one", 2, C, slab=sl, geo=(H, W, kh, kw)))
    return out


def _avg_cases(op):
    out = []
    for k in (2, 3):
        for H, W in HW:
            for C, al in ((16, True), (64, True), (50, True), (16, False)):
                out.append(case(f"k{k}-{H}x{W}-c{C}" + ("" if al else "-misaligned"), op, 1 if C % 8 == 0 and al else 0,
                                "one", 2, C, aligned=al, geo=(H, W, k, 0)))
    return out


STATS = _reduce("bn_stats") + [
    case("c256-flush64", "bn_stats", 1, "flush", 524288 + 560, 256),
    case("c50-scalar-flush256", "bn_stats", 0, "flush", 1310720 + 50, 50)]
CHANNEL_SUM = [case("c64", "channel_sum", 1, "noflush", ROWS, 64), case("c50-scalar", "channel_sum", 0, "noflush", ROWS, 50)]
SLAB_NROWS = [1, 7, 129, 897, 1024]
FINALIZE = [case(f"{op}-n{n}", op, 0, "uncapped", n, 50) for op in ("bn_finalize", "bn_bwd_finalize", "channel_sum_finalize")
            for n in SLAB_NROWS]
APPLY = _rowsC("bn_apply", slab_variants=False)
REDUCE = _reduce("bn_bwd_reduce")
BWD_APPLY = _rowsC("bn_bwd_apply")
BWD_POOL = [case(f"k{k}-{H}x{W}-c{C}" + ("-slab" if sl else ""), "bn_bwd_apply_pool", 2 if sl else 1,
                 "uncapped" if sl else "one", 2 * H * W, C, slab=sl, hw=(H, W), k=k)
            for k in (2, 3) for H, W in HW[::2] for C in (16, 64) for sl in (False, True)] + [
    # 262800 pixels: the slab grid (cap 1024) walks three times, the pixel -> window arithmetic past one pass
    case("k2-360x365-c16-slab-capped", "bn_bwd_apply_pool", 2, "many", 2 * 360 * 365, 16, slab=True, hw=(360, 365), k=2)]
ADD, RELU_BWD, DROPOUT, CAST = _flat("add"), _flat("relu_bwd"), _flat("dropout"), _flat("cast")
ADD_STATS, RELU_BWD_SUM = _slab_only("add_stats"), _slab_only("relu_bwd_sum")
# 2 x 301 x 303 at C 50: 2.27 M outputs and 9.1 M inputs, past grid_for's 8192 x 256 on the scalar kernels
MAXPOOL = _maxpool_cases("maxpool") + [
    case("2x2-301x303-c50-scalar-capped", "maxpool", 0, "many", 2, 50, geo=(301, 303, 2, 2))]
MAXPOOL_FUSED = _fused_cases("maxpool_fused", (False, True)) + [
    case("1x2-260x1030-c16-slab-capped", "maxpool_fused", 2, "many", 2, 16, slab=True, geo=(260, 1030, 1, 2))]
MAXPOOL_BN = _fused_cases("maxpool_bwd_argmax_bn", (True,)) + [
    case("1x2-260x1030-c16-slab-capped", "maxpool_bwd_argmax_bn", 2, "many", 2, 16, slab=True, geo=(260, 1030, 1, 2)),
    # tall and narrow: 2000 pooled rows over 32 workgroups, 63 each: k_maxpool_bwd8i_bn's flush every 16 rows
    case("1x2-1000x4-c16-flush16", "maxpool_bwd_argmax_bn", 2, "uncapped", 2, 16, slab=True, geo=(1000, 4, 1, 2),
         flush16=True)]
AVGPOOL = _avg_cases("avgpool") + [
    case("k2-301x303-c50-scalar-capped", "avgpool", 0, "many", 2, 50, geo=(301, 303, 2, 0))]
HEAD = [
    case("axis-small", "axis_pool", 0, "one", 7, 50, L=5), case("axis-capped", "axis_pool", 0, "many", ROWS_GCAP50, 50, L=3),
    case("dense-small", "dense_fwd", 0, "one", 7, 50, I=13), case("dense-capped", "dense_fwd", 0, "many", ROWS_GCAP50, 50, I=51),
    case("densew-capped", "dense_bwd_w", 0, "many", 701, 50, B=37),
    case("loss-small", "loss", 0, "one", 7, 50), case("loss-wide", "loss", 0, "many", 5, 300),
    case("sigmoid-small", "sigmoid", 0, "one", 8 * ROWS + 3), case("sigmoid-capped", "sigmoid", 0, "many", N_GCAP),
    case("adam-small", "adam", 0, "one", 8 * ROWS + 3), case("adam-capped", "adam", 0, "many", N_ADAM),
]
# ops the pool / head tests run beside the op their cases are named for (same geometry, same variant)
COMPANIONS = {"maxpool": ["maxpool_bwd"], "maxpool_fused": ["maxpool_bwd_argmax"], "avgpool": ["avgpool_bwd"],
              "axis_pool": ["axis_pool_bwd"], "dense_fwd": ["dense_bwd"]}
ALL_CASES = (STATS + CHANNEL_SUM + FINALIZE + APPLY + REDUCE + BWD_APPLY + BWD_POOL + ADD + RELU_BWD + DROPOUT + CAST +
             ADD_STATS + RELU_BWD_SUM + MAXPOOL + MAXPOOL_FUSED + MAXPOOL_BN + AVGPOOL + HEAD)


def check_plan(c, info, op=None):
    """The launch plan of case c (of a companion op run beside it when `op` is
    given) is the variant and passes regime the case is named for; returns it."""
    companion = op is not None and op != c["op"]
    op = op or c["op"]
    slab, variant = c["slab"], c["variant"]
    if op == "maxpool_bwd_argmax":  # never writes a slab
        slab, variant = False, 1
    plan = info(op, c["rows"], c["I"] if op == "dense_bwd" else c["C"], c["aligned"], slab, c["geo"])
    assert plan is not None, (c["id"], op, "ACFE_E_INVAL")
    assert plan["variant"] == variant, (c["id"], op, plan)
    cap = CAPS["adam"] if op == "adam" else 8192 if op == "dense_bwd_w" else CAPS[("scalar", "vec", "slab")[variant]]
    how = c["passes"]
    if companion and how != "one" and op not in ("axis_pool_bwd", "dense_bwd", "maxpool_bwd", "avgpool_bwd"):
        how = None
    if how == "one":
        assert plan["passes"] == 1, (c["id"], op, plan)
    elif how == "uncapped":
        assert plan["grid"] < cap, (c["id"], op, plan)
    elif how == "many":
        assert plan["passes"] >= 2 and (op == "loss" or plan["grid"] == cap), (c["id"], op, plan)
    elif how in ("flush", "noflush"):
        assert (plan["passes"] > (64 if variant else 256)) == (how == "flush"), (c["id"], op, plan)
        assert plan["grid"] == c.get("grid", plan["grid"]), (c["id"], plan)
    plan["how"] = how
    return plan


def _ids(cases):
    return [c["id"] for c in cases]


# ------------------------------------------------------------------ device buffers
@pytest.fixture(scope="module")
def env(cuda):
    from acfe import ops
    from acfe._lib import call, lib, nn_launch_info
    from acfe._torch import ptr, stream

    return ops, call, lib, ptr, stream, nn_launch_info


class Buf:
    """A device tensor inside a sentinel-filled byte buffer: TAIL sentinel bytes
    behind it and, when misaligned, one element of sentinel in front (the view
    then starts one element past a 16-B boundary)."""

    def __init__(self, shape, dtype, device, aligned=True, fill=None):
        es = torch.empty((), dtype=dtype).element_size()
        n = math.prod(shape) * es
        self.off = 0 if aligned else es
        self.raw = torch.full((self.off + n + TAIL,), SENTINEL, dtype=torch.uint8, device=device)
        self.t = self.raw[self.off:self.off + n].view(dtype).view(shape)
        assert (self.t.data_ptr() % 16 == 0) == aligned
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.raw[:self.off] == SENTINEL).all() and (self.raw[-TAIL:] == SENTINEL).all())


def put(t, dtype, device, aligned=True):
    b = Buf(tuple(t.shape), dtype, device, aligned)
    b.t.copy_(t.to(dtype))
    return b


def out_buf(shape, dtype, device, aligned=True):
    return Buf(shape, dtype, device, aligned, fill=float("nan") if dtype.is_floating_point else SENTINEL)


def code(dtype):
    return 1 if dtype == BF else 0


def act(shape, seed, scale=1.0):
    """bf16-rounded normals, in float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).to(F64)


def coarse(shape, seed):
    """Multiples of 1/2 in [-2, 2]: ties in every max-pool window."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).to(F64) * 0.5


def params(C, seed):
    """scale with both signs, shift, as the f32 values the kernels read."""
    g = torch.Generator().manual_seed(seed)
    sc = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    sh = torch.randn(C, generator=g) * 0.3
    return sc.to(F32).to(F64), sh.to(F32).to(F64)


def ulp_bf16(ref):
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(ref), e - 8)


def stored(t, dtype):
    return R.to_bf16(t) if dtype == BF else R.to_f32(t)


def check_pointwise(what, got, ref, mag, dtype, sel=None, extra=None):
    bound = 8 * U * mag + (ulp_bf16(ref) if dtype == BF else 0)
    if extra is not None:
        bound = bound + extra
    err = (got.detach().to(F64).cpu() - ref).abs()
    bad = ~(err <= bound)  # (a NaN -- an element never written -- is bad)
    if sel is not None:
        bad = bad & sel
    ratio = torch.where(sel if sel is not None else torch.ones_like(bad), err / bound.clamp_min(1e-300),
                        torch.zeros_like(err)).nan_to_num(nan=float("inf")).max().item()
    print(f"{what}: max |err| / bound {ratio:.3f} (bound 8 u sum|terms|" + (" + 1 bf16 ulp)" if dtype == BF else ")"))
    assert not bad.any(), (what, int(bad.sum()), ratio)


def ambiguous(x, sc, sh):
    """Elements whose BN sign test a contracted fma may decide either way."""
    return (x * sc + sh).abs() <= 2.0 ** -22 * ((x * sc).abs() + sh.abs())


def check_share(what, amb):
    share = amb.double().mean().item()
    print(f"{what}: sign-ambiguous share {share:.2e} (bound 1e-4)")
    assert share <= 1e-4, (what, share)


def check_slab(what, slab, ref, mag, L, C, slack=None):
    """sum over the slab's rows against the float64 sums ref[2][C]."""
    s = slab.detach().cpu().sum(0)[:, :C]
    bound = (L * U if L > 1 else 1e-12) * mag
    if slack is not None:
        bound = bound + slack
    err = (s - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max().item()
    print(f"{what}: slab max |err| / bound {ratio:.3e} (bound {'%d u' % L if L > 1 else '1e-12'} sum|v|)")
    assert (err <= bound).all(), (what, ratio)


def check_rel(what, got, ref, tol=1e-6):
    got = got.detach().to(F64).cpu()
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-30)).nan_to_num(nan=float("inf")).max().item()
    print(f"{what}: max rel err {err:.3e} (bound {tol:g})")
    assert err <= tol, (what, err)


def rel_l2(a, b):
    a, b = a.detach().to(F64).cpu(), b.detach().to(F64).cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def slab_rows(lib, rows):
    return lib.acfe_reduce_blocks(rows)


# ------------------------------------------------------------------ BN forward
def _stats_input(c, cuda):
    rows, C = c["rows"], c["C"]
    if rows * C > 40_000_000:  # the two flush cases: generated on the device, copied back once
        g = torch.Generator(device=cuda).manual_seed(rows)
        xd = torch.randn((rows, C), generator=g, device=cuda).to(BF)
        xd[:, 1] = 0.75
        return xd.cpu().to(F64), xd
    x = act((rows, C), 100 + C)
    x[:, 1] = 0.75  # a constant channel: variance 0
    return x, None


@pytest.mark.parametrize("c", STATS, ids=_ids(STATS))
def test_bn_stats_finalize_apply_chain(env, cuda, c):
    """acfe_bn_stats (k_bn_stats / k_bn_stats8, with and without a flush of the
    f32 partials) against float64 sums, then acfe_bn_finalize (training) on
    that slab against float64 of the slab read back."""
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    rows, C, al = c["rows"], c["C"], c["aligned"]
    x, xd = _stats_input(c, cuda)
    dtypes = (BF,) if rows > 2000 else (BF, F32)
    for dt in dtypes:
        xb = xd if xd is not None else put(x, dt, cuda, al).t
        nb = slab_rows(lib, rows)
        assert nb == plan["grid"]
        slab = out_buf((nb, 2, C), F64, cuda)
        call("acfe_bn_stats", ptr(xb), rows, C, code(dt), ptr(slab.t), stream())
        torch.cuda.synchronize()
        assert slab.intact()
        ref, mag = R.bn_stats(x), torch.stack([x.abs().sum(0), (x * x).sum(0)])
        check_slab(f"bn_stats {c['id']} {dt}", slab.t, ref, mag, 64 if c["variant"] else 256, C)
        # finalize, training: from the slab as the device holds it
        g = torch.Generator().manual_seed(C)
        # |gamma|, |beta|, moving_mean >= 0.5 against |mean| of order 0.03 (0.75 in the constant
        # channel, where |mean scale| > 11): no output is a difference of near-equal terms
        gamma, beta, mm0, mv0 = signed(C, g), signed(C, g), positive(C, g), positive(C, g)
        outs = {k: out_buf((C,), F32, cuda) for k in ("scale", "shift", "mean", "invstd")}
        mm, mv = put(mm0, F32, cuda), put(mv0, F32, cuda)
        gm, bt = put(gamma, F32, cuda), put(beta, F32, cuda)
        call("acfe_bn_finalize", ptr(slab.t), nb, C, C, float(rows), ptr(gm.t), ptr(bt.t), 1e-3, 0.99, ptr(mm.t),
             ptr(mv.t), 1, ptr(outs["scale"].t), ptr(outs["shift"].t), ptr(outs["mean"].t), ptr(outs["invstd"].t),
             stream())
        torch.cuda.synchronize()
        fin = R.bn_finalize(slab.t.cpu().sum(0), rows, gamma, beta, mm0, mv0)
        for k, b in outs.items():
            assert b.intact()
            check_rel(f"bn_finalize {c['id']} {k}", b.t, fin[k])
        check_rel(f"bn_finalize {c['id']} moving_mean", mm.t, fin["moving_mean"])
        check_rel(f"bn_finalize {c['id']} moving_var", mv.t, fin["moving_var"])
        assert mm.intact() and mv.intact()
        # the constant channel: variance 0 (up to the rounding of 0.5625 - 0.75^2)
        check_rel(f"bn_finalize {c['id']} invstd at variance 0", outs["invstd"].t[1:2],
                  torch.tensor([1 / math.sqrt(1e-3)], dtype=F64))


def signed(C, g):
    """Magnitudes in [0.5, 1.5) with random signs, as f32 values."""
    return ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.4, -1.0, 1.0)).to(F32).to(F64)


def positive(C, g):
    return (torch.rand(C, generator=g) + 0.5).to(F32).to(F64)


@pytest.mark.parametrize("c", CHANNEL_SUM, ids=_ids(CHANNEL_SUM))
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_channel_sum(env, cuda, c, beta):
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    rows, C = c["rows"], c["C"]
    x = act((rows, C), 7)
    xb = put(x, BF, cuda)
    slab = out_buf((slab_rows(lib, rows), 2, C), F64, cuda)
    old = torch.arange(C, dtype=F64) + 1000  # (the column sums, of order 30, cannot cancel it)
    out = put(old, F32, cuda)
    call("acfe_channel_sum", ptr(xb.t), rows, C, 1, ptr(slab.t), ptr(out.t), beta, stream())
    torch.cuda.synchronize()
    assert slab.intact() and out.intact()
    check_slab(f"channel_sum {c['id']}", slab.t, R.bn_stats(x), torch.stack([x.abs().sum(0), (x * x).sum(0)]),
               64 if c["variant"] else 256, C)
    check_rel(f"channel_sum {c['id']} beta {beta} out", out.t, beta * old + slab.t.cpu().sum(0)[0])


def _synthetic_slab(nrows, C, ld, seed, cuda):
    """A slab of `nrows` rows whose sums give a mean in [0.5, 0.75] and a
    variance of about 1 at count 16 nrows (positive sums: the finalizers'
    outputs are then no differences of near-equal terms, given the signs their
    callers choose); the columns past C are NaN (never to be read)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.full((nrows, 2, ld), float("nan"), dtype=F64)
    s[:, 0, :C] = 8 + 4 * torch.rand((nrows, C), generator=g, dtype=F64)
    s[:, 1, :C] = 16 * (1 + torch.rand((nrows, C), generator=g, dtype=F64))
    return s, put(s, F64, cuda)


@pytest.mark.parametrize("c", FINALIZE, ids=_ids(FINALIZE))
def test_finalizers_on_slabs(env, cuda, c):
    """The three slab finalizers at nrows in {1, 7, 129, 897, 1024} (1, 2 and 8
    loads per thread of slab_sum, ragged and full row groups) and, for
    acfe_bn_finalize, a padded leading dimension ld > C; eval mode; accumulate
    0 / 1; beta 0 / 1."""
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    nrows, C, op = c["rows"], c["C"], c["op"]
    assert plan["block"] == 1024 and plan["passes"] == -(-nrows // 128)
    count = 16.0 * nrows
    g = torch.Generator().manual_seed(nrows)
    f32 = lambda t: t.to(F32).to(F64)  # noqa: E731
    if op == "bn_finalize":
        for ld in (C, C + 14):
            s, sb = _synthetic_slab(nrows, C, ld, nrows + ld, cuda)
            gamma, mm0, mv0 = signed(C, g), positive(C, g), positive(C, g)
            beta = -torch.sign(gamma) * positive(C, g)  # shift = beta - mean scale: both terms of one sign
            for training in (1, 0):
                outs = {k: out_buf((C,), F32, cuda) for k in ("scale", "shift", "mean", "invstd")}
                mm, mv = put(mm0, F32, cuda), put(mv0, F32, cuda)
                gm, bt = put(gamma, F32, cuda), put(beta, F32, cuda)
                call("acfe_bn_finalize", ptr(sb.t), nrows, ld, C, count, ptr(gm.t), ptr(bt.t), 1e-3, 0.99, ptr(mm.t), ptr(mv.t), training, ptr(outs["scale"].t),
                     ptr(outs["shift"].t), ptr(outs["mean"].t), ptr(outs["invstd"].t), stream())
                torch.cuda.synchronize()
                fin = R.bn_finalize(s[:, :, :C].sum(0), count, gamma, beta, mm0, mv0, training=bool(training))
                for k, b in outs.items():
                    assert b.intact()
                    check_rel(f"bn_finalize n{nrows} ld{ld} training{training} {k}", b.t, fin[k])
                check_rel(f"bn_finalize n{nrows} ld{ld} training{training} moving_mean", mm.t, fin["moving_mean"])
                check_rel(f"bn_finalize n{nrows} ld{ld} training{training} moving_var", mv.t, fin["moving_var"])
                assert mm.intact() and mv.intact() and sb.intact()
    elif op == "bn_bwd_finalize":
        s, sb = _synthetic_slab(nrows, C, C, nrows, cuda)
        # a negative mean: coef c = -scale (mg - mgx invstd mean) adds two terms of one sign
        scale, mean, invstd = signed(C, g), -positive(C, g), positive(C, g)
        dgamma, dbeta, coef = R.bn_bwd_finalize(s.sum(0), count, scale, mean, invstd)
        old_g, old_b = f32(50 + torch.rand(C, generator=g)) * nrows, f32(50 + torch.rand(C, generator=g)) * nrows
        for acc in (0, 1):
            dg, db = put(old_g, F32, cuda), put(old_b, F32, cuda)
            cf = out_buf((3, C), F32, cuda)
            pb = [put(t, F32, cuda) for t in (scale, mean, invstd)]
            args = (ptr(sb.t), nrows, C, count, *[ptr(b.t) for b in pb], ptr(dg.t), ptr(db.t), ptr(cf.t))
            if acc:
                call("acfe_bn_bwd_finalize_ex", *args, 1, stream())
            else:
                call("acfe_bn_bwd_finalize", *args, stream())
            torch.cuda.synchronize()
            assert dg.intact() and db.intact() and cf.intact()
            check_rel(f"bn_bwd_finalize n{nrows} acc{acc} dgamma", dg.t, dgamma + acc * old_g)
            check_rel(f"bn_bwd_finalize n{nrows} acc{acc} dbeta", db.t, dbeta + acc * old_b)
            check_rel(f"bn_bwd_finalize n{nrows} acc{acc} coef", cf.t, coef)
    else:
        s, sb = _synthetic_slab(nrows, C, C, nrows, cuda)
        old = f32(50 + torch.rand(C, generator=g)) * nrows
        for beta in (0.0, 1.0):
            out = put(old, F32, cuda)
            call("acfe_channel_sum_finalize", ptr(sb.t), nrows, C, beta, ptr(out.t), stream())
            torch.cuda.synchronize()
            assert out.intact()
            check_rel(f"channel_sum_finalize n{nrows} beta{beta}", out.t, s[:, 0].sum(0) + beta * old)


def _bn_apply_run(env, cuda, x, sc, sh, relu, dti, dto, aligned):
    ops, call, lib, ptr, stream, info = env
    rows, C = x.shape
    xb, y = put(x, dti, cuda, aligned), out_buf((rows, C), dto, cuda, aligned)
    scb, shb = put(sc, F32, cuda), put(sh, F32, cuda)
    call("acfe_bn_apply", ptr(xb.t), code(dti), rows, C, ptr(scb.t), ptr(shb.t), relu, ptr(y.t), code(dto), stream())
    torch.cuda.synchronize()
    assert y.intact() and xb.intact()
    return y.t


@pytest.mark.parametrize("c", APPLY, ids=_ids(APPLY))
def test_bn_apply(env, cuda, c):
    """acfe_bn_apply: k_bn_apply8 (register path at 256 % (C / 8) == 0, LDS
    path at C = 48) and k_bn_apply; relu 0 / 1, f32 and bf16 in and out."""
    check_plan(c, env[5])
    rows, C, al = c["rows"], c["C"], c["aligned"]
    x = act((rows, C), 200 + C)
    sc, sh = params(C, C)
    big = rows > 2000
    for relu in ((1,) if big else (0, 1)):
        ref = R.bn_apply(x, sc, sh, relu)
        mag = (x * sc).abs() + sh.abs()
        for dti, dto in (((BF, BF),) if big else ((BF, BF), (BF, F32), (F32, BF), (F32, F32))):
            got = _bn_apply_run(env, cuda, x, sc, sh, relu, dti, dto, al)
            check_pointwise(f"bn_apply {c['id']} relu{relu} {dti}->{dto}", got, ref, mag, dto)
            if not al:  # the scalar kernel of the misaligned view stores what the eight-wide one does
                assert check_plan(dict(c, aligned=True, variant=1), env[5])["variant"] == 1
                assert torch.equal(got, _bn_apply_run(env, cuda, x, sc, sh, relu, dti, dto, True))


def dyadic(rows, C, seed):
    """x on multiples of 1/8, scale +- a power of two, shift a multiple of 1/8,
    with exact zeros of x scale + shift: exact in f32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 17, (rows, C), generator=g).to(F64) / 8
    sc = torch.tensor([0.5, -2.0, 1.0, -0.25] * (C // 4), dtype=F64)
    sh = torch.randint(-8, 9, (C,), generator=g).to(F64) / 8
    assert ((x * sc + sh) == 0).double().mean() > 0.005
    return x, sc, sh


@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "scalar"])
def test_bn_apply_dyadic(env, cuda, aligned):
    """Exact arithmetic: bit for bit, and a pre-activation of exactly 0 stores 0."""
    c = case("dyadic", "bn_apply", int(aligned), "one", ROWS, 16, aligned=aligned)
    check_plan(c, env[5])
    x, sc, sh = dyadic(ROWS, 16, 1)
    for relu in (0, 1):
        got = _bn_apply_run(env, cuda, x, sc, sh, relu, BF, F32, aligned)
        assert torch.equal(got.cpu().to(F64), R.bn_apply(x, sc, sh, relu))


# ------------------------------------------------------------------ BN backward
def _stat_params(x, seed):
    C = x.shape[1]
    g = torch.Generator().manual_seed(seed)
    mean = (x.mean(0) + 0.01 * torch.randn(C, generator=g, dtype=F64)).to(F32).to(F64)
    invstd = (1 / torch.sqrt(x.var(0, unbiased=False) + 1e-3)).to(F32).to(F64)
    return mean, invstd


# The (x, scale, shift) whose sign test x scale + shift > 0 a case's kernels decide: one function
# per family, so that tests/test_nn_ref.py checks the sign-ambiguous share of every case on the CPU
def reduce_sign_inputs(c):
    x = act((c["rows"], c["C"]), 300 + c["C"])
    x[:, 1] = 0.75
    return (x,) + params(c["C"], c["C"] + 1)


def bwd_apply_sign_inputs(c):
    return (act((c["rows"], c["C"]), 400 + c["C"]),) + params(c["C"], c["C"] + 2)


def bwd_pool_sign_inputs(c):
    return (act((c["rows"], c["C"]), 500 + c["C"]),) + params(c["C"], c["C"] + 3)


def maxpool_bn_sign_inputs(c):
    H, W = c["geo"][:2]
    return (act((2 * H * W, c["C"]), 720 + c["C"]),) + params(c["C"], c["C"] + 4)


def sign_cases():
    return ([(reduce_sign_inputs, c) for c in REDUCE] + [(bwd_apply_sign_inputs, c) for c in BWD_APPLY] +
            [(bwd_pool_sign_inputs, c) for c in BWD_POOL] + [(maxpool_bn_sign_inputs, c) for c in MAXPOOL_BN])


@pytest.mark.parametrize("c", REDUCE, ids=_ids(REDUCE))
@pytest.mark.parametrize("relu", [0, 1])
def test_bn_bwd_reduce(env, cuda, c, relu):
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    rows, C, al = c["rows"], c["C"], c["aligned"]
    x, sc, sh = reduce_sign_inputs(c)
    dy = act((rows, C), 301 + C, 0.5)
    mean, invstd = _stat_params(x, C)
    amb = ambiguous(x, sc, sh) if relu else torch.zeros_like(x, dtype=torch.bool)
    check_share(f"bn_bwd_reduce {c['id']}", amb)
    g = R.bn_masked_grad(dy, x, sc, sh, relu)
    v = g * (x - mean) * invstd
    vall = dy * (x - mean) * invstd
    ref, mag = torch.stack([g.sum(0), v.sum(0)]), torch.stack([g.abs().sum(0), v.abs().sum(0)])
    slack = torch.stack([(dy.abs() * amb).sum(0), (vall.abs() * amb).sum(0)])
    dts = ((BF, BF),) if rows > 2000 else ((BF, BF), (F32, BF), (BF, F32))
    for dtg, dtx in dts:
        dyb, xb = put(dy, dtg, cuda, al), put(x, dtx, cuda, al)
        slab = out_buf((plan["grid"], 2, C), F64, cuda)
        assert plan["grid"] == slab_rows(lib, rows)
        pb = [put(t, F32, cuda) for t in (sc, sh, mean, invstd)]
        call("acfe_bn_bwd_reduce", ptr(dyb.t), code(dtg), ptr(xb.t), code(dtx), rows, C, *[ptr(b.t) for b in pb], relu,
             ptr(slab.t), stream())
        torch.cuda.synchronize()
        assert slab.intact()
        check_slab(f"bn_bwd_reduce {c['id']} relu{relu} {dtg}/{dtx}", slab.t, ref, mag, 64 if c["variant"] else 256, C, slack)


def _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, add, rate, slab_on, dto, aligned, fn="ex", pool=None):
    """One acfe_bn_bwd_apply* call: (dx, slab or None)."""
    ops, call, lib, ptr, stream, info = env
    rows, C = x.shape
    dyb, xb = put(dy, BF, cuda, aligned), put(x, BF, cuda, aligned)
    dx = out_buf((rows, C), dto, cuda, aligned)
    ab = None if add is None else put(add, dto, cuda, aligned)
    slab = out_buf((slab_rows(lib, rows), 2, C), F64, cuda) if slab_on else None
    held = [put(t, F32, cuda) for t in (sc, sh, coef)]
    pp, cf = [ptr(held[0].t), ptr(held[1].t)], ptr(held[2].t)
    head = (ptr(dyb.t), 1, ptr(xb.t), 1)
    if fn == "plain":
        call("acfe_bn_bwd_apply", *head, rows, C, *pp, relu, cf, None if ab is None else ptr(ab.t), ptr(dx.t), code(dto),
             stream())
    elif fn == "dropout":
        call("acfe_bn_bwd_apply_dropout", *head, rows, C, *pp, relu, cf, rate, SEED, ptr(dx.t), code(dto), stream())
    elif fn == "ex":
        call("acfe_bn_bwd_apply_ex", *head, rows, C, *pp, relu, cf, None if ab is None else ptr(ab.t), rate, SEED,
             ptr(dx.t), code(dto), None if slab is None else ptr(slab.t), stream())
    else:
        N, H, W, k, gp = pool
        gb = put(gp, dto, cuda)
        call("acfe_bn_bwd_apply_" + fn, *head, N, H, W, C, *pp, relu, cf, ptr(gb.t), k, ptr(dx.t), code(dto),
             None if slab is None else ptr(slab.t), stream())
    torch.cuda.synchronize()
    assert dx.intact() and (slab is None or slab.intact())
    return dx.t, None if slab is None else slab.t


def _bwd_apply_check(what, got, slab, dy, x, sc, sh, coef, relu, add, rate, dto, amb):
    """dx and the channel-sum slab of one backward-apply call against float64;
    amb: the sign-ambiguous elements (from the reference, before the launch)."""
    C = x.shape[1]
    if not relu & 1:
        amb = torch.zeros_like(amb)
    ref = R.bn_bwd_apply(dy, x, sc, sh, coef, relu, add)
    g = R.bn_masked_grad(dy, x, sc, sh, relu & 1)
    mag = (coef[0] * g).abs() + (coef[1] * x).abs() + coef[2].abs() + (0 if add is None else add.abs())
    mag = mag + (coef[0] * dy).abs() * amb  # (not selected, but keeps the bound finite there)
    sel = ~amb
    if rate > 0:
        keep = torch.from_numpy(R.dropout_keep(SEED, np.arange(x.numel(), dtype=np.uint64), rate)).view(x.shape)
        scl = float(R.dropout_scale(rate))
        gotc = got.detach().to(F64).cpu()
        assert (gotc[~keep] == 0).all(), (what, "a dropped element is not 0")
        pre_bound = 8 * U * mag + (ulp_bf16(ref) if dto == BF else 0)
        refd = ref * scl
        extra = scl * pre_bound + U * refd.abs() - 8 * U * mag  # (check_pointwise adds 8 u mag + ulp(refd))
        check_pointwise(what + " kept", got, refd, mag, dto, sel & keep, extra)
        # the zero pattern is the mask wherever the value is not within its bound of 0
        clear = keep & sel & (refd.abs() > 2 * (scl * pre_bound + U * refd.abs() + ulp_bf16(refd)))
        assert (gotc[clear] != 0).all(), (what, "a kept element is 0")
    else:
        check_pointwise(what, got, ref, mag, dto, sel)
    if slab is not None:
        st = got.detach().to(F64).cpu()  # the slab sums the stored values
        check_slab(what, slab, torch.stack([st.sum(0), torch.zeros(C, dtype=F64)]),
                   torch.stack([st.abs().sum(0), torch.zeros(C, dtype=F64)]), 1, C)
        assert (slab[:, 1] == 0).all(), (what, "second slab row not zero")


@pytest.mark.parametrize("c", BWD_APPLY, ids=_ids(BWD_APPLY))
def test_bn_bwd_apply(env, cuda, c):
    """acfe_bn_bwd_apply / _dropout / _ex: k_bn_bwd_apply (scalar),
    k_bn_bwd_apply8<REG = false> (LDS coefficients, vgrid) and <REG = true>
    (slab grid, register coefficients); relu flags 0..3, with and without the
    residual add, with and without the dropout backward."""
    check_plan(c, env[5])
    rows, C, al, slab_on = c["rows"], c["C"], c["aligned"], c["slab"]
    x, sc, sh = bwd_apply_sign_inputs(c)
    dy = act((rows, C), 401 + C, 0.5)
    amb = ambiguous(x, sc, sh)
    check_share(f"bn_bwd_apply {c['id']}", amb)
    g = torch.Generator().manual_seed(C)
    coef = (torch.randn((3, C), generator=g) * 0.5).to(F32).to(F64)
    big = rows > 2000
    add = act((rows, C), 402 + C, 0.5)
    forms = [(3, True, 0.0)] if rows * C > 20_000_000 else [(3, True, 0.0), (1, False, 0.1)] if big else \
        [(r, a, 0.0) for r in range(4) for a in (False, True)] + [(0, False, 0.1), (1, False, 0.1), (3, False, 0.1)]
    for relu, with_add, rate in forms:
        for dto in ((BF,) if big else (BF, F32)):
            a = add if with_add else None
            what = f"bn_bwd_apply {c['id']} relu{relu} add{int(with_add)} rate{rate} {dto}"
            got, slab = _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, a, rate, slab_on, dto, al)
            _bwd_apply_check(what, got, slab, dy, x, sc, sh, coef, relu, a, rate, dto, amb)
            if not slab_on and rate == 0 and not big:  # the plain entry point is the same launch
                assert torch.equal(got, _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, a, 0.0, False, dto, al, "plain")[0])
            if not slab_on and rate > 0 and not big:
                assert torch.equal(got, _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, None, rate, False, dto, al, "dropout")[0])
            if not al:
                assert torch.equal(got, _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, a, rate, False, dto, True)[0])


@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "scalar"])
def test_bn_bwd_apply_dyadic(env, cuda, aligned):
    """Both sign tests on exact arithmetic: x scale + shift == 0 and x == 0 are
    not positive; nothing is left out."""
    c = case("dyadic", "bn_bwd_apply", int(aligned), "one", ROWS, 16, aligned=aligned)
    check_plan(c, env[5])
    x, sc, sh = dyadic(ROWS, 16, 2)
    g = torch.Generator().manual_seed(3)
    dy = torch.randint(-8, 9, (ROWS, 16), generator=g).to(F64) / 4
    coef = torch.stack([sc, torch.full((16,), 0.5, dtype=F64), torch.full((16,), -0.25, dtype=F64)])
    assert (x == 0).double().mean() > 0.01
    for relu in range(4):
        got, _ = _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, None, 0.0, False, F32, aligned)
        assert torch.equal(got.cpu().to(F64), R.bn_bwd_apply(dy, x, sc, sh, coef, relu)), relu


@pytest.mark.parametrize("c", BWD_POOL, ids=_ids(BWD_POOL))
def test_bn_bwd_apply_pool_sub(env, cuda, c):
    """acfe_bn_bwd_apply_pool / _sub: the residual is the average pool's (k 2,
    3; odd H, W) or the strided 1x1 shortcut's input gradient, formed on the fly."""
    check_plan(c, env[5])
    (H, W), k, C, N = c["hw"], c["k"], c["C"], 2
    rows = N * H * W
    assert rows == c["rows"]
    x, sc, sh = bwd_pool_sign_inputs(c)
    dy = act((rows, C), 501 + C, 0.5)
    amb = ambiguous(x, sc, sh)
    check_share(f"bn_bwd_apply_pool {c['id']}", amb)
    g = torch.Generator().manual_seed(C + k)
    coef = (torch.randn((3, C), generator=g) * 0.5).to(F32).to(F64)
    for fn, (P, Q) in (("pool", (-(-H // k), -(-W // k))), ("sub", ((H - 1) // k + 1, (W - 1) // k + 1))):
        gp = act((N, P, Q, C), 502 + C, 0.5)
        add = (R.avgpool_bwd(gp, H, W, k) if fn == "pool" else R.sub_bwd(gp, H, W, k)).reshape(rows, C)
        for relu in (1, 3):
            got, slab = _bwd_apply_run(env, cuda, dy, x, sc, sh, coef, relu, None, 0.0, c["slab"], BF, True, fn,
                                       (N, H, W, k, gp))
            _bwd_apply_check(f"bn_bwd_apply_{fn} {c['id']} relu{relu}", got, slab, dy, x, sc, sh, coef, relu, add, 0.0, BF,
                             amb)


# ------------------------------------------------------------------ elementwise
def _flat_inputs(n, seed):
    if n > 4_000_000:  # one normal draw, reused shifted: cheap at 33 M elements
        a = act((n,), seed)
        return a, a.roll(12345)
    return act((n,), seed), act((n,), seed + 1)


def _run_flat(env, cuda, name, n, dt, aligned, ins, extra=(), dto=None):
    ops, call, lib, ptr, stream, info = env
    dto = dto or dt
    bufs = [put(t, dt, cuda, aligned) for t in ins]
    y = out_buf((n,), dto, cuda, aligned)
    if name == "acfe_add":
        call(name, ptr(bufs[0].t), ptr(bufs[1].t), n, extra[0], ptr(y.t), code(dt), stream())
    elif name == "acfe_relu_bwd":
        call(name, ptr(bufs[0].t), ptr(bufs[1].t), n, ptr(y.t), code(dt), stream())
    elif name == "acfe_dropout":
        call(name, ptr(bufs[0].t), n, extra[0], SEED, ptr(y.t), code(dt), stream())
    else:
        call(name, ptr(bufs[0].t), code(dt), n, ptr(y.t), code(dto), stream())
    torch.cuda.synchronize()
    assert y.intact() and all(b.intact() for b in bufs)
    return y.t


def _both_alignments(env, cuda, c, name, n, dt, ins, extra=(), dto=None):
    got = _run_flat(env, cuda, name, n, dt, c["aligned"], ins, extra, dto)
    if not c["aligned"]:
        assert torch.equal(got, _run_flat(env, cuda, name, n, dt, True, ins, extra, dto)), "scalar != eight-wide"
    return got


@pytest.mark.parametrize("c", ADD, ids=_ids(ADD))
def test_add(env, cuda, c):
    check_plan(c, env[5])
    n = c["rows"]
    a, b = _flat_inputs(n, 600)
    for relu in ((1,) if n > 4_000_000 else (0, 1)):
        ref = (a + b).clamp_min(0) if relu else a + b
        for dt in ((BF,) if n > 4_000_000 else (BF, F32)):
            got = _both_alignments(env, cuda, c, "acfe_add", n, dt, (a, b), (relu,))
            check_pointwise(f"add {c['id']} relu{relu} {dt}", got, ref, a.abs() + b.abs(), dt)
    if n > 4_000_000:
        return
    # a + b > 0 on exact sums (multiples of 1/8, zeros included)
    g = torch.Generator().manual_seed(n)
    a, b = (torch.randint(-16, 17, (n,), generator=g).to(F64) / 8 for _ in range(2))
    got = _both_alignments(env, cuda, c, "acfe_add", n, BF, (a, b), (1,))
    assert torch.equal(got.cpu().to(F64), (a + b).clamp_min(0))


@pytest.mark.parametrize("c", RELU_BWD, ids=_ids(RELU_BWD))
def test_relu_bwd(env, cuda, c):
    check_plan(c, env[5])
    n = c["rows"]
    dy, y = _flat_inputs(n, 610)
    y = torch.where(y.abs() < 0.3, torch.zeros_like(y), y)  # exact zeros: not positive
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    for dt in ((BF,) if n > 4_000_000 else (BF, F32)):
        got = _both_alignments(env, cuda, c, "acfe_relu_bwd", n, dt, (dy, y))
        assert torch.equal(got.cpu().to(F64), ref), f"relu_bwd {c['id']} {dt}"
    print(f"relu_bwd {c['id']}: bit for bit")


@pytest.mark.parametrize("c", DROPOUT, ids=_ids(DROPOUT))
def test_dropout(env, cuda, c):
    """acfe_dropout, scalar and eight-wide: zeros, mask and kept values against
    the numpy pair hash; rate 0 keeps everything."""
    check_plan(c, env[5])
    n = c["rows"]
    x, _ = _flat_inputs(n, 620)
    for dt in ((BF,) if n > 4_000_000 else (BF, F32)):
        for rate in ((0.1,) if n > 4_000_000 else (0.1, 0.0)):
            ref, keep = R.dropout(x, SEED, rate, dt == BF)
            got = _both_alignments(env, cuda, c, "acfe_dropout", n, dt, (x,), (rate,))
            assert torch.equal(got.cpu().to(F64), ref), f"dropout {c['id']} {dt} rate {rate}"
            assert rate > 0 or bool(keep.all())
    print(f"dropout {c['id']}: bit for bit, keep share {keep.double().mean().item():.4f}")


@pytest.mark.parametrize("c", CAST, ids=_ids(CAST))
def test_cast(env, cuda, c):
    check_plan(c, env[5])
    n = c["rows"]
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(F64)  # f32 values that are not bf16 values
    for dti, dto in (((F32, BF),) if n > 4_000_000 else ((F32, BF), (BF, F32), (BF, BF), (F32, F32))):
        src = stored(x, dti)
        got = _both_alignments(env, cuda, c, "acfe_cast", n, dti, (src,), dto=dto)
        assert torch.equal(got.cpu().to(F64), stored(src, dto)), f"cast {c['id']} {dti}->{dto}"
    print(f"cast {c['id']}: bit for bit")


@pytest.mark.parametrize("c", ADD_STATS, ids=_ids(ADD_STATS))
def test_add_stats(env, cuda, c):
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    rows, C = c["rows"], c["C"]
    a, b = act((rows, C), 630 + C), act((rows, C), 631 + C)
    for relu in (0, 1):
        for dt in ((BF,) if rows > 2000 else (BF, F32)):
            ab, bb = put(a, dt, cuda), put(b, dt, cuda)
            z, slab = out_buf((rows, C), dt, cuda), out_buf((plan["grid"], 2, C), F64, cuda)
            call("acfe_add_stats", ptr(ab.t), ptr(bb.t), rows, C, relu, ptr(z.t), code(dt), ptr(slab.t), stream())
            torch.cuda.synchronize()
            assert z.intact() and slab.intact()
            ref = (a + b).clamp_min(0) if relu else a + b
            check_pointwise(f"add_stats {c['id']} relu{relu} {dt}", z.t, ref, a.abs() + b.abs(), dt)
            st = z.t.cpu().to(F64)
            check_slab(f"add_stats {c['id']} relu{relu} {dt}", slab.t, R.bn_stats(st),
                       torch.stack([st.abs().sum(0), (st * st).sum(0)]), 1, C)


@pytest.mark.parametrize("c", RELU_BWD_SUM, ids=_ids(RELU_BWD_SUM))
def test_relu_bwd_sum(env, cuda, c):
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    rows, C = c["rows"], c["C"]
    dy, y = act((rows, C), 640 + C), act((rows, C), 641 + C)
    y = torch.where(y.abs() < 0.3, torch.zeros_like(y), y)
    ref = torch.where(y > 0, dy, torch.zeros_like(dy))
    for dt in ((BF,) if rows > 2000 else (BF, F32)):
        dyb, yb = put(dy, dt, cuda), put(y, dt, cuda)
        dx, slab = out_buf((rows, C), dt, cuda), out_buf((plan["grid"], 2, C), F64, cuda)
        call("acfe_relu_bwd_sum", ptr(dyb.t), ptr(yb.t), rows, C, ptr(dx.t), code(dt), ptr(slab.t), stream())
        torch.cuda.synchronize()
        assert dx.intact() and slab.intact()
        assert torch.equal(dx.t.cpu().to(F64), ref)
        check_slab(f"relu_bwd_sum {c['id']} {dt}", slab.t, R.bn_stats(ref),
                   torch.stack([ref.abs().sum(0), (ref * ref).sum(0)]), 1, C)


# ------------------------------------------------------------------ pools
@pytest.mark.parametrize("c", MAXPOOL, ids=_ids(MAXPOOL))
def test_maxpool(env, cuda, c):
    """acfe_maxpool2d / _bwd: k_maxpool8 / k_maxpool_bwd8 at (1,2), (2,2), (3,3),
    the generic kernels at (2,3), C = 50 and the misaligned view; ties go to the
    first maximum, leftover rows and columns get zero.  Bit for bit."""
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    check_plan(c, info, "maxpool_bwd")
    (H, W, kh, kw), C, N, al = c["geo"], c["C"], 2, c["aligned"]
    x = coarse((N, H, W, C), H * W + C)
    yr, _ = R.maxpool(x, kh, kw)
    dy = act(tuple(yr.shape), 700 + C)
    dxr = R.maxpool_bwd(x, dy, kh, kw)
    for dt in ((BF,) if H * W > 10000 else (BF, F32)):
        for a in ((al,) if al else (False, True)):  # (both exact: the misaligned view stores what the aligned one does)
            xb, dyb = put(x, dt, cuda, a), put(dy, dt, cuda, a)
            y, dx = out_buf(tuple(yr.shape), dt, cuda, a), out_buf((N, H, W, C), dt, cuda, a)
            call("acfe_maxpool2d", ptr(xb.t), N, H, W, C, kh, kw, ptr(y.t), code(dt), stream())
            call("acfe_maxpool2d_bwd", ptr(xb.t), ptr(dyb.t), N, H, W, C, kh, kw, ptr(dx.t), code(dt), stream())
            torch.cuda.synchronize()
            assert y.intact() and dx.intact()
            assert torch.equal(y.t.cpu().to(F64), yr), f"maxpool {c['id']} {dt}"
            assert torch.equal(dx.t.cpu().to(F64), dxr), f"maxpool_bwd {c['id']} {dt}"
    print(f"maxpool {c['id']}: values and backward bit for bit")


@pytest.mark.parametrize("c", MAXPOOL_FUSED, ids=_ids(MAXPOOL_FUSED))
def test_maxpool_fused(env, cuda, c):
    """acfe_maxpool2d_fused / _bwd_argmax (k_maxpool8x, k_maxpool_bwd8i): values,
    argmax bytes, dropout (rate 0 and 0.1) and its backward bit for bit against
    the restatement and the numpy mask; the statistics slab on and off; argmax NULL."""
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    check_plan(c, info, "maxpool_bwd_argmax")
    (H, W, kh, kw), C, N = c["geo"], c["C"], 2
    big = H * W > 10000
    x = coarse((N, H, W, C), H * W + C + 1)
    yr, amr = R.maxpool(x, kh, kw)
    dy = act(tuple(yr.shape), 710 + C)
    rows = yr.numel() // C
    for dt in ((BF,) if big else (BF, F32)):
        xb, dyb = put(x, dt, cuda), put(dy, dt, cuda)
        for rate in (0.0, 0.1):
            yd = R.dropout(yr, SEED, rate, dt == BF)[0] if rate else yr
            gd = R.dropout(dy, SEED, rate, dt == BF)[0] if rate else dy
            for with_am in ((True,) if big else (False, True)):
                y = out_buf(tuple(yr.shape), dt, cuda)
                am = out_buf(tuple(yr.shape), torch.uint8, cuda) if with_am else None
                slab = out_buf((slab_rows(lib, rows), 2, C), F64, cuda) if c["slab"] else None
                assert slab is None or plan["grid"] == slab.t.shape[0]
                call("acfe_maxpool2d_fused", ptr(xb.t), N, H, W, C, kh, kw, ptr(y.t), None if am is None else ptr(am.t),
                     rate, SEED, None if slab is None else ptr(slab.t), code(dt), stream())
                torch.cuda.synchronize()
                assert y.intact() and (am is None or am.intact()) and (slab is None or slab.intact())
                assert torch.equal(y.t.cpu().to(F64), yd), f"maxpool_fused {c['id']} {dt} rate {rate}"
                if am is not None:
                    assert torch.equal(am.t.cpu(), amr), f"argmax {c['id']}"
                if slab is not None:
                    check_slab(f"maxpool_fused {c['id']} {dt} rate {rate}", slab.t, R.bn_stats(yd.reshape(-1, C)),
                               torch.stack([yd.abs().reshape(-1, C).sum(0), (yd * yd).reshape(-1, C).sum(0)]), 1, C)
            dx = out_buf((N, H, W, C), dt, cuda)
            call("acfe_maxpool2d_bwd_argmax", ptr(am.t), ptr(dyb.t), N, H, W, C, kh, kw, rate, SEED, ptr(dx.t), code(dt),
                 stream())
            torch.cuda.synchronize()
            assert dx.intact()
            assert torch.equal(dx.t.cpu().to(F64), R.maxpool_bwd_from_argmax(amr, gd, H, W, kh, kw)), \
                f"maxpool_bwd_argmax {c['id']} {dt} rate {rate}"
    print(f"maxpool_fused {c['id']}: values, argmax, dropout and backward bit for bit")


@pytest.mark.parametrize("c", MAXPOOL_BN, ids=_ids(MAXPOOL_BN))
def test_bn_maxpool_and_bwd_argmax_bn(env, cuda, c):
    """acfe_bn_maxpool2d_fused (the BN (+ReLU) output formed at load time) and
    acfe_maxpool2d_bwd_argmax_bn (the expanded gradient plus the BN backward
    reduce slab)."""
    ops, call, lib, ptr, stream, info = env
    plan = check_plan(c, info)
    fused = check_plan(dict(c, op="maxpool_fused"), info)
    (H, W, kh, kw), C, N = c["geo"], c["C"], 2
    assert plan["passes"] > 16 or not c.get("flush16")
    x2, sc, sh = maxpool_bn_sign_inputs(c)
    x = x2.reshape(N, H, W, C)
    amb = ambiguous(x2, sc, sh)
    check_share(f"maxpool_bwd_argmax_bn {c['id']}", amb)
    mean, invstd = _stat_params(x2, C)
    relu = 1
    xb = put(x, BF, cuda)
    pb = [put(t, F32, cuda) for t in (sc, sh, mean, invstd)]
    P, Q = H // kh, W // kw
    y, am = out_buf((N, P, Q, C), BF, cuda), out_buf((N, P, Q, C), torch.uint8, cuda)
    slab = out_buf((fused["grid"], 2, C), F64, cuda)
    call("acfe_bn_maxpool2d_fused", ptr(xb.t), N, H, W, C, ptr(pb[0].t), ptr(pb[1].t), relu, kh, kw, ptr(y.t), ptr(am.t),
         ptr(slab.t), 1, stream())
    torch.cuda.synchronize()
    assert y.intact() and am.intact() and slab.intact()
    # the pooled value is the maximum of the stored BN outputs: within the pointwise bound of
    # the float64 one; the argmax names a window position that attains the device's maximum
    bn = R.bn_apply(x, sc, sh, relu)
    mag = (x * sc).abs() + sh.abs()
    yr, _ = R.maxpool(bn, kh, kw)
    check_pointwise(f"bn_maxpool {c['id']}", y.t, yr, R.maxpool(mag, kh, kw)[0], BF)
    amd = am.t.cpu()
    assert int(amd.max()) < kh * kw
    yst = y.t.cpu().to(F64)
    picked = R.windows(bn, kh, kw).gather(3, amd.to(torch.int64).unsqueeze(3)).squeeze(3)
    check_pointwise(f"bn_maxpool {c['id']} argmax", yst, picked, R.maxpool(mag, kh, kw)[0], BF)
    check_slab(f"bn_maxpool {c['id']}", slab.t, R.bn_stats(yst.reshape(-1, C)),
               torch.stack([yst.abs().reshape(-1, C).sum(0), (yst * yst).reshape(-1, C).sum(0)]), 1, C)
    # backward from the device's own argmax bytes
    dy = act((N, P, Q, C), 721 + C, 0.5)
    dyb = put(dy, BF, cuda)
    dx = out_buf((N, H, W, C), BF, cuda)
    rslab = out_buf((plan["grid"], 2, C), F64, cuda)
    assert plan["grid"] == slab_rows(lib, N * H * W)
    call("acfe_maxpool2d_bwd_argmax_bn", ptr(am.t), ptr(dyb.t), N, H, W, C, kh, kw, ptr(dx.t), 1, ptr(xb.t),
         *[ptr(b.t) for b in pb], relu, ptr(rslab.t), stream())
    torch.cuda.synchronize()
    assert dx.intact() and rslab.intact()
    dxr = R.maxpool_bwd_from_argmax(amd, dy, H, W, kh, kw)
    assert torch.equal(dx.t.cpu().to(F64), dxr), f"maxpool_bwd_argmax_bn {c['id']} dx"
    g2 = dxr.reshape(-1, C)
    gm = R.bn_masked_grad(g2, x2, sc, sh, relu)
    v, vall = gm * (x2 - mean) * invstd, g2 * (x2 - mean) * invstd
    check_slab(f"maxpool_bwd_argmax_bn {c['id']}", rslab.t, torch.stack([gm.sum(0), v.sum(0)]),
               torch.stack([gm.abs().sum(0), v.abs().sum(0)]), 16 * kh * kw * -(-(Q * C // 8) // 256), C,
               torch.stack([(g2.abs() * amb).sum(0), (vall.abs() * amb).sum(0)]))


@pytest.mark.parametrize("c", AVGPOOL, ids=_ids(AVGPOOL))
def test_avgpool(env, cuda, c):
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    check_plan(c, info, "avgpool_bwd")
    (H, W, k, _), C, N, al = c["geo"], c["C"], 2, c["aligned"]
    x = act((N, H, W, C), 730 + C)
    yr = R.avgpool(x, k)
    dy = act(tuple(yr.shape), 731 + C)
    dxr = R.avgpool_bwd(dy, H, W, k)
    for dt in ((BF,) if H * W > 10000 else (BF, F32)):
        res = []
        for a in ((al,) if al else (False, True)):
            xb, dyb = put(x, dt, cuda, a), put(dy, dt, cuda, a)
            y, dx = out_buf(tuple(yr.shape), dt, cuda, a), out_buf((N, H, W, C), dt, cuda, a)
            call("acfe_avgpool2d", ptr(xb.t), N, H, W, C, k, ptr(y.t), code(dt), stream())
            call("acfe_avgpool2d_bwd", ptr(dyb.t), N, H, W, C, k, ptr(dx.t), code(dt), stream())
            torch.cuda.synchronize()
            assert y.intact() and dx.intact()
            check_pointwise(f"avgpool {c['id']} {dt}", y.t, yr, R.avgpool(x.abs(), k), dt)
            check_pointwise(f"avgpool_bwd {c['id']} {dt}", dx.t, dxr, dxr.abs(), dt)
            res.append((y.t, dx.t))
        if len(res) == 2:  # the scalar kernels of the misaligned view store what the eight-wide ones do
            assert torch.equal(res[0][0], res[1][0]), f"avgpool {c['id']} {dt}: scalar != eight-wide"
            assert torch.equal(res[0][1], res[1][1]), f"avgpool_bwd {c['id']} {dt}: scalar != eight-wide"


# ------------------------------------------------------------------ head
@pytest.mark.parametrize("c", [c for c in HEAD if c["op"] == "axis_pool"], ids=lambda c: c["id"])
@pytest.mark.parametrize("mode", [0, 1])
def test_axis_pool(env, cuda, c, mode):
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    check_plan(c, info, "axis_pool_bwd")
    outer, inner, L = c["rows"], c["C"], c["L"]
    x, dy = act((outer, L, inner), 800), act((outer, inner), 801).to(F32).to(F64)
    for dt in (BF, F32):
        xb, dyb = put(x, dt, cuda), put(dy, F32, cuda)
        y, dx = out_buf((outer, inner), F32, cuda), out_buf((outer, L, inner), dt, cuda)
        call("acfe_axis_pool", ptr(xb.t), code(dt), outer, L, inner, 5.0, mode, ptr(y.t), stream())
        call("acfe_axis_pool_bwd", ptr(xb.t), code(dt), ptr(dyb.t), outer, L, inner, 5.0, mode, ptr(dx.t), stream())
        torch.cuda.synchronize()
        assert y.intact() and dx.intact()
        dxr = R.axis_pool_bwd(x, dy, 5.0, mode)
        ef = rel_l2(y.t, R.axis_pool(x, 5.0, mode))
        if dt == F32:
            eb = rel_l2(dx.t, dxr)
        else:  # a bf16 gradient: the same 1e-5, per element, plus its one rounding
            eb = ((dx.t.cpu().to(F64) - dxr).abs() - ulp_bf16(dxr)).clamp_min(0).norm().item() / dxr.norm().item()
        print(f"axis_pool {c['id']} mode {mode} {dt}: fwd rel-L2 {ef:.2e} (1e-6), bwd {eb:.2e} (1e-5)")
        assert ef < 1e-6 and eb < 1e-5


@pytest.mark.parametrize("c", [c for c in HEAD if c["op"] == "dense_fwd"], ids=lambda c: c["id"])
def test_dense(env, cuda, c):
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    B, O, I = c["rows"], c["C"], c["I"]
    check_plan(c, info, "dense_bwd")
    g = torch.Generator().manual_seed(B)
    f32 = lambda t: t.to(F32).to(F64)  # noqa: E731
    x, w, b = f32(torch.randn((B, I), generator=g)), f32(torch.randn((I, O), generator=g) * 0.5), f32(torch.randn(O, generator=g) * 0.1)
    dz = f32(torch.randn((B, O), generator=g))
    xb, wb, bb, dzb = (put(t, F32, cuda) for t in (x, w, b, dz))
    z, dx, dw, db = (out_buf(s, F32, cuda) for s in ((B, O), (B, I), (I, O), (O,)))
    call("acfe_dense_fwd", ptr(xb.t), ptr(wb.t), ptr(bb.t), B, I, O, ptr(z.t), stream())
    call("acfe_dense_bwd", ptr(xb.t), ptr(wb.t), ptr(dzb.t), B, I, O, ptr(dx.t), ptr(dw.t), ptr(db.t), stream())
    torch.cuda.synchronize()
    assert z.intact() and dx.intact() and dw.intact() and db.intact()
    rx, rw, rb = R.dense_bwd(x, w, dz)
    errs = [rel_l2(z.t, R.dense(x, w, b)), rel_l2(dx.t, rx), rel_l2(dw.t, rw), rel_l2(db.t, rb)]
    print(f"dense {c['id']}: rel-L2 z {errs[0]:.2e} dx {errs[1]:.2e} dw {errs[2]:.2e} db {errs[3]:.2e} (1e-6)")
    assert max(errs) < 1e-6


def test_dense_bwd_w_capped(env, cuda):
    """(I + 1) O = 35050 outputs, one wave each: the 8192-workgroup cap of k_dense_bwd_w."""
    ops, call, lib, ptr, stream, info = env
    c = [c for c in HEAD if c["op"] == "dense_bwd_w"][0]
    check_plan(c, info)
    B, I, O = c["B"], c["rows"] - 1, c["C"]
    g = torch.Generator().manual_seed(9)
    x, w, dz = (torch.randn(s, generator=g).to(F64) for s in ((B, I), (I, O), (B, O)))
    xb, wb, dzb = (put(t, F32, cuda) for t in (x, w, dz))
    dw, db = out_buf((I, O), F32, cuda), out_buf((O,), F32, cuda)
    call("acfe_dense_bwd", ptr(xb.t), ptr(wb.t), ptr(dzb.t), B, I, O, None, ptr(dw.t), ptr(db.t), stream())
    torch.cuda.synchronize()
    assert dw.intact() and db.intact()
    _, rw, rb = R.dense_bwd(x, w, dz)
    ew, eb = rel_l2(dw.t, rw), rel_l2(db.t, rb)
    print(f"dense_bwd_w capped: rel-L2 dw {ew:.2e} db {eb:.2e} (1e-6)")
    assert ew < 1e-6 and eb < 1e-6


@pytest.mark.parametrize("c", [c for c in HEAD if c["op"] == "loss"], ids=lambda c: c["id"])
@pytest.mark.parametrize("mode", [0, 1])
def test_loss(env, cuda, c, mode):
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    B, L = c["rows"], c["C"]
    g = torch.Generator().manual_seed(B + L)
    z = (torch.randn((B, L), generator=g) * 2).to(F32).to(F64)
    y = (torch.rand((B, L), generator=g) < 0.1).to(F64)
    y[:, 0] = 1
    zb, yb = put(z, F32, cuda), put(y, F32, cuda)
    loss, dz, ws = out_buf((1,), F32, cuda), out_buf((B, L), F32, cuda), out_buf((B,), F32, cuda)
    call("acfe_loss", ptr(zb.t), ptr(yb.t), B, L, mode, 0.25, ptr(loss.t), ptr(dz.t), ptr(ws.t), stream())
    torch.cuda.synchronize()
    assert loss.intact() and dz.intact() and ws.intact()
    lr, dzr = R.loss(z, y, mode, 0.25)
    el, eg = abs(loss.t.item() - lr.item()) / max(1, abs(lr.item())), rel_l2(dz.t, dzr)
    print(f"loss {c['id']} mode {mode}: loss err {el:.2e} (1e-5), dz rel-L2 {eg:.2e} (1e-5)")
    assert el < 1e-5 and eg < 1e-5


@pytest.mark.parametrize("c", [c for c in HEAD if c["op"] in ("sigmoid", "adam")], ids=lambda c: c["id"])
def test_sigmoid_adam(env, cuda, c):
    ops, call, lib, ptr, stream, info = env
    check_plan(c, info)
    n = c["rows"]
    g = torch.Generator().manual_seed(n)
    f32 = lambda t: t.to(F32).to(F64)  # noqa: E731
    if c["op"] == "sigmoid":
        z = f32(torch.randn(n, generator=g) * 3)
        zb, p = put(z, F32, cuda), out_buf((n,), F32, cuda)
        call("acfe_sigmoid", ptr(zb.t), n, ptr(p.t), stream())
        torch.cuda.synchronize()
        assert p.intact()
        e = rel_l2(p.t, torch.sigmoid(z))
        print(f"sigmoid {c['id']}: rel-L2 {e:.2e} (1e-6)")
        assert e < 1e-6
        return
    p0, gr = f32(torch.randn(n, generator=g)), f32(torch.randn(n, generator=g) * 4)
    m0, v0 = f32(torch.randn(n, generator=g) * 0.1), f32(torch.rand(n, generator=g))
    pb, gb, mb, vb = (put(t, F32, cuda) for t in (p0, gr, m0, v0))
    call("acfe_adam_step", ptr(pb.t), ptr(gb.t), ptr(mb.t), ptr(vb.t), n, 0.25, 0.9, 0.999, 1e-7, R.adam_alpha(0.01, 3),
         stream())
    torch.cuda.synchronize()
    assert pb.intact() and mb.intact() and vb.intact()
    pr, mr, vr = R.adam(p0, gr, m0, v0, 0.25, 3)
    errs = [rel_l2(pb.t, pr), rel_l2(mb.t, mr), rel_l2(vb.t, vr)]
    print(f"adam {c['id']}: rel-L2 p {errs[0]:.2e} m {errs[1]:.2e} v {errs[2]:.2e} (1e-6)")
    assert max(errs) < 1e-6


# ------------------------------------------------------------------ the dropout mask's other users
@pytest.mark.parametrize("K", [64, 128])
def test_conv_dropout_mask(env, cuda, K):
    """acfe_conv2d_fwd_dropout's zero pattern is dropout_keep over the flat NHWC
    index of its output (elements whose undropped value is exactly 0 left out)."""
    ops, call, lib, ptr, stream, info = env
    N, H, W, C = 2, 12, 40, 64
    g = torch.Generator().manual_seed(K)
    x = torch.randn((N, H, W, C), generator=g).to(BF).to(cuda)
    w = (torch.randn((K, 3, 3, C), generator=g) * 0.05).to(cuda)
    b = (torch.randn((K,), generator=g) * 0.1).to(cuda)
    wp = ops.pack_weights(w, BF, False)
    y0, y1 = out_buf((N, H, W, K), BF, cuda), out_buf((N, H, W, K), BF, cuda)
    call("acfe_conv2d_fwd", ptr(x), N, H, W, C, ptr(wp), K, 3, 3, 1, 1, 1, H, W, ptr(b), ptr(y0.t), 1, None, stream())
    call("acfe_conv2d_fwd_dropout", ptr(x), N, H, W, C, ptr(wp), K, 3, 3, 1, 1, 1, H, W, ptr(b), ptr(y1.t), 1, None, 0.1,
         SEED, stream())
    torch.cuda.synchronize()
    assert y0.intact() and y1.intact()
    keep = torch.from_numpy(R.dropout_keep(SEED, np.arange(N * H * W * K, dtype=np.uint64), 0.1)).view(N, H, W, K)
    nz = y0.t.cpu() != 0
    print(f"conv dropout K {K}: undropped zeros {1 - nz.double().mean().item():.2e} (bound 1e-3)")
    assert 1 - nz.double().mean().item() < 1e-3
    assert torch.equal((y1.t.cpu() != 0)[nz], keep[nz])


def test_conv_dropout_keep_bits(env, cuda):
    """The keep bits of acfe_conv2d_fwd_dropout_keep: bit j of byte (pixel, c / 8)
    is dropout_keep of element (pixel, 8 (c / 8) + j)."""
    ops, call, lib, ptr, stream, info = env
    N, H, W, C, K = 6, 14, 100, 64, 64
    assert lib.acfe_conv2d_dropout_keep_supported(N, H, W, C, K, 1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((N, H, W, C), generator=g).to(BF).to(cuda)
    w = (torch.randn((K, 3, 3, C), generator=g) * 0.05).to(cuda)
    b = (torch.randn((K,), generator=g) * 0.1).to(cuda)
    wp = ops.pack_weights(w, BF, False)
    rows = lib.acfe_conv2d_stats_rows(N * H * W, K)
    y = out_buf((N, H, W, K), BF, cuda)
    st = torch.zeros((rows, 2, wp.shape[0]), dtype=F64, device=cuda)
    bits = out_buf((N, H, W, K // 8), torch.uint8, cuda)
    call("acfe_conv2d_fwd_dropout_keep", ptr(x), N, H, W, C, ptr(wp), K, 1, 1, ptr(b), ptr(y.t), ptr(st), 0.1, SEED,
         ptr(bits.t), stream())
    torch.cuda.synchronize()
    assert y.intact() and bits.intact()
    keep = R.dropout_keep(SEED, np.arange(N * H * W * K, dtype=np.uint64), 0.1).reshape(-1, 8)
    want = (keep.astype(np.uint8) << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8)
    assert np.array_equal(bits.t.cpu().numpy().reshape(-1), want)
