"""The front-end kernels of csrc/frontend.hip at the shapes where their launch
geometry changes, against the case table of oracle/frontend_cases.py (whose own
conditions tests/test_frontend_cases.py checks on the CPU): PCEN at row, chunk
and clamp edges with per-probe gradients, the n_fft 4096 mel kernels at odd /
single / long / empty / DC / Nyquist bands, k_mel<NC> at n_fft 2048 / 512 / 256,
and the exact data movement (normalize stats / apply, mix_up, copy_rows,
mel_from_spec).  Every output sits inside a sentinel-filled buffer.

Bounds (fp32 kernels vs the float64 oracle):
  PCEN:  |gpu - ref| <= 5e-5 on the [-1, 1] output, out.min() == -1, out.max() == 1
  dPCEN: per probe dout = g * mask, e = max_k |got_k - ref_k| / S_k <= 2e-3 * s,
         S_k = the case's largest |ref_k| over its probes, s = max_k |ref_k| / S_k
         (the project's 2e-3, per probe instead of per sum)
  mel:   |gpu - ref| <= 2e-5 * max(ref) per clip; mel_from_spec 2e-6 * max
  everything else bit for bit.

Measured on an MI355X (the largest over all cases):
  PCEN output   1.9e-6  ((1, 1, 5); (3, 70, 40) smooth 1.5: 1.8e-6)
  dPCEN e / s   6.5e-4  ((2, 33, 64) smooth 1.5, column t = 31; T == 1: 5.9e-4;
                         bf16 dout 5.0e-6; wide scope 2.0e-6)
  mel           8.4e-7  (n_fft 4096, the one-band plan, pad_end, power 2;
                         n_fft 2048 / 512 / 256: 3.7e-7)
"""
import numpy as np
import pytest
import torch

from oracle import frontend as of
from oracle import frontend_cases as fc

pytestmark = pytest.mark.gpu

SENT = -8192.0  # exact in bfloat16 too
PAD = 64  # floats of sentinel either side (256 B: keeps the 16-B and 8-B alignment of the base)


@pytest.fixture(scope="module")
def fe(cuda):
    from acfe import frontend

    return frontend


@pytest.fixture(scope="module")
def lib(fe):
    from acfe import _lib

    return _lib


def guarded(n, dev, dtype=torch.float32, pad=PAD):
    """(buffer, view of its n middle elements); the rest keeps SENT."""
    buf = torch.full((n + 2 * pad,), SENT, dtype=dtype, device=dev)
    return buf, buf[pad:pad + n]


def assert_guard(buf, n, what, pad=PAD):
    b = buf.float().cpu().numpy()
    assert (b[:pad] == SENT).all() and (b[pad + n:] == SENT).all(), f"{what}: write outside [0, {n})"


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=what)


# ---------------------------------------------------------------- PCEN

def pcen_stages(lib, x, params, shape, out_dtype=torch.float32, scope=None):
    """acfe_pcen_fwd + acfe_pcen_normalize into guarded buffers:
    (y [B,M,T], part [2 * np], out [B,M,T], stats [4]) on the device."""
    B, T, M = shape
    dev = x.device
    n, npart = B * M * T, lib.lib.acfe_pcen_partials(B, M)
    assert npart == -(-B * M // 64)
    ybuf, y = guarded(n, dev)
    pbuf, part = guarded(2 * npart, dev)
    obuf, out = guarded(n, dev, out_dtype)
    sbuf, stats = guarded(4, dev)
    lib.call("acfe_pcen_fwd", x.data_ptr(), B, T, M, params.data_ptr(), 1e-6, y.data_ptr(), part.data_ptr(), stream())
    lib.call("acfe_pcen_normalize", y.data_ptr(), n, part.data_ptr(), npart, None if scope is None else scope.data_ptr(),
             out.data_ptr(), lib.DTYPE_F32 if out_dtype == torch.float32 else lib.DTYPE_BF16, stats.data_ptr(), stream())
    torch.cuda.synchronize()
    for b, k, w in ((ybuf, n, "y"), (pbuf, 2 * npart, "part"), (obuf, n, "out"), (sbuf, 4, "stats")):
        assert_guard(b, k, w)
    return y.view(B, M, T), part, out.view(B, M, T), stats


def pcen_grads(lib, x, params, shape, stats, douts):
    """{probe: dparams [4]} through acfe_pcen_bwd; douts {probe: device [B,M,T]}."""
    B, T, M = shape
    dev = x.device
    npart = lib.lib.acfe_pcen_partials(B, M)
    wbuf, ws = guarded(32 * npart, dev)
    names = list(douts)
    gbuf, g = guarded(4 * len(names), dev)
    for i, k in enumerate(names):
        d = douts[k]
        lib.call("acfe_pcen_bwd", x.data_ptr(), B, T, M, params.data_ptr(), 1e-6, stats.data_ptr(), d.data_ptr(),
                 lib.DTYPE_F32 if d.dtype == torch.float32 else lib.DTYPE_BF16, ws.data_ptr(),
                 g[4 * i:].data_ptr(), stream())
    torch.cuda.synchronize()
    assert_guard(wbuf, 32 * npart, "bwd workspace")
    assert_guard(gbuf, 4 * len(names), "dparams")
    got = g.cpu().numpy().reshape(-1, 4)
    return {k: got[i] for i, k in enumerate(names)}


_dev_cache = {}


def dev_inputs(shape, dev, bf16=False):
    key = (shape, bf16)
    if key not in _dev_cache:
        x = torch.from_numpy(fc.pcen_input(shape)).to(dev)
        dt = torch.bfloat16 if bf16 else torch.float32
        douts = {k: d.to(dt).to(dev).contiguous() for k, d in fc.pcen_douts(shape, bf16).items()}
        _dev_cache[key] = (x, douts)
    return _dev_cache[key]


_run_cache = {}


def pcen_run(lib, dev, shape, pname):
    """One forward + every probe's backward per (shape, parameter set), shared
    by the forward and the backward test."""
    key = (shape, pname)
    if key not in _run_cache:
        x, douts = dev_inputs(shape, dev)
        p = torch.tensor(fc.PCEN_PARAMS[pname], dtype=torch.float32, device=dev)
        y, part, out, stats = pcen_stages(lib, x, p, shape)
        _run_cache[key] = dict(out=out.cpu().numpy(), y=y.cpu().numpy(), stats=stats.cpu().numpy(),
                               grads=pcen_grads(lib, x, p, shape, stats, douts))
    return _run_cache[key]


def assert_probes(got, ref, what):
    errs = fc.probe_errors(got, ref)
    worst = max(errs, key=lambda k: errs[k][0] / errs[k][1])
    print(f"MEASURE dpcen {what} max e/s {errs[worst][0] / errs[worst][1]:.3e} ({worst})")
    bad = {k: (e, s) for k, (e, s) in errs.items() if not e <= fc.DPCEN_BOUND * s}
    assert not bad, f"{what}: e > 2e-3 * s at {bad}"


SHAPE_IDS = [f"{b}x{t}x{m}" for b, t, m in fc.PCEN_SHAPES]


@pytest.mark.parametrize("shape", fc.PCEN_SHAPES, ids=SHAPE_IDS)
def test_pcen_stages(lib, cuda, shape):
    """acfe_pcen_fwd / acfe_pcen_normalize on their own terms: the partials are
    the min / max of the kernel's own y rows [64 i, 64 i + 64), the normalised
    output is the float32 formula of tfpcen.py:110 on that y, stats hold the
    extrema and their tie counts, the bf16 output is the rounded float32 one;
    a scope equal to the batch's own extrema changes nothing, and a wider one
    means: the same formula with the scope's values, extrema constant in the
    backward (no tie terms)."""
    B, T, M = shape
    x, douts = dev_inputs(shape, cuda)
    pname = "default"
    p = torch.tensor(fc.PCEN_PARAMS[pname], dtype=torch.float32, device=cuda)
    y_d, part_d, out_d, stats_d = pcen_stages(lib, x, p, shape)
    y, part, out, stats = (t.cpu().numpy() for t in (y_d, part_d, out_d, stats_d))
    rows = y.reshape(B * M, T)
    for i in range(len(part) // 2):
        blk = rows[64 * i: 64 * i + 64]
        assert_bits(part[2 * i: 2 * i + 2], [blk.min(), blk.max()], f"partials of workgroup {i}")
    mn, mx = y.min(), y.max()
    assert_bits(out, np.float32(2) * ((y - mn) / (mx - mn)) - np.float32(1), "normalised output")
    assert_bits(stats, [mn, mx, (y == mn).sum(), (y == mx).sum()], "stats")
    # the ties the recipe planted, as the kernel sees them
    assert stats[3] == (2 if B > 1 else 1) and stats[2] == max(int((x == 0).sum().item()), 1)
    _, _, ob, sb = pcen_stages(lib, x, p, shape, torch.bfloat16)
    assert torch.equal(ob.view(torch.int16), out_d.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(sb, stats_d)
    g0 = pcen_grads(lib, x, p, shape, stats_d, douts)
    # scope == the batch's own extrema: bit for bit the unscoped run
    scope = torch.tensor([mn, mx], dtype=torch.float32, device=cuda)
    y1, _, out1, stats1 = pcen_stages(lib, x, p, shape, scope=scope)
    assert torch.equal(y1, y_d) and torch.equal(out1, out_d) and torch.equal(stats1, stats_d)
    g1 = pcen_grads(lib, x, p, shape, stats1, douts)
    for k in g0:
        assert_bits(g1[k], g0[k], f"dparams under an equal scope, probe {k}")
    # a scope strictly wider than the data
    d = np.float32(mx - mn)
    smn, smx = np.float32(mn - np.float32(0.25) * d), np.float32(mx + np.float32(0.5) * d)
    assert smn < mn and smx > mx
    scope = torch.tensor([smn, smx], dtype=torch.float32, device=cuda)
    _, _, out2, stats2 = pcen_stages(lib, x, p, shape, scope=scope)
    assert_bits(out2.cpu().numpy(), np.float32(2) * ((y - smn) / (smx - smn)) - np.float32(1), "scoped output")
    assert_bits(stats2.cpu().numpy(), [smn, smx, 0, 0], "scoped stats")
    g2 = pcen_grads(lib, x, p, shape, stats2, douts)
    ref = fc.pcen_reference(shape, pname, scope=(float(smn), float(smx)))
    assert np.abs(out2.cpu().numpy() - ref["out"]).max() <= fc.PCEN_BOUND
    assert_probes(g2, ref["grads"], f"{shape} wide scope")


CASES = [(s, p) for s in fc.PCEN_SHAPES for p in fc.PCEN_PARAMS]
CASE_IDS = [f"{i}-{p}" for i in SHAPE_IDS for p in fc.PCEN_PARAMS]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pcen_forward(lib, cuda, case):
    shape, pname = case
    out = pcen_run(lib, cuda, shape, pname)["out"]
    ref = fc.pcen_reference(shape, pname)["out"]
    err = np.abs(out - ref).max()
    print(f"MEASURE pcen {shape} {pname} max |out - ref| {err:.3e}")
    assert err <= fc.PCEN_BOUND
    assert out.min() == -1.0 and out.max() == 1.0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pcen_backward(lib, cuda, case):
    """Every probe against float64 autograd of oracle.torch_ref.pcen_torch; a
    clamped parameter's gradient is exactly 0; at gain == 1.0 / root == 1.0
    the gradient is the whole TF one (MinimumGrad / MaximumGrad at a tie)."""
    shape, pname = case
    got = pcen_run(lib, cuda, shape, pname)["grads"]
    ref = fc.pcen_reference(shape, pname)["grads"]
    assert_probes(got, ref, f"{shape} {pname}")
    if pname in fc.PCEN_CLAMPED:
        k = fc.PCEN_CLAMPED[pname]
        assert all(g[k] == 0 for g in got.values()), "a clamped parameter has no gradient"
    if pname in ("gain=1", "root=1"):
        k = 0 if pname == "gain=1" else 2
        full = ref["full"][k]
        assert full != 0 and abs(got["full"][k] - full) < 0.01 * abs(full)  # not the halved one


@pytest.mark.parametrize("shape", [(3, 70, 40), (2, 33, 64)], ids=["3x70x40", "2x33x64"])
@pytest.mark.parametrize("pname", ["default", "interior"])
def test_pcen_backward_bf16_dout(lib, cuda, shape, pname):
    """A bf16 dL/dout: the reference takes the rounded values; same bound."""
    x, douts = dev_inputs(shape, cuda, bf16=True)
    assert all(d.dtype == torch.bfloat16 for d in douts.values())
    p = torch.tensor(fc.PCEN_PARAMS[pname], dtype=torch.float32, device=cuda)
    _, _, _, stats = pcen_stages(lib, x, p, shape)
    got = pcen_grads(lib, x, p, shape, stats, douts)
    assert_probes(got, fc.pcen_reference(shape, pname, bf16=True)["grads"], f"{shape} {pname} bf16 dout")


def test_pcen_module_path_matches_c_abi(fe, lib, cuda):
    """acfe.frontend.pcen (the autograd Function the model uses) gives the C
    ABI's numbers on a partial-workgroup shape, bf16 output and dout included."""
    shape = (3, 70, 40)
    x, douts = dev_inputs(shape, cuda)
    run = pcen_run(lib, cuda, shape, "default")
    p = torch.tensor(fc.PCEN_PARAMS["default"], dtype=torch.float32, device=cuda, requires_grad=True)
    out = fe.pcen(x, p)
    assert_bits(out.detach().cpu().numpy(), run["out"])
    out.backward(douts["full"])
    assert_bits(p.grad.cpu().numpy(), run["grads"]["full"])


# ---------------------------------------------------------------- mel

def mel_both(plan, x, st, pad, power, **kw):
    """plan.mel in both layouts into guarded buffers; asserts they agree bit for
    bit; returns [B, T, M] numpy."""
    b = x.shape[0] if x.dim() == 2 else kw["batch"]
    n = x.shape[1] if x.dim() == 2 else kw["n"]
    t, m = plan.num_frames(n, pad), plan.n_mels
    outs = []
    for layout, shp in (("btm", (b, t, m)), ("bmt", (b, m, t))):
        buf, v = guarded(b * t * m, x.device)
        o = plan.mel(x, st, pad_mode=pad, power=power, layout=layout, out=v.view(shp), **kw)
        torch.cuda.synchronize()
        assert_guard(buf, b * t * m, f"mel {layout}")
        outs.append(o.cpu().numpy())
    np.testing.assert_array_equal(outs[1], outs[0].transpose(0, 2, 1))
    return outs[0]


def assert_mel(out_btm, ref_bmt, what):
    ref = ref_bmt.transpose(0, 2, 1)
    assert out_btm.shape == ref.shape, (out_btm.shape, ref.shape)
    scale = np.abs(ref).reshape(ref.shape[0], -1).max(1)[:, None, None]
    err = (np.abs(out_btm - ref) / scale).max()
    print(f"MEASURE mel {what} max rel err {err:.3e}")
    assert err <= fc.MEL_BOUND, f"{what}: {err:.3e}"


PADS = ("end", "constant", "reflect")
PLANS4096 = ["m127", "m129", "m1", "m32_long", "custom"]


@pytest.mark.parametrize("pname,norm", [(p, False) for p in PLANS4096] + [("custom", True)],
                         ids=PLANS4096 + ["custom-norm"])
def test_mel_4096_band_edges(fe, lib, cuda, pname, norm):
    """k_mel_w4 and k_mel_w5 (1 and 3 frames per wave) on plans the default
    128-mel bank never reaches: odd n_mels (the middle band, in the first and
    in the second band round), one band, bands longer than 40 taps, and a
    custom bank with a DC tap, a Nyquist tap, an empty band and a band over all
    2049 bins; three framings, power 1 and 2, both layouts; one plan also with
    normalise-on-load."""
    kw = fc.mel4096_plans()[pname]
    plan = fe.MelPlan(**kw)
    if pname == "m32_long":
        assert fc.band_lengths(plan.weights).max() > 40
    raw = fc.mel_clips()
    x = torch.from_numpy(raw).to(cuda)
    st = fe.normalize_stats(x) if norm else None
    src = of.normalize(raw) if norm else raw.astype(np.float64)
    assert raw.shape[1] > 4096 // 2
    prev = lib.lib.acfe_mel_w5_frames(0)
    try:
        for pad in PADS:
            for power in (1, 2):
                lib.lib.acfe_mel_w5_frames(0)
                o4 = mel_both(plan, x, st, pad, power)
                for fpw in (1, 3):
                    lib.lib.acfe_mel_w5_frames(fpw)
                    np.testing.assert_array_equal(mel_both(plan, x, st, pad, power), o4)
                assert_mel(o4, fc.mel_reference(src, plan.weights, 4096, fc.HOP, power, pad),
                           f"4096 {pname} {pad} p{power}{' norm' if norm else ''}")
    finally:
        lib.lib.acfe_mel_w5_frames(prev)


@pytest.mark.parametrize("case", fc.small_fft_cases(), ids=lambda c: f"{c[0]}-{c[1]}-n{c[2]}-h{c[3]}")
def test_mel_small_fft(fe, cuda, case):
    """k_mel<NC> at n_fft 2048 and 256 (last Stockham pass radix 2) and 512
    (radix 4): a 64-mel default bank and a bank with a DC tap, a Nyquist tap
    and an empty band; a clip of n_fft / 2 + 1 samples (one frame, T % 4 != 0)
    and one of 3 n_fft + 7."""
    n_fft, bank, n, hop = case
    w = fc.small_bank(n_fft, bank)
    plan = fe.MelPlan(n_fft=n_fft, hop=hop, n_mels=w.shape[0], weights=w)
    raw = fc.mel_clips(n)
    x = torch.from_numpy(raw).to(cuda)
    assert n > n_fft // 2
    for pad in PADS:
        for power in (1, 2):
            out = mel_both(plan, x, None, pad, power)
            assert_mel(out, fc.mel_reference(raw.astype(np.float64), w, n_fft, hop, power, pad),
                       f"{n_fft} {bank} n{n} hop{hop} {pad} p{power}")


# ---------------------------------------------------------------- exact data movement

def _clips_at(rng, n, cs, batch, off, dev):
    """A float32 device buffer whose clips start at float offset `off` of a
    16-byte aligned base; the gaps between clips (and both ends) hold +-1e30,
    which a read outside a clip would turn into the min or the max."""
    total = off + (batch - 1) * cs + n + 8
    host = np.where(np.arange(total) % 2 == 0, np.float32(1e30), np.float32(-1e30)).astype(np.float32)
    clips = rng.normal(0, 1, (batch, n)).astype(np.float32)
    for b in range(batch):
        host[off + b * cs: off + b * cs + n] = clips[b]
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:], clips


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("case", fc.NORM_STATS_CASES, ids=lambda c: f"n{c[0]}-cs{c[1]}-b{c[2]}")
def test_normalize_stats_alignment(lib, cuda, case, off):
    """k_norm_stats' 16-byte path, its scalar path (a clip start that is not
    16-byte aligned), the n % 4 tail and both sides of the four-deep unrolled
    loop (4096 and 4097 float4 per clip); stride 4101 puts aligned and
    misaligned clips into one launch."""
    n, cs, batch = case
    rng = np.random.default_rng(n + off)
    buf, x, clips = _clips_at(rng, n, cs, batch, off, cuda)
    sbuf, st = guarded(2 * batch, cuda)
    lib.call("acfe_normalize_stats", x.data_ptr(), cs, batch, n, st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert_guard(sbuf, 2 * batch, "stats")
    mn, mx = clips.min(1), clips.max(1)
    assert_bits(st.cpu().numpy().reshape(batch, 2), np.stack([mn, mx - mn], 1))


@pytest.mark.parametrize("case", fc.NORM_STATS_CASES, ids=lambda c: f"n{c[0]}-cs{c[1]}-b{c[2]}")
def test_normalize_apply_and_mixup_exact(lib, cuda, case):
    n, cs, batch = case
    rng = np.random.default_rng(n)
    _, x, clips = _clips_at(rng, n, cs, batch, 0, cuda)
    mn, mx = clips.min(1), clips.max(1)
    st = torch.from_numpy(np.stack([mn, mx - mn], 1)).to(cuda)
    ybuf, y = guarded(batch * n, cuda)
    lib.call("acfe_normalize_apply", x.data_ptr(), cs, batch, n, st.data_ptr(), y.data_ptr(), stream())
    torch.cuda.synchronize()
    assert_guard(ybuf, batch * n, "normalize_apply")
    want = of.normalize_f32(clips)
    np.testing.assert_array_equal(bits(y.cpu().numpy().reshape(batch, n)), bits(want))
    if n == 1:
        assert np.isnan(want).all()  # 0 / 0, as the reference
    # mix_up with normalise-on-load of both inputs (dense [B, n])
    c2 = rng.normal(0, 2, (batch, n)).astype(np.float32)
    st2 = torch.from_numpy(np.stack([c2.min(1), c2.max(1) - c2.min(1)], 1)).to(cuda)
    lam = np.linspace(0, 1, batch).astype(np.float32) if batch > 1 else np.array([0.3], np.float32)
    x1, x2 = torch.from_numpy(clips).to(cuda), torch.from_numpy(c2).to(cuda)
    mbuf, m = guarded(batch * n, cuda)
    lib.call("acfe_mixup", x1.data_ptr(), st.data_ptr(), x2.data_ptr(), st2.data_ptr(),
             torch.from_numpy(lam).to(cuda).data_ptr(), batch, n, m.data_ptr(), stream())
    torch.cuda.synchronize()
    assert_guard(mbuf, batch * n, "mixup")
    want = of.mix_up_f32(of.normalize_f32(clips), of.normalize_f32(c2), lam)
    np.testing.assert_array_equal(bits(m.cpu().numpy().reshape(batch, n)), bits(want))


def _copy_rows(lib, dev, src, ss, srows, si, ds, drows, di, count, n, soff=0, doff=0):
    """acfe_copy_rows from a host matrix src [srows, ss] into a SENT-filled
    [drows, ds] destination; both bases moved by soff / doff floats.
    Returns (rc, destination as numpy)."""
    sb = torch.full((soff + srows * ss + 4,), SENT, dtype=torch.float32, device=dev)
    sb[soff: soff + srows * ss] = torch.from_numpy(src.reshape(-1)).to(dev)
    dbuf, d = guarded(doff + drows * ds, dev)
    assert sb.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    sid = None if si is None else torch.tensor(si, dtype=torch.int32, device=dev)
    did = None if di is None else torch.tensor(di, dtype=torch.int32, device=dev)
    rc = lib.lib.acfe_copy_rows(sb[soff:].data_ptr(), ss, srows, None if sid is None else sid.data_ptr(),
                                d[doff:].data_ptr(), ds, drows, None if did is None else did.data_ptr(), count, n,
                                stream())
    torch.cuda.synchronize()
    assert_guard(dbuf, doff + drows * ds, "copy_rows")
    assert (d[:doff] == SENT).all()
    return rc, d[doff:].cpu().numpy().reshape(drows, ds)


def _copy_want(src, si, ds, drows, di, count, n):
    want = np.full((drows, ds), SENT, np.float32)
    for i in range(count):
        want[i if di is None else di[i], :n] = src[i if si is None else si[i], :n]
    return want


COPY_CASES = {
    # name: (ss, srows, si, ds, drows, di, count, n, soff, doff)
    "scalar-n5": (7, 6, [4, 0, 5], 9, 5, [2, 4, 0], 3, 5, 0, 0),
    "scalar-null-src": (7, 6, None, 9, 5, [3, 1, 0, 4], 4, 5, 0, 0),
    "scalar-null-dst": (7, 6, [5, 5, 2], 9, 5, None, 3, 5, 0, 0),            # a repeated source row
    "scalar-null-both": (7, 6, None, 9, 5, None, 5, 5, 0, 0),
    "misaligned-src-n8": (12, 4, [3, 1], 16, 3, [0, 2], 2, 8, 1, 0),         # n % 4 == 0, base not 16-B aligned
    "misaligned-dst-n8": (12, 4, [3, 1], 16, 3, [0, 2], 2, 8, 0, 3),
    "odd-stride-n8": (13, 4, [0, 2], 16, 3, [1, 2], 2, 8, 0, 0),             # n % 4 == 0, stride % 4 != 0
    "vector": (12, 4, [3, 3, 0], 16, 4, [1, 0, 3], 3, 8, 0, 0),
    "vector-2-blocks": (8200, 3, [2, 0], 8196, 3, [0, 2], 2, 8196, 0, 0),    # 2049 float4: a second block of one thread
    "scalar-2-blocks": (2051, 3, [2, 0], 2050, 3, [0, 2], 2, 2049, 0, 0),
    "vector-null-both": (12, 4, None, 16, 4, None, 4, 8, 0, 0),
}


@pytest.mark.parametrize("name", list(COPY_CASES))
def test_copy_rows(lib, cuda, name):
    """k_copy_rows<float4> and k_copy_rows<float>: every condition of the vector
    path failing in turn, NULL index lists on either side, a repeated source
    row; rows and row tails that are not addressed keep their sentinel."""
    ss, srows, si, ds, drows, di, count, n, soff, doff = COPY_CASES[name]
    src = np.random.default_rng(len(name)).normal(0, 1, (srows, ss)).astype(np.float32)
    rc, got = _copy_rows(lib, cuda, src, ss, srows, si, ds, drows, di, count, n, soff, doff)
    assert rc == 0
    assert_bits(got, _copy_want(src, si, ds, drows, di, count, n), name)


def test_copy_rows_count_zero_and_errors(lib, cuda):
    src = np.ones((4, 8), np.float32)
    rc, got = _copy_rows(lib, cuda, src, 8, 4, None, 8, 4, None, 0, 8)
    assert rc == 0 and (got == SENT).all()
    for kw in (dict(ss=7, ds=8, count=2, srows=4, drows=4),    # src stride < n
               dict(ss=8, ds=7, count=2, srows=4, drows=4),    # dst stride < n
               dict(ss=8, ds=8, count=5, srows=4, drows=8),    # count > src rows, NULL src index
               dict(ss=8, ds=8, count=5, srows=8, drows=4)):   # count > dst rows, NULL dst index
        srcm = np.ones((kw["srows"], max(kw["ss"], 8)), np.float32)
        rc, got = _copy_rows(lib, cuda, srcm[:, :kw["ss"]].copy(), kw["ss"], kw["srows"], None, kw["ds"], kw["drows"],
                             None, kw["count"], 8)
        assert rc == lib.E_INVAL and (got == SENT).all(), kw


@pytest.mark.parametrize("M", [13, 64])
@pytest.mark.parametrize("T", [1, 63, 64, 65])
def test_mel_from_spec_shapes(fe, lib, cuda, T, M):
    """k_mel_spec away from M = 128 and the golden T: one frame, one short of /
    exactly / one past a 64-frame workgroup; M that is no multiple of the four
    waves; power 1 and 2; both layouts; and once through the C call with a clip
    stride larger than F * T."""
    F, B = 129, 2
    plan = fe.MelPlan(n_fft=256, n_mels=M)
    rng = np.random.default_rng(T * 100 + M)
    S = np.abs(rng.normal(0, 1, (B, F, T))).astype(np.float32)
    spec = torch.from_numpy(S).to(cuda)
    for power in (1, 2):
        ref = np.einsum("mf,bft->bmt", plan.weights.astype(np.float64), S.astype(np.float64) ** power)
        tol = 2e-6 * np.abs(ref).reshape(B, -1).max(1)[:, None, None]
        for layout, shp in (("btm", (B, T, M)), ("bmt", (B, M, T))):
            buf, v = guarded(B * T * M, cuda)
            out = plan.mel_from_spec(spec, power=power, layout=layout, out=v.view(shp))
            torch.cuda.synchronize()
            assert_guard(buf, B * T * M, f"mel_from_spec {layout}")
            o = out.cpu().numpy()
            o = o.transpose(0, 2, 1) if layout == "btm" else o
            assert (np.abs(o - ref) <= tol).all(), (power, layout, np.abs(o - ref).max() / tol.max() * 2e-6)
        # clip stride > F * T: sentinel rows between the clips
        cs = F * T + 5
        wide = torch.full((B * cs,), 1e30, dtype=torch.float32, device=cuda)
        for b in range(B):
            wide[b * cs: b * cs + F * T] = spec[b].reshape(-1)
        buf, v = guarded(B * T * M, cuda)
        lib.call("acfe_mel_from_spec", plan._h, wide.data_ptr(), cs, B, F, T, power, v.data_ptr(), lib.LAYOUT_BMT, stream())
        torch.cuda.synchronize()
        assert_guard(buf, B * T * M, "mel_from_spec strided")
        np.testing.assert_array_equal(v.cpu().numpy().reshape(B, M, T), o)
