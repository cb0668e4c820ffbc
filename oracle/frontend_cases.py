"""Case table of the front-end edge tests (ORACLE, test-only): the PCEN shapes,
input recipe, parameter sets and gradient probes, the mel plans and clips, and
the float64 references that go with them.  tests/test_frontend_cases.py checks
the table's own conditions on the CPU (tie counts, extremum gap, live probes,
float32 noise of the reference); tests/test_frontend_edges_gpu.py runs the HIP
kernels of csrc/frontend.hip against it.  See oracle/__init__.py.

PCEN launch geometry the shapes are chosen against (csrc/frontend.hip): a
workgroup owns PCEN_RB = 64 (clip, mel) rows, row = b * M + m, and walks T in
chunks of PCEN_TCH = 32 steps, prefetching the next chunk when
t0 + 32 < T."""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import frontend as of
from .torch_ref import pcen_torch

PCEN_RB, PCEN_TCH = 64, 32

# (B, T, M)
PCEN_SHAPES = [
    (3, 70, 40),    # 120 rows = 64 + 56; both workgroups span two clips; two chunks + 6 steps
    (2, 33, 64),    # two full workgroups; a one-step last chunk
    (1, 32, 64),    # exactly one chunk: the prefetch never fires
    (1, 31, 65),    # a single short chunk; a one-row second workgroup
    (2, 96, 13),    # one partial workgroup; three exact chunks
    (1, 1, 5),      # T == 1
    (1, 513, 128),  # the production row
]

# (gain, bias, root, smooth): interior, one parameter AT its bound, one BEYOND it
PCEN_PARAMS = {
    "default": (0.98, 2.0, 2.0, 0.04),
    "interior": (0.5, 1.5, 3.0, 0.2),
    "gain=1": (1.0, 2.0, 2.0, 0.04),
    "root=1": (0.98, 2.0, 1.0, 0.04),
    "smooth=1": (0.98, 2.0, 2.0, 1.0),
    "smooth=0": (0.98, 2.0, 2.0, 0.0),
    "gain>1": (1.3, 2.0, 2.0, 0.04),
    "root<1": (0.98, 2.0, 0.5, 0.04),
    "smooth<0": (0.98, 2.0, 2.0, -0.1),
    "smooth>1": (0.98, 2.0, 2.0, 1.5),
}
# index of the parameter whose gradient TF masks to exactly 0 in that set
PCEN_CLAMPED = {"gain>1": 0, "root<1": 2, "smooth<0": 3, "smooth>1": 3}

PROBE_COLUMNS = (0, 1, 7, 8, 31, 32, 33, 63, 64)  # and T - 1


def probe_rows(shape):
    B, T, M = shape
    return sorted({r for r in (0, M - 1, M, 63, 64, B * M - 1) if r < B * M})


def zero_row_mel(shape):
    """The all-zero row of clip 0: mel M // 2, moved up past the probed rows
    (its output is the constant -1, so a row probe on it has no gradient at
    all: (1, 513, 128) probes row 64 == M // 2)."""
    B, T, M = shape
    m = M // 2
    while m in probe_rows(shape) or m == 1:
        m += 1
    return m


# The live row of clip 0 whose first sample is zero (its EMA starts at 0, and
# stays there at smooth 0, so its y is ~1e6 times everybody else's): the row
# of the planted maximum, so that the maximum stays where it was planted at
# every parameter set; never the last row of the tensor.
ZERO_FIRST_MEL = 1


# shape -> (input seed, dout seed): the first pair, walking the diagonals
# from (0, 0), at which every condition of tests/test_frontend_cases.py holds
# with some margin for every parameter set -- conditions on the reference
# alone.  What fails at other seeds: at gain 1.0 the first sample after a
# zero EMA gives q ~ 1 / smooth whatever its size, so (row 1, t = 1) competes
# with the planted maximum and the gap can drop to 1e-5; and the corner
# one-hot is one element against sums over thousands, so a small g there
# leaves it under 1e-3 of the largest probe.
PCEN_SEEDS = {(3, 70, 40): (5, 2), (2, 33, 64): (4, 3), (1, 32, 64): (10, 0), (1, 31, 65): (1, 0),
              (2, 96, 13): (0, 0), (1, 1, 5): (1, 0), (1, 513, 128): (9, 2)}


def pcen_input(shape, seed=None) -> np.ndarray:
    """mel [B, T, M] float32 of the recipe (tests/test_frontend_cases.py checks
    what it promises)."""
    B, T, M = shape
    rng = np.random.default_rng(1000 * T + M + 100003 * (PCEN_SEEDS[shape][0] if seed is None else seed))
    x = np.exp(rng.normal(0.0, 2.0, (B, T, M))).astype(np.float32)
    if T == 1:
        # a_0 = x_0, so y depends on x only through q = x / (eps + x)^gain.
        # At gain 1 that is 1 - eps / x: values far above eps = 1e-6 all give
        # the same y and mx - mn is float32 rounding noise, in the reference
        # as much as in the kernel; at gain 0.5 values near eps give q ~ 1e-3
        # and the bias / root gradients cancel to noise.  So the five values
        # sit on chosen decades (mel 0..4: 1e-5, the planted maximum, 1e-7,
        # 10^-2.5, 1e-4) with the base's jitter damped to its fourth root: y
        # spreads over its range at every parameter set, the maximum (64
        # times the largest, q = 1 - 5e-6 at gain 1) keeps its distance, and
        # the probed rows 0 and M - 1 hold neither extremum (there out is the
        # constant -1 / +1 and has no gradient).
        x = np.sqrt(np.sqrt(x)) * np.float32(10.0) ** np.array([[[-5, -5, -7, -2.5, -4]]], np.float32)
        assert x.dtype == np.float32
        j = int(x.argmin())
        x[0, 0, [2, j]] = x[0, 0, [j, 2]]
    else:
        x[:, T // 2: T // 2 + T // 8, :] = 0.0
        x[0, :, zero_row_mel(shape)] = 0.0
        x[0, 0, ZERO_FIRST_MEL] = 0.0
    x[0, min(5, T - 1), 1] = np.float32(64.0) * x.max()
    if B > 1:
        x[B - 1] = x[0]
    return x


def pcen_douts(shape, bf16=False, seed=None):
    """{probe name: dout [B, M, T] float64}, dout = g * mask: one column per
    probed t, one row per probed row, the corner one-hot and the full tensor.
    bf16: g rounded to bfloat16 first (what a bf16 dout holds)."""
    B, T, M = shape
    g = torch.randn((B, M, T), generator=torch.Generator().manual_seed(7 + 31 * T + M + 100003 * (PCEN_SEEDS[shape][1] if seed is None else seed)), dtype=torch.float64)
    if bf16:
        g = g.to(torch.bfloat16).double()
    out = {}
    for t in sorted({t for t in PROBE_COLUMNS + (T - 1,) if t < T}):
        d = torch.zeros_like(g)
        d[:, :, t] = g[:, :, t]
        out[f"t{t}"] = d
    gr = g.reshape(B * M, T)
    for r in probe_rows(shape):
        d = torch.zeros_like(gr)
        d[r] = gr[r]
        out[f"row{r}"] = d.reshape(B, M, T)
    d = torch.zeros_like(g)
    d[B - 1, M - 1, T - 1] = g[B - 1, M - 1, T - 1]
    out["corner"] = d
    out["full"] = g
    return out


def _jacobian(x, params, dtype, scope):
    """out [B,M,T] and J[k] = d out / d params[k] of pcen_torch by forward-mode
    autograd (four tangents); every probe's gradient is then sum(dout * J[k]),
    which tests/test_frontend_cases.py pins to the reverse-mode backward."""
    import torch.autograd.forward_ad as fwAD

    xt = torch.from_numpy(x).to(dtype)
    p = torch.tensor(params, dtype=dtype)
    J = []
    for k in range(4):
        tang = torch.zeros(4, dtype=dtype)
        tang[k] = 1.0
        with fwAD.dual_level():
            o = pcen_torch(xt, fwAD.make_dual(p, tang), scope_minmax=scope)
            prim, tan = fwAD.unpack_dual(o)
            J.append(torch.zeros_like(prim) if tan is None else tan.clone())
    return prim.clone(), torch.stack(J)


@functools.lru_cache(maxsize=None)
def pcen_reference(shape, pname, dtype=torch.float64, scope=None, bf16=False, seeds=None):
    """dict(out [B,M,T], y (un-normalised) [B,M,T], grads {probe: [4]}) of
    pcen_torch in `dtype`; douts are float64 in either case."""
    xs, gs = seeds or (None, None)
    x = pcen_input(shape, xs)
    params = PCEN_PARAMS[pname]
    out, J = _jacobian(x, params, dtype, scope)
    y = of.pcen_unnormalised(x.astype(np.float64), *params).transpose(0, 2, 1)
    Jd = J.double()
    grads = {k: (d[None] * Jd).sum((1, 2, 3)).numpy() for k, d in pcen_douts(shape, bf16, gs).items()}
    return dict(out=out.double().numpy(), y=y, grads=grads)


def probe_scales(ref_grads):
    """S[k]: the largest |ref_k| over the case's probes (1 if zero);
    s[probe] = max_k |ref_k| / S[k]."""
    S = np.max([np.abs(g) for g in ref_grads.values()], axis=0)
    S = np.where(S == 0, 1.0, S)
    return S, {k: float(np.max(np.abs(g) / S)) for k, g in ref_grads.items()}


def probe_errors(got_grads, ref_grads):
    """{probe: (e, s)}, e = max_k |got_k - ref_k| / S[k].  The bound is
    e <= 2e-3 * s (the project's dPCEN bound, per probe)."""
    S, s = probe_scales(ref_grads)
    return {k: (float(np.max(np.abs(np.asarray(got_grads[k], np.float64) - ref_grads[k]) / S)), s[k])
            for k in ref_grads}


DPCEN_BOUND = 2e-3
PCEN_BOUND = 5e-5


def pcen_bwd_restated(x, params, dout, eps=1e-6, defect=None):
    """The one-pass backward of k_pcen_bwd / k_pcen_bwd_fin restated in float64
    numpy, with its launch geometry (64-row workgroups, 32-step chunks): the
    forward-mode dEMA/dw, the 14 accumulators and the finaliser with the TF
    tie and clamp rules.  x [B,T,M], dout [B,M,T] -> dparams [4].  `defect`
    plants one of the mistakes the probes are meant to catch:
      "last_step":  the last step of a partial chunk is left out
      "last_row":   the last row of a partial workgroup is left out
      "half_gain":  the gain gradient is halved at gain == 1.0."""
    x = np.asarray(x, np.float64)
    B, T, M = x.shape
    pg, pb, pr, pw = (float(v) for v in params)
    g, b, r, w = min(pg, 1.0), pb, max(pr, 1.0), min(max(pw, 0.0), 1.0)
    inv_r = 1.0 / r
    bpow = b ** inv_r
    xr = x.transpose(0, 2, 1).reshape(B * M, T)  # rows
    d = np.asarray(dout, np.float64).reshape(B * M, T)
    a, da = xr[:, 0].copy(), np.zeros(B * M)
    dy = np.zeros((4, B * M, T))
    y = np.zeros((B * M, T))
    for t in range(T):
        a_prev = a
        a = w * xr[:, t] + (1.0 - w) * a
        da = (xr[:, t] - a_prev) + (1.0 - w) * da
        s = eps + a
        q = xr[:, t] / s ** g
        u = q + b
        ur = u ** inv_r
        y[:, t] = ur - bpow
        dydu = inv_r * ur / u
        dy[0, :, t] = dydu * (-q * np.log(s))
        dy[1, :, t] = dydu - inv_r * bpow / b
        dy[2, :, t] = -(inv_r * inv_r) * (ur * np.log(u) - bpow * np.log(b))
        dy[3, :, t] = dydu * (-g * q / s) * da
    mn, mx = y.min(), y.max()
    use = np.ones((B * M, T), bool)
    if defect == "last_step" and T % PCEN_TCH:
        use[:, T - 1] = False
    if defect == "last_row" and (B * M) % PCEN_RB:
        use[B * M - 1] = False
    tot = np.zeros(14)
    for k in range(4):
        tot[k] = (d * dy[k])[use].sum()
        tot[4 + k] = dy[k][use & (y == mx)].sum()
        tot[8 + k] = dy[k][use & (y == mn)].sum()
    tot[12], tot[13] = d[use].sum(), (d * y)[use].sum()
    nmin, nmax = (y == mn).sum(), (y == mx).sum()
    D = mx - mn
    S1 = (2.0 / D) * (tot[13] - mn * tot[12])
    dmx, dmn = -S1 / D, (S1 - 2.0 * tot[12]) / D
    out = np.array([(2.0 / D) * tot[k] + dmx / nmax * tot[4 + k] + dmn / nmin * tot[8 + k] for k in range(4)])
    if not pg <= 1.0:
        out[0] = 0.0
    if not pr >= 1.0:
        out[2] = 0.0
    if not 0.0 <= pw <= 1.0:
        out[3] = 0.0
    if defect == "half_gain" and pg == 1.0:
        out[0] *= 0.5
    return out


# ---------------------------------------------------------------- mel

SR, HOP = 48000, 281
MEL_N, MEL_B = 5000, 2
MEL_BOUND = 2e-5


def mel_clips(n=MEL_N, b=MEL_B, seed=31) -> np.ndarray:
    """[b, n] float32: two linear chirps per clip plus 0.25 DC plus
    0.25 * (-1)^n, so that bins 0 and n_fft / 2 carry energy."""
    rng = np.random.default_rng(seed + n)
    t = np.arange(n) / SR
    out = np.zeros((b, n))
    for i in range(b):
        for _ in range(2):
            f0, f1 = rng.uniform(300, 10000, 2)
            out[i] += rng.uniform(0.05, 0.2) * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / max(t[-1], 1e-9) * t * t))
        out[i] += rng.normal(0, 0.01, n)
    out += 0.25 + 0.25 * (-1.0) ** np.arange(n)
    return out.astype(np.float32)


def default_bank(n_mels, n_fft, fmin=100, fmax=11000):
    return of.mel_f(SR, n_mels, fmin, fmax, n_fft, 1000)


def custom_bank_4096():
    """The default 128-mel bank with row 0 a single tap at bin 0 (DC), row 127
    a single tap at bin 2048 (Nyquist), row 5 empty and row 64 a band over all
    2049 bins."""
    w = default_bank(128, 4096).copy()
    w[0] = 0
    w[0, 0] = 0.5
    w[127] = 0
    w[127, 2048] = 0.5
    w[5] = 0
    w[64] = (1e-4 * (1.0 + 0.5 * np.cos(np.arange(2049) * 0.01))).astype(np.float32)
    return w


def edge_bank(n_mels, n_fft):
    """A default bank whose first row is one tap at bin 0, whose last row is one
    tap at bin n_fft / 2 and whose row 2 is empty."""
    w = default_bank(n_mels, n_fft).copy()
    w[0] = 0
    w[0, 0] = 0.5
    w[-1] = 0
    w[-1, n_fft // 2] = 0.5
    w[2] = 0
    return w


# n_fft 4096 plans: name -> MelPlan keyword arguments (weights: a dense bank)
def mel4096_plans():
    return {
        "m127": dict(n_mels=127),                       # odd: the middle band, first round
        "m129": dict(n_mels=129),                       # odd: the middle band in the second round
        "m1": dict(n_mels=1),
        "m32_long": dict(n_mels=32),                    # bands longer than 40 taps
        "custom": dict(n_mels=128, weights=custom_bank_4096()),
    }


def band_lengths(weights):
    return of.mel_bands(weights)[1]


def small_fft_cases():
    """(n_fft, bank name, n, hop) for k_mel<NC>."""
    out = []
    for n_fft in (2048, 512, 256):
        for bank in ("default64", "edge"):
            for n in (n_fft // 2 + 1, 3 * n_fft + 7):
                for hop in (281, 64) if n_fft == 256 else (281,):
                    out.append((n_fft, bank, n, hop))
    return out


def small_bank(n_fft, bank):
    return default_bank(64, n_fft) if bank == "default64" else edge_bank(16, n_fft)


def mel_reference(raw64, weights, n_fft, hop, power, pad_mode):
    """[B, M, T] float64 of the dense bank."""
    if pad_mode == "end":
        return of.raw_to_mel(raw64, weights, n_fft, hop, power=power)
    return of.get_spect(raw64, weights, n_fft, hop, power, pad_mode)


# ---------------------------------------------------------------- exact data movement

# (n, clip_stride, batch)
NORM_STATS_CASES = [(1, 1, 3), (3, 3, 2), (4099, 4101, 3), (16388, 16388, 2), (16384, 16384, 1)]
