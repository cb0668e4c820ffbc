"""The float64 reference of the resampling tests (test_resample_host.py,
test_resample_gpu.py), written from scipy.signal.resample_poly's definition
and independent of predict.resample_plan: the taps come from firwin here."""
import math

import numpy as np
from scipy.signal import firwin


def ratio(rate, sr=48000):
    g = math.gcd(rate, sr)
    return sr // g, rate // g


def taps(up, down):
    """resample_poly's float32 taps for a float32 input, and the offset t0 of
    output 0 on the up-sampled axis."""
    half_len = 10 * max(up, down)
    h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)).astype(np.float32)
    h *= up
    n_pre_pad = down - half_len % down
    n_pre_remove = (half_len + n_pre_pad) // down
    return h, n_pre_remove * down - n_pre_pad


def n_out(n_in, up, down):
    return -(-n_in * up // down)


def terms(h, up):
    """K: the most taps that meet one output."""
    return -(-len(h) // up)


def formula(x, h, up, down, t0, n=None):
    """out[n] = sum_k h[p + k up] x[j0 - k] in float64 for the output indices
    `n` (default: all n_out of them) -> (out, A) with A = sum_k |h x|."""
    x = np.asarray(x)
    h64 = np.asarray(h, np.float64)
    if n is None:
        n = np.arange(n_out(len(x), up, down), dtype=np.int64)
    n = np.asarray(n, np.int64)
    t = n * down + t0
    p, j0 = t % up, t // up
    out, a = np.zeros(len(n)), np.zeros(len(n))
    for k in range(terms(h64, up)):
        ih, jx = p + k * up, j0 - k
        ok = (ih < len(h64)) & (jx >= 0) & (jx < len(x))
        term = h64[ih[ok]] * x[jx[ok]].astype(np.float64)
        out[ok] += term
        a[ok] += np.abs(term)
    return out, a
