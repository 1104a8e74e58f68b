"""The pitch resampler in float64: the definition of include/mio_hip.h ("pitch"), restated once for
tests/test_pitch_gpu.py and tests/test_pitch_host.py. x = 0 outside [0, n); r is the f32 ratio
widened to double; the table entries are the f32 ones the device holds."""
import math

import numpy as np

Z, Q, BETA = 16, 512, 0.1102 * (80.0 - 8.7)
_U = np.arange(Z * Q + 1) / Q
TABLE = (np.sinc(_U) * np.i0(BETA * np.sqrt(1.0 - (_U / Z) ** 2)) / np.i0(BETA)).astype(np.float32).astype(np.float64)


def taps(r):
    """(c, K): the cutoff min(1, 1 / r) in f32 and K = ceil(Z / c); the sum has 2 K taps."""
    c = float(np.float32(1.0) / np.float32(r)) if np.float32(r) > 1 else 1.0
    return c, math.ceil(Z / c)


def pitch(x, r, first=0):
    """(y[first:], S[first:]) for the n_out = ceil(n / r) outputs: y[j] = c sum_k x[i_j + k] h(c (k - f_j))
    and S_j = c sum_k |x[i_j + k]| |h(c (k - f_j))|, the scale of the f32 kernel's rounding error."""
    r, x = float(np.float32(r)), np.asarray(x, np.float64)
    (c, K), n_out = taps(r), math.ceil(len(x) / r)
    t = np.arange(first, n_out, dtype=np.float64) * r
    i = np.floor(t)
    k = np.arange(-K + 1, K + 1)
    p = np.abs(c * (k[None, :] - (t - i)[:, None])) * Q
    ip = np.minimum(p.astype(np.int64), Z * Q - 1)
    h = np.where(p < Z * Q, TABLE[ip] + (p - ip) * (TABLE[ip + 1] - TABLE[ip]), 0.0)
    xv = np.concatenate([np.zeros(K), x, np.zeros(K + 1)])[i.astype(np.int64)[:, None] + k[None, :] + K]
    return c * (xv * h).sum(1), c * (np.abs(xv) * np.abs(h)).sum(1)
