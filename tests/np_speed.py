"""WSOLA speaking rate in float64: the definition of include/mio_hip.h ("speaking rate"), restated
once for tests/test_speed_gpu.py. x = 0 outside [0, n); s is the f32 speed widened to double."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

N, HS, D = 1024, 512, 512
PAD = 4096  # zeros either side: every index the definition reaches lies inside
W = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32).astype(np.float64)
LAGS = np.arange(-D, D)


def voiced(n=30011, rate=44100.0):
    """Eight harmonics of an f0 gliding 90 -> 220 Hz over 30011 samples, under a 3 Hz envelope,
    silent on [12000, 17000) (longer than 2 N); the first n samples."""
    t = np.arange(30011) / rate
    phase = 2 * np.pi * (90.0 * t + 0.5 * (220.0 - 90.0) / t[-1] * t * t)
    x = sum(np.sin(h * phase + 0.3 * h) / h for h in range(1, 9)) * (0.3 + 0.15 * np.sin(2 * np.pi * 3.0 * t))
    x[12000:17000] = 0.0
    return x[:n].astype(np.float32)


def sizes(n, s):
    """(n_out, nominal frame starts p[F])."""
    s = float(np.float32(s))
    n_out = math.ceil(n / s)
    return n_out, np.floor((np.arange(-(-n_out // HS) + 1) - 1) * HS * s + 0.5).astype(np.int64)


def scores(xp, p_m, a_prev):
    """c(d) for d in [-D, D) and ||t||, on the padded signal xp."""
    t = xp[PAD + a_prev + HS:PAD + a_prev + HS + N]
    win = sliding_window_view(xp[PAD + p_m - D:PAD + p_m + D + N - 1], N)
    return win @ t / np.sqrt((win * win).sum(1) + 1e-12), float(np.sqrt(t @ t))


def pick(c):
    cand = LAGS[c == c.max()]
    return int(cand[np.lexsort((cand, np.abs(cand)))][0])


def wsola(x, s, forced=None):
    """y, offsets, and per frame m >= 1 (score of the offset used, best score, ||t||). forced: use
    these offsets (teacher forcing: each frame's template follows the forced a_{m-1})."""
    n_out, p = sizes(len(x), s)
    xp = np.concatenate([np.zeros(PAD), np.asarray(x, np.float64), np.zeros(PAD)])
    off, rows = np.zeros(len(p), np.int64), []
    for m in range(1, len(p)):
        c, tn = scores(xp, int(p[m]), int(p[m - 1] + off[m - 1]))
        off[m] = pick(c) if forced is None else forced[m]
        rows.append((c[off[m] + D], c.max(), tn))
    y = np.zeros(len(p) * HS + HS)
    for m in range(len(p)):  # frame m covers outputs [(m - 1) Hs, (m + 1) Hs): stored shifted by Hs
        a = PAD + int(p[m] + off[m])
        y[m * HS:m * HS + N] += W * xp[a:a + N]
    return y[HS:HS + n_out], off, np.array(rows).reshape(-1, 3)
