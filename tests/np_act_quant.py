"""numpy float32 restatement of the decode step's three activation forms (llm_device.h
quant_regs): Q8_K as ggml's quantize_row_q8_K_ref, Q8_0 as quantize_row_q8_0_ref with an f16 d,
and the bf16 rounding of ggml_compute_fp32_to_bf16; optionally behind ggml_rms_norm + mul.

Every float operation is one float32 operation in the kernels' order. The float -> int
conversion is the hardware's: NaN -> 0, out-of-range values saturate to INT32_MIN / INT32_MAX;
a code is the low byte of the (clamped) conversion and a Q8_K bsum the low 16 bits of the sum of
its 16 conversions. With finite, normal inputs this is exactly ggml's reference (pinned to the
oracle's quantizers in test_act_quant_ref.py); it also says what comes out where ggml's
reference is undefined (an infinite or subnormal maximum, NaNs).

The `mutant` argument of q8_k builds a deliberately wrong quantizer, for the tests that show
the test inputs tell each from the reference."""
import numpy as np

F32 = np.float32
MUTANTS = ("last_max", "half_away", "clamp_128", "bsums_shifted", "d_from_abs")


def _cvt_i32(t: np.ndarray) -> np.ndarray:
    """float32 -> int32 as v_cvt_i32_f32 (truncation of an integral value): NaN -> 0, saturating."""
    t = np.asarray(t, np.float64)
    return np.where(np.isnan(t), 0.0, np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def _roundf(v: np.ndarray) -> np.ndarray:
    """C roundf on float32 (half away from zero), exact; inf and NaN pass through."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        r = np.trunc(v)
        frac = v - r
        return np.where(np.abs(frac) >= F32(0.5), r + np.copysign(F32(1), v), r).astype(F32)


def rms_norm(x: np.ndarray, w: np.ndarray, eps: float) -> np.ndarray:
    """ggml_rms_norm + mul: (x * 1/sqrtf((float)(sum_d(x*x) / n) + eps)) * w, the squares float32,
    their sum double."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    n = x.shape[0]
    tot = np.sum((x * x).astype(np.float64))
    mean = F32(tot * (1.0 / n)) if n & (n - 1) == 0 else F32(tot / n)
    scale = F32(1) / np.sqrt(F32(mean + F32(eps)))
    return ((x * scale).astype(F32) * w).astype(F32)


def q8_k(x: np.ndarray, mutant: str = None):
    """-> (qs int8[k], d float32[k/256], bsums int16[k/16])."""
    assert mutant is None or mutant in MUTANTS
    x = np.asarray(x, F32).reshape(-1, 256)
    nsb = x.shape[0]
    qs = np.zeros((nsb, 256), np.int8)
    d = np.zeros(nsb, F32)
    bs = np.zeros((nsb, 16), np.int16)
    for i, blk in enumerate(x):
        ax = np.where(np.isnan(blk), F32(-1), np.abs(blk))  # a NaN never is the maximum
        amax = ax.max()
        if not amax > 0:
            continue
        hit = np.flatnonzero(ax == amax)
        mx = blk[hit[-1] if mutant == "last_max" else hit[0]]
        if mutant == "d_from_abs":
            mx = np.abs(mx)
        with np.errstate(all="ignore"):
            iscale = F32(-127) / mx
            p = (iscale * blk).astype(F32)
            t = _roundf(p) if mutant == "half_away" else np.rint(p)
            q = np.minimum(_cvt_i32(t), 128 if mutant == "clamp_128" else 127)
            d[i] = F32(1) / iscale
        qs[i] = (q & 0xFF).astype(np.uint8).view(np.int8)
        grp = np.roll(q, 1) if mutant == "bsums_shifted" else q
        bs[i] = (grp.reshape(16, 16).sum(1) & 0xFFFF).astype(np.uint16).view(np.int16)
    return qs.reshape(-1), d, bs.reshape(-1)


def q8_0(x: np.ndarray):
    """-> (qs int8[k], d float32[k/32], the f16-rounded scale)."""
    x = np.asarray(x, F32).reshape(-1, 32)
    with np.errstate(all="ignore"):
        amax = np.where(np.isnan(x), F32(0), np.abs(x)).max(1)
        dd = (amax / F32(127)).astype(F32)
        idv = np.where(dd != 0, F32(1) / np.where(dd != 0, dd, F32(1)), F32(0)).astype(F32)
        q = _cvt_i32(_roundf((x * idv[:, None]).astype(F32)))
        d = dd.astype(np.float16).astype(F32)
    return (q & 0xFF).astype(np.uint8).view(np.int8).reshape(-1), d


def bf16(x: np.ndarray) -> np.ndarray:
    """-> uint16[k], ggml_compute_fp32_to_bf16: nearest even, a NaN kept quiet."""
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    r = ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 64, r).astype(np.uint16)


# ---------------------------------------------------------------------------- test inputs
def inputs(k: int, blk: int = 256):
    """name -> x[k]: the inputs of the quantizer tests. `blk` is the quantization block (256 for
    Q8_K, 32 for Q8_0 / bf16); positions are taken inside blocks of that size."""
    rng = np.random.default_rng(k * 7 + blk)
    nb = k // blk
    out = {"random": (rng.standard_normal(k) * 3).astype(F32)}
    # +a / -a ties (a above every other value) in both orders: within a lane's four values,
    # across lanes of a 16-lane group, across lane groups (lane = position / 4)
    a = F32(13.25)
    pairs = {"lane": (5, 6), "lanes": (10, 37), "groups": (3, 130)} if blk == 256 else \
            {"lane": (5, 6), "lanes": (2, 9), "groups": (1, 30)}
    for nm, (p0, p1) in pairs.items():
        for order, (s0, s1) in (("pos_first", (1, -1)), ("neg_first", (-1, 1))):
            x = rng.standard_normal(k).astype(F32)
            x.reshape(nb, blk)[:, p0] = s0 * a
            x.reshape(nb, blk)[:, p1] = s1 * a
            out[f"tie_{nm}_{order}"] = x
    x = (rng.standard_normal(k) * 2).astype(F32)  # an all-zero block between non-zero ones
    x.reshape(nb, blk)[1 if nb > 2 else 0] = 0
    out["zero_block"] = x
    x = np.zeros(k, F32)  # a single non-zero value
    x[(nb - 1) * blk + blk // 2 + 1] = F32(-0.375)
    out["single"] = x
    # max = +-127 (scale exactly -+1) and values at j + 0.5: nearest-even both ways, and -max -> +127
    for sgn in (1, -1):
        x = (np.arange(k) % 125 + 0.5).astype(F32) * np.where(np.arange(k) % 2, 1, -1).astype(F32)
        x.reshape(nb, blk)[:, 7] = sgn * 127
        x.reshape(nb, blk)[:, 19] = -sgn * 127
        out[f"half_max{'+' if sgn > 0 else '-'}127"] = x
    x = np.zeros(k, F32)  # a subnormal maximum: 127 / max overflows
    x[::3] = F32(1e-40)
    x[1::3] = F32(-3e-41)
    x.reshape(nb, blk)[:, 11] = F32(-1e-40)
    out["subnormal_max"] = x
    out["huge_1e30"] = (rng.standard_normal(k) * 1e30).astype(F32)
    return out


def nonfinite_inputs(k: int, blk: int = 256):
    rng = np.random.default_rng(k + 99)
    nb = k // blk
    x = rng.standard_normal(k).astype(F32)
    x[::17] = np.nan
    y = rng.standard_normal(k).astype(F32)
    y.reshape(nb, blk)[:, 9] = -np.inf
    z = np.zeros(k, F32)
    z[::2] = np.nan
    return {"nan_values": x, "inf_max": y, "nan_and_zero": z}
