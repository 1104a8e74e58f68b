"""float64 restatement of the Q8_0 KV cache's row format (include/mio_hip.h, mio_hip_llm_load_kv):
ggml's quantize_row_q8_0_ref, every f32 operation as the exact float64 one rounded to f32 once, and
the f16 value attention consumes."""
import numpy as np

_f32 = lambda a: a.astype(np.float32).astype(np.float64)


def rows(x):
    """x [..., k] (f16-exact values) -> (codes int8 [..., k], scales f16 [..., k / 32], f16 [..., k])."""
    x = np.asarray(x)
    b = x.astype(np.float64).reshape(-1, 32)
    d = _f32(np.abs(b).max(axis=1) / 127.0)
    inv = np.where(d != 0, _f32(1.0 / np.where(d != 0, d, 1.0)), 0.0)
    t = _f32(b * inv[:, None])
    q = (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int8)  # roundf: half away from zero
    d16 = d.astype(np.float16)                                     # round to nearest even
    deq = (d16.astype(np.float64)[:, None] * q).astype(np.float16)  # of the stored code: exact product, one rounding
    return q.reshape(x.shape), d16.reshape(x.shape[:-1] + (-1,)), deq.reshape(x.shape)
