"""TEST INFRASTRUCTURE — attention of one decode position in plain numpy float64.

The reference's operation (llama.cpp attention over an F16 K/V cache) for the attention launches
of csrc/hip/llm_attention.h, with no chunks and no online softmax:

  * q heads and the new k row: + bias (qwen2), RMSNorm with attn_q_norm / attn_k_norm (qwen3,
    lfm2), RoPE in the model's pairing (NEOX (i, i + hd/2) or NORM (2i, 2i + 1)) at `pos`,
    rounded to f16; the new v row (+ bias) rounded to f16;
  * scores = q.K / sqrt(hd) over cache rows 0..pos-1 as given and the new row at pos; softmax; P.V.

The RoPE angles are ggml's rope cache (theta = pos, theta *= base^(-2/hd) per pair, in f32): the
recurrence is part of the operation, so it is kept in f32; cos / sin of each f32 angle are
rounded to f32 as the table the model reads holds them. Everything else is float64.

Unambiguous inputs (`nudge`): the GPU prepares q and k in f32, and an f32-ulp difference flips an
f16 rounding that falls next to a rounding midpoint. `nudge` moves raw elements by 1 + 2^-13 until
no prepared q, k or v element y lies within 2^-18 |y| + 2^-20 T of a midpoint, T being the summed
magnitudes of the terms y is the sum of (the rotation's x0 cos and x1 sin, a value and its bias).
The second part covers a rotation that cancels: the f32 preparation errs by at most about
6 * 2^-24 T there (norm scale and weight 3, table value 2, product 1, in units of 2^-24 of each
term), whatever |y| is. With such inputs the f16 rows are the same bits on both sides and the
tests need no allowance for flipped roundings.

`bound` is the f32 error model of the kernels (derived in tests/test_attention_gpu.py);
`chunked` restates the kernels' chunk / merge-batch structure in float64, which must agree with
the plain softmax to rounding and carries the mutants of the CPU teeth test.
"""
from __future__ import annotations

import numpy as np

from miotts_amd import gguf_np

CHUNK = 64        # kAttChunk: positions per attention chunk
MERGE_BATCH = 8   # merge_out4: chunk records per batch
U = 2.0 ** -24    # f32 unit roundoff
MARGIN = 2.0 ** -18        # of the prepared value
MARGIN_TERMS = 2.0 ** -20  # of the terms it is summed from


class Model:
    """Head shape, norm weights, biases and RoPE settings of a GGUF LLM."""

    def __init__(self, path: str):
        g = gguf_np.GGUFReader(path)
        a = g.kv["general.architecture"]
        kv = lambda k, d=None: g.kv.get(f"{a}.{k}", d)
        self.arch = a
        self.n_layer = kv("block_count")
        self.n_head = kv("attention.head_count")
        hkv = kv("attention.head_count_kv", self.n_head)
        self.n_kv = max(hkv) if isinstance(hkv, list) else hkv
        self.hd = kv("attention.key_length", kv("embedding_length") // self.n_head)
        self.G = self.n_head // self.n_kv
        self.eps = float(np.float32(kv("attention.layer_norm_rms_epsilon", 1e-6)))
        self.neox = a in ("qwen2", "qwen3", "lfm2")
        self.qk_norm = a in ("qwen3", "lfm2")
        self.base = float(np.float32(kv("rope.freq_base", 10000.0)))
        f64 = lambda n: g.tensor(n).array().astype(np.float64).reshape(-1) if n in g.by_name else None
        self.layers = []
        for i in range(self.n_layer):
            p = f"blk.{i}."
            self.layers.append({"q_norm": f64(p + "attn_q_norm.weight"), "k_norm": f64(p + "attn_k_norm.weight"),
                                "bq": f64(p + "attn_q.bias"), "bk": f64(p + "attn_k.bias"),
                                "bv": f64(p + "attn_v.bias")})
        self.n_qkv = (self.n_head + 2 * self.n_kv) * self.hd

    def rope_row(self, pos: int):
        """(cos, sin) [hd / 2] of position pos: ggml's f32 angle recurrence, f32 table values."""
        ts = np.float32(self.base ** (-2.0 / self.hd))
        th = np.float32(pos)
        c, s = np.zeros(self.hd // 2), np.zeros(self.hd // 2)
        for i in range(self.hd // 2):
            c[i], s[i] = np.float32(np.cos(np.float64(th))), np.float32(np.sin(np.float64(th)))
            th = np.float32(th * ts)
        return c, s

    def _prep(self, il: int, raw: np.ndarray, rope_pos: int):
        """Prepared (q [H, hd], k [Hkv, hd], v [Hkv, hd]) in float64 before the f16 rounding, and
        for each the magnitude of the terms its elements are summed from."""
        L, H, Hk, hd = self.layers[il], self.n_head, self.n_kv, self.hd
        raw = np.asarray(raw, np.float32).astype(np.float64).reshape(-1)
        assert raw.size == self.n_qkv
        q, k, v = raw[:H * hd].reshape(H, hd), raw[H * hd:(H + Hk) * hd].reshape(Hk, hd), raw[(H + Hk) * hd:].reshape(Hk, hd)
        vmag = np.abs(v)
        if L["bq"] is not None:
            q, k = q + L["bq"].reshape(H, hd), k + L["bk"].reshape(Hk, hd)
            vmag = vmag + np.abs(L["bv"].reshape(Hk, hd))
            v = v + L["bv"].reshape(Hk, hd)
        if self.qk_norm:
            norm = lambda x, w: x * (1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + self.eps)) * w
            q, k = norm(q, L["q_norm"]), norm(k, L["k_norm"])
        c, s = self.rope_row(rope_pos)
        i0 = np.arange(hd // 2) if self.neox else 2 * np.arange(hd // 2)
        i1 = i0 + hd // 2 if self.neox else i0 + 1

        def rope(x):
            y, mag = np.empty_like(x), np.empty_like(x)
            x0, x1 = x[:, i0], x[:, i1]
            y[:, i0], y[:, i1] = x0 * c - x1 * s, x0 * s + x1 * c
            mag[:, i0], mag[:, i1] = np.abs(x0 * c) + np.abs(x1 * s), np.abs(x0 * s) + np.abs(x1 * c)
            return y, mag

        (q, qmag), (k, kmag) = rope(q), rope(k)
        return (q, k, v), (qmag, kmag, vmag), (i0, i1)

    def prepare(self, il: int, raw: np.ndarray, pos: int, rope_pos: int = None):
        """f16-rounded q [H, hd], k [Hkv, hd], v [Hkv, hd] (float16 arrays) of the raw row at pos."""
        (q, k, v), _, _ = self._prep(il, raw, pos if rope_pos is None else rope_pos)
        return q.astype(np.float16), k.astype(np.float16), v.astype(np.float16)

    def ambiguous(self, il: int, raw: np.ndarray, pos: int):
        """Boolean masks (q, k, v shaped) of prepared elements within MARGIN of an f16 rounding
        midpoint."""
        vals, mags, _ = self._prep(il, raw, pos)
        return [midpoint_distance(y) < MARGIN * np.abs(y) + MARGIN_TERMS * m for y, m in zip(vals, mags)]

    def nudge(self, il: int, raw: np.ndarray, pos: int, max_rounds: int = 200) -> np.ndarray:
        """raw with elements multiplied by about 1 + 2^-13 until `ambiguous` finds none: for an offending
        q / k element, the element of its rotation pair whose term is the larger one (the other
        may be multiplied by a cos or sin near 0); for a v element, itself. The step is 16 times
        the margin, and small enough that under a q/k norm, where it rescales the whole head by
        about 2^-13 / hd, it rarely pushes another element of the head into a margin. Asserts
        convergence."""
        raw = np.array(raw, np.float32).reshape(-1)
        H, Hk, hd = self.n_head, self.n_kv, self.hd
        L = self.layers[il]
        c, s = self.rope_row(pos)
        i0 = np.arange(hd // 2) if self.neox else 2 * np.arange(hd // 2)
        i1 = i0 + hd // 2 if self.neox else i0 + 1
        pair = np.empty(hd, np.int64)   # element -> index of its rotation pair
        pair[i0] = pair[i1] = np.arange(hd // 2)

        def bump(i, mag):
            # by a fraction of the element, or of the terms beside it where it is small against
            # them (a zero raw value beside a bias)
            raw[i] += np.float32((step - 1.0) * max(abs(raw[i]), mag)) * (-1 if raw[i] < 0 else 1)

        for rnd in range(max_rounds):
            # 2^-13 .. 2^-12, another fraction every round: a fixed step can equal the f16 spacing
            # at the prepared value and land beside the next midpoint every time
            step = 1.0 + 2.0 ** -13 * (1.0 + (rnd * 0.6180339887) % 1.0)
            vals, mags, _ = self._prep(il, raw, pos)
            aq, ak, av = [midpoint_distance(y) < MARGIN * np.abs(y) + MARGIN_TERMS * g for y, g in zip(vals, mags)]
            if not (aq.any() or ak.any() or av.any()):
                return raw
            for base, a, bias, mg in ((0, aq, L["bq"], mags[0]), (H * hd, ak, L["bk"], mags[1])):
                for h, e in zip(*np.nonzero(a)):
                    j = pair[e]
                    x = raw[base + h * hd:base + (h + 1) * hd].astype(np.float64)
                    if bias is not None:
                        x = x + bias[h * hd:(h + 1) * hd]
                    # y[i0] = x0 c - x1 s, y[i1] = x0 s + x1 c
                    t0, t1 = (x[i0[j]] * c[j], x[i1[j]] * s[j]) if e == i0[j] else (x[i0[j]] * s[j], x[i1[j]] * c[j])
                    # under a norm the raw scale is arbitrary: there the element's own size is used
                    bump(base + h * hd + (i0[j] if abs(t0) >= abs(t1) else i1[j]), 0.0 if self.qk_norm else mg[h, e])
            for h, e in zip(*np.nonzero(av)):
                bump((H + Hk) * hd + h * hd + e, mags[2][h, e])
        raise AssertionError(f"nudge: still ambiguous after {max_rounds} rounds")


def midpoint_distance(y: np.ndarray) -> np.ndarray:
    """|y - m| for the f16 rounding midpoint m nearest to each (finite, f16-range) y."""
    y = np.asarray(y, np.float64)
    h = y.astype(np.float16)
    hf = h.astype(np.float64)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    return np.minimum(np.abs(y - 0.5 * (hf + up)), np.abs(y - 0.5 * (hf + dn)))


def attend(q: np.ndarray, K: np.ndarray, V: np.ndarray):
    """One head: q [hd], K, V [T, hd] (f16-exact values, any float dtype) -> (out [hd], scores
    [T], softmax weights [T]) in float64."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    s = (K @ q) / np.sqrt(q.size)
    p = np.exp(s - s.max())
    w = p / p.sum()
    return w @ V, s, w


def bound(q: np.ndarray, K: np.ndarray, V: np.ndarray, s: np.ndarray, w: np.ndarray, v_floor: float = 0.0):
    """Per-output error bound [hd] of the kernels' f32 arithmetic for one head (model and
    derivation: tests/test_attention_gpu.py). v_floor: absolute floor per V element (0 unless
    the hardware flushes f16 subnormals)."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    T, hd = K.shape
    nch = (T + CHUNK - 1) // CHUNK
    nb = (nch + MERGE_BATCH - 1) // MERGE_BATCH
    A = (np.abs(K) @ np.abs(q)) / np.sqrt(hd)
    M = s.max()
    E = U * (hd * A + 2 * np.abs(s)) + 4.5 * U * (M - s) + 2 * U * (nb + 2) + 2.0 ** -22
    Ebar = w @ E
    coef = w * (E * (1 - 2 * w) + Ebar)
    absV = np.abs(V) + v_floor
    S = w @ absV
    gamma = (CHUNK + 10 * nb + 4) * U
    pad = np.full(nch * CHUNK, -np.inf)
    pad[:T] = s
    Mc = np.repeat(pad.reshape(nch, CHUNK).max(axis=1), CHUNK)[:T]
    Lg = np.exp(s - M).sum()
    a = np.minimum(w, 2.0 ** -25 * np.exp(Mc - M) / Lg)
    return 4.0 * (coef @ absV + 2 * gamma * S + a @ absV) + 2.0 ** -95 * absV.max()


def chunked(q: np.ndarray, K: np.ndarray, V: np.ndarray, mutant: str = None, arg: int = 0) -> np.ndarray:
    """The kernels' structure in float64: CHUNK-position partial records {O, m, l}, merged in
    batches of MERGE_BATCH with a running max. mutant (teeth of the tests): 'drop' / 'double'
    position arg, 'skip_chunk' arg, 'p_f16' (P rounded to f16, no low part), 'no_rescale' (the
    accumulators not rescaled when a batch raises the max)."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    T, hd = K.shape
    s = (K @ q) / np.sqrt(hd)
    recs = []
    for c0 in range(0, T, CHUNK):
        if mutant == "skip_chunk" and c0 // CHUNK == arg:
            continue
        idx = np.arange(c0, min(c0 + CHUNK, T))
        if mutant == "drop":
            idx = idx[idx != arg]
        if mutant == "double" and c0 <= arg < c0 + CHUNK:
            idx = np.append(idx, arg)
        if idx.size == 0:
            continue
        m = s[idx].max()
        p = np.exp(s[idx] - m)
        pv = p.astype(np.float16).astype(np.float64) if mutant == "p_f16" else p
        recs.append((pv @ V[idx], m, p.sum()))
    Mx, L, O = -np.inf, 0.0, np.zeros(hd)
    for b0 in range(0, len(recs), MERGE_BATCH):
        batch = recs[b0:b0 + MERGE_BATCH]
        mb = max(Mx, max(r[1] for r in batch))
        a = 0.0 if Mx == -np.inf else (1.0 if mutant == "no_rescale" else np.exp(Mx - mb))
        L, O = L * a, O * a
        for o, m, l in batch:
            wgt = np.exp(m - mb)
            L, O = L + wgt * l, O + wgt * o
        Mx = mb
    return O / L


# ---------------------------------------------------------------- cases of the attention tests
N_CTX = 32768
# first chunk edge; 8 -> 9 and 16 -> 17 records (merge batches); mid range; the last chunk
POSITIONS = (0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 4095, 4096, 32703, 32704, 32767)
PATTERNS = ("census", "flat", "flat_census", "peaked8", "peaked40", "dominant", "far_apart", "range", "vsubnormal", "poison")
F16_MAX = 65504.0


class Cases:
    """Inputs of the attention tests for layer 0 of one model: cached K/V states written with
    set_kv_rows (f16-exact by construction) and raw q|k|v rows.

    The cached keys of kv head j are K[t] = f16(c_t * b_j + 0.1 * noise_t), b_j along the sum of
    the head group's prepared q rows and scaled so that c_t * b_j scores about c_t: the pattern
    chooses c_t. The raw q row of a position is the inverse preparation (bias, norm weight,
    rotation at that position) of fixed target rows, so the prepared q is nearly the same at
    every position and one state serves them all. Aligned keys keep sum |q_i k_i| near |score|,
    which keeps the score term of the error bound tight."""

    def __init__(self, model: Model, seed: int = 1, n_ctx: int = N_CTX):
        self.m, self.n_ctx = model, n_ctx
        H, Hk, hd, G = model.n_head, model.n_kv, model.hd, model.G
        rng = np.random.default_rng(seed)
        z = rng.standard_normal((H, hd))
        z /= np.sqrt((z * z).mean(axis=1, keepdims=True))
        L = model.layers[0]
        self.qstar = z * (L["q_norm"] if model.qk_norm else 1.0)
        qs = self.qstar.reshape(Hk, G, hd)
        self.ssum = qs.sum(axis=1)
        self.b = self.ssum * (np.sqrt(hd) / (qs * qs).sum(axis=2).mean(axis=1))[:, None]
        self.noise = rng.standard_normal((Hk, n_ctx, hd), dtype=np.float32)
        self.vnoise = rng.standard_normal((Hk, n_ctx, hd), dtype=np.float32)
        self.seed = seed

    # ---- raw q|k|v rows
    def raw(self, pos: int, census: bool = False) -> np.ndarray:
        m = self.m
        H, Hk, hd = m.n_head, m.n_kv, m.hd
        L = m.layers[0]
        c, s = m.rope_row(pos)
        i0 = np.arange(hd // 2) if m.neox else 2 * np.arange(hd // 2)
        i1 = i0 + hd // 2 if m.neox else i0 + 1
        x = np.empty_like(self.qstar)
        y0, y1 = self.qstar[:, i0], self.qstar[:, i1]
        x[:, i0], x[:, i1] = y0 * c + y1 * s, -y0 * s + y1 * c
        if m.qk_norm:
            x = x / L["q_norm"]
        if L["bq"] is not None:
            x = x - L["bq"].reshape(H, hd)
        rng = np.random.default_rng(1000 * self.seed + pos)
        k = 0.3 * rng.standard_normal((Hk, hd))
        v = 0.3 * rng.standard_normal((Hk, hd))
        if census:  # the new row joins the census: key 0 (before any bias), value one-hot
            k[:] = 0.0
            v[:] = 0.0
            v[:, pos % hd] = 1.0
        raw = np.concatenate([x.reshape(-1), k.reshape(-1), v.reshape(-1)]).astype(np.float32)
        return m.nudge(0, raw, pos)

    # ---- cached states
    def keys(self, c: np.ndarray) -> np.ndarray:
        """c [n_ctx] (or [Hkv, n_ctx]) target scores -> K [Hkv, n_ctx, hd] f16."""
        c = np.broadcast_to(np.asarray(c, np.float32), (self.m.n_kv, self.n_ctx))
        return (c[:, :, None] * self.b[:, None, :].astype(np.float32) + np.float32(0.1) * self.noise).astype(np.float16)

    def state(self, pattern: str):
        """(K, V) [Hkv, n_ctx, hd] f16 of a pattern, before the per-position edits."""
        Hk, hd, n = self.m.n_kv, self.m.hd, self.n_ctx
        rng = np.random.default_rng(77 + self.seed)
        V = self.vnoise.astype(np.float16)
        if pattern == "census":
            K = np.zeros((Hk, n, hd), np.float16)
            V = np.zeros((Hk, n, hd), np.float16)
            V[:, np.arange(n), np.arange(n) % hd] = 1.0
            return K, V
        if pattern in ("flat", "dominant", "range", "poison"):
            return self.keys(np.zeros(n)), V
        if pattern == "flat_census":  # flat scores over the census values: out[d] = sum of p_t, t % hd == d
            return self.keys(np.zeros(n)), self.state("census")[1]
        if pattern == "vsubnormal":  # every V element below the smallest normal f16 (2^-14)
            return self.keys(np.zeros(n)), (self.vnoise * np.float32(2.0 ** -17)).astype(np.float16)
        if pattern in ("peaked8", "peaked40"):
            return self.keys(float(pattern[6:]) * rng.standard_normal((Hk, n))), V
        if pattern == "far_apart":
            # chunk maxima near -60 / +60 in alternate merge batches, rising by 0.5 per batch
            batch = np.arange(n) // (CHUNK * MERGE_BATCH)
            return self.keys(np.where(batch % 2 == 1, 60.0, -60.0) + 0.5 * batch), V
        raise ValueError(pattern)

    def edits(self, pattern: str, pos: int):
        """Sub-cases of a pattern at a position: [(label, [(t, K rows [Hkv, hd] f16, V rows)])],
        rows that replace cache rows t < pos of the state for that sub-case."""
        Hk, hd = self.m.n_kv, self.m.hd
        if pattern == "dominant":
            last = CHUNK * (pos // CHUNK)
            mid = CHUNK * ((pos // CHUNK) // 2 + 1) - 1
            out = []
            for t in sorted({t for t in (0, mid, last, pos - 1) if 0 <= t < pos}):
                k = (80.0 * self.b + 0.1 * self.noise[:, t]).astype(np.float16)
                v = np.broadcast_to(((-1.0) ** np.arange(hd) * (1 + np.arange(hd) / hd) * 3), (Hk, hd)).astype(np.float16)
                out.append((f"t*={t}", [(t, k, v)]))
            return out
        if pattern == "range":
            if pos < 8:
                return []
            big = (-60000.0 * np.sign(self.ssum)).astype(np.float16)
            vmax = np.broadcast_to((-1.0) ** np.arange(hd) * F16_MAX, (Hk, hd)).astype(np.float16)
            far = [(t, big, vmax if j % 2 == 0 else -vmax) for j, t in enumerate(sorted({1, pos // 2, pos - 1}))]
            win = pos // 3
            kwin = (80.0 * self.b + 0.1 * self.noise[:, win]).astype(np.float16)
            return [("underflow", far), ("winner", [e for e in far if e[0] != win] + [(win, kwin, vmax)])]
        return [("", [])]
