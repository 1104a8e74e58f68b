"""Records the decode step's attention and row-dot outputs as bit patterns:
    python tools/record_decode_bits.py [FILE]     (on the GPU, at the commit to pin)
writes tests/golden/decode_bits_parent.npz (or FILE), which tests/test_decode_bits_gpu.py compares with bit
for bit. The fixture in the tree was written at 15e1913, before the merge, head-preparation and
row-dot instruction streams were shortened: those changes may not move a bit.

Inputs come from fixed numpy seeds and the deterministic synthetic presets; only outputs are
stored. The case generators below are the test's too, so both sides see the same inputs.

Attention (head preparation, chunk, merge): mio_hip_llm_debug_attention on K/V written with
mio_hip_llm_set_kv_rows, layer 0 of the presets with head shapes (128, 2), (64, 3), (64, 4), every
launch the entry accepts (1: attention, 10: attention + O; the two are recorded as one array,
they must agree), at positions on both sides of every 8-chunk merge batch edge, for two states:
  ordinary   target scores 2 N(0, 1)
  far        chunk c's scores near 25 (c // 8) + (-115, -100, -90, -88, -40, -1, 0, -104)[c % 8]:
             inside a batch the merge weights exp(m_j - mb) underflow to 0 (-115, -104), land in
             the f32 denormals (-100 .. -88) and the running maximum moves in every batch.
Stored per case: the attention output [n_head, hd] and the K / V cache rows the launch appended.

Row dots: mio_hip_debug_matvec and mio_hip_debug_matvec_swiglu for types 12, 13, 14, 8, 30,
K in {256, 2048, 2560, 6144} (one pass, a partly filled second pass, three passes), rows in
{1, 5, 64, 67}."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "miotts-llama.cpp_amd", "python"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import miotts_amd as m  # noqa: E402
import np_attn as A  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "decode_bits_parent.npz")
N_CTX = 2048
PRESETS = (17, 9, 18)  # (hd 128, G 2), (64, 3), (64, 4)
LAUNCHES = (1, 10)
POSITIONS = (0, 63, 64, 447, 511, 512, 575, 767, 1023, 1024, 1087, N_CTX - 1)
PATTERNS = ("ordinary", "far")
FAR = np.array([-115.0, -100.0, -90.0, -88.0, -40.0, -1.0, 0.0, -104.0])
QTYPES = (12, 13, 14, 8, 30)
KS = (256, 2048, 2560, 6144)
ROWS = (1, 5, 64, 67)


def attention_state(C, pattern):
    """(K, V) [n_kv, N_CTX, hd] f16 of a pattern for the np_attn.Cases C."""
    if pattern == "ordinary":
        c = 2.0 * np.random.default_rng(4242).standard_normal(C.n_ctx)
    else:
        chunk = np.arange(C.n_ctx) // A.CHUNK
        c = 25.0 * (chunk // A.MERGE_BATCH) + FAR[chunk % A.MERGE_BATCH]
    return C.keys(c), C.vnoise.astype(np.float16)


def attention_outputs(g, C, pattern):
    """{key: array} of one (model, pattern): per position the output of every launch (one array,
    asserted equal between launches) and the appended K / V rows (uint16 bit patterns)."""
    K16, V16 = attention_state(C, pattern)
    g.set_kv_rows(0, 0, K16, V16)
    out = {}
    for pos in POSITIONS:
        raw = C.raw(pos)
        end = min(A.CHUNK * (pos // A.CHUNK + 1), N_CTX)
        atts = []
        for which in LAUNCHES:
            atts.append(g.debug_attention(0, pos, which, raw))
            kg, vg = g.kv_rows(0, pos + 1)
            rows = np.stack([kg[:, pos], vg[:, pos]]).view(np.uint16)
            if which != LAUNCHES[0]:
                assert np.array_equal(rows, out[f"kv_{pos}"]), (pos, which)
            out[f"kv_{pos}"] = rows
            g.set_kv_rows(0, pos, K16[:, pos:end], V16[:, pos:end])
        for which, att in zip(LAUNCHES[1:], atts[1:]):
            assert att.tobytes() == atts[0].tobytes(), (pos, which)
        out[f"att_{pos}"] = atts[0].view(np.uint32)
    return out


def matvec_outputs(dev, qtype):
    """{key: array} of one weight type: the plain and the SwiGLU row streams' outputs."""
    out = {}
    for k in KS:
        rng = np.random.default_rng(qtype * 100000 + k)
        wg = m.quantize_rows(qtype, (rng.standard_normal((max(ROWS), k)) * 0.05).astype(np.float32))
        wu = m.quantize_rows(qtype, (rng.standard_normal((max(ROWS), k)) * 0.05).astype(np.float32))
        x = rng.standard_normal(k).astype(np.float32)
        x[3] = -9.0
        for rows in ROWS:
            out[f"mv_{k}_{rows}"] = m.debug_matvec(dev, qtype, wg[:rows], k, x).view(np.uint32)
            out[f"sw_{k}_{rows}"] = m.debug_matvec_swiglu(dev, qtype, wg[:rows], wu[:rows], k, x).view(np.uint32)
    return out


def main():
    import tempfile

    dev = m.Device(0)
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        for preset in PRESETS:
            path = m.synth_llm(os.path.join(d, f"llm{preset}.gguf"), preset, 1)
            g, C = m.Llm(dev, path, N_CTX), A.Cases(A.Model(path), n_ctx=N_CTX)
            for pattern in PATTERNS:
                for key, v in attention_outputs(g, C, pattern).items():
                    rec[f"p{preset}_{pattern}_{key}"] = v
            g.close()
    for qtype in QTYPES:
        for key, v in matvec_outputs(dev, qtype).items():
            rec[f"t{qtype}_{key}"] = v
    dev.close()
    dst = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    np.savez_compressed(dst, **rec)
    print(f"{dst}: {len(rec)} arrays, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
