// Synthetic LLM GGUF writer (see synth.h). Tensor names / KV keys follow llama.cpp's
// GGUF conventions; quant types follow llama.cpp's Q4_K_M recipe: Q4_K everywhere,
// Q6_K for attn_v / ffn_down on "use_more_bits" layers and for the (tied) output. Q5_K_M is the
// same recipe with Q5_K for Q4_K; Q5_K_S has Q5_K everywhere and a Q6_K output. MOSTLY_Q6_K is
// Q6_K for every matrix, the embedding and the output included.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "gguf.h"
#include "quant.h"
#include "synth.h"

namespace mio {

static inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

float synth_normal_fast(uint64_t key, uint64_t i) {
    const uint64_t h = mix64(key ^ mix64(i));
    const float s = (float)(h & 0xFFFF) + (float)((h >> 16) & 0xFFFF) + (float)((h >> 32) & 0xFFFF) +
                    (float)(h >> 48);
    return (s * (1.0f / 65536.0f) - 2.0f) * 1.7320508f;  // var(sum of 4 U(0,1)) = 1/3
}

SynthLlmCfg synth_llm_preset(int p) {
    SynthLlmCfg c;
    switch (p) {
        case 0: break;
        case 1:
            c.name = "tiny-q4km", c.arch = "qwen3", c.n_layer = 3, c.n_ff = 768, c.qtype = 15;
            c.rope_base = 1000000.f;
            break;
        case 2:
            c.name = "MioTTS-0.1B-synthetic", c.n_embd = 576, c.n_layer = 24, c.n_head = 9,
            c.n_head_kv = 3, c.head_dim = 64, c.n_ff = 1536, c.n_vocab = 49152 + 12800;
            break;
        case 3:
            c.name = "MioTTS-1.7B-synthetic", c.arch = "qwen3", c.n_embd = 2048, c.n_layer = 28,
            c.n_head = 16, c.n_head_kv = 8, c.head_dim = 128, c.n_ff = 6144,
            c.n_vocab = 151936 + 12800, c.qtype = 15, c.rope_base = 1000000.f;
            break;
        case 5:
            c.name = "tiny-qwen2-bias", c.arch = "qwen2", c.qkv_bias = true, c.rope_base = 1000000.f;
            break;
        case 4:
            c.name = "MioTTS-2.6B-synthetic", c.n_embd = 2048, c.n_layer = 32, c.n_head = 32,
            c.n_head_kv = 8, c.head_dim = 64, c.n_ff = 10752, c.n_vocab = 65536 + 12800;
            break;
        case 6:  // LFM2-2.6B shape: 30 layers, attention on 8 of them (i % 4 == 2, and 29)
            c.name = "MioTTS-2.6B-lfm2-synthetic", c.arch = "lfm2", c.n_embd = 2048, c.n_layer = 30,
            c.n_head = 32, c.n_head_kv = 8, c.head_dim = 64, c.n_ff = 10752, c.n_vocab = 65536 + 12800;
            c.rope_base = 1000000.f, c.rms_eps = 1e-5f, c.attn_mod = 4, c.attn_at0 = 2, c.attn_at1 = -1;
            break;
        case 7:
            c.name = "tiny-lfm2", c.arch = "lfm2", c.n_layer = 5, c.attn_mod = 3, c.attn_at0 = 1;
            c.rope_base = 1000000.f, c.rms_eps = 1e-5f;
            break;
        case 8:
            c.name = "tiny-lfm2-q4km", c.arch = "lfm2", c.n_layer = 5, c.attn_mod = 3, c.attn_at0 = 1, c.qtype = 15;
            c.rope_base = 1000000.f, c.rms_eps = 1e-5f;
            break;
        case 9:
            c.name = "tiny-q4km-576", c.arch = "qwen3", c.n_embd = 576, c.n_layer = 3, c.n_head = 9,
            c.n_head_kv = 3, c.head_dim = 64, c.n_ff = 1536, c.qtype = 15, c.rope_base = 1000000.f;
            break;
        case 10:
            c.name = "tiny-q4_0", c.qtype = 2;
            break;
        case 11:
            c.name = "tiny-bf16", c.arch = "qwen3", c.n_layer = 3, c.n_ff = 768, c.qtype = 30;
            c.rope_base = 1000000.f;
            break;
        case 12:  // the 1.7B shape as the published BF16 file (README.md:196)
            c = synth_llm_preset(3);
            c.name = "MioTTS-1.7B-bf16-synthetic", c.qtype = 30;
            break;
        case 13:  // use_more_bits picks layer 2 of 3: both attn_v / ffn_down mixes occur
            c.name = "tiny-q5km", c.arch = "qwen3", c.n_layer = 3, c.n_ff = 768, c.qtype = 17;
            c.rope_base = 1000000.f;
            break;
        case 14:
            c.name = "tiny-q5ks", c.qtype = 16, c.tied = false;
            break;
        case 15:
            c = synth_llm_preset(8);
            c.name = "tiny-lfm2-q5km", c.qtype = 17;
            break;
        case 16:
            c = synth_llm_preset(3);
            c.name = "MioTTS-1.7B-q5km-synthetic", c.qtype = 17;
            break;
        // the big models' head shapes at tiny widths (attention parity tests at n_ctx 32768): the
        // attention launches take the (hd, G, W_o type) instantiations of presets 3 and 4
        case 17:
            c.name = "tiny-hd128-g2-q4km", c.arch = "qwen3", c.n_head = 4, c.n_head_kv = 2, c.head_dim = 128;
            c.qtype = 15, c.rope_base = 1000000.f, c.qk_norm_varied = true;
            break;
        case 18:
            c.name = "tiny-hd64-g4", c.n_head = 8, c.n_head_kv = 2, c.head_dim = 64;
            break;
        default: break;
    }
    return c;
}

bool synth_llm_qtype_known(int q) {
    return q == 8 || q == 15 || q == 16 || q == 17 || q == 18 || q == 2 || q == 30 || q == 11 || q == 12 || q == 13;
}

const char *synth_llm_check(const SynthLlmCfg &c) {
    // llama-quantize turns Q5_K rows that are not whole 256-element superblocks into Q5_1, which
    // the loader refuses: such a file would be of no use
    // (Q3_K rows likewise become IQ4_NL, refused too: the same message for Q3_K_S / _M / _L)
    const bool q3 = c.qtype == 11 || c.qtype == 12 || c.qtype == 13;
    if ((c.qtype == 16 || c.qtype == 17 || q3) && (c.n_embd % 256 || c.n_ff % 256 || (c.n_head * c.head_dim) % 256))
        return "Q5_K_S / Q5_K_M need n_embd, n_ff and n_head * head_dim to be multiples of 256";
    return nullptr;
}

// GPT-2 byte-level unicode for byte b (bytes_to_unicode), UTF-8 encoded
static std::string byte_token(int b) {
    int cp;
    if ((b >= 33 && b <= 126) || (b >= 161 && b <= 172) || (b >= 174 && b <= 255)) {
        cp = b;
    } else {
        int n = 0;
        for (int x = 0; x < b; ++x)
            if (!((x >= 33 && x <= 126) || (x >= 161 && x <= 172) || (x >= 174 && x <= 255))) ++n;
        cp = 256 + n;
    }
    std::string s;
    if (cp < 0x80) {
        s += (char)cp;
    } else {
        s += (char)(0xC0 | (cp >> 6));
        s += (char)(0x80 | (cp & 0x3F));
    }
    return s;
}

static bool use_more_bits(int i, int n) { return i < n / 8 || i >= 7 * n / 8 || (i - n / 8) % 3 == 2; }

bool synth_lfm2_is_attn(const SynthLlmCfg &c, int i) {
    const int r = i % c.attn_mod;
    return r == c.attn_at0 || r == c.attn_at1 || (c.n_layer == 30 && i == 29);
}

bool synth_write_llm(const std::string &path, const SynthLlmCfg &c) {
    if (synth_llm_check(c)) return false;
    GgufWriter w;
    const std::string a = c.arch;
    const bool lfm2 = a == "lfm2";
    w.kv_str("general.architecture", a);
    w.kv_str("general.name", c.name);
    // llama_ftype: 7 MOSTLY_Q8_0, 15 MOSTLY_Q4_K_M, 16 MOSTLY_Q5_K_S, 17 MOSTLY_Q5_K_M, 18 MOSTLY_Q6_K,
    // 2 MOSTLY_Q4_0, 32 MOSTLY_BF16, 11 MOSTLY_Q3_K_S, 12 MOSTLY_Q3_K_M, 13 MOSTLY_Q3_K_L
    const bool q3mix = c.qtype == 11 || c.qtype == 12 || c.qtype == 13;
    const bool kmix = c.qtype == 15 || c.qtype == 16 || c.qtype == 17 || c.qtype == 18 || q3mix;
    w.kv_u32("general.file_type", kmix ? c.qtype : (c.qtype == 2 ? 2 : (c.qtype == 30 ? 32 : 7)));
    w.kv_u32(a + ".context_length", c.n_ctx);
    w.kv_u32(a + ".embedding_length", c.n_embd);
    w.kv_u32(a + ".block_count", c.n_layer);
    w.kv_u32(a + ".feed_forward_length", c.n_ff);
    w.kv_u32(a + ".attention.head_count", c.n_head);
    if (lfm2) {
        // llama.cpp LFM2: head_count_kv per layer, 0 marks a short-conv (recurrent) layer
        std::vector<int32_t> kv;
        for (int i = 0; i < c.n_layer; ++i) kv.push_back(synth_lfm2_is_attn(c, i) ? c.n_head_kv : 0);
        w.kv_arr_i32(a + ".attention.head_count_kv", kv);
        w.kv_u32(a + ".shortconv.l_cache", 3);
    } else {
        w.kv_u32(a + ".attention.head_count_kv", c.n_head_kv);
    }
    w.kv_u32(a + ".attention.key_length", c.head_dim);
    w.kv_u32(a + ".attention.value_length", c.head_dim);
    w.kv_f32(a + ".rope.freq_base", c.rope_base);
    w.kv_f32(a + ".attention.layer_norm_rms_epsilon", c.rms_eps);
    // vocabulary
    std::vector<std::string> toks;
    std::vector<int32_t> types;
    for (int b = 0; b < 256; ++b) toks.push_back(byte_token(b)), types.push_back(1);
    for (const char *sp : {"<|startoftext|>", "<|im_start|>", "<|im_end|>", "<|endoftext|>"})
        toks.push_back(sp), types.push_back(3);
    for (int i = 0; i < kSynthNumSpeech; ++i) toks.push_back("<|s_" + std::to_string(i) + "|>"), types.push_back(4);
    for (int i = (int)toks.size(); i < c.n_vocab; ++i)
        toks.push_back("<|x_" + std::to_string(i) + "|>"), types.push_back(5);
    w.kv_str("tokenizer.ggml.model", "gpt2");
    w.kv_str("tokenizer.ggml.pre", "default");
    w.kv_arr_str("tokenizer.ggml.tokens", toks);
    w.kv_arr_i32("tokenizer.ggml.token_type", types);
    w.kv_arr_str("tokenizer.ggml.merges", {});
    w.kv_u32("tokenizer.ggml.bos_token_id", kSynthTokStartOfText);
    w.kv_u32("tokenizer.ggml.eos_token_id", kSynthTokEndOfText);
    w.kv_bool("tokenizer.ggml.add_bos_token", false);

    struct T {
        std::string name;
        uint32_t type;
        int64_t k, rows;
        int fill;  // 0 quantized N(0, w_std) rows, 1 ones, 2 f32 N(0, 0.5) (biases / conv taps),
                   // 3 f32 1 + N(0, 0.25) (q/k norm weights of qk_norm_varied)
    };
    std::vector<T> ts;
    auto pick = [&](uint32_t k_mix, uint32_t q4) -> uint32_t {
        return kmix ? k_mix : (c.qtype == 2 ? q4 : (c.qtype == 30 ? (uint32_t)GGML_BF16 : GGML_Q8_0));
    };
    // K-quant mixes: base everywhere, `more` for attn_v / ffn_down on use_more_bits layers (the
    // _S mix has none), Q6_K for the output matrix (the tied embedding is one). MOSTLY_Q6_K has
    // Q6_K as its base, so every matrix is one.
    // The Q3_K mixes (llama_tensor_get_type): Q3_K everywhere but attn_v (_S Q3_K; _M Q5_K on the
    // first two attention layers, Q4_K after; _L Q5_K), attn_output (Q3_K / Q4_K / Q5_K) and ffn_down
    // (_S Q3_K; _M Q5_K on layers i < n_layer / 16, Q4_K after; _L Q5_K); the untied embedding is
    // Q3_K, the output matrix Q6_K.
    const uint32_t kbase = q3mix ? GGML_Q3_K : (c.qtype == 15 ? GGML_Q4_K : (c.qtype == 18 ? GGML_Q6_K : GGML_Q5_K));
    const uint32_t base = pick(kbase, GGML_Q4_0), more = pick(c.qtype == 16 ? kbase : GGML_Q6_K, GGML_Q4_0);
    int i_attn = 0;  // attention layers so far (llama-quant's i_attention_wv)
    auto q3_v = [&](int ia) -> uint32_t {
        return c.qtype == 11 ? GGML_Q3_K : (c.qtype == 13 ? GGML_Q5_K : (ia < 2 ? GGML_Q5_K : GGML_Q4_K));
    };
    const uint32_t q3_o = c.qtype == 11 ? GGML_Q3_K : (c.qtype == 12 ? GGML_Q4_K : GGML_Q5_K);
    auto q3_down = [&](int i) -> uint32_t {
        return c.qtype == 11 ? GGML_Q3_K : (c.qtype == 13 ? GGML_Q5_K : (i < c.n_layer / 16 ? GGML_Q5_K : GGML_Q4_K));
    };
    const uint32_t outp = pick(GGML_Q6_K, GGML_Q4_0);
    const int q_dim = c.n_head * c.head_dim, kv_dim = c.n_head_kv * c.head_dim;
    const uint32_t emb = c.tied ? outp : pick(c.qtype == 15 ? GGML_Q6_K : kbase, GGML_Q4_0);  // (Q3_K mixes: Q3_K)
    ts.push_back({"token_embd.weight", emb, c.n_embd, c.n_vocab, false});
    for (int i = 0; i < c.n_layer; ++i) {
        const std::string p = "blk." + std::to_string(i) + ".";
        const bool mb = use_more_bits(i, c.n_layer);
        ts.push_back({p + "attn_norm.weight", GGML_F32, c.n_embd, 1, true});
        if (lfm2 && !synth_lfm2_is_attn(c, i)) {
            // gated short conv: in_proj -> B | C | X, depthwise taps [n_embd][3], out_proj
            ts.push_back({p + "shortconv.in_proj.weight", base, c.n_embd, 3 * c.n_embd, false});
            ts.push_back({p + "shortconv.conv.weight", GGML_F32, 3, c.n_embd, 2});
            ts.push_back({p + "shortconv.out_proj.weight", base, c.n_embd, c.n_embd, false});
        } else {
        ts.push_back({p + "attn_q.weight", base, c.n_embd, q_dim, false});
        ts.push_back({p + "attn_k.weight", base, c.n_embd, kv_dim, false});
        ts.push_back({p + "attn_v.weight", q3mix ? q3_v(i_attn++) : (mb ? more : base), c.n_embd, kv_dim, false});
        ts.push_back({p + "attn_output.weight", q3mix ? q3_o : base, q_dim, c.n_embd, false});
        if (c.qkv_bias) {
            ts.push_back({p + "attn_q.bias", GGML_F32, q_dim, 1, 2});
            ts.push_back({p + "attn_k.bias", GGML_F32, kv_dim, 1, 2});
            ts.push_back({p + "attn_v.bias", GGML_F32, kv_dim, 1, 2});
        }
        if (a == "qwen3" || lfm2) {
            ts.push_back({p + "attn_q_norm.weight", GGML_F32, c.head_dim, 1, c.qk_norm_varied ? 3 : 1});
            ts.push_back({p + "attn_k_norm.weight", GGML_F32, c.head_dim, 1, c.qk_norm_varied ? 3 : 1});
        }
        }
        ts.push_back({p + "ffn_norm.weight", GGML_F32, c.n_embd, 1, true});
        ts.push_back({p + "ffn_gate.weight", base, c.n_embd, c.n_ff, false});
        ts.push_back({p + "ffn_up.weight", base, c.n_embd, c.n_ff, false});
        ts.push_back({p + "ffn_down.weight", q3mix ? q3_down(i) : (mb ? more : base), c.n_ff, c.n_embd, false});
    }
    // lfm2's final norm is token_embd_norm (llama.cpp model.tok_norm)
    ts.push_back({lfm2 ? "token_embd_norm.weight" : "output_norm.weight", GGML_F32, c.n_embd, 1, true});
    if (!c.tied) ts.push_back({"output.weight", outp, c.n_embd, c.n_vocab, false});
    // llama-quantize: a K-quant needs rows of whole 256-element super-blocks
    if (c.kq_fallback)
        for (auto &t : ts)
            if (t.k % 256 != 0) {
                if (t.type == GGML_Q4_K) t.type = GGML_Q5_0;
                if (t.type == GGML_Q6_K) t.type = GGML_Q8_0;
            }
    for (auto &t : ts) {
        if (t.rows == 1)
            w.add_tensor(t.name, t.type, {t.k});
        else
            w.add_tensor(t.name, t.type, {t.k, t.rows});
    }
    return w.write(path, [&](size_t idx, uint8_t *dst, size_t nbytes) {
        const T &t = ts[idx];
        if (t.fill >= 1) {
            float *f = (float *)dst;
            const uint64_t key = synth_key(c.seed, t.name);
            for (int64_t i = 0; i < t.k * t.rows; ++i)
                f[i] = t.fill == 1 ? 1.0f
                                   : (t.fill == 2 ? 0.5f : 0.25f) * synth_normal_fast(key, (uint64_t)i) +
                                         (t.fill == 3 ? 1.0f : 0.0f);
            return;
        }
        const size_t rb = ggml_row_bytes(t.type, t.k);
        const uint64_t key = synth_key(c.seed, t.name);
#pragma omp parallel
        {
            std::vector<float> row(t.k);
#pragma omp for schedule(static)
            for (int64_t r = 0; r < t.rows; ++r) {
                for (int64_t j = 0; j < t.k; ++j) row[j] = c.w_std * synth_normal_fast(key, (uint64_t)r * t.k + j);
                quantize_row(t.type, row.data(), dst + (size_t)r * rb, t.k);
            }
        }
        (void)nbytes;
    });
}

}  // namespace mio
