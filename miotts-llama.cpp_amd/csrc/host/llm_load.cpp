// LLM load (see llm.h): GGUF -> split-layout weights in one HBM arena, F16 KV cache, the
// per-step buffers, RoPE table. Replaces llama_model_load_from_file (test-to-speech.cpp:47-49)
// and llama_init_from_model (:103-108) for the MioTTS path.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "gguf.h"
#include "llm_model.h"
#include "quant.h"

bool Stager::init() {
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess;
}
uint8_t *Stager::acquire(size_t bytes) {
    const int i = cur;
    if (used[i] && hipEventSynchronize(ev[i]) != hipSuccess) return nullptr;
    if (cap[i] < bytes) {
        if (buf[i]) hipHostFree(buf[i]);
        buf[i] = nullptr, cap[i] = 0;
        const size_t want = std::max(bytes, (size_t)64 << 20);
        if (hipHostMalloc(&buf[i], want, hipHostMallocDefault) != hipSuccess) return nullptr;
        cap[i] = want;
    }
    return (uint8_t *)buf[i];
}
bool Stager::submit(void *dst, size_t bytes) {
    const int i = cur;
    cur ^= 1;
    used[i] = true;
    return hipMemcpyAsync(dst, buf[i], bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
           hipEventRecord(ev[i], s) == hipSuccess;
}
bool Stager::finish() { return !s || hipStreamSynchronize(s) == hipSuccess; }
Stager::~Stager() {
    finish();
    for (int i = 0; i < 2; ++i) {
        if (buf[i]) hipHostFree(buf[i]);
        if (ev[i]) hipEventDestroy(ev[i]);
    }
    if (s) hipStreamDestroy(s);
}

namespace {

// What the load steps below share besides the model.
struct Load {
    const mio::GgufFile &g;
    std::string arch;
    // lfm2 (LiquidAI LFM2, the <|startoftext|><|im_start|> template family): attention layers
    // (NEOX RoPE, q/k RMSNorm) interleaved with gated short-conv layers (llama.cpp build_lfm2)
    bool lfm2;
    int n_ctx;
    std::vector<int64_t> kv_arr;  // per-layer head_count_kv (lfm2: 0 marks a short-conv layer), or empty
    float rope_base = 10000.0f;
};

template <class T>
T *dalloc(mio_hip_llm *m, size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, n * sizeof(T) + 16) != hipSuccess) return nullptr;
    m->allocs.push_back(p);
    // zero-filled on the null stream and waited for here: the weight upload that follows
    // runs on the stager's non-blocking stream, which does not order itself after it
    if (hipMemset(p, 0, n * sizeof(T) + 16) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
        return nullptr;
    return (T *)p;
}

bool upload_qmat(mio_hip_llm *m, const mio::GgufTensor *t, mio::QMat &q) {
    if (!t || t->n_dims != 2) {
        mio::set_error("llm: matrix tensor %s missing or not 2-D", t ? t->name.c_str() : "?");
        return false;
    }
    const bool repack = mio::repacks_to_q8_0(t->type);
    if (!mio::is_weight_type((int)t->type) && !repack) {
        std::string names;  // every weight type of the table, by its ggml name
        for (int wt : mio::kWeightTypes) names += std::string(mio::ggml_type_name(wt)) + ", ";
        mio::set_error("llm: tensor %s has type %s; supported: %sq5_0 / q4_0 (run as q8_0)", t->name.c_str(),
                       mio::ggml_type_name(t->type), names.c_str());
        return false;
    }
    if (t->type == mio::GGML_BF16 && t->ne[0] % 32) {
        mio::set_error("llm: bf16 tensor %s: row length %lld is not a multiple of 32", t->name.c_str(),
                       (long long)t->ne[0]);
        return false;
    }
    // Q5_0 (llama-quantize's Q4_K fallback for rows not a multiple of 256) and Q4_0 rows run as
    // the Q8_0 rows they equal exactly (quant.h repack_to_q8_0)
    const uint32_t type = repack ? (uint32_t)mio::GGML_Q8_0 : t->type;
    std::vector<uint8_t> q80;
    const void *src = t->data;
    if (repack) {
        q80.resize((size_t)t->ne[1] * (size_t)(t->ne[0] / 32) * sizeof(mio::BlockQ8_0));
        if (!mio::repack_to_q8_0(t->type, t->data, t->ne[1], t->ne[0], q80.data())) {
            mio::set_error("llm: repacking %s (%s) as q8_0 failed", t->name.c_str(), mio::ggml_type_name(t->type));
            return false;
        }
        src = q80.data();
    }
    const mio::SplitLayout L = mio::split_layout(type, t->ne[1], t->ne[0]);
    const auto it = m->arena_off.find(t->name);
    uint8_t *dp = (m->arena && it != m->arena_off.end()) ? m->arena + it->second : dalloc<uint8_t>(m, L.bytes);
    uint8_t *host = dp && m->stager ? m->stager->acquire(L.bytes) : nullptr;
    if (!host) {
        mio::set_error("llm: staging / device buffer for %s failed", t->name.c_str());
        return false;
    }
    if (!mio::to_split(type, src, t->ne[1], t->ne[0], host)) {
        mio::set_error("llm: re-layout of %s failed", t->name.c_str());
        return false;
    }
    if (!m->stager->submit(dp, L.bytes)) {
        mio::set_error("llm: upload of %s failed", t->name.c_str());
        return false;
    }
    q.type = (int)type;
    if (type == mio::GGML_BF16)
        m->bf16 = true;
    else
        m->int8 = true;
    q.rows = (int)t->ne[1];
    q.k = (int)t->ne[0];
    q.p0 = dp + L.off[0];
    q.p1 = dp + L.off[1];
    q.p2 = dp + L.off[2];
    q.p3 = dp + L.off[3];
    // the bytes the split layout streams (Q3_K: 114 B per superblock, not the GGUF's 110). Q4_0 /
    // Q5_0 files keep counting their GGUF bytes although they stream as Q8_0
    m->weight_bytes += repack ? t->nbytes : (uint64_t)t->ne[1] * mio::row_bytes((int)type, t->ne[0]);
    return true;
}

float *upload_f32(mio_hip_llm *m, const mio::GgufFile &g, const std::string &name, int64_t n) {
    const mio::GgufTensor *t = g.tensor(name);
    if (!t || t->type != mio::GGML_F32 || t->nelements() != n) {
        mio::set_error("llm: norm tensor %s missing or not f32[%lld]", name.c_str(), (long long)n);
        return nullptr;
    }
    const auto it = m->arena_off.find(t->name);
    float *p = (m->arena && it != m->arena_off.end()) ? (float *)(m->arena + it->second) : dalloc<float>(m, n);
    if (p) hipMemcpy(p, t->data, n * 4, hipMemcpyHostToDevice);
    m->weight_bytes += n * 4;
    return p;
}

// The architecture's hyper-parameters -> m->dims, and what this runner has kernels for.
int read_dims(Load &ld, mio_hip_llm *m) {
    const mio::GgufFile &g = ld.g;
    const std::string &arch = ld.arch;
    mio::LlmDims &D = m->dims;
    D.n_embd = (int)g.get_int(arch + ".embedding_length", 0);
    m->n_layer = (int)g.get_int(arch + ".block_count", 0);
    D.n_ff = (int)g.get_int(arch + ".feed_forward_length", 0);
    D.n_head = (int)g.get_int(arch + ".attention.head_count", 0);
    // head_count_kv: a scalar, or per layer (lfm2: 0 marks a short-conv layer)
    if (const mio::GgufValue *hv = g.get(arch + ".attention.head_count_kv"); hv && !hv->arr_i.empty()) {
        ld.kv_arr = hv->arr_i;
        D.n_kv = 0;
        for (int64_t v : ld.kv_arr) D.n_kv = std::max(D.n_kv, (int)v);
    } else {
        D.n_kv = (int)g.get_int(arch + ".attention.head_count_kv", D.n_head);
    }
    D.hd = (int)g.get_int(arch + ".attention.key_length", D.n_head ? D.n_embd / D.n_head : 0);
    D.eps = (float)g.get_float(arch + ".attention.layer_norm_rms_epsilon", 1e-6);
    ld.rope_base = (float)g.get_float(arch + ".rope.freq_base", 10000.0);
    D.neox = (arch == "qwen3" || arch == "qwen2" || ld.lfm2) ? 1 : 0;
    D.qk_norm = (arch == "qwen3" || ld.lfm2) ? 1 : 0;
    MIO_REQUIRE(!ld.lfm2 || g.get_int(arch + ".shortconv.l_cache", mio::kConvL) == mio::kConvL, MIO_ERR_UNSUPPORTED,
                "llm_load: lfm2 shortconv.l_cache %lld not supported (%d)",
                (long long)g.get_int(arch + ".shortconv.l_cache", 0), mio::kConvL);
    D.n_ctx = ld.n_ctx;
    D.scale = 1.0f / sqrtf((float)D.hd);
    D.split = mio::kAttChunk;
    D.max_splits = (ld.n_ctx + D.split - 1) / D.split;
    // matvec workgroups: one per CU (MIO_WGM=2..4 launches that many per CU, for A/B)
    D.n_wg = (m->d->n_cu > 0 ? m->d->n_cu : 256) * env_int("MIO_WGM", 1, 1, 4);
    D.n_layer = m->n_layer;
    MIO_REQUIRE(ld.n_ctx <= 32768, MIO_ERR_UNSUPPORTED, "llm_load: n_ctx %d > 32768", ld.n_ctx);
    const int G = D.n_kv ? D.n_head / D.n_kv : 0;
    MIO_REQUIRE(D.n_embd > 0 && m->n_layer > 0 && D.n_head > 0 && D.n_kv > 0 && D.n_head % D.n_kv == 0 &&
                    (G == 1 || G == 2 || G == 3 || G == 4 || G == 8) && (D.hd == 64 || D.hd == 128) &&
                    (D.n_embd % 256 == 0 || D.n_embd % 32 == 0),
                MIO_ERR_UNSUPPORTED, "llm_load: unsupported dims (n_embd %d, heads %d/%d, head_dim %d)", D.n_embd,
                D.n_head, D.n_kv, D.hd);
    return MIO_OK;
}

// One arena for every weight: layer matrices in step order, then the lm_head, then the
// embedding table, then every f32 norm vector (kept out of many small allocations: one large
// mapping serves all of them).
int plan_arena(const Load &ld, mio_hip_llm *m) {
    std::vector<std::string> order;
    static const char *mats[] = {"attn_q",   "attn_k",  "attn_v",   "shortconv.in_proj", "attn_output",
                                 "shortconv.out_proj", "ffn_gate", "ffn_up", "ffn_down"};
    for (int i = 0; i < m->n_layer; ++i)
        for (const char *n : mats) order.push_back("blk." + std::to_string(i) + "." + n + ".weight");
    order.push_back("output.weight");
    order.push_back("token_embd.weight");
    static const char *norms[] = {"attn_norm", "ffn_norm", "attn_q_norm", "attn_k_norm", "shortconv.conv"};
    for (int i = 0; i < m->n_layer; ++i)
        for (const char *n : norms) order.push_back("blk." + std::to_string(i) + "." + n + ".weight");
    order.push_back("output_norm.weight");
    order.push_back("token_embd_norm.weight");
    size_t total = 0;
    for (const std::string &n : order) {
        const mio::GgufTensor *t = ld.g.tensor(n);
        if (!t) continue;
        size_t bytes = 0;
        if (t->n_dims == 2 && t->type != mio::GGML_F32) {
            const uint32_t ty = mio::repacks_to_q8_0(t->type) ? (uint32_t)mio::GGML_Q8_0 : t->type;
            bytes = mio::split_layout(ty, t->ne[1], t->ne[0]).bytes;
        } else if (t->type == mio::GGML_F32) {
            bytes = (size_t)t->nelements() * 4;
        }
        if (!bytes) continue;
        m->arena_off[n] = total;
        total += (bytes + 255) & ~(size_t)255;
    }
    m->arena = dalloc<uint8_t>(m, total);
    MIO_REQUIRE(m->arena, MIO_ERR_OOM, "llm_load: weight arena of %zu bytes: allocation failed", total);
    return MIO_OK;
}

// Embedding table, lm_head (or the tied table), final norm.
int upload_globals(const Load &ld, mio_hip_llm *m) {
    mio::LlmDims &D = m->dims;
    const mio::GgufTensor *te = ld.g.tensor("token_embd.weight");
    MIO_REQUIRE(te && te->ne[0] == D.n_embd, MIO_ERR_FORMAT, "llm_load: token_embd.weight missing");
    D.n_vocab = (int)te->ne[1];
    MIO_REQUIRE(D.n_vocab <= 128 * 8 * D.n_wg, MIO_ERR_UNSUPPORTED, "llm_load: vocab %d > %d", D.n_vocab,
                128 * 8 * D.n_wg);
    // the output matrix (or the tied table) as Q3_K does not occur in llama-quantize's files (they
    // carry Q6_K there): no lm_head kernel is instantiated for it
    const mio::GgufTensor *tl = ld.g.tensor("output.weight") ? ld.g.tensor("output.weight") : te;
    MIO_REQUIRE(tl->type != mio::GGML_Q3_K, MIO_ERR_UNSUPPORTED,
                "llm: tensor %s has type %s as the output matrix; supported there: bf16, q8_0, q4_K, q5_K, q6_K",
                tl->name.c_str(), mio::ggml_type_name(tl->type));
    // a Q3_K table's row lookup is built into the launches of a Q3_K model only (layer 0's first
    // matrix Q3_K: llm_device.h dequant_elem), which is where llama-quantize's files have one
    if (te->type == mio::GGML_Q3_K) {
        const mio::GgufTensor *t0 = ld.g.tensor("blk.0.attn_q.weight");
        if (!t0) t0 = ld.g.tensor("blk.0.shortconv.in_proj.weight");
        MIO_REQUIRE(t0 && t0->type == mio::GGML_Q3_K, MIO_ERR_UNSUPPORTED,
                    "llm: tensor %s has type %s beside a layer 0 that is not q3_K: not supported", te->name.c_str(),
                    mio::ggml_type_name(te->type));
    }
    const uint64_t before = m->weight_bytes;
    if (!upload_qmat(m, te, m->tok)) return MIO_ERR_FORMAT;
    const uint64_t embd_bytes = m->weight_bytes - before;
    m->weight_bytes -= embd_bytes;  // one embedding row per step, not the whole table
    if (const mio::GgufTensor *to = ld.g.tensor("output.weight")) {
        if (!upload_qmat(m, to, m->lm)) return MIO_ERR_FORMAT;
    } else {
        m->lm = m->tok;  // tied embeddings: the table is streamed as the lm_head every step
        m->weight_bytes += embd_bytes;
    }
    // lfm2's final norm is token_embd_norm (llama.cpp model.tok_norm)
    m->out_norm = upload_f32(m, ld.g, ld.lfm2 ? "token_embd_norm.weight" : "output_norm.weight", D.n_embd);
    return m->out_norm ? MIO_OK : MIO_ERR_FORMAT;
}

// Layer i's norms and matrices -> m->layers[i], and the shape / quant-family checks.
int upload_layer(const Load &ld, mio_hip_llm *m, int i) {
    const mio::GgufFile &g = ld.g;
    const mio::LlmDims &D = m->dims;
    const std::string p = "blk." + std::to_string(i) + ".";
    auto fam = [](int t) { return t == mio::GGML_Q8_0 ? 0 : (t == mio::GGML_BF16 ? 2 : 1); };
    mio::LayerW L{};
    if (!(L.attn_norm = upload_f32(m, g, p + "attn_norm.weight", D.n_embd)) ||
        !(L.ffn_norm = upload_f32(m, g, p + "ffn_norm.weight", D.n_embd)))
        return MIO_ERR_FORMAT;
    L.conv = g.tensor(p + "shortconv.in_proj.weight") ? 1 : 0;
    MIO_REQUIRE(!(ld.lfm2 && (size_t)i < ld.kv_arr.size() && (ld.kv_arr[i] == 0) != (L.conv != 0)), MIO_ERR_FORMAT,
                "llm_load: layer %d: head_count_kv %lld disagrees with its tensors", i, (long long)ld.kv_arr[i]);
    if (L.conv) {
        // gated short conv: in_proj [3 n_embd][n_embd], taps [n_embd][3] f32, out_proj
        MIO_REQUIRE(ld.lfm2, MIO_ERR_UNSUPPORTED, "llm_load: layer %d: short-conv tensors in a '%s' model", i,
                    ld.arch.c_str());
        const mio::GgufTensor *tc = g.tensor(p + "shortconv.conv.weight");
        MIO_REQUIRE(tc && tc->type == mio::GGML_F32 && tc->ne[0] == mio::kConvL && tc->ne[1] == D.n_embd,
                    MIO_ERR_FORMAT, "llm_load: layer %d: shortconv.conv.weight must be f32 [%d][%d]", i, D.n_embd,
                    mio::kConvL);
        if (!(L.conv_w = upload_f32(m, g, p + "shortconv.conv.weight", (int64_t)D.n_embd * mio::kConvL)) ||
            !upload_qmat(m, g.tensor(p + "shortconv.in_proj.weight"), L.in_proj) ||
            !upload_qmat(m, g.tensor(p + "shortconv.out_proj.weight"), L.out_proj) ||
            !upload_qmat(m, g.tensor(p + "ffn_gate.weight"), L.gate) ||
            !upload_qmat(m, g.tensor(p + "ffn_up.weight"), L.up) ||
            !upload_qmat(m, g.tensor(p + "ffn_down.weight"), L.down))
            return MIO_ERR_FORMAT;
        MIO_REQUIRE(L.in_proj.rows == 3 * D.n_embd && L.in_proj.k == D.n_embd && L.out_proj.rows == D.n_embd &&
                        L.out_proj.k == D.n_embd && L.gate.rows == D.n_ff && L.down.k == D.n_ff &&
                        L.gate.type == L.up.type && D.n_ff <= 12288 && D.n_embd <= 64 * 8 * D.n_wg,
                    MIO_ERR_UNSUPPORTED, "llm_load: layer %d (short conv) shapes / quant families not supported", i);
        m->has_conv = true;
        m->layers.push_back(L);
        m->gate_repacked.push_back(mio::repacks_to_q8_0(g.tensor(p + "ffn_gate.weight")->type));
        return MIO_OK;
    }
    if (D.qk_norm) {
        if (!(L.q_norm = upload_f32(m, g, p + "attn_q_norm.weight", D.hd)) ||
            !(L.k_norm = upload_f32(m, g, p + "attn_k_norm.weight", D.hd)))
            return MIO_ERR_FORMAT;
    }
    if (!upload_qmat(m, g.tensor(p + "attn_q.weight"), L.wq) || !upload_qmat(m, g.tensor(p + "attn_k.weight"), L.wk) ||
        !upload_qmat(m, g.tensor(p + "attn_v.weight"), L.wv) ||
        !upload_qmat(m, g.tensor(p + "attn_output.weight"), L.wo) ||
        !upload_qmat(m, g.tensor(p + "ffn_gate.weight"), L.gate) ||
        !upload_qmat(m, g.tensor(p + "ffn_up.weight"), L.up) || !upload_qmat(m, g.tensor(p + "ffn_down.weight"), L.down))
        return MIO_ERR_FORMAT;
    // qwen2 q/k/v projection biases, one f32 vector in qkv order (added before RoPE by the
    // attention kernels' head preparation)
    const mio::GgufTensor *bt[3] = {g.tensor(p + "attn_q.bias"), g.tensor(p + "attn_k.bias"),
                                    g.tensor(p + "attn_v.bias")};
    const int64_t bn[3] = {(int64_t)D.n_head * D.hd, (int64_t)D.n_kv * D.hd, (int64_t)D.n_kv * D.hd};
    if (bt[0] || bt[1] || bt[2]) {
        std::vector<float> hb;
        for (int j = 0; j < 3; ++j) {
            MIO_REQUIRE(bt[j] && bt[j]->type == mio::GGML_F32 && bt[j]->nelements() == bn[j], MIO_ERR_FORMAT,
                        "llm_load: layer %d: attn_q/k/v.bias must all be f32 of the projection sizes", i);
            const float *f = (const float *)bt[j]->data;
            hb.insert(hb.end(), f, f + bn[j]);
        }
        float *db = dalloc<float>(m, hb.size());
        MIO_REQUIRE(db && hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice) == hipSuccess, MIO_ERR_OOM,
                    "llm_load: bias upload failed");
        L.bqkv = db;
        m->weight_bytes += hb.size() * 4;
    }
    MIO_REQUIRE(L.wq.rows == D.n_head * D.hd && L.wk.rows == D.n_kv * D.hd && L.wv.rows == D.n_kv * D.hd &&
                    L.gate.rows == D.n_ff && L.down.k == D.n_ff && fam(L.wq.type) == fam(L.wk.type) &&
                    fam(L.wq.type) == fam(L.wv.type) && L.wq.type == L.wk.type && L.gate.type == L.up.type &&
                    D.n_ff <= 12288 && D.n_embd <= 64 * 8 * D.n_wg,
                MIO_ERR_UNSUPPORTED, "llm_load: layer %d shapes / quant families not supported", i);
    MIO_REQUIRE(mio::attn_v_supported(L.wq.type, L.wv.type), MIO_ERR_UNSUPPORTED,
                "llm_load: layer %d: attn_v %s beside attn_q %s has no kernel", i, mio::ggml_type_name(L.wv.type),
                mio::ggml_type_name(L.wq.type));
    m->layers.push_back(L);
    m->gate_repacked.push_back(mio::repacks_to_q8_0(g.tensor(p + "ffn_gate.weight")->type));
    return MIO_OK;
}

// KV cache, pinned host mirrors, and every per-step buffer (activations, partials, state,
// token rings, RoPE table, prefill staging) carved from ONE allocation: one large mapping
// instead of many small ones (the activation vectors are read by every CU at the start of
// every launch). *rope receives the device RoPE table.
int carve_buffers(const Load &ld, mio_hip_llm *m, float2 **rope) {
    const mio::LlmDims &D = m->dims;
    const int n_ctx = ld.n_ctx;
    const int qkv = (D.n_head + 2 * D.n_kv) * D.hd;
    // q|k|v rows, or an lfm2 short-conv layer's B | C | X rows
    const int qkv_rows = std::max(qkv, m->has_conv ? 3 * D.n_embd : 0);
    const size_t kv = (size_t)m->n_layer * D.n_kv * n_ctx * D.hd;
    m->kc = dalloc<_Float16>(m, kv);
    m->vc = dalloc<_Float16>(m, kv);
    std::vector<std::pair<void **, size_t>> carve;
    auto want = [&](auto *&ptr, size_t count) {
        carve.push_back({reinterpret_cast<void **>(&ptr), count * sizeof(*ptr)});
    };
    float2 *dr = nullptr;
    want(m->buf.x, D.n_embd);
    want(m->buf.qkv, qkv_rows);
    if (m->has_conv) want(m->buf.ring, (size_t)m->n_layer * mio::kConvSlots * D.n_embd);
    want(m->buf.h, D.n_ff);
    want(m->buf.logits, D.n_vocab);
    want(m->buf.part, (size_t)D.n_head * D.max_splits * (D.hd + 4));
    want(m->buf.att, (size_t)D.n_head * D.hd);
    want(m->buf.att_cnt, (size_t)mio::kAttCntInts);  // + k_att_o's merge counters and timeout flag
    want(m->buf.smp, 2 * std::max(mio::lm_head_blocks(D), 4 * D.n_wg) + 16);
    want(m->buf.st, 1);
    want(m->d_cfg, 1);
    m->max_steps = n_ctx;
    for (mio_hip_llm::Snap &sn : m->snaps)
        MIO_REQUIRE(hipHostMalloc((void **)sn.st.put(), sizeof(mio::StepState), hipHostMallocDefault) == hipSuccess &&
                        hipHostMalloc((void **)sn.tok.put(), (size_t)m->max_steps * 4, hipHostMallocDefault) ==
                            hipSuccess &&
                        hipEventCreate(sn.ev.put()) == hipSuccess,
                    MIO_ERR_OOM, "llm_load: pinned host buffers / events failed");
    MIO_REQUIRE(hipHostMalloc((void **)m->host_done.put(), sizeof(int),
                              hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                    hipHostGetDevicePointer((void **)&m->host_done_dev, m->host_done, 0) == hipSuccess,
                MIO_ERR_OOM, "llm_load: mapped host end-token word failed");
    std::memset(m->host_done, 0, sizeof(int));
    want(m->d_tokens, m->max_steps);
    want(m->d_force, m->max_steps);
    want(m->d_prompt, n_ctx);
    want(m->pf.x, (size_t)mio::kPrefillB * D.n_embd);
    want(m->pf.qkv, (size_t)mio::kPrefillB * qkv_rows);
    want(m->pf.h, (size_t)mio::kPrefillB * D.n_ff);
    want(m->pf.part, (size_t)mio::kPrefillB * D.n_head * D.max_splits * (D.hd + 4));
    want(m->pf.att, (size_t)mio::kPrefillB * D.n_head * D.hd);
    want(m->pf.att_cnt, (size_t)mio::kPrefillB * D.n_kv);
    want(m->pf.qcnt, (size_t)mio::kQcntInts);  // batched decode in-launch quantization counters
    want(m->pf.act, mio::prefill_act_bytes(
                        mio::prefill_rec_k(std::max(std::max(D.n_embd, D.n_ff), D.n_head * D.hd), m->bf16 ? 30 : 8)));
    want(dr, (size_t)n_ctx * (D.hd / 2));
    want(m->d_iota, (size_t)n_ctx + mio::kPrefillB);
    size_t io_bytes = 0;
    for (auto &c : carve) io_bytes += (c.second + 255) & ~(size_t)255;
    uint8_t *io = dalloc<uint8_t>(m, (io_bytes + (2u << 20) - 1) & ~(size_t)((2u << 20) - 1));
    // a failed allocation leaves every carved pointer null
    MIO_REQUIRE(m->kc && m->vc && io, MIO_ERR_OOM, "llm_load: device allocation failed");
    size_t off = 0;
    for (auto &c : carve) {
        *c.first = io + off;
        off += (c.second + 255) & ~(size_t)255;
    }
    m->buf.cfg = m->d_cfg;
    m->pf.tokens = m->d_prompt;
    m->pf.ring = m->buf.ring;  // the single-stream prefill is sequence 0 of the decode rings
    m->pf.seq_ring = 0;
    m->buf.rope = dr;
    m->pf.rope = dr;
    *rope = dr;
    return MIO_OK;
}

// RoPE table, ggml rope-cache recurrence (theta = p; theta *= base^(-2/hd) per pair), and
// the iota list.
void upload_tables(const Load &ld, mio_hip_llm *m, float2 *dr) {
    const int n_ctx = ld.n_ctx, hd = m->dims.hd;
    std::vector<float2> rope((size_t)n_ctx * (hd / 2));
    const float theta_scale = powf(ld.rope_base, -2.0f / hd);
    for (int p = 0; p < n_ctx; ++p) {
        float theta = (float)p;
        for (int i = 0; i < hd / 2; ++i) {
            rope[(size_t)p * (hd / 2) + i] = make_float2(cosf(theta), sinf(theta));
            theta *= theta_scale;
        }
    }
    hipMemcpy(dr, rope.data(), rope.size() * sizeof(float2), hipMemcpyHostToDevice);
    std::vector<int> iota((size_t)n_ctx + mio::kPrefillB);
    for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int)i;
    hipMemcpy(m->d_iota, iota.data(), iota.size() * 4, hipMemcpyHostToDevice);
}

}  // namespace

extern "C" int mio_hip_llm_load(mio_hip_device *d, const char *path, int n_ctx, mio_hip_llm **out) {
    MIO_REQUIRE(d && path && out, MIO_ERR_INVALID, "llm_load: null argument");
    if (n_ctx <= 0) n_ctx = 2048;  // test-to-speech.cpp:104
    int rc = mio::bind(d);
    if (rc) return rc;
    const auto t_load0 = std::chrono::steady_clock::now();
    mio::GgufFile g;
    if (!g.open(path)) return MIO_ERR_IO;
    Load ld{g, g.get_str("general.architecture"), false, n_ctx};
    const std::string &arch = ld.arch;
    ld.lfm2 = arch == "lfm2";
    MIO_REQUIRE(arch == "llama" || arch == "qwen3" || arch == "qwen2" || arch == "mistral" || ld.lfm2,
                MIO_ERR_UNSUPPORTED, "llm_load: architecture '%s' not supported (llama, mistral, qwen2, qwen3, lfm2)",
                arch.c_str());
    // the only bias tensors any supported block has are qwen2's attn_{q,k,v}.bias: anything
    // else (output / ffn biases) would be silently dropped, so refuse the file instead
    for (const mio::GgufTensor &t : g.tensors()) {
        const std::string &n = t.name;
        MIO_REQUIRE(!(n.size() > 5 && n.compare(n.size() - 5, 5, ".bias") == 0 &&
                      !(n.find(".attn_q.bias") != std::string::npos || n.find(".attn_k.bias") != std::string::npos ||
                        n.find(".attn_v.bias") != std::string::npos)),
                    MIO_ERR_UNSUPPORTED, "llm_load: bias tensor %s is not supported (only attn_{q,k,v}.bias)",
                    n.c_str());
    }
    // owned from here on: every return below releases the model and what it has allocated
    auto m = std::make_unique<mio_hip_llm>();
    m->d = d;
    m->stager = std::make_unique<Stager>();
    MIO_REQUIRE(m->stager->init(), MIO_ERR_HIP, "llm_load: staging stream failed");
    if ((rc = read_dims(ld, m.get())) || (rc = plan_arena(ld, m.get())) || (rc = upload_globals(ld, m.get())))
        return rc;
    for (int i = 0; i < m->n_layer; ++i)
        if ((rc = upload_layer(ld, m.get(), i))) return rc;
    float2 *rope = nullptr;
    if ((rc = carve_buffers(ld, m.get(), &rope))) return rc;
    upload_tables(ld, m.get(), rope);
    // every memset / copy above ran on the null stream or the staging stream; the runner's
    // stream is non-blocking
    MIO_REQUIRE(m->stager->finish() && hipDeviceSynchronize() == hipSuccess, MIO_ERR_HIP,
                "llm_load: device synchronize failed");
    m->stager.reset();
    m->step = mio::StepCtx{m->dims, m->layers.data(), m->kc, m->vc, m->out_norm, m->lm, m->tok};
    // the decode-step graphs are captured here, as llama_init_from_model reserves its compute
    // graphs at context creation: the first generate replays them instead of capturing
    if ((rc = ensure_graph(m.get()))) return rc;
    m->load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_load0).count();
    *out = m.release();
    return MIO_OK;
}

extern "C" void mio_hip_llm_free(mio_hip_llm *m) { delete m; }
