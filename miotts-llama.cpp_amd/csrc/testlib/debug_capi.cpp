// Test-support C-ABI (libmiotts_test.so, include/mio_hip_test.h): parity entry points of the
// matvec / batched-matmul kernels on raw GGUF rows, and the host quantizer the synthetic
// models are built with. Not part of the product library.
#include <cstring>
#include <vector>

#include "common.h"
#include "gguf.h"
#include "llm.h"
#include "llm_kernels.h"
#include "mio_hip_test.h"
#include "quant.h"

namespace {
// An f32 output of n values between two 256-byte guard zones, the whole allocation filled with
// MIO_DEBUG_SENTINEL_F32 (init != nullptr: an in/out operand's values between the guards), so
// that a row no wave wrote comes back as the sentinel and a write outside the rows is an error.
constexpr size_t kGuardF = 256 / 4;
struct GuardedY {
    float *base = nullptr;
    size_t n = 0;
    hipError_t make(size_t count, const float *init) {
        n = count;
        hipError_t e = hipMalloc(&base, (n + 2 * kGuardF) * 4);
        if (e != hipSuccess) return e;
        std::vector<uint32_t> fill(n + 2 * kGuardF, MIO_DEBUG_SENTINEL_F32);
        if (init) memcpy(fill.data() + kGuardF, init, n * 4);
        return hipMemcpy(base, fill.data(), fill.size() * 4, hipMemcpyHostToDevice);
    }
    float *body() const { return base + kGuardF; }
    // download: the body into y; *zone = the guard zone that no longer holds the sentinel
    hipError_t finish(float *y, const char **zone) const {
        std::vector<uint32_t> all(n + 2 * kGuardF);
        const hipError_t e = hipMemcpy(all.data(), base, all.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        *zone = nullptr;
        for (size_t i = 0; i < kGuardF; ++i) {
            if (all[kGuardF + n + i] != MIO_DEBUG_SENTINEL_F32) *zone = "after the last row";
            if (all[i] != MIO_DEBUG_SENTINEL_F32) *zone = "before row 0";
        }
        memcpy(y, all.data() + kGuardF, n * 4);
        return hipSuccess;
    }
};

// y = W x, or with gguf_up y = silu(W x) * (up x), on the decode step's streaming matvec engine;
// su > 0: on its single-group row stream of su units per wave over `grid` workgroups
int debug_matvec(mio_hip_device *d, uint32_t type, const void *gguf_rows, const void *gguf_up, int rows, int k,
                 const float *x, float *y, int su = 0, int grid = 0) {
    MIO_REQUIRE(d && gguf_rows && x && y && rows > 0 && k > 0, MIO_ERR_INVALID, "debug_matvec: bad args");
    MIO_REQUIRE(mio::is_weight_type((int)type) || (!gguf_up && mio::repacks_to_q8_0(type)), MIO_ERR_UNSUPPORTED, "debug_matvec: type %u", type);
    MIO_REQUIRE(k % (mio::is_kquant((int)type) ? 256 : 32) == 0, MIO_ERR_INVALID, "debug_matvec: k %d", k);
    int rc = mio::bind(d);
    if (rc) return rc;
    // Q4_0 / Q5_0 run as the Q8_0 rows they equal (llm_load does the same)
    std::vector<uint8_t> q80;
    if (mio::repacks_to_q8_0(type)) {
        q80.resize((size_t)rows * (k / 32) * sizeof(mio::BlockQ8_0));
        mio::repack_to_q8_0(type, gguf_rows, rows, k, q80.data());
        gguf_rows = q80.data();
        type = mio::GGML_Q8_0;
    }
    const mio::SplitLayout L = mio::split_layout(type, rows, k);
    const int nm = gguf_up ? 2 : 1;
    std::vector<uint8_t> host(L.bytes * nm);
    mio::to_split(type, gguf_rows, rows, k, host.data());
    if (gguf_up) mio::to_split(type, gguf_up, rows, k, host.data() + L.bytes);
    uint8_t *dw = nullptr;
    float *dx = nullptr;
    GuardedY out;
    MIO_HIP_CHECK(hipMalloc(&dw, L.bytes * nm));
    MIO_HIP_CHECK(hipMalloc(&dx, (size_t)k * 4));
    MIO_HIP_CHECK(out.make((size_t)rows, nullptr));
    float *dy = out.body();
    hipMemcpy(dw, host.data(), L.bytes * nm, hipMemcpyHostToDevice);
    hipMemcpy(dx, x, (size_t)k * 4, hipMemcpyHostToDevice);
    auto qm = [&](uint8_t *base) {
        return mio::QMat{(int)type, rows, k, base + L.off[0], base + L.off[1], base + L.off[2], base + L.off[3]};
    };
    const mio::QMat q = qm(dw), up = qm(dw + (gguf_up ? L.bytes : 0));
    bool launched = true;
    if (su > 0)
        launched = mio::launch_debug_matvec_group(q, gguf_up ? &up : nullptr, dx, dy, su, grid, d->stream);
    else
        mio::launch_debug_matvec(q, gguf_up ? &up : nullptr, dx, dy, d->n_cu > 0 ? d->n_cu : 256, d->stream);
    if (!launched) {
        hipFree(dw), hipFree(dx), hipFree(out.base);
        MIO_REQUIRE(false, MIO_ERR_INVALID, "debug_matvec_group: su %d / grid %d for %d rows, k %d", su, grid, rows, k);
    }
    hipError_t e = hipStreamSynchronize(d->stream);
    const char *zone = nullptr;
    if (e == hipSuccess) e = out.finish(y, &zone);
    hipFree(dw), hipFree(dx), hipFree(out.base);
    MIO_HIP_CHECK(e);
    MIO_REQUIRE(!zone, MIO_ERR_HIP, "debug_matvec: the guard zone %s of y[%d] was written", zone, rows);
    return MIO_OK;
}
}  // namespace

extern "C" int mio_hip_debug_matvec(mio_hip_device *d, uint32_t type, const void *gguf_rows, int rows, int k,
                                    const float *x, float *y) {
    return debug_matvec(d, type, gguf_rows, nullptr, rows, k, x, y);
}

extern "C" int mio_hip_debug_matvec_swiglu(mio_hip_device *d, uint32_t type, const void *gguf_gate,
                                           const void *gguf_up, int rows, int k, const float *x, float *y) {
    MIO_REQUIRE(gguf_up, MIO_ERR_INVALID, "debug_matvec_swiglu: bad args");
    return debug_matvec(d, type, gguf_gate, gguf_up, rows, k, x, y);
}

extern "C" int mio_hip_debug_matvec_group(mio_hip_device *d, uint32_t type, const void *gguf_gate,
                                          const void *gguf_up, int rows, int k, int su, int grid, const float *x,
                                          float *y) {
    MIO_REQUIRE(su > 0 && grid > 0 && grid <= 4096, MIO_ERR_INVALID, "debug_matvec_group: su %d / grid %d", su, grid);
    MIO_REQUIRE(mio::is_weight_type((int)type), MIO_ERR_UNSUPPORTED, "debug_matvec_group: type %u", type);
    return debug_matvec(d, type, gguf_gate, gguf_up, rows, k, x, y, su, grid);
}

extern "C" int mio_hip_debug_act_quant(mio_hip_device *d, uint32_t type, const float *x, const float *w, int k,
                                       float eps, int sc1, int8_t *qs, float *dd, int16_t *bs) {
    MIO_REQUIRE(d && x && qs && dd && bs && k > 0, MIO_ERR_INVALID, "debug_act_quant: bad args");
    MIO_REQUIRE(type == mio::GGML_Q8_0 || type == mio::GGML_Q4_K || type == mio::GGML_BF16, MIO_ERR_UNSUPPORTED,
                "debug_act_quant: type %u", type);
    MIO_REQUIRE(k % (type == mio::GGML_Q4_K ? 256 : 32) == 0 && k <= 12288, MIO_ERR_INVALID,
                "debug_act_quant: k %d", k);
    int rc = mio::bind(d);
    if (rc) return rc;
    const size_t nb = mio::debug_act_record_bytes(k);
    float *dx = nullptr, *dw = nullptr;
    char *dr = nullptr;
    MIO_HIP_CHECK(hipMalloc(&dx, (size_t)k * 4));
    MIO_HIP_CHECK(hipMalloc(&dw, (size_t)k * 4));
    MIO_HIP_CHECK(hipMalloc(&dr, nb));
    hipMemcpy(dx, x, (size_t)k * 4, hipMemcpyHostToDevice);
    if (w) hipMemcpy(dw, w, (size_t)k * 4, hipMemcpyHostToDevice);
    mio::launch_debug_act_quant((int)type, dx, w ? dw : nullptr, k, eps, sc1 != 0, dr, d->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    std::vector<char> rec(nb);
    if (e == hipSuccess) e = hipMemcpy(rec.data(), dr, nb, hipMemcpyDeviceToHost);
    hipFree(dx), hipFree(dw), hipFree(dr);
    MIO_HIP_CHECK(e);
    // the record's layout (llm_device.h carve): qs [2k] | d f32[k/32 + 8] | bs i16[k/16 + 8]
    memcpy(qs, rec.data(), (size_t)k * 2);
    memcpy(dd, rec.data() + (size_t)k * 2, (size_t)(k / 32 + 8) * 4);
    memcpy(bs, rec.data() + (size_t)k * 2 + (size_t)(k / 32 + 8) * 4, (size_t)(k / 16 + 8) * 2);
    return MIO_OK;
}

extern "C" int mio_hip_debug_mmq(mio_hip_device *d, uint32_t type, const void *gguf_rows, int rows, int k,
                                 const float *x, int nt, int mode, const void *gguf_up, float *y) {
    MIO_REQUIRE(d && gguf_rows && x && y && rows > 0 && k > 0 && nt > 0 && nt <= 4096 && mode >= 0 && mode <= 2 &&
                    (mode != 2 || gguf_up),
                MIO_ERR_INVALID, "debug_mmq: bad args");
    MIO_REQUIRE(type == mio::GGML_Q8_0 || mio::is_kquant((int)type), MIO_ERR_UNSUPPORTED, "debug_mmq: type %u", type);
    MIO_REQUIRE(k % mio::block_elems((int)type) == 0, MIO_ERR_INVALID, "debug_mmq: k %d", k);
    int rc = mio::bind(d);
    if (rc) return rc;
    const mio::SplitLayout L = mio::split_layout(type, rows, k);
    const int nm = mode == 2 ? 2 : 1;
    std::vector<uint8_t> host(L.bytes * nm);
    mio::to_split(type, gguf_rows, rows, k, host.data());
    if (nm == 2) mio::to_split(type, gguf_up, rows, k, host.data() + L.bytes);
    uint8_t *dw = nullptr;
    float *dx = nullptr;
    char *da = nullptr;
    GuardedY out;
    MIO_HIP_CHECK(hipMalloc(&dw, L.bytes * nm));
    MIO_HIP_CHECK(hipMalloc(&dx, (size_t)nt * k * 4));
    MIO_HIP_CHECK(out.make((size_t)nt * rows, mode == 1 ? y : nullptr));  // mode 1 adds to y
    float *dy = out.body();
    MIO_HIP_CHECK(hipMalloc(&da, (size_t)nt * mio::debug_act_bytes(k)));
    hipMemcpy(dw, host.data(), L.bytes * nm, hipMemcpyHostToDevice);
    hipMemcpy(dx, x, (size_t)nt * k * 4, hipMemcpyHostToDevice);
    auto qm = [&](uint8_t *base) {
        return mio::QMat{(int)type, rows, k, base + L.off[0], base + L.off[1], base + L.off[2], base + L.off[3]};
    };
    const mio::QMat q = qm(dw), up = nm == 2 ? qm(dw + L.bytes) : mio::QMat{};
    mio::launch_debug_mmq(q, up, mode, dx, nt, da, dy, d->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    const char *zone = nullptr;
    if (e == hipSuccess) e = out.finish(y, &zone);
    hipFree(dw), hipFree(dx), hipFree(out.base), hipFree(da);
    MIO_HIP_CHECK(e);
    MIO_REQUIRE(!zone, MIO_ERR_HIP, "debug_mmq: the guard zone %s of y[%d][%d] was written", zone, nt, rows);
    return MIO_OK;
}

// The attention launches on injected K/V rows and an injected q|k|v row: the work is done next
// to the runner's state (csrc/host/llm.cpp), exported here so the product library carries no
// test entry point.
extern "C" int mio_hip_llm_set_kv_rows(mio_hip_llm *m, int il, int p0, int n_pos, const uint16_t *k,
                                       const uint16_t *v) {
    return mio::llm_set_kv_rows(m, il, p0, n_pos, k, v);
}

extern "C" int mio_hip_llm_debug_attention(mio_hip_llm *m, int il, int pos, int which, const float *qkv,
                                           float *att) {
    return mio::llm_debug_attention(m, il, pos, which, qkv, att);
}

extern "C" int mio_hip_llm_handoff_words(mio_hip_llm *m, int reset, int32_t *words) {
    return mio::llm_handoff_words(m, reset, words);
}

extern "C" int mio_hip_llm_debug_sample_chain(mio_hip_llm *m, const float *logits, const int32_t *history,
                                              int n_history, const mio_sampling *s, float temperature, uint64_t seed,
                                              int step, int32_t lo, int32_t hi, int32_t *token, int32_t *kept,
                                              int32_t *cut_id, float *penalised) {
    MIO_REQUIRE(m && s, MIO_ERR_INVALID, "llm_debug_sample_chain: null argument");
    int info[8];
    if (int rc = mio_hip_llm_info(m, info)) return rc;
    MIO_REQUIRE(lo >= 0 && lo < info[0] && hi <= info[0], MIO_ERR_INVALID,
                "llm_debug_sample_chain: window [%d, %d) outside the %d-id vocabulary", lo, hi, info[0]);
    mio::SamplingParams sp;
    sp.temperature = temperature, sp.seed = seed, sp.allow_lo = lo, sp.allow_hi = hi < 0 ? 0 : hi;
    sp.top_k = s->top_k, sp.top_p = s->top_p, sp.min_p = s->min_p, sp.repeat_penalty = s->repeat_penalty;
    sp.frequency_penalty = s->frequency_penalty, sp.presence_penalty = s->presence_penalty;
    sp.repeat_last_n = s->repeat_last_n;
    return mio::llm_debug_sample_chain(m, logits, history, n_history, sp, step, token, kept, cut_id, penalised);
}

extern "C" int mio_quantize_rows(uint32_t type, const float *x, int rows, int k, void *out) {
    MIO_REQUIRE(x && out && rows > 0 && k > 0, MIO_ERR_INVALID, "quantize_rows: bad args");
    const size_t rb = mio::ggml_row_bytes(type, k);
    MIO_REQUIRE(rb, MIO_ERR_UNSUPPORTED, "quantize_rows: type %u / k %d", type, k);
    for (int r = 0; r < rows; ++r)
        if (!mio::quantize_row(type, x + (size_t)r * k, (uint8_t *)out + r * rb, k)) return MIO_ERR_UNSUPPORTED;
    return MIO_OK;
}

extern "C" int mio_dequantize_rows(uint32_t type, const void *rows_bytes, int rows, int k, float *out) {
    MIO_REQUIRE(rows_bytes && out && rows > 0 && k > 0, MIO_ERR_INVALID, "dequantize_rows: bad args");
    const size_t rb = mio::ggml_row_bytes(type, k);
    MIO_REQUIRE(rb, MIO_ERR_UNSUPPORTED, "dequantize_rows: type %u / k %d", type, k);
    for (int r = 0; r < rows; ++r)
        if (!mio::dequantize_row(type, (const uint8_t *)rows_bytes + r * rb, out + (size_t)r * k, k))
            return MIO_ERR_UNSUPPORTED;
    return MIO_OK;
}

// The split layout of GGUF rows (quant.h to_split), host only: *nbytes receives the layout's
// size and the four planes' byte offsets go to off[4]; out (may be null: sizes only) must hold
// that many bytes.
extern "C" int mio_debug_to_split(uint32_t type, const void *rows_bytes, int rows, int k, uint8_t *out,
                                  uint64_t *nbytes, uint64_t *off) {
    MIO_REQUIRE(rows_bytes && nbytes && off && rows > 0 && k > 0, MIO_ERR_INVALID, "debug_to_split: bad args");
    const mio::SplitLayout L = mio::split_layout(type, rows, k);
    MIO_REQUIRE(L.bytes && mio::ggml_row_bytes(type, k), MIO_ERR_UNSUPPORTED, "debug_to_split: type %u / k %d", type, k);
    *nbytes = L.bytes;
    for (int i = 0; i < 4; ++i) off[i] = L.off[i];
    if (out && !mio::to_split(type, rows_bytes, rows, k, out)) return MIO_ERR_UNSUPPORTED;
    return MIO_OK;
}

// The weight-type table (csrc/weight_types.h) as the host sites read it, host only: stride[4] =
// the planes' row strides of a [rows][k] matrix, off[4] = split_layout's plane offsets,
// moved[4] = the bytes qmat_rows(q, r0, n) moves each plane pointer by (0: no such plane).
extern "C" int mio_debug_weight_layout(uint32_t type, int rows, int k, int r0, int n, uint64_t *stride, uint64_t *off,
                                       uint64_t *moved) {
    MIO_REQUIRE(stride && off && moved && rows > 0 && k > 0 && r0 >= 0 && n >= 0 && r0 + n <= rows, MIO_ERR_INVALID,
                "debug_weight_layout: bad args");
    MIO_REQUIRE(mio::is_weight_type((int)type), MIO_ERR_UNSUPPORTED, "debug_weight_layout: type %u", type);
    const mio::SplitLayout L = mio::split_layout(type, rows, k);
    std::vector<uint8_t> buf(L.bytes);
    const mio::QMat q{(int)type, rows, k, buf.data() + L.off[0], buf.data() + L.off[1], buf.data() + L.off[2],
                      buf.data() + L.off[3]};
    const mio::QMat v = mio::qmat_rows(q, r0, n);
    const uint8_t *qp[4] = {q.p0, q.p1, q.p2, q.p3}, *vp[4] = {v.p0, v.p1, v.p2, v.p3};
    for (int p = 0; p < 4; ++p) {
        stride[p] = mio::plane_row_bytes((int)type, k, p);
        off[p] = L.off[p];
        moved[p] = (uint64_t)(vp[p] - qp[p]);
    }
    return v.rows == n && v.k == k && v.type == (int)type ? MIO_OK : MIO_ERR_INVALID;
}

// attn_v_supported(tq, tv): 1 where the q|k|v launches exist for v of type tv beside q|k of type tq.
extern "C" int mio_debug_attn_v_supported(int tq, int tv) { return mio::attn_v_supported(tq, tv) ? 1 : 0; }
