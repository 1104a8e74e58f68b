// Test-support C-ABI (libmiotts_test.so, include/mio_hip_test.h): one launch of each MioCodec
// kernel (csrc/hip/codec_kernels.hip) on host arrays, the output between sentinel-filled
// guard zones. Not part of the product library.
#include <cstring>
#include <vector>

#include "codec_kernels.h"
#include "common.h"
#include "mio_hip_test.h"

namespace {

constexpr size_t kGuard = 256;  // bytes before and after every output

// Device allocations of one call, freed on every return path.
struct Pool {
    std::vector<void *> ptrs;
    bool ok = true;
    ~Pool() {
        for (void *p : ptrs) hipFree(p);
    }
    void *raw(size_t bytes) {
        void *p = nullptr;
        if (!ok || hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) {
            ok = false;
            return nullptr;
        }
        ptrs.push_back(p);
        return p;
    }
    // upload of a host operand (nullptr stays nullptr)
    template <class T>
    T *in(const T *host, size_t n) {
        if (!host) return nullptr;
        T *p = (T *)raw(n * sizeof(T));
        if (p && hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return p;
    }
};

// An output of `bytes` bytes between two guard zones. The whole allocation is filled with the
// 32-bit sentinel pattern; `init` (in/out operands) then replaces the part between the guards.
struct Guarded {
    uint8_t *base = nullptr;
    size_t bytes = 0;
    uint32_t pattern = 0;
    bool make(Pool &pool, size_t nbytes, uint32_t pat, const void *init) {
        bytes = nbytes, pattern = pat;
        const size_t total = bytes + 2 * kGuard;
        base = (uint8_t *)pool.raw(total);
        if (!base) return false;
        std::vector<uint32_t> fill((total + 3) / 4, pat);
        if (init) std::memcpy((uint8_t *)fill.data() + kGuard, init, bytes);
        if (hipMemcpy(base, fill.data(), total, hipMemcpyHostToDevice) != hipSuccess) pool.ok = false;
        return pool.ok;
    }
    template <class T>
    T *body() const {
        return (T *)(base + kGuard);
    }
    // download: the body into `host`, *intact = both guard zones still hold the sentinel
    hipError_t finish(void *host, int *intact) const {
        const size_t total = bytes + 2 * kGuard;
        std::vector<uint32_t> all((total + 3) / 4);
        const hipError_t e = hipMemcpy(all.data(), base, total, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        const uint8_t *b = (const uint8_t *)all.data();
        std::vector<uint32_t> ref((total + 3) / 4, pattern);
        const uint8_t *r = (const uint8_t *)ref.data();
        const bool okg = std::memcmp(b, r, kGuard) == 0 &&
                         std::memcmp(b + kGuard + bytes, r + kGuard + bytes, kGuard) == 0;
        std::memcpy(host, b + kGuard, bytes);
        if (intact) *intact = okg ? 1 : 0;
        return hipSuccess;
    }
};

constexpr uint32_t kS32 = MIO_DEBUG_SENTINEL_F32;
constexpr uint32_t kS16 = MIO_DEBUG_SENTINEL_F16 | (MIO_DEBUG_SENTINEL_F16 << 16);

// after the launch: launch error, completion, download
int conclude(mio_hip_device *d, const Guarded &out, void *host, int *guards_ok) {
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(d->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = out.finish(host, guards_ok);
    MIO_HIP_CHECK(e);
    return MIO_OK;
}

}  // namespace

extern "C" int mio_hip_debug_codec_gemm(mio_hip_device *d, const mio_debug_gemm *g, const float *A,
                                        const float *B, float *C, const float *bias, const float *aux,
                                        const float *aux2, int *guards_ok) {
    MIO_REQUIRE(d && g && A && B && C, MIO_ERR_INVALID, "debug_codec_gemm: null argument");
    MIO_REQUIRE(g->M > 0 && g->N > 0 && g->K > 0 && g->a_rows > 0 && g->a_seg > 0 && g->ldc > 0 && g->c_rows > 0,
                MIO_ERR_INVALID, "debug_codec_gemm: sizes");
    MIO_REQUIRE(g->K % 4 == 0 && g->a_seg % 4 == 0, MIO_ERR_INVALID,
                "debug_codec_gemm: K %d and a_seg %d must be multiples of 4 (float4 operand loads)", g->K, g->a_seg);
    MIO_REQUIRE((long)g->a_rows * g->a_seg < (1L << 29) && (long)g->N * g->K < (1L << 29) &&
                    ((long)g->M + (g->a_row_off < 0 ? -(long)g->a_row_off : g->a_row_off) + 64) * g->a_seg + g->K <
                        (1L << 29),
                MIO_ERR_INVALID, "debug_codec_gemm: operand past the 2 GiB buffer range");
    MIO_REQUIRE(g->epi >= mio::EPI_STORE && g->epi <= mio::EPI_HEAD, MIO_ERR_INVALID, "debug_codec_gemm: epi %d",
                g->epi);
    MIO_REQUIRE(g->kg == 0 || g->kg == 1 || g->kg == 2 || g->kg == 4, MIO_ERR_INVALID, "debug_codec_gemm: kg %d",
                g->kg);
    MIO_REQUIRE(g->a_f16 == 0 || g->a_f16 == 1, MIO_ERR_INVALID, "debug_codec_gemm: a_f16 %d", g->a_f16);
    const int epi = g->epi;
    const bool convt = epi == mio::EPI_CONVT || epi == mio::EPI_CONVT_SNAKE;
    const bool snake = epi == mio::EPI_CONVT_SNAKE || epi == mio::EPI_SNAKE;
    size_t ncol = (size_t)g->N;  // length of bias / aux / aux2
    if (convt) {
        MIO_REQUIRE(g->f > 0 && g->cout > 0 && g->N == g->f * g->cout && g->trim >= 0 && g->rows_out > 0 &&
                        g->ldc >= g->cout && g->c_rows >= g->rows_out,
                    MIO_ERR_INVALID, "debug_codec_gemm: ConvT remap (f %d, cout %d, N %d, trim %d, rows_out %d)",
                    g->f, g->cout, g->N, g->trim, g->rows_out);
        ncol = (size_t)g->cout;
    } else if (epi == mio::EPI_SWIGLU) {
        MIO_REQUIRE(g->N % 32 == 0 && g->ldc >= g->N / 2 && g->c_rows >= g->M, MIO_ERR_INVALID,
                    "debug_codec_gemm: SWIGLU needs N %% 32 == 0 (gate|up rows interleaved per 16)");
    } else if (epi == mio::EPI_HEAD) {
        MIO_REQUIRE(g->N % 32 == 0 && g->cout > 0 && g->cout <= g->N / 2 && g->ldc >= 2 * g->cout &&
                        g->c_rows >= g->M,
                    MIO_ERR_INVALID, "debug_codec_gemm: HEAD needs N %% 32 == 0, cout = n_freq <= N / 2");
    } else {
        MIO_REQUIRE(g->ldc >= g->N && g->c_rows >= g->M, MIO_ERR_INVALID, "debug_codec_gemm: C smaller than M x N");
    }
    MIO_REQUIRE(bias || epi == mio::EPI_STORE || epi == mio::EPI_RESID || epi == mio::EPI_GATED ||
                    epi == mio::EPI_SWIGLU,
                MIO_ERR_INVALID, "debug_codec_gemm: epilogue %d reads bias", epi);
    MIO_REQUIRE(aux || !(snake || epi == mio::EPI_GATED), MIO_ERR_INVALID, "debug_codec_gemm: epilogue %d reads aux",
                epi);
    MIO_REQUIRE(aux2 || !snake, MIO_ERR_INVALID, "debug_codec_gemm: epilogue %d reads aux2", epi);
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    mio::GemmArgs a{};
    a.A = pool.in(A, (size_t)g->a_rows * g->a_seg);
    a.B = pool.in(B, (size_t)g->N * g->K);
    a.bias = pool.in(bias, ncol);
    a.aux = pool.in(aux, ncol);
    a.aux2 = pool.in(aux2, ncol);
    out.make(pool, (size_t)g->c_rows * g->ldc * 4, kS32, C);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_gemm: device allocation or upload failed");
    a.a_seg = g->a_seg, a.a_row_off = g->a_row_off, a.a_rows = g->a_rows;
    a.M = g->M, a.N = g->N, a.K = g->K;
    a.C = out.body<float>(), a.ldc = g->ldc;
    a.f = g->f, a.trim = g->trim, a.cout = g->cout, a.rows_out = g->rows_out;
    a.m_major = g->m_major, a.a_f16 = g->a_f16;
    if (g->kg == 0) {
        mio::launch_gemm_f32(a, epi, d->stream);
    } else {
        MIO_REQUIRE(mio::launch_gemm_f32_cfg(a, epi, g->kg, 11, d->stream) == 0, MIO_ERR_UNSUPPORTED,
                    "debug_codec_gemm: tile configuration kg %d not built", g->kg);
    }
    return conclude(d, out, C, guards_ok);
}

extern "C" int mio_hip_debug_codec_conv(mio_hip_device *d, const uint16_t *xa, int L, int Cin, int taps, int pad,
                                        const uint16_t *w, int Cout, const float *bias, int resid_mode,
                                        const float *resid, float *y, int *guards_ok) {
    MIO_REQUIRE(d && xa && w && bias && y, MIO_ERR_INVALID, "debug_codec_conv: null argument");
    MIO_REQUIRE(L > 0 && Cin > 0 && Cout > 0 && taps > 0 && pad >= 0 && pad < taps, MIO_ERR_INVALID,
                "debug_codec_conv: sizes");
    MIO_REQUIRE(Cin % 8 == 0, MIO_ERR_INVALID, "debug_codec_conv: Cin %d must be a multiple of 8 (16-byte f16 loads)",
                Cin);
    MIO_REQUIRE(((long)L + 64 + taps) * Cin * taps < (1L << 30) && (long)(Cout + 64) * taps * Cin < (1L << 30),
                MIO_ERR_INVALID, "debug_codec_conv: operand past the 2 GiB buffer range");
    MIO_REQUIRE(resid_mode >= 0 && resid_mode <= 2 && (resid_mode != 1 || resid), MIO_ERR_INVALID,
                "debug_codec_conv: resid_mode %d", resid_mode);
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    mio::ConvArgs a{};
    a.Xa = (const _Float16 *)pool.in(xa, (size_t)L * Cin);
    a.B = (const _Float16 *)pool.in(w, (size_t)Cout * taps * Cin);
    a.bias = pool.in(bias, (size_t)Cout);
    const float *dres = resid_mode == 1 ? pool.in(resid, (size_t)L * Cout) : nullptr;
    out.make(pool, (size_t)L * Cout * 4, kS32, resid_mode == 2 ? y : nullptr);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_conv: device allocation or upload failed");
    a.L = L, a.Cin = Cin, a.taps = taps, a.pad = pad, a.Cout = Cout;
    a.Y = out.body<float>();
    a.resid = resid_mode == 1 ? dres : resid_mode == 2 ? a.Y : nullptr;
    mio::launch_conv_f16(a, d->stream);
    return conclude(d, out, y, guards_ok);
}

extern "C" int mio_hip_debug_codec_rownorm(mio_hip_device *d, const float *x, int M, int D, float eps, int mode,
                                           const float *p0, const float *p1, int in_place, float *y,
                                           int *guards_ok) {
    MIO_REQUIRE(d && x && y && M > 0, MIO_ERR_INVALID, "debug_codec_rownorm: bad args");
    MIO_REQUIRE(D >= 64 && D <= 1024 && D % 64 == 0, MIO_ERR_INVALID,
                "debug_codec_rownorm: D %d must be a multiple of 64, at most 1024", D);
    MIO_REQUIRE(mode >= 0 && mode <= 2 && (mode == 0 || p0) && (mode != 2 || p1), MIO_ERR_INVALID,
                "debug_codec_rownorm: mode %d / parameters", mode);
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    const float *dx = in_place ? nullptr : pool.in(x, (size_t)M * D);
    const float *d0 = pool.in(p0, (size_t)D), *d1 = pool.in(p1, (size_t)D);
    out.make(pool, (size_t)M * D * 4, kS32, in_place ? x : nullptr);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_rownorm: device allocation or upload failed");
    mio::launch_rownorm(in_place ? out.body<float>() : dx, out.body<float>(), M, D, eps, mode, d0, d1, d->stream);
    return conclude(d, out, y, guards_ok);
}

extern "C" int mio_hip_debug_codec_groupnorm(mio_hip_device *d, const float *x, int L, int C, int G, float eps,
                                             const float *gamma, const float *beta, uint16_t *xa,
                                             int *guards_ok) {
    MIO_REQUIRE(d && x && gamma && beta && xa && L > 0, MIO_ERR_INVALID, "debug_codec_groupnorm: bad args");
    MIO_REQUIRE(C > 0 && C % 8 == 0 && C <= 1024, MIO_ERR_INVALID,
                "debug_codec_groupnorm: C %d must be a multiple of 8, at most 1024", C);
    MIO_REQUIRE(G > 0 && G <= 64 && C % G == 0 && 64 % (C / G) == 0, MIO_ERR_INVALID,
                "debug_codec_groupnorm: G %d (at most 64 groups, C / G dividing 64)", G);
    MIO_REQUIRE((long)L * C < (1L << 28), MIO_ERR_INVALID, "debug_codec_groupnorm: L %d too long", L);
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    const float *dx = pool.in(x, (size_t)L * C);
    const float *dg = pool.in(gamma, (size_t)C), *db = pool.in(beta, (size_t)C);
    mio::GnScratch gs{};
    gs.part = (double *)pool.raw((size_t)mio::kGnPartDoubles * sizeof(double));
    gs.stat = (float2 *)pool.raw(64 * sizeof(float2));
    out.make(pool, (size_t)L * C * 2, kS16, nullptr);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_groupnorm: device allocation or upload failed");
    mio::launch_groupnorm_apply(dx, L, C, G, eps, dg, db, gs, out.body<_Float16>(), d->stream);
    return conclude(d, out, xa, guards_ok);
}

extern "C" int mio_hip_debug_codec_band_attention(mio_hip_device *d, const float *qkv, int S, int H, int window,
                                                  const float *rope, float *outp, int *guards_ok) {
    MIO_REQUIRE(d && qkv && rope && outp && S > 0 && H > 0 && H <= 16, MIO_ERR_INVALID,
                "debug_codec_band_attention: bad args");
    MIO_REQUIRE(window >= 1 && window / 2 <= 32, MIO_ERR_INVALID,
                "debug_codec_band_attention: window %d (half width at most 32)", window);
    MIO_REQUIRE((long)S * 3 * H * 64 < (1L << 28), MIO_ERR_INVALID, "debug_codec_band_attention: S %d too long", S);
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    const float *dq = pool.in(qkv, (size_t)S * 3 * H * 64);
    const float *dr = pool.in(rope, (size_t)S * 64);
    out.make(pool, (size_t)S * H * 64 * 4, kS32, nullptr);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_band_attention: device allocation or upload failed");
    mio::launch_band_attention(dq, out.body<float>(), S, H, window, (const float2 *)dr, d->stream);
    return conclude(d, out, outp, guards_ok);
}

extern "C" int mio_hip_debug_codec_cond_gemv(mio_hip_device *d, const float *W, const float *b, const float *e,
                                             int R, int A, int e_f16, float *y, int *guards_ok) {
    MIO_REQUIRE(d && W && b && e && y && R > 0 && A > 0 && (long)R * A < (1L << 28) && (e_f16 == 0 || e_f16 == 1),
                MIO_ERR_INVALID, "debug_codec_cond_gemv: bad args");
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    const float *dW = pool.in(W, (size_t)R * A), *db = pool.in(b, (size_t)R), *de = pool.in(e, (size_t)A);
    out.make(pool, (size_t)R * 4, kS32, nullptr);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_cond_gemv: device allocation or upload failed");
    mio::launch_cond_gemv(dW, db, de, R, A, out.body<float>(), e_f16, d->stream);
    return conclude(d, out, y, guards_ok);
}

extern "C" int mio_hip_debug_codec_embed(mio_hip_device *d, const float *table, int n_rows, int D,
                                         const int32_t *codes, int T, float *x, int *guards_ok) {
    MIO_REQUIRE(d && table && codes && x && n_rows > 0 && T > 0 && D > 0 && (long)n_rows * D < (1L << 28) &&
                    (long)T * D < (1L << 28),
                MIO_ERR_INVALID, "debug_codec_embed: bad args");
    MIO_REQUIRE(D % 4 == 0, MIO_ERR_INVALID, "debug_codec_embed: D %d must be a multiple of 4 (float4 copies)", D);
    for (int t = 0; t < T; ++t)
        MIO_REQUIRE(codes[t] >= 0 && codes[t] < n_rows, MIO_ERR_INVALID, "debug_codec_embed: code %d at %d", codes[t],
                    t);
    int rc = mio::bind(d);
    if (rc) return rc;
    Pool pool;
    Guarded out;
    const float *dt = pool.in(table, (size_t)n_rows * D);
    const int *dc = pool.in(codes, (size_t)T);
    out.make(pool, (size_t)T * D * 4, kS32, nullptr);
    MIO_REQUIRE(pool.ok, MIO_ERR_HIP, "debug_codec_embed: device allocation or upload failed");
    mio::launch_embed(dt, dc, T, D, out.body<float>(), d->stream);
    return conclude(d, out, x, guards_ok);
}
