// C-ABI: the output-rate resampler (include/mio_hip.h, "output rate"): filter design in float64,
// the LDS layout of the phase table, the stream state, and the launches of pcm_resample.hip.
#include "common.h"
#include "pcm_resample.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

struct mio_hip_resampler {
    mio_hip_device *d = nullptr;  // null: design only
    int dev = 0;                  // d's GPU index: destroy must not read *d, which may be closed by then
    int f_in = 0, f_out = 0, L = 0, M = 0, P = 0;
    int cs = 0, nt = 0, tab_words = 0;  // LDS row stride, threads per workgroup, table image size
    std::vector<float> c;               // c[L][P]
    float *d_table = nullptr, *d_hist = nullptr, *d_part = nullptr;  // d_hist: 2 x (P - 1)
    int hist_cur = 0;
    long long seen = 0, out_next = 0;
};

namespace {

constexpr int kRates[] = {8000, 16000, 22050, 24000, 32000, 48000};
constexpr double kAtten = 80.0;
constexpr int kBanks = 64;

// modified Bessel function I0 by its power series (beta is about 7.9: 40 terms are ample)
double bessel_i0(double x) {
    long double q = (long double)x * x / 4, term = 1, sum = 1;
    for (int k = 1; k < 200 && term > sum * 1e-22L; ++k) {
        term *= q / ((long double)k * k);
        sum += term;
    }
    return (double)sum;
}

// h[n] of mio_hip.h, as c[phi][j] = h[j L + phi]
void design(int L, int M, int *P_out, std::vector<float> &c) {
    const int F = std::max(L, M);
    const double beta = 0.1102 * (kAtten - 8.7);
    const double n_min = (kAtten - 7.95) / (2.285 * 0.2 * M_PI / F) + 1;
    int P = (int)std::ceil(n_min / L);
    P += P & 1;
    const long long N = (long long)P * L;
    const double ctr = (N - 1) / 2.0, wc = 0.9 * M_PI / F, i0b = bessel_i0(beta);
    c.assign((size_t)N, 0.0f);
    for (long long n = 0; n < N; ++n) {
        const double y = M_PI * (wc * (n - ctr) / M_PI);
        const double r = (n - ctr) / ctr;
        const double w = bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
        c[(size_t)(n % L) * P + (size_t)(n / L)] = (float)(L * (wc / M_PI) * (std::sin(y) / y) * w);
    }
    *P_out = P;
}

// Lane j of a wave reads table word row_j * cs + t, row_j = (row_0 + j (M mod L)) mod L: the
// sum over the waves' first rows of the most lanes that meet in one of the 64 banks on distinct
// words (equal rows read one word, a broadcast). The shift by t rotates the banks and changes
// nothing.
long long stride_cost(int L, int M, int cs) {
    long long cost = 0;
    const int d = M % L, starts = std::min(L, 256);
    for (int r0 = 0; r0 < starts; ++r0) {
        int hits[kBanks] = {0}, worst = 0;
        for (int j = 0; j < std::min(64, L); ++j) {  // lanes 64 apart in row order repeat rows
            const int bank = (int)(((long long)((r0 + (long long)j * d) % L) * cs) % kBanks);
            worst = std::max(worst, ++hits[bank]);
        }
        cost += worst;
    }
    return cost;
}

}  // namespace

extern "C" int mio_hip_resampler_create(mio_hip_device *d, int f_in, int f_out, mio_hip_resampler **out) {
    MIO_REQUIRE(out, MIO_ERR_INVALID, "resampler_create: null out");
    *out = nullptr;
    MIO_REQUIRE(f_in > 0, MIO_ERR_INVALID, "resampler_create: input rate %d", f_in);
    MIO_REQUIRE(std::find(std::begin(kRates), std::end(kRates), f_out) != std::end(kRates) && f_out != f_in,
                MIO_ERR_UNSUPPORTED,
                "resampler_create: output rate %d Hz from %d Hz is not supported (8000, 16000, 22050, 24000, "
                "32000 or 48000, other than the input rate)",
                f_out, f_in);
    const int g = std::gcd(f_in, f_out), L = f_out / g, M = f_in / g;
    // the table is about 200 * max(L, M) bytes (and at least 8 L): refuse before designing it
    MIO_REQUIRE(std::max(L, M) <= 1024 && L <= 16384, MIO_ERR_UNSUPPORTED,
                "resampler_create: %d Hz from %d Hz needs a phase table over 128 KB", f_out, f_in);
    auto *h = new mio_hip_resampler();
    h->d = d, h->dev = d ? d->dev : 0, h->f_in = f_in, h->f_out = f_out, h->L = L, h->M = M;
    design(L, M, &h->P, h->c);
    const int P = h->P;
    if ((size_t)L * P * 4 > 128 * 1024) {
        mio::set_error("resampler_create: %d Hz from %d Hz needs a phase table of %zu bytes (over 128 KB)", f_out,
                       f_in, (size_t)L * P * 4);
        delete h;
        return MIO_ERR_UNSUPPORTED;
    }
    // row stride: the least-colliding one in [P, P + 64) that leaves LDS for a full tile; then
    // the largest tile that fits beside the table (a full one unless stride P itself is too wide)
    long long best = -1;
    for (int cs = P; cs < P + kBanks; ++cs) {
        const int words = (L * cs + 3) & ~3;
        if (cs > P && mio::resample_lds_bytes(words, L, M, P, mio::RS_NT_MAX) + mio::RS_LDS_STATIC > (size_t)mio::RS_LDS_MAX) break;
        const long long cost = L > 1 ? stride_cost(L, M, cs) : 0;
        if (best < 0 || cost < best) best = cost, h->cs = cs;
    }
    h->tab_words = (L * h->cs + 3) & ~3;
    for (h->nt = mio::RS_NT_MAX; h->nt > 64; h->nt /= 2)
        if (mio::resample_lds_bytes(h->tab_words, L, M, P, h->nt) + mio::RS_LDS_STATIC <= (size_t)mio::RS_LDS_MAX) break;
    if (mio::resample_lds_bytes(h->tab_words, L, M, P, h->nt) + mio::RS_LDS_STATIC > (size_t)mio::RS_LDS_MAX) {
        mio::set_error("resampler_create: %d Hz from %d Hz does not fit the LDS", f_out, f_in);
        delete h;
        return MIO_ERR_UNSUPPORTED;
    }
    if (d) {
        std::vector<float> img((size_t)h->tab_words, 0.0f);  // tap order: column t holds c[phi][P - 1 - t]
        for (int phi = 0; phi < L; ++phi)
            for (int t = 0; t < P; ++t) img[(size_t)phi * h->cs + t] = h->c[(size_t)phi * P + (P - 1 - t)];
        // each step leaves its own error text (MIO_HIP_CHECK); the handle is freed on any failure
        const int rc = [&]() -> int {
            int r = mio::bind(d);
            if (r || (r = mio::resample_prepare())) return r;
            MIO_HIP_CHECK(hipMalloc((void **)&h->d_table, img.size() * 4));
            MIO_HIP_CHECK(hipMalloc((void **)&h->d_hist, (size_t)2 * P * 4));
            MIO_HIP_CHECK(hipMalloc((void **)&h->d_part, (mio::RS_MAX_PARTS + 1) * 4));
            MIO_HIP_CHECK(hipMemcpy(h->d_table, img.data(), img.size() * 4, hipMemcpyHostToDevice));
            return MIO_OK;
        }();
        if (rc) {
            mio_hip_resampler_destroy(h);
            return rc;
        }
    }
    *out = h;
    return MIO_OK;
}

extern "C" void mio_hip_resampler_destroy(mio_hip_resampler *h) {
    if (!h) return;
    if (h->d) {
        hipSetDevice(h->dev);  // hipFree waits for the device: no launch still reads these
        if (h->d_table) hipFree(h->d_table);
        if (h->d_hist) hipFree(h->d_hist);
        if (h->d_part) hipFree(h->d_part);
    }
    delete h;
}

extern "C" int mio_hip_resampler_info(const mio_hip_resampler *h, int *info) {
    MIO_REQUIRE(h && info, MIO_ERR_INVALID, "resampler_info: null");
    info[0] = h->L, info[1] = h->M, info[2] = h->P, info[3] = h->P / 2, info[4] = h->nt;
    return MIO_OK;
}

extern "C" int mio_hip_resampler_coeffs(const mio_hip_resampler *h, float *out, int cap) {
    MIO_REQUIRE(h && out && cap >= (int)h->c.size(), MIO_ERR_INVALID, "resampler_coeffs: null or short buffer");
    std::copy(h->c.begin(), h->c.end(), out);
    return MIO_OK;
}

extern "C" int mio_hip_resampler_reset(mio_hip_resampler *h) {
    MIO_REQUIRE(h, MIO_ERR_INVALID, "resampler_reset: null");
    h->seen = h->out_next = 0;
    return MIO_OK;
}

namespace {

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

int grid_of(const mio_hip_resampler *h, long long n_out) {
    // one resident workgroup per compute unit holds the table; more only re-stage it
    return (int)std::clamp<long long>(ceil_div(n_out, h->nt), 1, std::max(1, h->d->n_cu));
}

int check_run(const mio_hip_resampler *h, const float *in, int64_t n, const void *o32, const void *o16,
              const int64_t *n_out, const char *who) {
    MIO_REQUIRE(h && n_out && n >= 0, MIO_ERR_INVALID, "%s: bad argument", who);
    MIO_REQUIRE(h->d, MIO_ERR_INVALID, "%s: a design-only handle (created without a device) runs nothing", who);
    MIO_REQUIRE((o32 != nullptr) != (o16 != nullptr), MIO_ERR_INVALID, "%s: exactly one output buffer", who);
    MIO_REQUIRE(in || n == 0, MIO_ERR_INVALID, "%s: null input", who);
    // sample counts stay far below 2^63 / M: n M is formed in 64 bits on the device
    MIO_REQUIRE(n < (1LL << 40), MIO_ERR_INVALID, "%s: %lld samples", who, (long long)n);
    return MIO_OK;
}

}  // namespace

extern "C" int mio_hip_resample(mio_hip_resampler *h, const float *in, int64_t n, float gain, float *out_f32,
                                int16_t *out_pcm16, int64_t out_cap, int64_t *n_out, int flush, void *stream) {
    int rc = check_run(h, in, n, out_f32, out_pcm16, n_out, "resample");
    if (rc) return rc;
    const long long total = h->seen + n;
    MIO_REQUIRE(total < (1LL << 40), MIO_ERR_INVALID, "resample: stream of %lld samples", total);
    // output m is complete once input floor(m M / L) + P/2 has been seen
    long long end = flush ? ceil_div(total * h->L, h->M)
                          : (total > h->P / 2 ? ceil_div((total - h->P / 2) * h->L, h->M) : 0);
    end = std::max(end, h->out_next);
    const long long cnt = end - h->out_next;
    MIO_REQUIRE(cnt <= out_cap, MIO_ERR_INVALID, "resample: %lld outputs for a buffer of %lld", cnt,
                (long long)out_cap);
    *n_out = cnt;
    if (n > 0 || cnt > 0) {
        if ((rc = mio::bind(h->d))) return rc;
        mio::RsArgs a{};
        a.in = in, a.n_in = n, a.seen = h->seen;
        a.hist = h->d_hist + (size_t)h->hist_cur * h->P;
        a.hist_next = flush ? nullptr : h->d_hist + (size_t)(h->hist_cur ^ 1) * h->P;
        a.out0 = h->out_next, a.n_out = cnt;
        a.table = h->d_table, a.tab_words = h->tab_words;
        a.L = h->L, a.M = h->M, a.P = h->P, a.cs = h->cs;
        a.gain = gain;
        a.out = out_f32 ? (void *)out_f32 : (void *)out_pcm16;
        if ((rc = mio::resample_launch(a, out_pcm16 != nullptr, grid_of(h, cnt), h->nt, mio::pick_stream(h->d, stream))))
            return rc;
        if (!flush) h->hist_cur ^= 1;
    }
    h->seen = flush ? 0 : total;
    h->out_next = flush ? 0 : end;
    return MIO_OK;
}

extern "C" int mio_hip_pcm_finish_rate(mio_hip_resampler *h, const float *samples, int64_t n, int normalize,
                                       float *out_f32, int16_t *out_pcm16, int64_t out_cap, int64_t *n_out,
                                       float *peak, void *stream) {
    int rc = check_run(h, samples, n, out_f32, out_pcm16, n_out, "pcm_finish_rate");
    if (rc) return rc;
    const long long cnt = ceil_div((long long)n * h->L, h->M);
    MIO_REQUIRE(cnt <= out_cap, MIO_ERR_INVALID, "pcm_finish_rate: %lld outputs for a buffer of %lld", cnt,
                (long long)out_cap);
    *n_out = cnt;
    if (peak) *peak = 0.0f;
    if (n == 0) return MIO_OK;
    MIO_REQUIRE(((uintptr_t)samples & 15) == 0, MIO_ERR_INVALID, "pcm_finish_rate: samples must be 16-byte aligned");
    if ((rc = mio::bind(h->d))) return rc;
    hipStream_t s = mio::pick_stream(h->d, stream);
    mio::RsArgs a{};
    a.in = samples, a.n_in = n, a.n_out = cnt;
    a.table = h->d_table, a.tab_words = h->tab_words;
    a.L = h->L, a.M = h->M, a.P = h->P, a.cs = h->cs;
    a.gain = 1.0f;
    if (normalize) {
        if ((rc = mio::pcm_peak_launch(samples, n, h->d_part, &a.n_parts, s))) return rc;
        a.part = h->d_part;
        a.peak_out = peak ? h->d_part + mio::RS_MAX_PARTS : nullptr;
    }
    a.out = out_f32 ? (void *)out_f32 : (void *)out_pcm16;
    if ((rc = mio::resample_launch(a, out_pcm16 != nullptr, grid_of(h, cnt), h->nt, s))) return rc;
    if (a.peak_out) {
        MIO_HIP_CHECK(hipMemcpyAsync(peak, a.peak_out, sizeof(float), hipMemcpyDeviceToHost, s));
        MIO_HIP_CHECK(hipStreamSynchronize(s));
    }
    return MIO_OK;
}
