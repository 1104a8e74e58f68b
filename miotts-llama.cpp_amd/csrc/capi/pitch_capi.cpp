// C-ABI: pitch (include/mio_hip.h, "pitch"): argument checks, the two ratios and the sizes, the
// device's workspace (prototype table + the time-scaled intermediate), the WSOLA step through
// mio_hip_pcm_speed and the launch of pcm_pitch.hip.
#include "common.h"
#include "pcm_pitch.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr long long kMaxSamples = 1LL << 30;  // mio_hip_pcm_speed's limit; positions stay far inside a double

long long len_after(long long n, float step) { return (long long)std::ceil((double)n / (double)step); }
long long quads(long long n) { return (n + 3) & ~3LL; }  // every intermediate starts 16-byte aligned

double bessel_i0(double x) {  // power series; beta is about 7.9: 40 terms are ample
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 40; ++k) {
        term *= (x / (2.0 * k)) * (x / (2.0 * k));
        sum += term;
    }
    return sum;
}

// h(i / Q), i = 0 .. Z Q: sinc(u) times the Kaiser window over [-Z, Z], in float64, rounded to f32
void design_table(std::vector<float> &tab) {
    tab.assign(mio::PT_TAB_WORDS, 0.0f);
    const double i0b = bessel_i0(mio::PT_BETA);
    for (int i = 0; i < mio::PT_TAB; ++i) {
        const double u = (double)i / mio::PT_Q, w = (double)i / (mio::PT_Z * mio::PT_Q);
        const double sinc = i == 0 ? 1.0 : std::sin(M_PI * u) / (M_PI * u);
        tab[i] = (float)(sinc * bessel_i0(mio::PT_BETA * std::sqrt(1.0 - w * w)) / i0b);
    }
}

// the table, then `floats` of intermediate. Growing frees the old block (hipFree waits for the
// device, so no launch still reads it); a call inside the reserved size allocates nothing.
int ensure_ws(mio_hip_device *d, long long floats) {
    if (d->pitch_ws && d->pitch_floats >= floats) return MIO_OK;
    floats = std::max(floats, 2 * d->pitch_floats);
    if (d->pitch_ws) MIO_HIP_CHECK(hipFree(d->pitch_ws));
    d->pitch_ws = nullptr, d->pitch_floats = 0;
    const size_t bytes = sizeof(float) * ((size_t)mio::PT_TAB_WORDS + (size_t)floats);
    if (hipMalloc(&d->pitch_ws, bytes) != hipSuccess) {
        d->pitch_ws = nullptr;
        mio::set_error("pcm_pitch: workspace of %zu bytes failed", bytes);
        return MIO_ERR_OOM;
    }
    std::vector<float> tab;
    design_table(tab);
    MIO_HIP_CHECK(hipMemcpy(d->pitch_ws, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    d->pitch_floats = floats;
    return MIO_OK;
}

}  // namespace

extern "C" int mio_hip_pcm_pitch_reserve(mio_hip_device *d, int64_t n_max) {
    MIO_REQUIRE(d && n_max >= 0 && n_max <= kMaxSamples, MIO_ERR_INVALID, "pcm_pitch_reserve: bad argument");
    int rc = mio_hip_pcm_speed_reserve(d, n_max);
    if (rc) return rc;
    return ensure_ws(d, quads(2 * n_max) + 4 * mio::PT_MAX_B);
}

extern "C" int mio_hip_pcm_pitch(mio_hip_device *d, const float *const *in, const int64_t *n, int B, float speed,
                                 float semitones, float *const *out, const int64_t *out_cap, int64_t *n_out,
                                 void *stream) {
    MIO_REQUIRE(d && in && n && out && out_cap && n_out, MIO_ERR_INVALID, "pcm_pitch: null argument");
    MIO_REQUIRE(B >= 1 && B <= mio::PT_MAX_B, MIO_ERR_INVALID, "pcm_pitch: %d utterances (1 to %d)", B,
                mio::PT_MAX_B);
    MIO_REQUIRE(semitones >= -12.0f && semitones <= 12.0f, MIO_ERR_UNSUPPORTED,
                "pcm_pitch: %g semitones is not supported (-12 to 12)", (double)semitones);
    const float r = (float)std::exp2((double)semitones / 12.0);
    if (r == 1.0f) return mio_hip_pcm_speed(d, in, n, B, speed, out, out_cap, n_out, nullptr, stream);
    const float s1 = speed / r;
    MIO_REQUIRE(s1 >= 0.5f && s1 <= 2.0f, MIO_ERR_UNSUPPORTED,
                "pcm_pitch: speed %g at %g semitones needs a time-scale of %g, which is not supported (0.5 to 2.0)",
                (double)speed, (double)semitones, (double)s1);
    const bool scale = s1 != 1.0f;
    std::vector<int64_t> mid_n((size_t)B), mid_cap((size_t)B);
    long long mid_total = 0, tiles = 0;
    for (int b = 0; b < B; ++b) {
        MIO_REQUIRE(n[b] >= 0 && n[b] <= kMaxSamples && (in[b] || n[b] == 0), MIO_ERR_INVALID,
                    "pcm_pitch: utterance %d: %lld samples%s", b, (long long)n[b], in[b] ? "" : " at a null pointer");
        mid_n[b] = scale ? len_after(n[b], s1) : n[b];
        mid_cap[b] = quads(mid_n[b]);
        const long long no = len_after(mid_n[b], r);
        MIO_REQUIRE(out_cap[b] >= no && (out[b] || no == 0), MIO_ERR_INVALID,
                    "pcm_pitch: utterance %d: %lld outputs for a buffer of %lld", b, no, (long long)out_cap[b]);
        if (scale) mid_total += mid_cap[b];
        tiles = std::max(tiles, (no + mio::PT_TILE - 1) / mio::PT_TILE);
    }
    int rc;
    if ((rc = mio::bind(d)) || (rc = ensure_ws(d, mid_total))) return rc;
    float *ws = static_cast<float *>(d->pitch_ws);
    mio::PtArgs a{};
    a.table = ws;
    a.r = r, a.c = r > 1.0f ? 1.0f / r : 1.0f, a.B = B;
    a.K = (int)std::ceil((double)mio::PT_Z / (double)a.c);
    std::vector<float *> mid((size_t)B);
    float *next = ws + mio::PT_TAB_WORDS;
    for (int b = 0; b < B; ++b) {
        mid[b] = next;
        if (scale) next += mid_cap[b];
    }
    if (scale && (rc = mio_hip_pcm_speed(d, in, n, B, s1, mid.data(), mid_cap.data(), mid_n.data(), nullptr, stream)))
        return rc;
    for (int b = 0; b < B; ++b) {
        mio::PtUtt &u = a.u[b];
        u.in = scale ? mid[b] : in[b], u.out = out[b], u.n = mid_n[b];
        u.n_out = n_out[b] = len_after(mid_n[b], r);
    }
    // enough workgroups to fill the device three deep; each walks its share of an utterance's tiles
    const long long fill = std::max(1, (3 * std::max(d->n_cu, 1) + B - 1) / B);
    return mio::pitch_launch(a, (int)std::min(tiles, fill), mio::pick_stream(d, stream));
}
