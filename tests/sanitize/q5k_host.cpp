// Q5_K on the host under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sanitize_q5k.py):
// quantize_row_q5_K, dequantize_row and the split-layout re-pack (split_layout / to_split) of the
// product's own quant.cpp on rows of one and nine superblocks, one and 37 rows. Every buffer is
// allocated at its exact size, so a byte read or written past a plane is a report. Also checks
// what the planes must hold: the nibbles and the fifth-bit plane byte for byte, the header's
// re-packed scales against get_scale_min_k4, and that the layout has GGUF's bytes per weight.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gguf.h"
#include "quant.h"

namespace mio {
static std::string g_err;
void set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
const char *last_error() { return g_err.c_str(); }
}  // namespace mio

static int fails = 0;
#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static float rnd() {  // uniform in [-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((rng_state >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

static void run(int64_t R, int64_t K) {
    using namespace mio;
    const size_t rb = ggml_row_bytes(GGML_Q5_K, K);
    EXPECT(rb == (size_t)(K / 256) * sizeof(BlockQ5_K));
    std::vector<float> x((size_t)R * K), y((size_t)R * K);
    for (float &v : x) v = 0.02f * (rnd() + rnd() + rnd());
    // an all-zero and an all-negative superblock: the d == 0 and max < 0 branches
    for (int64_t i = 0; i < 256 && R > 1; ++i) x[(size_t)K + i] = 0.0f;
    for (int64_t i = 0; i < 256; ++i) x[i] = -std::fabs(x[i]) - 0.001f;
    std::vector<uint8_t> q((size_t)R * rb);
    for (int64_t r = 0; r < R; ++r) EXPECT(quantize_row(GGML_Q5_K, x.data() + r * K, q.data() + r * rb, K));
    for (int64_t r = 0; r < R; ++r) EXPECT(dequantize_row(GGML_Q5_K, q.data() + r * rb, y.data() + r * K, K));
    double se = 0, sx = 0;
    for (size_t i = 0; i < x.size(); ++i) se += (double)(x[i] - y[i]) * (x[i] - y[i]), sx += (double)x[i] * x[i];
    EXPECT(std::sqrt(se / sx) < 0.1);
    const SplitLayout L = split_layout(GGML_Q5_K, R, K);
    EXPECT(L.bytes >= (size_t)R * rb && L.off[0] == 0 && L.off[1] >= (size_t)R * K / 2 &&
           L.off[2] >= L.off[1] + (size_t)R * K / 8 && L.bytes >= L.off[2] + (size_t)R * (K / 256) * 16);
    // same bytes per weight as GGUF: 128 + 32 + 16 per superblock
    EXPECT((size_t)R * K / 2 + (size_t)R * K / 8 + (size_t)R * (K / 256) * 16 == (size_t)R * rb);
    std::vector<uint8_t> s(L.bytes);
    EXPECT(to_split(GGML_Q5_K, q.data(), R, K, s.data()));
    for (int64_t r = 0; r < R; ++r)
        for (int64_t i = 0; i < K / 256; ++i) {
            const BlockQ5_K *b = (const BlockQ5_K *)(q.data() + r * rb) + i;
            EXPECT(!std::memcmp(s.data() + L.off[0] + (size_t)r * K / 2 + 128 * i, b->qs, 128));
            EXPECT(!std::memcmp(s.data() + L.off[1] + (size_t)r * K / 8 + 32 * i, b->qh, 32));
            const uint8_t *hd = s.data() + L.off[2] + ((size_t)r * (K / 256) + i) * 16;
            EXPECT(!std::memcmp(hd, &b->d, 2) && !std::memcmp(hd + 2, &b->dmin, 2));
            for (int j = 0; j < 8; ++j) {
                const uint8_t *sc = b->scales;
                const uint32_t d = j < 4 ? (sc[j] & 63u) : ((sc[j + 4] & 0xFu) | ((uint32_t)(sc[j - 4] >> 6) << 4));
                const uint32_t m = j < 4 ? (sc[j + 4] & 63u) : ((uint32_t)(sc[j + 4] >> 4) | ((uint32_t)(sc[j] >> 6) << 4));
                const uint8_t *p = hd + 4 + 3 * (j / 2);
                const uint32_t F = ((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16)) >> (12 * (j & 1));
                EXPECT((F & 63) == d && ((F >> 6) & 63) == m);
            }
        }
}

int main() {
    for (int64_t K : {256, 2304})
        for (int64_t R : {1, 37}) run(R, K);
    // a length that is no multiple of 256 has no Q5_K rows
    EXPECT(mio::ggml_row_bytes(mio::GGML_Q5_K, 576) == 0);
    if (fails) return 1;
    std::puts("q5k_host: clean");
    return 0;
}
