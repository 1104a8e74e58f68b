// Test-support kernel (libmiotts_test.so): y = W x with x re-quantized to the vec_dot_type
// in the decode prologue's way, on the decode step's streaming matvec engine (llm_device.h),
// for mio_hip_debug_matvec's parity tests of every weight type, and the decode prologue's
// activation quantizer on its own (mio_hip_debug_act_quant).
#include "llm_device.h"

#pragma clang fp contract(off)

namespace mio {
namespace {
// NM == 2: U is the up matrix beside the gate W, y = silu(W x) * (U x) (the gate|up launch's
// stream of row pairs and its SwiGLU epilogue)
template <int NP, int T, int NM>
__global__ __launch_bounds__(MT) void k_debug_matvec(QMat W, QMat U, const float *x, float *y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = W.k;
    const Smem s = carve(smem, K);
    XRegs<NP> xr;
    load_x(x, nullptr, K, xr);
    int lo, hi;
    wave_range(W.rows, lo, hi, blockIdx.x, gridDim.x);
    Frag ga[Cfg<NP>::U], gb[Cfg<NP>::U];
    load_first<T, NP, NM>(W, U, lo, hi, ga, gb);
    plain_quant(xr, K, akind(T), s);
    stream_rows_lanes<T, NP, NM>(W, U, lo, hi, ga, gb, s.a, [&](int row, float v, float u) {
        y[row] = NM == 2 ? silu_f(v) * u : v;
    });
}

// The same on the product's single-group row stream (SU units per wave, issued as one group
// before the prologue: the form the decode step's q|k|v, O, gate|up and down launches run), the
// host having checked that no wave of the grid owns more than SU units.
template <int NP, int T, int NM, int SU>
__global__ __launch_bounds__(MT) void k_debug_matvec_group(QMat W, QMat U, const float *x, float *y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int K = W.k;
    const Smem s = carve(smem, K);
    XRegs<NP> xr;
    load_x(x, nullptr, K, xr);
    int lo, hi;
    wave_range(W.rows, lo, hi, blockIdx.x, gridDim.x);
    Frag ga[Cfg<NP, SU>::U], gb[Cfg<NP, SU>::U];
    load_first<T, NP, NM, SU>(W, U, lo, hi, ga, gb);
    plain_quant(xr, K, akind(T), s);
    stream_rows_lanes<T, NP, NM, SU>(W, U, lo, hi, ga, gb, s.a, [&](int row, float v, float u) {
        y[row] = NM == 2 ? silu_f(v) * u : v;
    });
}

// One workgroup runs the decode prologue's quantizer (rmsnorm_quant when w is given, else
// plain_quant; SC1: the sc1 activation loads of the in-launch hand-offs) on x[K] and copies the
// LDS record {qs | d | bs} (smem_bytes(K) - 128 bytes, the unwritten parts undefined) to out.
template <int NP, int T, int XAUX>
__global__ __launch_bounds__(MT) void k_debug_act_quant(const float *x, const float *w, int K, float eps,
                                                        uint32_t *out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Smem s = carve(smem, K);
    XRegs<NP> xr;
    load_x<NP, XAUX>(x, w, K, xr);
    if (w)
        rmsnorm_quant(xr, K, eps, akind(T), s);
    else
        plain_quant(xr, K, akind(T), s);
    const int n = (int)((smem_bytes(K) - 128) / 4);
    for (int i = MIO_TIDX; i < n; i += MT) out[i] = reinterpret_cast<const uint32_t *>(smem)[i];
}
}  // namespace

size_t debug_act_record_bytes(int K) { return smem_bytes(K) - 128; }

void launch_debug_act_quant(int type, const float *x, const float *w, int K, float eps, bool sc1, void *out,
                            hipStream_t s) {
    dispatch_nt(K, type, [&]<int NP, int T>() {
        if (sc1)
            hipLaunchKernelGGL((k_debug_act_quant<NP, T, 16>), dim3(1), dim3(MT), matvec_lds(K), s, x, w, K, eps,
                               (uint32_t *)out);
        else
            hipLaunchKernelGGL((k_debug_act_quant<NP, T, 0>), dim3(1), dim3(MT), matvec_lds(K), s, x, w, K, eps,
                               (uint32_t *)out);
    });
}

void launch_debug_matvec(const QMat &W, const QMat *up, const float *x, float *y, int n_wg, hipStream_t s) {
    LlmDims d{};
    d.n_wg = n_wg;
    dispatch_nt(W.k, W.type, [&]<int NP, int T>() {
        if (up)
            hipLaunchKernelGGL((k_debug_matvec<NP, T, 2>), dim3(matvec_grid(d, W.rows)), dim3(MT), matvec_lds(W.k), s,
                               W, *up, x, y);
        else
            hipLaunchKernelGGL((k_debug_matvec<NP, T, 1>), dim3(matvec_grid(d, W.rows)), dim3(MT), matvec_lds(W.k), s,
                               W, W, x, y);
    });
}

// The single-group sizes the decode step launches (dispatch_su), SU even for row pairs. False:
// no such instantiation, or a wave of the grid would own more than su units.
bool launch_debug_matvec_group(const QMat &W, const QMat *up, const float *x, float *y, int su, int grid,
                               hipStream_t s) {
    const int np = pick_np(W.k), nm = up ? 2 : 1;
    if (grid < 1 || np > 3) return false;
    for (int b = 0; b < grid; ++b) {  // wave_range's shares
        const int ra = (int)((long long)W.rows * b / grid), rb = (int)((long long)W.rows * (b + 1) / grid);
        for (int w = 0; w < MW; ++w)
            if (((rb - ra) * (w + 1) / MW - (rb - ra) * w / MW) * np * nm > su) return false;
    }
    bool ok = false;
    dispatch_nt(W.k, W.type, [&]<int NP, int T>() {
        auto go = [&]<int NM, int SU>() {
            hipLaunchKernelGGL((k_debug_matvec_group<NP, T, NM, SU>), dim3(grid), dim3(MT), matvec_lds(W.k), s, W,
                               up ? *up : W, x, y);
            ok = true;
        };
        if constexpr (NP == 1) {
            if (nm == 1 && su == 2) go.template operator()<1, 2>();
            if (nm == 1 && su == 3) go.template operator()<1, 3>();
            if (nm == 1 && su == 4) go.template operator()<1, 4>();
            if (nm == 1 && su == 6) go.template operator()<1, 6>();
            if (nm == 2 && su == 2) go.template operator()<2, 2>();
            if (nm == 2 && su == 4) go.template operator()<2, 4>();
            if (nm == 2 && su == 6) go.template operator()<2, 6>();
        } else if constexpr (NP == 3) {
            if (nm == 1 && su == 3) go.template operator()<1, 3>();
        }
    });
    return ok;
}

}  // namespace mio
