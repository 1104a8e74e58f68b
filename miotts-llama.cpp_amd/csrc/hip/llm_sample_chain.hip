// The sampler chain of the decode step (the llama.cpp sampler order the reference could be
// given in place of its temp + dist pair, test-to-speech.cpp:127-130): repetition / frequency /
// presence penalties -> top-k -> top-p -> min-p -> temperature -> draw, as ONE launch between
// the lm_head launches and whatever reduces their sampling partials (the next step's layer-0
// k_attn_in, the flush k_sample, k_bt_sample). One workgroup per stream.
//
// The launch reads the stream's logits row over the window [lo, hi), the last repeat_last_n
// tokens this generate sampled (cfg.out_tokens[first_step .. step)), and overwrites the
// stream's sampling partials: partial 0 = {winning value, winning id}, every other partial
// {-inf, INT_MAX}. The reducers stay as they are and pick that id.
//
// Total order of the ids: penalised logit l' descending, then id ascending. Every truncation
// keeps a prefix of it, written as a cut (ck, r): an id is kept iff key(l') > ck, or key(l') ==
// ck and fewer than r ids of that value precede it (key = the order-preserving integer image of
// the f32). Passes over the row (each wave owns a contiguous segment, so "ids that precede" is
// wave, then iteration, then lane):
//   penalties   the <= 256 history ids, in place in the logits row (the bits are put back at the
//               end: the row stays the model's output)
//   load        a window of at most 13 * 1024 ids (the speech ids) stays in registers from here on
//   max         l'_max (top-p, min-p)
//   top-k       radix select by count, 8-bit digits from the top: 4 passes, LDS histograms
//   top-p       radix select by mass over the top-k survivors: 4 passes. The mass of an id is
//               the INTEGER floor(expf(l' - l'_max) * 2^40), accumulated with integer LDS
//               atomics: sums are exact and the same whatever order the waves arrive in (no
//               floating-point atomics, no order-dependent rounding). Z <= 2^18 ids * 2^40.
//   min-p       one threshold key, no pass
//   ties        ids equal to the cut value per wave (only where the cut splits a run of equals)
//   draw        Gumbel argmax over the kept ids (the lm_head kernels' expression), kept count,
//               cut id
#include "llm_device.h"

#pragma clang fp contract(off)

namespace mio {
namespace {

constexpr int CT = 1024, CW = CT / 64;  // threads, waves
constexpr int kRep = 8;                 // histogram replicas (lane & 7): a hot digit's atomics spread over 8 words
constexpr uint32_t kAllTies = 0xFFFFFFFFu;
typedef unsigned long long u64;

struct ChainLds {
    uint32_t hc[kRep][256];
    u64 hm[kRep][256];
    uint32_t c0[256];
    u64 m0[256];
    int hid[kChainHistMax];
    uint32_t horig[kChainHistMax];
    int hown[kChainHistMax];
    float rf[CW];
    int ri[CW];
    uint32_t ru[CW], wties[CW];
    u64 rq[CW];
    uint32_t sel_d, sel_n, cnt_gt;
    u64 mass_gt, target, total;
};

// larger float <-> larger key; -0 counts as +0 (they compare equal)
__device__ __forceinline__ uint32_t order_key(float l) {
    const uint32_t u = __float_as_uint(l + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// floor(exp(l - lmax) * 2^40): 2^40 for the maximum itself (also where it is -inf)
__device__ __forceinline__ u64 mass_of(float l, float lmax) {
    const float d = l == lmax ? 0.0f : l - lmax;
    return (u64)(expf(d) * 1099511627776.0f);
}

// The penalties on one logit, every operation a rounded f32 one in this order. Plain operators
// under this file's `fp contract(off)`: hipcc contracts a * b + c across statements by default,
// and the __fmul_rn / __fadd_rn wrappers are plain operators of a header compiled without the
// pragma, which the backend fuses all the same.
__device__ __forceinline__ float penalised(float l, float c, float rep, float freq, float pres) {
    const float a = l > 0.0f ? l / rep : l * rep;
    const float b = c * freq;
    const float s = b + pres;
    return a - s;
}

// f(i, l, ok) for every id i of the row, 4 loads in flight per lane; every lane of a wave makes
// the same calls (ok = the id exists), so f may ballot
// REG: the window has at most kRegIds * CT ids (the 12,800 speech ids do) and every thread
// keeps its kRegIds values of the penalised row in registers, so only the first of the ten or
// so passes goes to memory; wider windows (a whole vocabulary) read the row from L2 every pass.
constexpr int kRegIds = 13;  // 13 * 1024 = 13,312 ids: the speech window, with room
template <bool REG>
struct Row {
    const float *p;
    int n;
    float v[REG ? kRegIds : 1];
};

template <bool REG, class F>
__device__ __forceinline__ void sweep(const Row<REG> &r, F f) {
    const int lane = MIO_TIDX & 63, wave = MIO_TIDX >> 6;
    const int S = ((r.n + CW - 1) / CW + 63) & ~63;
    const int b = wave * S, e = min(b + S, r.n);
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < kRegIds; ++k)
            if (b + 64 * k < e) f(b + 64 * k + lane, r.v[k], b + 64 * k + lane < e);
    } else {
        for (int i0 = b; i0 < e; i0 += 256) {
            float l[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) l[u] = r.p[min(i0 + 64 * u + lane, e - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) f(i0 + 64 * u + lane, l[u], i0 + 64 * u + lane < e);
        }
    }
}

// the thread's values of the (penalised) row: all loads in flight at once
template <bool REG>
__device__ __forceinline__ void load_row(Row<REG> &r) {
    if constexpr (REG) {
        const int lane = MIO_TIDX & 63, wave = MIO_TIDX >> 6;
        const int S = ((r.n + CW - 1) / CW + 63) & ~63;
        const int b = wave * S, e = min(b + S, r.n);
#pragma unroll
        for (int k = 0; k < kRegIds; ++k) r.v[k] = b + 64 * k < e ? r.p[min(b + 64 * k + lane, e - 1)] : 0.0f;
    }
}

struct Cut {
    uint32_t ck, n_ck, cnt_gt;  // the selected value's key, ids of that value, ids above it
    u64 mass_gt, target;        // mass above it; the mass target (by_mass)
};

// Radix select over the keys, 8-bit digits from the top. by_mass false: the value holding the
// K-th id of the order. by_mass true: the value at which the mass of the ids before it first
// reaches max(1, floor(p * total)). has_k: only the top-k survivors count, ids above ck_k and
// r_k ids of the value ck_k itself. Whole workgroup; every thread returns the same Cut.
template <bool REG>
__device__ Cut descend(ChainLds &L, const Row<REG> &row, float lmax, bool by_mass, uint32_t K, float p, bool has_k,
                       uint32_t ck_k, uint32_t r_k) {
    const int tid = MIO_TIDX, lane = tid & 63;
    uint32_t prefix = 0, mask = 0, cnt_gt = 0, n_ck = 0;
    u64 mass_gt = 0, target = K;
    const u64 q_k = has_k && by_mass ? mass_of(key_value(ck_k), lmax) : 0;
    for (int lvl = 0; lvl < 4; ++lvl) {
        const int shift = 24 - 8 * lvl;
        for (int i = tid; i < kRep * 256; i += CT) (&L.hc[0][0])[i] = 0, (&L.hm[0][0])[i] = 0;
        __syncthreads();
        const int rep = tid & (kRep - 1);
        sweep(row, [&](int, float l, bool ok) {
            const uint32_t key = order_key(l);
            if (ok && (key & mask) == prefix && (!has_k || key > ck_k)) {
                const uint32_t dg = (key >> shift) & 255u;
                atomicAdd(&L.hc[rep][dg], 1u);
                if (by_mass) atomicAdd(&L.hm[rep][dg], mass_of(l, lmax));
            }
        });
        __syncthreads();
        if (tid < 256) {
            uint32_t c = 0;
            u64 m = 0;
            for (int r = 0; r < kRep; ++r) c += L.hc[r][tid], m += L.hm[r][tid];
            if (has_k && (ck_k & mask) == prefix && ((ck_k >> shift) & 255u) == (uint32_t)tid) c += r_k, m += r_k * q_k;
            L.c0[tid] = c, L.m0[tid] = m;
        }
        __syncthreads();
        if (tid < 64) {
            // lane: digits 255 - 4 lane - j, j = 0..3 (lanes ascending = digits descending)
            uint32_t c[4], sc = 0;
            u64 m[4], sm = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = L.c0[255 - 4 * lane - j], m[j] = L.m0[255 - 4 * lane - j];
                sc += c[j], sm += m[j];
            }
            uint32_t ic = sc;
            u64 im = sm;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t tc = __shfl_up(ic, o);
                const u64 tm = __shfl_up(im, o);
                if (lane >= o) ic += tc, im += tm;
            }
            if (lvl == 0 && by_mass) {
                const u64 total = __shfl(im, 63);
                target = (u64)((double)p * (double)total);
                target = target < 1 ? 1 : target;
            }
            const u64 incl = by_mass ? mass_gt + im : (u64)cnt_gt + ic;
            const u64 hits = __ballot(incl >= target);
            const u64 some = __ballot(sc > 0);
            // no bucket reaches the target (cannot happen for a target <= the total): the last id
            const int sel = hits ? __ffsll((long long)hits) - 1 : (some ? 63 - __clzll((long long)some) : 0);
            if (lane == sel) {
                uint32_t rc = cnt_gt + (ic - sc);
                u64 rm = mass_gt + (im - sm);
                int js = -1;
                uint32_t cn = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u64 cum = by_mass ? rm + m[j] : (u64)rc + c[j];
                    bool take = hits ? cum >= target : false;
                    if (!hits) {  // the lowest digit of this lane that has ids
                        take = c[j] > 0;
#pragma unroll
                        for (int jj = j + 1; jj < 4; ++jj) take = take && c[jj] == 0;
                    }
                    take = (take || j == 3) && js < 0;
                    if (take)
                        js = j, cn = c[j];
                    else if (js < 0)
                        rc += c[j], rm += m[j];
                }
                L.sel_d = 255 - 4 * lane - js, L.sel_n = cn, L.cnt_gt = rc, L.mass_gt = rm, L.target = target;
            }
        }
        __syncthreads();
        prefix |= L.sel_d << shift, mask |= 255u << shift;
        cnt_gt = L.cnt_gt, mass_gt = L.mass_gt, target = L.target, n_ck = L.sel_n;
    }
    return Cut{prefix, n_ck, cnt_gt, mass_gt, target};
}

// Everything after the penalties: the cut, the draw over the kept ids, the partials, and the row's
// own bits back. grow: the stream's window of the logits row (penalised in place).
template <bool REG>
__device__ __forceinline__ void cut_and_draw(const ChainArgs &a, ChainLds &L, const SampleCfg &sc, int t, int step,
                                             float *grow, int n, int hn) {
    const int tid = MIO_TIDX, lane = tid & 63, wave = tid >> 6;
    Row<REG> row;
    row.p = grow, row.n = n;
    load_row(row);
    // ---- the cut
    const bool on_k = sc.top_k > 0 && sc.top_k < n, on_p = sc.top_p < 1.0f, on_m = sc.min_p > 0.0f;
    uint32_t ck = 0, r = kAllTies;
    if (on_k || on_p || on_m) {
        uint32_t kmax = 0;
        sweep(row, [&](int, float l, bool ok) { kmax = ok ? max(kmax, order_key(l)) : kmax; });
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o));
        if (lane == 0) L.ru[wave] = kmax;
        __syncthreads();
        for (int w = 0; w < CW; ++w) kmax = max(kmax, L.ru[w]);
        __syncthreads();
        const float lmax = key_value(kmax);
        uint32_t r_k = 0;
        if (on_k) {
            const Cut c = descend(L, row, lmax, false, (uint32_t)sc.top_k, 0.0f, false, 0, 0);
            ck = c.ck, r = r_k = (uint32_t)sc.top_k - c.cnt_gt;
            if (r >= c.n_ck) r = kAllTies, r_k = c.n_ck;
        }
        if (on_p) {
            const Cut c = descend(L, row, lmax, true, 0, fmaxf(sc.top_p, 0.0f), on_k, ck, r_k);
            const u64 q = mass_of(key_value(c.ck), lmax);
            const u64 need = c.target - c.mass_gt;  // > 0: the first id of this value is kept
            const u64 rp = q ? (need + q - 1) / q : (u64)c.n_ck;
            // a prefix of the survivors (c.n_ck counts survivors): never looser than the top-k cut
            if (c.ck > ck)
                ck = c.ck, r = rp >= c.n_ck ? kAllTies : (uint32_t)rp;
            else if (rp < c.n_ck)
                r = (uint32_t)rp;
        }
        if (on_m) {
            const uint32_t km = order_key(lmax + logf(sc.min_p));
            if (km > kmax)  // min_p > 1: no id passes, the first id of the order stays
                ck = kmax, r = 1;
            else if (km > ck)
                ck = km, r = kAllTies;
        }
    }

    // ---- ids of the cut value per wave (where the cut splits a run of equals)
    uint32_t tie_base = 0;
    if (r != kAllTies) {
        uint32_t cnt = 0;
        sweep(row, [&](int, float l, bool ok) { cnt += __popcll(__ballot(ok && order_key(l) == ck)); });
        if (lane == 0) L.wties[wave] = cnt;
        __syncthreads();
        for (int w = 0; w < wave; ++w) tie_base += L.wties[w];
    }

    // ---- draw over the kept ids; kept count; the last kept id of the order
    const uint64_t seed = ((uint64_t)sc.seed_hi << 32) | sc.seed_lo;
    float best = -INFINITY;
    int bi = INT_MAX;
    uint32_t kept = 0, seen = tie_base;
    u64 last = ~0ull;  // min of (key, ~id)
    sweep(row, [&](int i, float l, bool ok) {
        const uint32_t key = order_key(l);
        const bool tie = ok && key == ck;
        bool keep = ok && key > ck;
        if (r == kAllTies) {
            keep = keep || tie;
        } else {
            const u64 bal = __ballot(tie);
            const uint32_t rank = seen + __popcll(bal & ((1ull << lane) - 1));
            seen += __popcll(bal);
            keep = keep || (tie && rank < r);
        }
        if (keep) {
            const int id = sc.lo + i;
            const float v = sc.temp > 0.0f ? l / sc.temp + gumbel(seed, step, id) : l;
            if (v > best || (v == best && id < bi)) best = v, bi = id;
            ++kept;
            const u64 pk = ((u64)key << 32) | (uint32_t)~(uint32_t)id;
            last = pk < last ? pk : last;
        }
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
        kept += __shfl_xor((int)kept, o);
        const u64 ol = __shfl_xor(last, o);
        last = ol < last ? ol : last;
    }
    if (lane == 0) L.rf[wave] = best, L.ri[wave] = bi, L.ru[wave] = kept, L.rq[wave] = last;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CW; ++w) {
            if (L.rf[w] > best || (L.rf[w] == best && L.ri[w] < bi)) best = L.rf[w], bi = L.ri[w];
            kept += L.ru[w];
            last = L.rq[w] < last ? L.rq[w] : last;
        }
        if (a.dbg) a.dbg[3 * t] = (int)kept, a.dbg[3 * t + 1] = (int)~(uint32_t)last, a.dbg[3 * t + 2] = 1;
        L.rf[0] = best, L.ri[0] = bi;
    }
    __syncthreads();
    best = L.rf[0], bi = L.ri[0];
    float *smp = a.smp + (size_t)t * a.nblk * 2;
    for (int i = tid; i < a.nblk; i += CT) {
        smp[2 * i] = i == 0 ? best : -INFINITY;
        smp[2 * i + 1] = __int_as_float(i == 0 ? bi : INT_MAX);
    }
    // the row goes back to the model's logits (a.keep: the penalised row stays, parity entry)
    if (hn > 0 && !a.keep && tid < hn && L.hown[tid]) grow[L.hid[tid] - sc.lo] = __uint_as_float(L.horig[tid]);
}

__global__ __launch_bounds__(CT) void k_sample_chain(ChainArgs a) {
    __shared__ ChainLds L;
    const int t = blockIdx.x, tid = MIO_TIDX, lane = tid & 63, wave = tid >> 6;
    const SampleCfg sc = a.cfg[t];
    const StepState *st = a.st + t;
    const int step = st->step;
    // as the neighbouring launches: nothing after an end token or past the step budget; a forced
    // step keeps the lm_head partials (the reducer overrides them)
    if (st->done || step >= sc.max_steps || step < sc.first_step) return;
    if (sc.force && step < sc.n_force && sc.force[step] >= 0) return;
    const int n = sc.hi - sc.lo;
    if (n <= 0) return;
    float *row = a.logits + (size_t)t * a.stride + sc.lo;

    // ---- penalties: history entry j is owned by the first thread that holds its id
    int hn = min(min(sc.repeat_last_n, kChainHistMax), step - sc.first_step);
    if (sc.repeat_penalty == 1.0f && sc.frequency_penalty == 0.0f && sc.presence_penalty == 0.0f) hn = 0;
    if (hn > 0) {
        if (tid < hn) L.hid[tid] = sc.out_tokens[step - hn + tid];
        __syncthreads();
        if (tid < hn) {
            const int id = L.hid[tid];
            int c = 0;
            bool own = id >= sc.lo && id < sc.hi;
            for (int i = 0; i < hn; ++i) {
                const bool eq = L.hid[i] == id;
                c += eq;
                own = own && !(eq && i < tid);
            }
            L.hown[tid] = own;
            if (own) {
                const float l = row[id - sc.lo];
                L.horig[tid] = __float_as_uint(l);
                row[id - sc.lo] = penalised(l, (float)c, sc.repeat_penalty, sc.frequency_penalty, sc.presence_penalty);
            }
        }
        __threadfence_block();
        __syncthreads();
    }

    if (n <= kRegIds * CT)
        cut_and_draw<true>(a, L, sc, t, step, row, n, hn);
    else
        cut_and_draw<false>(a, L, sc, t, step, row, n, hn);
}

}  // namespace

void launch_sample_chain(const ChainArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_sample_chain, dim3(B), dim3(CT), 0, s, a);
}

}  // namespace mio
