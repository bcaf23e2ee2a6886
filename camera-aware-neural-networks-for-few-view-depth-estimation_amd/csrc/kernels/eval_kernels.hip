// Offline evaluation: the twelve per-sample sums of DepthMetrics::compute
// (src/evaluation/depth_metrics.h:40-88, 147-233) in one pass over pred / gt / mask.
//
//   valid   gt > min_depth && gt < max_depth (both strict) [&& mask != 0]        (:154-161)
//   p       clamp(pred, min_depth, max_depth) when clamp_pred                     (:66); with a scale
//           alignment (eval_align_kernels.hip) the clamp is applied to scale * pred + shift
//   sums    {n, |p-g|/g, (p-g)^2/g, (p-g)^2, (ln p - ln g)^2, |p-g|, |log10 p - log10 g|,
//            #(r < 1.25), #(r < 1.25^2), #(r < 1.25^3), p, g},  r = max(p/g, g/p)  (:169-233)
//
// Per-pixel terms are fp32 (plain /, logf, log10f, as the reference's ATen ops), accumulated in double.
// Two stages without atomics: k_eval_partials writes nb partial rows per sample, k_eval_final adds them
// in index order into the evaluator's device table.  The work of a sample is split in quads of four
// consecutive pixels: quad q goes to thread q % 256 of block (q / 256) % nb, which walks its quads in
// increasing order and the four pixels of a quad in order.  The 16-byte path (float4 / uchar4 loads) and
// the scalar path share that mapping, and nb depends on H*W alone, so a sample's sums are the same bits
// on either path, in any batch, on every run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace cad {
namespace {

constexpr int kEvalSums = 12;
constexpr int kEvalThreads = 256;
constexpr int kStrataMaxBins = 16;   // CAD_STRATA_MAX_BINS

struct EvalAcc {
    double v[kEvalSums];
};

__device__ __forceinline__ void eval_pixel(EvalAcc& a, float pr, float g, bool mask_ok, float lo, float hi, int clamp_pred) {
#pragma clang fp contract(off)
    if (!(g > lo && g < hi && mask_ok)) return;
    const float p = clamp_pred ? fminf(fmaxf(pr, lo), hi) : pr;
    const float d = p - g;
    const float ad = fabsf(d);
    const float sq = d * d;
    const float ld = logf(p) - logf(g);
    const float l10 = fabsf(log10f(p) - log10f(g));
    const float r = fmaxf(p / g, g / p);
    const float t1 = 1.25f, t2 = 1.25f * 1.25f, t3 = 1.25f * 1.25f * 1.25f;   // depth_metrics.h:224
    a.v[0] += 1.0;
    a.v[1] += (double)(ad / g);
    a.v[2] += (double)(sq / g);
    a.v[3] += (double)sq;
    a.v[4] += (double)(ld * ld);
    a.v[5] += (double)ad;
    a.v[6] += (double)l10;
    a.v[7] += r < t1 ? 1.0 : 0.0;
    a.v[8] += r < t2 ? 1.0 : 0.0;
    a.v[9] += r < t3 ? 1.0 : 0.0;
    a.v[10] += (double)p;
    a.v[11] += (double)g;
}

// scale * pred + shift of an aligned evaluation: one fp32 multiply and one fp32 add
__device__ __forceinline__ float align_pred(float pr, float s, float t) {
#pragma clang fp contract(off)
    const float m = s * pr;
    return m + t;
}

// grid (nb, B), 256 threads.  VEC: HW % 4 == 0 and 16-byte (mask: 4-byte) aligned sample bases.
// ALIGN: score scale * pred + shift with the sample's row of `align` ([rows][2], row base + b).
template <bool VEC, bool ALIGN>
__global__ __launch_bounds__(kEvalThreads) void k_eval_partials(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const uint8_t* __restrict__ mask, int64_t HW, float lo,
                                                                float hi, int clamp_pred, double* __restrict__ part, int nb,
                                                                const float* __restrict__ align, int64_t base) {
    const int b = blockIdx.y;
    float as = 1.f, at = 0.f;
    if constexpr (ALIGN) {
        as = align[(base + b) * 2];
        at = align[(base + b) * 2 + 1];
    }
    const auto ap = [&](float pr) { return ALIGN ? align_pred(pr, as, at) : pr; };
    const float* ps = pred + (int64_t)b * HW;
    const float* gs = gt + (int64_t)b * HW;
    const uint8_t* ms = mask ? mask + (int64_t)b * HW : nullptr;
    const int64_t nq = (HW + 3) / 4;
    EvalAcc a;
    for (int k = 0; k < kEvalSums; ++k) a.v[k] = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * kEvalThreads + threadIdx.x; q < nq; q += (int64_t)nb * kEvalThreads) {
        const int64_t i = q * 4;
        if constexpr (VEC) {
            const float4 p4 = *reinterpret_cast<const float4*>(ps + i);
            const float4 g4 = *reinterpret_cast<const float4*>(gs + i);
            uchar4 m4 = make_uchar4(1, 1, 1, 1);
            if (ms) m4 = *reinterpret_cast<const uchar4*>(ms + i);
            eval_pixel(a, ap(p4.x), g4.x, m4.x != 0, lo, hi, clamp_pred);
            eval_pixel(a, ap(p4.y), g4.y, m4.y != 0, lo, hi, clamp_pred);
            eval_pixel(a, ap(p4.z), g4.z, m4.z != 0, lo, hi, clamp_pred);
            eval_pixel(a, ap(p4.w), g4.w, m4.w != 0, lo, hi, clamp_pred);
        } else {
            const int n = (int)(HW - i < 4 ? HW - i : 4);   // the last quad may be short
            for (int j = 0; j < n; ++j) eval_pixel(a, ap(ps[i + j]), gs[i + j], ms ? ms[i + j] != 0 : true, lo, hi, clamp_pred);
        }
    }
    __shared__ double red[kEvalThreads / 64][kEvalSums];
    for (int k = 0; k < kEvalSums; ++k) {
        double x = a.v[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kEvalSums)
        part[((int64_t)b * nb + blockIdx.x) * kEvalSums + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// grid (B), 64 threads: row base + b of the table = the sample's nb partial rows added in index order
__global__ __launch_bounds__(64) void k_eval_final(const double* __restrict__ part, int nb, double* __restrict__ table,
                                                   int64_t base) {
    const int b = blockIdx.x;
    if (threadIdx.x >= kEvalSums) return;
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[((int64_t)b * nb + i) * kEvalSums + threadIdx.x];
    table[(base + b) * kEvalSums + threadIdx.x] = s;
}

// ---------------- stratified evaluation ----------------
// The same twelve sums per sample and per stratum on two per-pixel axes (cad.h, "stratified evaluation"):
// the depth bin of gt and the bin of the pixel's ray angle off the optical axis.  One pass: a pixel's terms
// are evaluated once and go to the thread's total accumulator (the order of k_eval_partials, so the total
// row keeps its bits) and to its bin on each enabled axis.  Bins are accumulated per wave in an LDS row
// [slot][12] with a single writer (slots: depth bins, then angle bins): per trip the wave walks the distinct
// bins present among its lanes' four pixels; for each, a lane adds its pixels of that bin in pixel order,
// the wave adds the lanes with a fixed xor butterfly (lanes without such a pixel contribute 0), and lane k
// adds sum k to the row.  Waves are added in index order into the block's partial row, k_strata_final adds
// the nb partial rows in index order.  Every step is a function of the sample's pixels and of nb alone.
struct EvalTerms {
    float r[8];   // |d|/g, d^2/g, d^2, dln^2, |d|, |dlog10|, p, g
    int d1, d2, d3;
};

// eval_pixel's expressions, kept as terms
__device__ __forceinline__ bool eval_terms(EvalTerms& t, float pr, float g, bool mask_ok, float lo, float hi, int clamp_pred) {
#pragma clang fp contract(off)
    if (!(g > lo && g < hi && mask_ok)) return false;
    const float p = clamp_pred ? fminf(fmaxf(pr, lo), hi) : pr;
    const float d = p - g;
    const float ad = fabsf(d);
    const float sq = d * d;
    const float ld = logf(p) - logf(g);
    const float l10 = fabsf(log10f(p) - log10f(g));
    const float r = fmaxf(p / g, g / p);
    const float t1 = 1.25f, t2 = 1.25f * 1.25f, t3 = 1.25f * 1.25f * 1.25f;
    t.r[0] = ad / g;
    t.r[1] = sq / g;
    t.r[2] = sq;
    t.r[3] = ld * ld;
    t.r[4] = ad;
    t.r[5] = l10;
    t.r[6] = p;
    t.r[7] = g;
    t.d1 = r < t1;
    t.d2 = r < t2;
    t.d3 = r < t3;
    return true;
}

__device__ __forceinline__ void eval_add_terms(EvalAcc& a, const EvalTerms& t) {
    a.v[0] += 1.0;
    a.v[1] += (double)t.r[0];
    a.v[2] += (double)t.r[1];
    a.v[3] += (double)t.r[2];
    a.v[4] += (double)t.r[3];
    a.v[5] += (double)t.r[4];
    a.v[6] += (double)t.r[5];
    a.v[7] += t.d1 ? 1.0 : 0.0;
    a.v[8] += t.d2 ? 1.0 : 0.0;
    a.v[9] += t.d3 ? 1.0 : 0.0;
    a.v[10] += (double)t.r[6];
    a.v[11] += (double)t.r[7];
}

// number of cuts c_j <= x (a NaN x: 0)
__device__ __forceinline__ int strata_bin(const float* cuts, int m, float x) {
    int bin = 0;
    for (int j = 0; j < m; ++j) bin += cuts[j] <= x ? 1 : 0;
    return bin;
}

// rho^2 of pixel (col, row): individually rounded fp32 operations, no epsilon
__device__ __forceinline__ float strata_rho2(int col, int row, float fx, float fy, float cx, float cy) {
#pragma clang fp contract(off)
    const float x = ((float)col - cx) / fx;
    const float y = ((float)row - cy) / fy;
    const float xx = x * x;
    const float yy = y * y;
    return xx + yy;
}

// One trip's pixels of a wave into its LDS row (wrow: [bins][12] of this axis).  rem: the thread's valid
// slots (bit j = pixel j of its quad).  Must be reached by all lanes of the wave.
__device__ __forceinline__ void strata_deposit(double* wrow, const EvalTerms (&t)[4], const int (&bin)[4], unsigned rem) {
    const int lane = threadIdx.x & 63;
    unsigned long long act = __ballot(rem != 0u);
    while (act) {
        const int leader = __ffsll(act) - 1;
        int first = 0;
#pragma unroll
        for (int j = 3; j >= 0; --j)
            if ((rem >> j) & 1u) first = bin[j];
        const int b0 = __shfl(first, leader);
        double x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = 0.0;
        unsigned long long cnt = 0ull;   // four 16-bit counts: n, a1, a2, a3 (at most 256 each per wave)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (((rem >> j) & 1u) && bin[j] == b0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] += (double)t[j].r[k];
                cnt += 1ull | ((unsigned long long)t[j].d1 << 16) | ((unsigned long long)t[j].d2 << 32) |
                       ((unsigned long long)t[j].d3 << 48);
                rem &= ~(1u << j);
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double y = x[k];
            for (int o = 32; o > 0; o >>= 1) y += __shfl_xor(y, o);
            const int col = k < 6 ? k + 1 : k + 4;   // the sum's column in the row of twelve
            if (lane == col) mine = y;
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) mine = (double)(cnt & 0xFFFFull);
        if (lane >= 7 && lane <= 9) mine = (double)((cnt >> (16 * (lane - 6))) & 0xFFFFull);
        if (lane < kEvalSums) wrow[b0 * kEvalSums + lane] += mine;
        act = __ballot(rem != 0u);
    }
}

// grid (nb, B), 256 threads, 4 * nbt * 96 bytes of LDS (at most 12 KiB).  part as k_eval_partials;
// spart: [B][nb][nbt][12], nbt = depth bins (0 when off) + angle bins (0 when off).
template <bool VEC, bool ALIGN>
__global__ __launch_bounds__(kEvalThreads) void k_eval_strata_partials(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                       const uint8_t* __restrict__ mask, int64_t HW, float lo,
                                                                       float hi, int clamp_pred, double* __restrict__ part, int nb,
                                                                       const float* __restrict__ align, int64_t base,
                                                                       const float* __restrict__ K, int W, EvalStrata sp,
                                                                       double* __restrict__ spart) {
    __shared__ double rows[kEvalThreads / 64][2 * kStrataMaxBins * kEvalSums];
    __shared__ double red[kEvalThreads / 64][kEvalSums];
    const int b = blockIdx.y;
    const int nd = sp.n_depth_cuts > 0 ? sp.n_depth_cuts + 1 : 0;
    const int na = sp.n_angle_cuts > 0 ? sp.n_angle_cuts + 1 : 0;
    const int nbt = nd + na;
    for (int i = threadIdx.x; i < (kEvalThreads / 64) * 2 * kStrataMaxBins * kEvalSums; i += kEvalThreads) (&rows[0][0])[i] = 0.0;
    float as = 1.f, at = 0.f;
    if constexpr (ALIGN) {
        as = align[(base + b) * 2];
        at = align[(base + b) * 2 + 1];
    }
    float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f;
    if (na) {
        const float* Kb = K + (int64_t)b * 9;
        fx = Kb[0];
        cx = Kb[2];
        fy = Kb[4];
        cy = Kb[5];
    }
    const float* ps = pred + (int64_t)b * HW;
    const float* gs = gt + (int64_t)b * HW;
    const uint8_t* ms = mask ? mask + (int64_t)b * HW : nullptr;
    const int64_t nq = (HW + 3) / 4;
    double* wrow = rows[threadIdx.x >> 6];
    EvalAcc a;
    for (int k = 0; k < kEvalSums; ++k) a.v[k] = 0.0;
    __syncthreads();
    // the walk of k_eval_partials, with the same trip count for every thread of the block
    for (int64_t qb = (int64_t)blockIdx.x * kEvalThreads; qb < nq; qb += (int64_t)nb * kEvalThreads) {
        const int64_t q = qb + threadIdx.x;
        const int64_t i = q * 4;
        float p[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
        bool m[4] = {false, false, false, false};
        if (q < nq) {
            if constexpr (VEC) {
                const float4 p4 = *reinterpret_cast<const float4*>(ps + i);
                const float4 g4 = *reinterpret_cast<const float4*>(gs + i);
                uchar4 m4 = make_uchar4(1, 1, 1, 1);
                if (ms) m4 = *reinterpret_cast<const uchar4*>(ms + i);
                p[0] = p4.x; p[1] = p4.y; p[2] = p4.z; p[3] = p4.w;
                g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
                m[0] = m4.x != 0; m[1] = m4.y != 0; m[2] = m4.z != 0; m[3] = m4.w != 0;
            } else {
                const int n = (int)(HW - i < 4 ? HW - i : 4);   // the last quad may be short
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) {
                        p[j] = ps[i + j];
                        g[j] = gs[i + j];
                        m[j] = ms ? ms[i + j] != 0 : true;
                    }
            }
        }
        EvalTerms t[4];
        int dbin[4], abin[4];
        unsigned rem = 0u;
        int row = 0, col = 0;
        if (na && q < nq) {
            row = (int)((unsigned)i / (unsigned)W);   // HW < 2^31 with strata (checked by the host)
            col = (int)((unsigned)i - (unsigned)row * (unsigned)W);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dbin[j] = abin[j] = 0;
            if (eval_terms(t[j], ALIGN ? align_pred(p[j], as, at) : p[j], g[j], m[j], lo, hi, clamp_pred)) {
                eval_add_terms(a, t[j]);
                rem |= 1u << j;
                if (nd) dbin[j] = strata_bin(sp.depth_cuts, sp.n_depth_cuts, g[j]);
                if (na) abin[j] = strata_bin(sp.angle_cuts, sp.n_angle_cuts, strata_rho2(col, row, fx, fy, cx, cy));
            }
            if (++col == W) {
                col = 0;
                ++row;
            }
        }
        if (nd) strata_deposit(wrow, t, dbin, rem);
        if (na) strata_deposit(wrow + nd * kEvalSums, t, abin, rem);
    }
    for (int k = 0; k < kEvalSums; ++k) {
        double x = a.v[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kEvalSums)
        part[((int64_t)b * nb + blockIdx.x) * kEvalSums + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    double* sp_out = spart + ((int64_t)b * nb + blockIdx.x) * nbt * kEvalSums;
    for (int i = threadIdx.x; i < nbt * kEvalSums; i += kEvalThreads)
        sp_out[i] = ((rows[0][i] + rows[1][i]) + rows[2][i]) + rows[3][i];
}

// grid (B), 256 threads: rows [base + b][nbt][12] of the strata table = the sample's nb partial rows added
// in index order
__global__ __launch_bounds__(kEvalThreads) void k_strata_final(const double* __restrict__ spart, int nb, int nbt,
                                                               double* __restrict__ stable, int64_t base) {
    const int b = blockIdx.x;
    const int n = nbt * kEvalSums;
    for (int k = threadIdx.x; k < n; k += kEvalThreads) {
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += spart[((int64_t)b * nb + i) * n + k];
        stable[(base + b) * n + k] = s;
    }
}

}  // namespace

int eval_blocks(int64_t HW) {
    const int64_t nq = (HW + 3) / 4;
    return (int)std::max<int64_t>(1, std::min<int64_t>(128, (nq + kEvalThreads - 1) / kEvalThreads));
}

void eval_update(const float* pred, const float* gt, const uint8_t* mask, int B, int64_t HW, float min_depth,
                 float max_depth, int clamp_pred, double* part, int nb, double* table, int64_t base, hipStream_t st,
                 const float* align) {
    const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(gt) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb, B), dim3(kEvalThreads), 0, st, pred, gt, mask, HW, min_depth, max_depth, clamp_pred,
                           part, nb, align, base);
    };
    if (align) vec ? launch(k_eval_partials<true, true>) : launch(k_eval_partials<false, true>);
    else vec ? launch(k_eval_partials<true, false>) : launch(k_eval_partials<false, false>);
    hipLaunchKernelGGL(k_eval_final, dim3(B), dim3(64), 0, st, part, nb, table, base);
}

void eval_update_strata(const float* pred, const float* gt, const uint8_t* mask, const float* K, int B, int64_t HW, int W,
                        float min_depth, float max_depth, int clamp_pred, double* part, int nb, double* table, int64_t base,
                        hipStream_t st, const float* align, const EvalStrata& sp, double* spart, double* stable) {
    const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(gt) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
    const int nbt = (sp.n_depth_cuts > 0 ? sp.n_depth_cuts + 1 : 0) + (sp.n_angle_cuts > 0 ? sp.n_angle_cuts + 1 : 0);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nb, B), dim3(kEvalThreads), 0, st, pred, gt, mask, HW, min_depth, max_depth, clamp_pred,
                           part, nb, align, base, K, W, sp, spart);
    };
    if (align) vec ? launch(k_eval_strata_partials<true, true>) : launch(k_eval_strata_partials<false, true>);
    else vec ? launch(k_eval_strata_partials<true, false>) : launch(k_eval_strata_partials<false, false>);
    hipLaunchKernelGGL(k_eval_final, dim3(B), dim3(64), 0, st, part, nb, table, base);
    hipLaunchKernelGGL(k_strata_final, dim3(B), dim3(kEvalThreads), 0, st, spart, nb, nbt, stable, base);
}

}  // namespace cad
