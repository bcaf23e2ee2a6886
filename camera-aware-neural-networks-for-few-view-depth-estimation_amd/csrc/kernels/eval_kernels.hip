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

}  // namespace cad
