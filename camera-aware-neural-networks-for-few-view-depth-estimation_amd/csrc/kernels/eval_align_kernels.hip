// Scale-aligned evaluation: per-sample (scale, shift) computed on the device between the forward pass
// and the metrics pass of eval_kernels.hip (no reference counterpart: the reference scores raw predictions).
//
//   valid   the evaluator's set: gt > min_depth && gt < max_depth (strict) [&& mask != 0]; statistics
//           use the raw pred, before the clamp
//   stats   {n, n_pos, sum p, sum g, sum p^2, sum pg, sum(ln g - ln p) over pred > 0} per sample: products
//           and logs in double from the fp32 inputs, double sums (the log sum only in log_mean mode).
//           Same quad-to-thread mapping and two-stage reduction as k_eval_partials / k_eval_final (no
//           floating-point atomics, fixed order), so the 16-byte and scalar paths give the same bits and a
//           sample does not depend on its batch.
//   select  exact ranks (n-1)/2 and n/2 of pred and of gt among the valid pixels by radix select on the
//           order-preserving key (bits ^ 0x80000000 for non-negative values, ~bits for negative ones),
//           four passes of eight bits, most significant digit first.  Per pass k_align_hist (grid (nb, B))
//           counts the digit of every pixel whose higher digits equal a selector's prefix into 256 LDS bins
//           per selector and adds its non-zero bins to the sample's global bins with integer atomics
//           (order-independent, hence deterministic); k_align_pick (one block per sample) scans the bins,
//           narrows each selector's prefix and rank, and clears the bins for the next pass.  Four selectors
//           per sample (pred low / high rank, gt low / high rank), each with its own prefix; while the two
//           ranks of a tensor share their prefix only the first is counted and the second reads its bins.
//           The valid count n is the total of the first pass, so median mode needs no statistics pass.
//   solve   one thread per sample: eval_solve_alignment (eval_align.hpp) -> row base + b of the table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "eval_align.hpp"
#include "kernels.hpp"

namespace cad {
namespace {

constexpr int kThreads = 256;
constexpr int kBins = 256;       // eight bits per pass
constexpr int kSel = 4;          // pred (n-1)/2, pred n/2, gt (n-1)/2, gt n/2
constexpr int kSelStride = 12;   // per-sample selector state: prefix[4], rank[4], n, 3 unused

__device__ __forceinline__ unsigned order_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// The evaluator's walk over one sample (eval_kernels.hip): quad q goes to thread q % 256 of block
// (q / 256) % nb, quads in increasing order, the four pixels of a quad in order.  The trip count is the
// same for every thread of the block and f runs for all four slots of every trip (ok = false for a slot
// past the sample or an invalid pixel), so f may use wave-wide operations.
template <bool VEC, class F>
__device__ __forceinline__ void for_each_pixel(const float* __restrict__ ps, const float* __restrict__ gs,
                                               const uint8_t* __restrict__ ms, int64_t HW, int nb, float lo, float hi, F&& f) {
    const int64_t nq = (HW + 3) / 4;
    for (int64_t qb = (int64_t)blockIdx.x * kThreads; qb < nq; qb += (int64_t)nb * kThreads) {
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
                for (int j = 0; j < 4; ++j)
                    if (j < n) {
                        p[j] = ps[i + j];
                        g[j] = gs[i + j];
                        m[j] = ms ? ms[i + j] != 0 : true;
                    }
            }
        }
        for (int j = 0; j < 4; ++j) f(p[j], g[j], m[j] && g[j] > lo && g[j] < hi);
    }
}

// ---------------- statistics ----------------
// grid (nb, B), 256 threads: part[b][block][7].  LOGS = false (least squares, which does not read it)
// leaves the log sum 0: the two double logarithms per pixel are most of this pass's time.
template <bool VEC, bool LOGS>
__global__ __launch_bounds__(kThreads) void k_align_stats_partials(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                   const uint8_t* __restrict__ mask, int64_t HW, float lo,
                                                                   float hi, double* __restrict__ part, int nb) {
    const int b = blockIdx.y;
    double a[kAlignStats];
    for (int k = 0; k < kAlignStats; ++k) a[k] = 0.0;
    for_each_pixel<VEC>(pred + (int64_t)b * HW, gt + (int64_t)b * HW, mask ? mask + (int64_t)b * HW : nullptr, HW, nb, lo, hi,
                        [&](float p, float g, bool ok) {
#pragma clang fp contract(off)
                            if (!ok) return;
                            const double dp = (double)p, dg = (double)g;
                            a[0] += 1.0;
                            a[2] += dp;
                            a[3] += dg;
                            a[4] += dp * dp;
                            a[5] += dp * dg;
                            if (p > 0.f) {
                                a[1] += 1.0;
                                if constexpr (LOGS) a[6] += log(dg) - log(dp);
                            }
                        });
    __shared__ double red[kThreads / 64][kAlignStats];
    for (int k = 0; k < kAlignStats; ++k) {
        double x = a[k];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kAlignStats)
        part[((int64_t)b * nb + blockIdx.x) * kAlignStats + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// grid (B), 256 threads: stats[b] = the sample's nb partial rows added in index order.  The rows are staged
// in LDS with coalesced loads first, so the ordered sum does not wait for one global load per term.
constexpr int kMaxBlocks = 128;   // eval_blocks()' upper bound
__global__ __launch_bounds__(kThreads) void k_align_stats_final(const double* __restrict__ part, int nb, double* __restrict__ stats) {
    __shared__ double rows[kMaxBlocks * kAlignStats];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < nb * kAlignStats; i += kThreads) rows[i] = part[(int64_t)b * nb * kAlignStats + i];
    __syncthreads();
    if (threadIdx.x >= kAlignStats) return;
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += rows[i * kAlignStats + threadIdx.x];
    stats[(int64_t)b * kAlignStats + threadIdx.x] = s;
}

// ---------------- radix select ----------------
// Aggregated per wave: the digit of the first matching lane gets one LDS add of the number of lanes that
// share it, then the same for the first lane left, then one add per remaining lane.  A constant (or
// two-valued) image costs one or two LDS adds per wave instead of 64 serialised ones on a single bin.
// Must be reached by all lanes of the wave.
__device__ __forceinline__ void hist_add(unsigned* h, bool match, unsigned digit) {
    unsigned long long act = __ballot(match);
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < 2 && act; ++r) {
        const int leader = __ffsll((unsigned long long)act) - 1;
        const unsigned d0 = __shfl(digit, leader);
        const unsigned long long same = __ballot(match && digit == d0);
        if (lane == leader) atomicAdd(&h[d0], (unsigned)__popcll(same));
        match = match && digit != d0;
        act &= ~same;
    }
    if (match) atomicAdd(&h[digit], 1u);
}

// grid (nb, B), 256 threads, 4 KiB of LDS: hist[b][selector][256] += the block's counts
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_align_hist(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const uint8_t* __restrict__ mask, int64_t HW, float lo, float hi,
                                                         const unsigned* __restrict__ sel, int pass, unsigned* __restrict__ hist,
                                                         int nb) {
    __shared__ unsigned h[kSel * kBins];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < kSel * kBins; i += kThreads) h[i] = 0u;
    unsigned pre[kSel] = {0u, 0u, 0u, 0u}, himask = 0u;   // first pass: every valid pixel matches
    if (pass > 0) {
        for (int j = 0; j < kSel; ++j) pre[j] = sel[(int64_t)b * kSelStride + j];
        himask = 0xFFFFFFFFu << (32 - 8 * pass);
    }
    const bool same_p = pre[0] == pre[1], same_g = pre[2] == pre[3];
    const int shift = 24 - 8 * pass;
    __syncthreads();
    for_each_pixel<VEC>(pred + (int64_t)b * HW, gt + (int64_t)b * HW, mask ? mask + (int64_t)b * HW : nullptr, HW, nb, lo, hi,
                        [&](float p, float g, bool ok) {
                            const unsigned kp = order_key(p), kg = order_key(g);
                            const unsigned dp = (kp >> shift) & 255u, dg = (kg >> shift) & 255u;
                            hist_add(h, ok && ((kp ^ pre[0]) & himask) == 0u, dp);
                            if (!same_p) hist_add(h + kBins, ok && ((kp ^ pre[1]) & himask) == 0u, dp);
                            hist_add(h + 2 * kBins, ok && ((kg ^ pre[2]) & himask) == 0u, dg);
                            if (!same_g) hist_add(h + 3 * kBins, ok && ((kg ^ pre[3]) & himask) == 0u, dg);
                        });
    __syncthreads();
    for (int i = threadIdx.x; i < kSel * kBins; i += kThreads) {
        const unsigned c = h[i];
        if (c) atomicAdd(&hist[(int64_t)b * kSel * kBins + i], c);
    }
}

// grid (B), 256 threads (one per bin): narrows the four selectors of sample b by this pass's digit and
// clears the sample's bins.  After the last pass the prefixes are the keys of the ranked values:
// med[b] = {(pred_lo + pred_hi) * 0.5f, (gt_lo + gt_hi) * 0.5f}, or {0, 0} without a valid pixel.
__global__ __launch_bounds__(kBins) void k_align_pick(unsigned* __restrict__ hist, unsigned* __restrict__ sel, int pass,
                                                      float* __restrict__ med) {
    __shared__ unsigned st[kSelStride], wsum[kBins / 64], res_d[kSel], res_ex[kSel];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned* hb = hist + (int64_t)b * kSel * kBins;
    unsigned* sb = sel + (int64_t)b * kSelStride;
    unsigned c[kSel];
    for (int j = 0; j < kSel; ++j) {
        c[j] = hb[j * kBins + t];
        hb[j * kBins + t] = 0u;
    }
    if (t < kSelStride) st[t] = pass > 0 ? sb[t] : 0u;
    if (t < kSel) res_d[t] = res_ex[t] = 0u;
    __syncthreads();
    const bool same_p = st[0] == st[1], same_g = st[2] == st[3];
    unsigned n = st[8], rank[kSel];
    for (int j = 0; j < kSel; ++j) {
        const unsigned src = ((j & 1) && (j < 2 ? same_p : same_g)) ? c[j - 1] : c[j];
        unsigned x = src;   // inclusive scan over the 256 bins
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        unsigned off = 0u;
        for (int i = 0; i < w; ++i) off += wsum[i];
        const unsigned incl = x + off, excl = incl - src;
        if (pass == 0) {
            n = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];   // the same for pred and gt: they share the valid set
            rank[j] = n ? ((j & 1) ? n / 2u : (n - 1u) / 2u) : 0u;
        } else {
            rank[j] = st[kSel + j];
        }
        if (src && excl <= rank[j] && rank[j] < incl) {   // exactly one bin when n > 0
            res_d[j] = (unsigned)t;
            res_ex[j] = excl;
        }
        __syncthreads();
    }
    const int shift = 24 - 8 * pass;
    if (t < kSel) {
        const unsigned key = st[t] | (res_d[t] << shift);
        sb[t] = key;
        sb[kSel + t] = rank[t] - res_ex[t];
        st[t] = key;
    }
    if (t == 0) sb[8] = n;
    if (pass == 3) {
        __syncthreads();
        if (t < 2) med[(int64_t)b * 2 + t] = n ? (key_value(st[2 * t]) + key_value(st[2 * t + 1])) * 0.5f : 0.f;
    }
}

// one thread per sample
__global__ __launch_bounds__(64) void k_align_solve(int mode, const double* __restrict__ stats, const unsigned* __restrict__ sel,
                                                    const float* __restrict__ med, float* __restrict__ table,
                                                    uint8_t* __restrict__ flags, int64_t base, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double st[kAlignStats];
    float m2[2] = {0.f, 0.f}, out[2];
    for (int k = 0; k < kAlignStats; ++k) st[k] = 0.0;
    if (mode == kAlignMedian) {
        st[0] = (double)sel[(int64_t)b * kSelStride + 8];
        m2[0] = med[(int64_t)b * 2];
        m2[1] = med[(int64_t)b * 2 + 1];
    } else {
        for (int k = 0; k < kAlignStats; ++k) st[k] = stats[(int64_t)b * kAlignStats + k];
    }
    const int ok = eval_solve_alignment(mode, st, m2, out);
    table[(base + b) * 2] = out[0];
    table[(base + b) * 2 + 1] = out[1];
    flags[base + b] = (uint8_t)ok;
}

bool vec_ok(const float* pred, const float* gt, const uint8_t* mask, int64_t HW) {
    return HW % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0 && (reinterpret_cast<uintptr_t>(gt) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t eval_align_ws_bytes(int Bmax, int nb) {
    const size_t B = (size_t)Bmax;
    return up256(sizeof(double) * kAlignStats * B * nb) + up256(sizeof(double) * kAlignStats * B) +
           up256(sizeof(unsigned) * kSel * kBins * B) + up256(sizeof(unsigned) * kSelStride * B) + up256(sizeof(float) * 2 * B);
}

EvalAlignWs eval_align_ws_carve(void* base, int Bmax, int nb) {
    const size_t B = (size_t)Bmax;
    char* p = static_cast<char*>(base);
    EvalAlignWs ws;
    ws.part = reinterpret_cast<double*>(p);
    p += up256(sizeof(double) * kAlignStats * B * nb);
    ws.stats = reinterpret_cast<double*>(p);
    p += up256(sizeof(double) * kAlignStats * B);
    ws.hist = reinterpret_cast<unsigned*>(p);
    p += up256(sizeof(unsigned) * kSel * kBins * B);
    ws.sel = reinterpret_cast<unsigned*>(p);
    p += up256(sizeof(unsigned) * kSelStride * B);
    ws.med = reinterpret_cast<float*>(p);
    return ws;
}

void eval_valid_medians(const float* pred, const float* gt, const uint8_t* mask, int B, int64_t HW, float min_depth,
                        float max_depth, const EvalAlignWs& ws, int nb, float* med, hipStream_t st) {
    const bool vec = vec_ok(pred, gt, mask, HW);
    for (int pass = 0; pass < 4; ++pass) {
        if (vec)
            hipLaunchKernelGGL(k_align_hist<true>, dim3(nb, B), dim3(kThreads), 0, st, pred, gt, mask, HW, min_depth, max_depth,
                               ws.sel, pass, ws.hist, nb);
        else
            hipLaunchKernelGGL(k_align_hist<false>, dim3(nb, B), dim3(kThreads), 0, st, pred, gt, mask, HW, min_depth, max_depth,
                               ws.sel, pass, ws.hist, nb);
        hipLaunchKernelGGL(k_align_pick, dim3(B), dim3(kBins), 0, st, ws.hist, ws.sel, pass, med);
    }
}

void eval_align(int mode, const float* pred, const float* gt, const uint8_t* mask, int B, int64_t HW, float min_depth,
                float max_depth, const EvalAlignWs& ws, int nb, float* table, uint8_t* flags, int64_t base, hipStream_t st) {
    if (nb > kMaxBlocks) throw std::invalid_argument("eval_align: more blocks per sample than eval_blocks() gives");
    if (mode == kAlignMedian) {
        eval_valid_medians(pred, gt, mask, B, HW, min_depth, max_depth, ws, nb, ws.med, st);
    } else {
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(nb, B), dim3(kThreads), 0, st, pred, gt, mask, HW, min_depth, max_depth, ws.part, nb);
        };
        const bool vec = vec_ok(pred, gt, mask, HW);
        if (mode == kAlignLogMean) vec ? launch(k_align_stats_partials<true, true>) : launch(k_align_stats_partials<false, true>);
        else vec ? launch(k_align_stats_partials<true, false>) : launch(k_align_stats_partials<false, false>);
        hipLaunchKernelGGL(k_align_stats_final, dim3(B), dim3(kThreads), 0, st, ws.part, nb, ws.stats);
    }
    hipLaunchKernelGGL(k_align_solve, dim3((B + 63) / 64), dim3(64), 0, st, mode, ws.stats, ws.sel, ws.med, table, flags, base, B);
}

}  // namespace cad
