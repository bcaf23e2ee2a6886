// TensorBoard histograms of a flat fp32 slab (parameters or gradients) on the device, one row per segment.
//
//   buckets  TensorBoard's default edges (cad_tb_default_bins, generated once on the host in double).  The
//            bucket of an fp32 value is decided by integer comparison only: the host turns edge k into
//            ukey[k] = order_key(smallest fp32 >= edge k), so  v >= edge k  <=>  order_key(v) >= ukey[k]
//            exactly, and the bucket is an upper-bound binary search over ukey staged in LDS.  numpy.histogram's
//            rule: half-open bins, the last one closed (key_hi = order_key(largest fp32 <= the last edge)),
//            values outside [edge 0, last edge] in no bucket, -0.0 counted as 0.0.
//   stats    {num, min, max, sum, sum_squares, nonfinite} per segment.  Non-finite values only count in
//            nonfinite.  min / max travel as order keys (integers); sums are double, products formed in
//            double (exact for fp32 inputs).
//   order    A host-built chunk table maps chunk -> (segment, first element, length); one block walks whole
//            chunks (grid-stride over the table), so a chunk's partial row does not depend on the grid.  Inside
//            a chunk thread t takes elements in a fixed order; wave __shfl_xor, then LDS, then the chunk's
//            partial row; k_hist_final adds a segment's partial rows in index order.  Bucket counts go to LDS
//            bins with integer atomics (aggregated per wave, so a constant tensor costs one add per wave
//            instead of 64 serialised ones), and the non-zero bins to the segment's global bins with integer
//            atomics: order-independent, hence deterministic.  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "kernels.hpp"

namespace cad {
namespace {

constexpr int kThreads = 256;
constexpr int kBins = kHistBins;
constexpr int kEdges = kBins + 1;
constexpr int kMaxGrid = 2048;   // as the export kernels

__device__ __forceinline__ unsigned order_key_bits(unsigned u) { return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u); }
__device__ __forceinline__ float key_to_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// eval_align_kernels.hip's aggregated add: must be reached by all lanes of the wave
__device__ __forceinline__ void hist_add(unsigned* h, bool match, unsigned bin) {
    unsigned long long act = __ballot(match);
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < 2 && act; ++r) {
        const int leader = __ffsll((unsigned long long)act) - 1;
        const unsigned b0 = __shfl(bin, leader);
        const unsigned long long same = __ballot(match && bin == b0);
        if (lane == leader) atomicAdd(&h[b0], (unsigned)__popcll(same));
        match = match && bin != b0;
        act &= ~same;
    }
    if (match) atomicAdd(&h[bin], 1u);
}

struct Acc {
    double sum = 0.0, sq = 0.0;
    unsigned n = 0u, bad = 0u;
    unsigned kmin = 0xFFFFFFFFu, kmax = 0u;
};

// one element; `on` false for lanes without one (the wave-level add needs every lane here)
__device__ __forceinline__ void hist_value(Acc& a, unsigned* bins, const unsigned* ukey, unsigned key_hi, bool on, float v) {
    unsigned u = __float_as_uint(v);
    const bool finite = (u & 0x7F800000u) != 0x7F800000u;
    if (on && !finite) ++a.bad;
    on = on && finite;
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;   // -0.0 is 0.0 (integer test: no denormal is taken for zero)
    const unsigned k = order_key_bits(u);
    if (on) {
        const double d = (double)__uint_as_float(u);
        a.sum += d;
        a.sq += d * d;
        ++a.n;
        a.kmin = min(a.kmin, k);
        a.kmax = max(a.kmax, k);
    }
    // upper bound: number of edges with ukey <= k
    int lo = 0, hi = kEdges;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ukey[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    const bool in = on && lo > 0 && k <= key_hi;
    hist_add(bins, in, (unsigned)max(0, min(lo - 1, kBins - 1)));
}

// grid-stride over the chunk table, 256 threads, 2 x 6 KiB of LDS.
__global__ __launch_bounds__(kThreads) void k_hist_chunks(const float* __restrict__ base, const HistSegment* __restrict__ segs,
                                                          const HistChunk* __restrict__ chunks, int nchunks,
                                                          const unsigned* __restrict__ ukey_g, unsigned key_hi,
                                                          unsigned* __restrict__ gbins, double* __restrict__ part) {
    __shared__ unsigned ukey[kEdges];
    __shared__ unsigned bins[kBins];
    __shared__ double red[kThreads / 64][4];
    __shared__ unsigned redk[kThreads / 64][2];
    const int t = threadIdx.x;
    for (int i = t; i < kEdges; i += kThreads) ukey[i] = ukey_g[i];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const HistChunk ch = chunks[c];
        const HistSegment sg = segs[ch.seg];
        for (int i = t; i < kBins; i += kThreads) bins[i] = 0u;
        __syncthreads();   // bins cleared, ukey staged, the previous chunk's red[] read
        const float* p = base + sg.offset + ch.start;
        const int len = ch.len;
        const unsigned period = (unsigned)sg.period, keep = (unsigned)sg.keep;
        const unsigned ph0 = (unsigned)(ch.start % sg.period);   // phase of the chunk's first element
        const unsigned iperiod = (unsigned)sg.inner_period, ikeep = (unsigned)sg.inner_keep;
        const auto counted = [&](int j) {
            if (period == 1u) return true;
            const unsigned r = (ph0 + (unsigned)j) % period;   // position inside the period
            return r < keep && (iperiod == 0u || r % iperiod < ikeep);
        };
        // scalar head up to the first 16-byte boundary, float4 body, scalar tail
        const int mis = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u);
        const int head = min(len, (4 - mis) & 3);
        const int nvec = (len - head) >> 2;
        const int tail = len - head - 4 * nvec;
        Acc a;
        {
            int j = -1;
            if (t < head) j = t;
            else if (t >= 4 && t - 4 < tail) j = head + 4 * nvec + (t - 4);
            const bool on = j >= 0 && counted(j);
            hist_value(a, bins, ukey, key_hi, on, on ? p[j] : 0.f);
        }
        const float4* p4 = reinterpret_cast<const float4*>(p + head);
        for (int q0 = 0; q0 < nvec; q0 += kThreads) {   // uniform trip count: every lane reaches hist_value
            const int q = q0 + t;
            const bool has = q < nvec;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has) v = p4[q];
            const int j = head + 4 * q;
            hist_value(a, bins, ukey, key_hi, has && counted(j), v.x);
            hist_value(a, bins, ukey, key_hi, has && counted(j + 1), v.y);
            hist_value(a, bins, ukey, key_hi, has && counted(j + 2), v.z);
            hist_value(a, bins, ukey, key_hi, has && counted(j + 3), v.w);
        }
        // wave, then LDS, then the chunk's partial row
        double s = a.sum, q2 = a.sq, n = (double)a.n, bad = (double)a.bad;
        unsigned kmin = a.kmin, kmax = a.kmax;
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o);
            q2 += __shfl_xor(q2, o);
            n += __shfl_xor(n, o);
            bad += __shfl_xor(bad, o);
            kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o));
            kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
        }
        if ((t & 63) == 0) {
            red[t >> 6][0] = n; red[t >> 6][1] = s; red[t >> 6][2] = q2; red[t >> 6][3] = bad;
            redk[t >> 6][0] = kmin; redk[t >> 6][1] = kmax;
        }
        __syncthreads();   // red[] written, every LDS bin add done
        if (t < 4) {
            const int slot = t == 0 ? 0 : t == 1 ? 3 : t == 2 ? 4 : 5;   // num, sum, sum_squares, nonfinite
            part[(int64_t)c * kHistStats + slot] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        } else if (t == 4) {
            const unsigned k = min(min(redk[0][0], redk[1][0]), min(redk[2][0], redk[3][0]));
            part[(int64_t)c * kHistStats + 1] = (double)key_to_float(k);    // no finite value: a NaN that k_hist_final skips
        } else if (t == 5) {
            const unsigned k = max(max(redk[0][1], redk[1][1]), max(redk[2][1], redk[3][1]));
            part[(int64_t)c * kHistStats + 2] = (double)key_to_float(k);
        }
        unsigned* gb = gbins + (int64_t)ch.seg * kBins;
        for (int i = t; i < kBins; i += kThreads) {
            const unsigned cnt = bins[i];
            if (cnt) atomicAdd(&gb[i], cnt);
        }
        __syncthreads();   // bins and red[] read before the next chunk clears them
    }
}

// grid (nseg), 64 threads: the segment's partial rows in index order.  A chunk without a finite value has
// num == 0 and its min / max slots are skipped (they hold the decoded sentinels).
__global__ __launch_bounds__(64) void k_hist_final(const double* __restrict__ part, const HistSegment* __restrict__ segs,
                                                   double* __restrict__ stats) {
    const int s = blockIdx.x, t = threadIdx.x;
    if (t >= kHistStats) return;
    const int c0 = segs[s].first_chunk, nc = segs[s].nchunks;
    double r = 0.0;
    bool any = false;
    for (int i = 0; i < nc; ++i) {
        const double* row = part + (int64_t)(c0 + i) * kHistStats;
        if (t == 1 || t == 2) {
            if (row[0] > 0.0) {
                const double v = row[t];
                r = !any ? v : (t == 1 ? fmin(r, v) : fmax(r, v));
                any = true;
            }
        } else {
            r += row[t];
        }
    }
    stats[(int64_t)s * kHistStats + t] = r;
}

}  // namespace

void hist_run(const float* base, const HistSegment* segs, int nseg, const HistChunk* chunks, int nchunks, const unsigned* ukey,
              unsigned key_hi, double* stats, unsigned* bins, double* part, int64_t span, hipStream_t st) {
    if (nseg <= 0 || nchunks <= 0) return;
    const int64_t out_bytes = (int64_t)nseg * (kHistStats * 8 + kHistBins * 4);
    CAD_NO_ALIAS("hist", {aview(stats, 1, out_bytes, 0, out_bytes, 1, "stats and bins"),
                          aview(part, 1, (int64_t)nchunks * kHistStats, 0, (int64_t)nchunks * kHistStats, 8, "partials")},
                 {aview(base, 1, span, 0, span, 4, "values")});
    if (hipMemsetAsync(bins, 0, sizeof(unsigned) * (size_t)nseg * kHistBins, st) != hipSuccess)
        throw std::runtime_error("hist: clearing the bins failed");
    hipLaunchKernelGGL(k_hist_chunks, dim3(std::min(nchunks, kMaxGrid)), dim3(kThreads), 0, st, base, segs, chunks, nchunks, ukey,
                       key_hi, bins, part);
    hipLaunchKernelGGL(k_hist_final, dim3(nseg), dim3(64), 0, st, part, segs, stats);
}

}  // namespace cad
