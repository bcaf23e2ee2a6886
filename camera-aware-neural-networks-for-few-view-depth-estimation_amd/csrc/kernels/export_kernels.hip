// Inference export: what turns a predicted depth map (B,1,H,W) into files, on the device
// (the reference's DepthVisualizer, src/visualization/depth_viz.h:23-148 and depth_visualizer.h, which
// round-trips every map through the host and OpenCV; the point cloud has no reference counterpart).
//
//   range    per image (min, max) of v = sub ? |d - sub| : d over its valid pixels
//            (isfinite(v), d > 0 [, sub > 0] [, mask != 0]); (0, 0) without one.  Two stages, no atomics:
//            k_range_partials (grid (nb, B)) -> k_range_final (grid B).  min / max do not depend on the
//            order, so nb may follow the batch size.
//   render   one pass over the depth, two nullable outputs: RGB8 HWC through a 256 x 3 table
//            (normalizeDepth :88-107: t = (v - lo) / (hi - lo) as fp32 subtract, subtract, IEEE divide,
//            clamped, idx = rintf(t * 255); hi - lo < 1e-6 -> idx 0) written at a row stride and column
//            offset (panes of one panel buffer), and uint16 rintf(d * units_per_metre) clamped to 65535.
//   image    (B,3,H,W) fp32 rgb -> RGB8 HWC pane, rintf(clamp(c, 0, 1) * 255) (the panel's first pane)
//   points   ordered stream compaction fused with the unprojection: candidates are the pixels of the
//            stride grid in row-major order, in tiles of 1024 (four steps of 256 threads).
//            k_points_count: valid candidates per tile; k_points_scan: exclusive scan of an image's tile
//            counts (+ its total); k_points_write: rank = tile offset + the valid candidates of earlier
//            steps and waves of the tile + popcount(__ballot below the lane), one 16-byte store
//            {X, Y, Z, rgba} at b * cap + rank.  No atomics: the placement is the same on every run, and a
//            tile's counts do not depend on which block walks it, so an image is the same bytes in any batch.
//   flips    hflip and flip_mean (0.5f * (a[x] + b[W-1-x])) for flip test-time augmentation.
//
// Grids are capped at 2048 blocks of 256 threads and stride over the rest.  Every per-pixel value is
// computed by one expression from its own inputs, so the 16-byte and the scalar load / store paths give the
// same bits; the wide paths are taken only when the addresses allow it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace cad {
namespace {

constexpr int kT = 256;
constexpr int kMaxGrid = 2048;
constexpr int kSteps = kPointTile / kT;   // 4
static_assert(kPointTile % kT == 0, "a point tile is a whole number of block steps");

__device__ __forceinline__ unsigned to_u8(float c) {
#pragma clang fp contract(off)
    return (unsigned)(int)rintf(fminf(fmaxf(c, 0.f), 1.f) * 255.0f);   // NaN -> 0
}

// ---------------- range ----------------
__device__ __forceinline__ float export_value(float d, float s, bool has_sub) {
#pragma clang fp contract(off)
    return has_sub ? fabsf(d - s) : d;
}
__device__ __forceinline__ bool export_valid(float v, float d, float s, bool has_sub, bool mask_ok) {
    return __builtin_isfinite(v) && d > 0.f && (!has_sub || s > 0.f) && mask_ok;
}

// the four pixels of quad q of one image (n < 4 in its last quad when HW % 4 != 0)
template <bool VEC>
__device__ __forceinline__ int load_quad(const float* __restrict__ ds, const float* __restrict__ ss,
                                         const uint8_t* __restrict__ ms, int64_t i, int64_t HW, float d[4], float s[4],
                                         bool m[4]) {
    if constexpr (VEC) {
        const float4 d4 = *reinterpret_cast<const float4*>(ds + i);
        d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
        if (ss) {
            const float4 s4 = *reinterpret_cast<const float4*>(ss + i);
            s[0] = s4.x; s[1] = s4.y; s[2] = s4.z; s[3] = s4.w;
        }
        if (ms) {
            const uchar4 m4 = *reinterpret_cast<const uchar4*>(ms + i);
            m[0] = m4.x != 0; m[1] = m4.y != 0; m[2] = m4.z != 0; m[3] = m4.w != 0;
        }
        return 4;
    } else {
        const int n = (int)(HW - i < 4 ? HW - i : 4);
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                d[j] = ds[i + j];
                if (ss) s[j] = ss[i + j];
                if (ms) m[j] = ms[i + j] != 0;
            }
        return n;
    }
}

// grid (nb, B), 256 threads: part[b][block] = {min, max} (+inf, -inf without a valid pixel)
template <bool VEC>
__global__ __launch_bounds__(kT) void k_range_partials(const float* __restrict__ depth, const float* __restrict__ sub,
                                                       const uint8_t* __restrict__ mask, int64_t HW,
                                                       float* __restrict__ part) {
    const int b = blockIdx.y, nb = gridDim.x;
    const float* ds = depth + (int64_t)b * HW;
    const float* ss = sub ? sub + (int64_t)b * HW : nullptr;
    const uint8_t* ms = mask ? mask + (int64_t)b * HW : nullptr;
    const int64_t nq = (HW + 3) / 4;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < nq; q += (int64_t)nb * kT) {
        float d[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {1.f, 1.f, 1.f, 1.f};
        bool m[4] = {true, true, true, true};
        const int n = load_quad<VEC>(ds, ss, ms, q * 4, HW, d, s, m);
        for (int j = 0; j < 4; ++j) {
            const float v = export_value(d[j], s[j], ss != nullptr);
            if (j < n && export_valid(v, d[j], s[j], ss != nullptr, m[j])) {
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    __shared__ float red[kT / 64][2];
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = mn;
        red[threadIdx.x >> 6][1] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + ((int64_t)b * nb + blockIdx.x) * 2;
        p[0] = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
        p[1] = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
    }
}

// grid (B), 64 threads: table[b] (and out[b] when given) = the image's range, (0, 0) when it is empty
__global__ __launch_bounds__(64) void k_range_final(const float* __restrict__ part, int nb, float* __restrict__ table,
                                                    float* __restrict__ out) {
    const int b = blockIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += 64) {
        mn = fminf(mn, part[((int64_t)b * nb + i) * 2]);
        mx = fmaxf(mx, part[((int64_t)b * nb + i) * 2 + 1]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (threadIdx.x == 0) {
        if (mx < mn) mn = mx = 0.f;
        table[(int64_t)b * 2] = mn;
        table[(int64_t)b * 2 + 1] = mx;
        if (out) {
            out[(int64_t)b * 2] = mn;
            out[(int64_t)b * 2 + 1] = mx;
        }
    }
}

// ---------------- render ----------------
__device__ __forceinline__ int color_index(float v, float lo, float hi) {
#pragma clang fp contract(off)
    const float range = hi - lo;
    if (range < 1e-6f) return 0;   // normalizeDepth :99-101
    const float t = (v - lo) / range;
    return (int)rintf(fminf(fmaxf(t, 0.f), 1.f) * 255.0f);
}
__device__ __forceinline__ unsigned depth_u16(float d, float units) {
#pragma clang fp contract(off)
    if (!(__builtin_isfinite(d) && d > 0.f)) return 0u;
    return (unsigned)fminf(fmaxf(rintf(d * units), 0.f), 65535.f);
}

// 4 RGB pixels (r | g << 8 | b << 16 each) -> 12 bytes at p: three 4-byte stores when the address allows
__device__ __forceinline__ void store_rgb(uint8_t* p, const unsigned c[4], int n) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(p);
        w[0] = c[0] | (c[1] << 24);
        w[1] = (c[1] >> 8) | (c[2] << 16);
        w[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
        for (int j = 0; j < n; ++j) {
            p[3 * j] = (uint8_t)c[j];
            p[3 * j + 1] = (uint8_t)(c[j] >> 8);
            p[3 * j + 2] = (uint8_t)(c[j] >> 16);
        }
    }
}

// destination of an HWC pane: image b starts image_stride pixels after image b - 1, a row is row_stride
// pixels, the pane's first column is col_off
struct PaneDst {
    uint8_t* rgb;
    int64_t row_stride, col_off, image_stride;
};
// pixels i .. i + n - 1 of image b (n <= 4); they may straddle a row end
__device__ __forceinline__ void store_pane(const PaneDst& p, int b, int64_t i, int W, const unsigned c[4], int n) {
    uint8_t* img = p.rgb + ((int64_t)b * p.image_stride + p.col_off) * 3;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    if (x + n <= W) {
        store_rgb(img + ((int64_t)y * p.row_stride + x) * 3, c, n);
    } else {
        for (int j = 0; j < n; ++j) {
            const int yy = (int)((i + j) / W), xx = (int)(i + j - (int64_t)yy * W);
            store_rgb(img + ((int64_t)yy * p.row_stride + xx) * 3, c + j, 1);
        }
    }
}

struct RenderArgs {
    const float* depth;
    const float* sub;
    const uint8_t* mask;
    const float* table;   // [B][2] {lo, hi} per image, or null: lo / hi below
    float lo, hi;
    const uint8_t* lut;   // 768 bytes, 4-byte aligned
    unsigned invalid;     // r | g << 8 | b << 16
    PaneDst dst;          // rgb == null: no colour output
    uint16_t* u16;        // null: no 16-bit output
    float units;
    int W;
    int64_t HW;
};

// grid (nb, B), 256 threads
template <bool VEC>
__global__ __launch_bounds__(kT) void k_render(RenderArgs a) {
    __shared__ uint32_t lut32[192];
    if (a.dst.rgb)
        for (int i = threadIdx.x; i < 192; i += kT) lut32[i] = reinterpret_cast<const uint32_t*>(a.lut)[i];
    __syncthreads();
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(lut32);
    const int b = blockIdx.y;
    const float* ds = a.depth + (int64_t)b * a.HW;
    const float* ss = a.sub ? a.sub + (int64_t)b * a.HW : nullptr;
    const uint8_t* ms = a.mask ? a.mask + (int64_t)b * a.HW : nullptr;
    const float lo = a.table ? a.table[(int64_t)b * 2] : a.lo, hi = a.table ? a.table[(int64_t)b * 2 + 1] : a.hi;
    const int64_t nq = (a.HW + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kT) {
        const int64_t i = q * 4;
        float d[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {1.f, 1.f, 1.f, 1.f};
        bool m[4] = {true, true, true, true};
        const int n = load_quad<VEC>(ds, ss, ms, i, a.HW, d, s, m);
        if (a.dst.rgb) {
            unsigned c[4];
            for (int j = 0; j < 4; ++j) {
                const float v = export_value(d[j], s[j], ss != nullptr);
                if (export_valid(v, d[j], s[j], ss != nullptr, m[j])) {
                    const uint8_t* e = lut + 3 * color_index(v, lo, hi);
                    c[j] = (unsigned)e[0] | (unsigned)e[1] << 8 | (unsigned)e[2] << 16;
                } else {
                    c[j] = a.invalid;
                }
            }
            store_pane(a.dst, b, i, a.W, c, n);
        }
        if (a.u16) {
            unsigned z[4];
            for (int j = 0; j < 4; ++j) z[j] = depth_u16(d[j], a.units);
            uint16_t* o = a.u16 + (int64_t)b * a.HW + i;
            if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
                *reinterpret_cast<uint2*>(o) = make_uint2(z[0] | z[1] << 16, z[2] | z[3] << 16);
            } else {
                for (int j = 0; j < n; ++j) o[j] = (uint16_t)z[j];
            }
        }
    }
}

// grid (nb, B), 256 threads: rgb (B,3,H,W) fp32 -> RGB8 HWC pane
template <bool VEC>
__global__ __launch_bounds__(kT) void k_image(const float* __restrict__ rgb, int64_t HW, int W, PaneDst dst) {
    const int b = blockIdx.y;
    const float* r = rgb + (int64_t)b * 3 * HW;
    const int64_t nq = (HW + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kT) {
        const int64_t i = q * 4;
        float ch[3][4] = {};
        int n = 4;
        for (int k = 0; k < 3; ++k) {
            bool m[4];
            n = load_quad<VEC>(r + k * HW, nullptr, nullptr, i, HW, ch[k], nullptr, m);
        }
        unsigned c[4];
        for (int j = 0; j < 4; ++j) c[j] = to_u8(ch[0][j]) | to_u8(ch[1][j]) << 8 | to_u8(ch[2][j]) << 16;
        store_pane(dst, b, i, W, c, n);
    }
}

// ---------------- points ----------------
struct PointArgs {
    const float* depth;
    const float* K;       // (B,3,3)
    const float* rgb;     // (B,3,H,W) or null
    const uint8_t* mask;  // or null
    int W, stride, Ws;
    int cap;              // Hs * Ws candidates per image
    int ntiles;           // ceil(cap / kPointTile)
    int64_t HW;
    float lo, hi;
};

// candidate j of image b: its pixel, its depth, and whether it is emitted
__device__ __forceinline__ bool point_valid(const PointArgs& a, int b, int j, float& Z, int& y, int& x, int64_t& pix) {
    if (j >= a.cap) return false;
    const int ys = j / a.Ws, xs = j - ys * a.Ws;
    y = ys * a.stride;
    x = xs * a.stride;
    pix = (int64_t)y * a.W + x;
    Z = a.depth[(int64_t)b * a.HW + pix];
    return __builtin_isfinite(Z) && Z > a.lo && Z < a.hi && (!a.mask || a.mask[(int64_t)b * a.HW + pix] != 0);
}

// grid (nb, B), 256 threads: tilecnt[b][tile]
__global__ __launch_bounds__(kT) void k_points_count(PointArgs a, int* __restrict__ tilecnt) {
    __shared__ int wc[kT / 64];
    const int b = blockIdx.y;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        int cnt = 0;
        for (int s = 0; s < kSteps; ++s) {
            float Z;
            int y, x;
            int64_t pix;
            const bool v = point_valid(a, b, tile * kPointTile + s * kT + threadIdx.x, Z, y, x, pix);
            cnt += __popcll(__ballot(v));
        }
        if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) tilecnt[(int64_t)b * a.ntiles + tile] = (wc[0] + wc[1]) + (wc[2] + wc[3]);
        __syncthreads();
    }
}

// grid (B), 256 threads: tileoff[b][t] = sum of tilecnt[b][< t]; counts[b] = the image's total
__global__ __launch_bounds__(kT) void k_points_scan(const int* __restrict__ tilecnt, int ntiles, int* __restrict__ tileoff,
                                                    int* __restrict__ counts) {
    __shared__ int ws[kT / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < ntiles; base += kT) {
        const int t = base + threadIdx.x;
        const int c = t < ntiles ? tilecnt[(int64_t)b * ntiles + t] : 0;
        int x = c;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) ws[w] = x;
        __syncthreads();
        int off = 0;
        for (int i = 0; i < w; ++i) off += ws[i];
        if (t < ntiles) tileoff[(int64_t)b * ntiles + t] = carry + off + x - c;
        carry += (ws[0] + ws[1]) + (ws[2] + ws[3]);
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[b] = carry;
}

// grid (nb, B), 256 threads: records[b * cap + rank] = {X, Y, Z, rgba}
__global__ __launch_bounds__(kT) void k_points_write(PointArgs a, const int* __restrict__ tileoff, uint4* __restrict__ records) {
#pragma clang fp contract(off)
    __shared__ int wc[kSteps][kT / 64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* Kb = a.K + (int64_t)b * 9;
    const float fx = Kb[0], cx = Kb[2], fy = Kb[4], cy = Kb[5];
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        float Z[kSteps];
        int y[kSteps], x[kSteps];
        int64_t pix[kSteps];
        bool v[kSteps];
        unsigned long long bal[kSteps];
        for (int s = 0; s < kSteps; ++s) {
            v[s] = point_valid(a, b, tile * kPointTile + s * kT + threadIdx.x, Z[s], y[s], x[s], pix[s]);
            bal[s] = __ballot(v[s]);
            if (lane == 0) wc[s][w] = __popcll(bal[s]);
        }
        __syncthreads();
        int base = tileoff[(int64_t)b * a.ntiles + tile];
        for (int s = 0; s < kSteps; ++s) {
            int before = 0;   // the tile's valid candidates in earlier waves of this step
            for (int i = 0; i < kT / 64; ++i) before += i < w ? wc[s][i] : 0;
            if (v[s]) {
                const int rank = base + before + __popcll(bal[s] & ((1ull << lane) - 1ull));
                const float X = ((float)x[s] - cx) / fx * Z[s];
                const float Y = ((float)y[s] - cy) / fy * Z[s];
                unsigned c = 0x00FFFFFFu;
                if (a.rgb) {
                    const float* r = a.rgb + (int64_t)b * 3 * a.HW + pix[s];
                    c = to_u8(r[0]) | to_u8(r[a.HW]) << 8 | to_u8(r[2 * a.HW]) << 16;
                }
                records[(int64_t)b * a.cap + rank] =
                    make_uint4(__float_as_uint(X), __float_as_uint(Y), __float_as_uint(Z[s]), c | 0xFF000000u);
            }
            base += (wc[s][0] + wc[s][1]) + (wc[s][2] + wc[s][3]);
        }
        __syncthreads();
    }
}

// ---------------- flips ----------------
// n = rows * W elements (VEC: quads, W % 4 == 0), 1-D grid stride
template <bool VEC, bool MEAN>
__global__ __launch_bounds__(kT) void k_flip(const float* a, const float* bsrc, float* out, unsigned W, unsigned n) {   // out may be a
#pragma clang fp contract(off)
    const unsigned per = VEC ? W / 4 : W, total = VEC ? n / 4 : n;
    for (unsigned i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
        const unsigned row = i / per, c = i - row * per;
        if constexpr (VEC) {
            const int64_t at = (int64_t)row * W + 4 * c, mir = (int64_t)row * W + (W - 4 - 4 * c);
            const float4 m = *reinterpret_cast<const float4*>(bsrc + mir);
            float4 o = make_float4(m.w, m.z, m.y, m.x);
            if constexpr (MEAN) {
                const float4 p = *reinterpret_cast<const float4*>(a + at);
                o = make_float4(0.5f * (p.x + o.x), 0.5f * (p.y + o.y), 0.5f * (p.z + o.z), 0.5f * (p.w + o.w));
            }
            *reinterpret_cast<float4*>(out + at) = o;
        } else {
            const int64_t at = (int64_t)row * W + c, mir = (int64_t)row * W + (W - 1 - c);
            const float m = bsrc[mir];
            out[at] = MEAN ? 0.5f * (a[at] + m) : m;
        }
    }
}

bool a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool quad_ok(const float* depth, const float* sub, const uint8_t* mask, int64_t HW) {
    return HW % 4 == 0 && a16(depth) && a16(sub) && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
}
// blocks per image so that B of them stay within the grid cap
int blocks_per_image(int64_t work_blocks, int B) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(work_blocks, kMaxGrid / std::max(1, B)));
}

}  // namespace

int export_range_blocks(int64_t HW, int B) { return blocks_per_image(((HW + 3) / 4 + kT - 1) / kT, B); }

void export_range(const float* depth, const float* sub, const uint8_t* mask, int B, int64_t HW, float* part, float* table,
                  float* out, hipStream_t st) {
    const int nb = export_range_blocks(HW, B);
    if (quad_ok(depth, sub, mask, HW))
        hipLaunchKernelGGL(k_range_partials<true>, dim3(nb, B), dim3(kT), 0, st, depth, sub, mask, HW, part);
    else
        hipLaunchKernelGGL(k_range_partials<false>, dim3(nb, B), dim3(kT), 0, st, depth, sub, mask, HW, part);
    hipLaunchKernelGGL(k_range_final, dim3(B), dim3(64), 0, st, part, nb, table, out);
}

void export_render(const float* depth, const float* sub, const uint8_t* mask, int B, int H, int W, const float* table, float lo,
                   float hi, const uint8_t* lut, const uint8_t invalid[3], uint8_t* rgb, int64_t row_stride, int64_t col_off,
                   int64_t image_stride, uint16_t* u16, float units, hipStream_t st) {
    RenderArgs a;
    a.depth = depth; a.sub = sub; a.mask = mask; a.table = table; a.lo = lo; a.hi = hi; a.lut = lut;
    a.invalid = (unsigned)invalid[0] | (unsigned)invalid[1] << 8 | (unsigned)invalid[2] << 16;
    a.dst = PaneDst{rgb, row_stride, col_off, image_stride};
    a.u16 = u16; a.units = units; a.W = W; a.HW = (int64_t)H * W;
    const int nb = export_range_blocks(a.HW, B);
    if (quad_ok(depth, sub, mask, a.HW)) hipLaunchKernelGGL(k_render<true>, dim3(nb, B), dim3(kT), 0, st, a);
    else hipLaunchKernelGGL(k_render<false>, dim3(nb, B), dim3(kT), 0, st, a);
}

void export_image(const float* rgb, int B, int H, int W, uint8_t* dst, int64_t row_stride, int64_t col_off, int64_t image_stride,
                  hipStream_t st) {
    const int64_t HW = (int64_t)H * W;
    const int nb = export_range_blocks(HW, B);
    const PaneDst p{dst, row_stride, col_off, image_stride};
    if (HW % 4 == 0 && a16(rgb)) hipLaunchKernelGGL(k_image<true>, dim3(nb, B), dim3(kT), 0, st, rgb, HW, W, p);
    else hipLaunchKernelGGL(k_image<false>, dim3(nb, B), dim3(kT), 0, st, rgb, HW, W, p);
}

int export_point_tiles(int H, int W, int stride) {
    const int64_t cap = (int64_t)((H + stride - 1) / stride) * ((W + stride - 1) / stride);
    return (int)((cap + kPointTile - 1) / kPointTile);
}

void export_points(const float* depth, const float* K, const float* rgb, const uint8_t* mask, int B, int H, int W, int stride,
                   float min_depth, float max_depth, int* tilecnt, int* tileoff, void* records, int* counts, hipStream_t st) {
    PointArgs a;
    a.depth = depth; a.K = K; a.rgb = rgb; a.mask = mask; a.W = W; a.stride = stride;
    a.Ws = (W + stride - 1) / stride;
    a.cap = ((H + stride - 1) / stride) * a.Ws;
    a.ntiles = export_point_tiles(H, W, stride);
    a.HW = (int64_t)H * W; a.lo = min_depth; a.hi = max_depth;
    const int nb = blocks_per_image(a.ntiles, B);
    hipLaunchKernelGGL(k_points_count, dim3(nb, B), dim3(kT), 0, st, a, tilecnt);
    hipLaunchKernelGGL(k_points_scan, dim3(B), dim3(kT), 0, st, tilecnt, a.ntiles, tileoff, counts);
    hipLaunchKernelGGL(k_points_write, dim3(nb, B), dim3(kT), 0, st, a, tileoff, static_cast<uint4*>(records));
}

void export_flip(const float* a, const float* b, float* out, int64_t rows, int W, hipStream_t st) {
    const unsigned n = (unsigned)(rows * W);
    const bool vec = W % 4 == 0 && a16(a) && a16(b) && a16(out);
    const unsigned total = vec ? n / 4 : n;
    const int grid = (int)std::max<unsigned>(1u, std::min<unsigned>((total + kT - 1) / kT, (unsigned)kMaxGrid));
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kT), 0, st, a, b, out, (unsigned)W, n); };
    if (a) vec ? launch(k_flip<true, true>) : launch(k_flip<false, true>);
    else vec ? launch(k_flip<true, false>) : launch(k_flip<false, false>);
}

}  // namespace cad
