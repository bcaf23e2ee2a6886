// Geometric evaluation: surface-normal angular error and 3-D point error from K (cad.h, "geometric
// evaluation"; no reference counterpart: the reference scores depth ratios only).
//
//   valid   the evaluator's set: gt > min_depth && gt < max_depth (strict) [&& mask != 0]
//   p       the metrics pass's prediction: clamp(scale * pred + shift) with the sample's alignment row
//   normal  of a depth map d at pixel (u, v), x = (u - cx) / fx, y = (v - cy) / fy, central differences in
//           the cancellation-free closed form
//             a = d(u+1,v) - d(u-1,v)   A = (d(u+1,v) + d(u-1,v)) / fx
//             b = d(u,v+1) - d(u,v-1)   B = (d(u,v+1) + d(u,v-1)) / fy
//             c = (-a B, -A b, A B + x a B + y A b),   n = -c / |c|
//           normal-valid: the pixel and its four neighbours are valid (hence interior) and both c are
//           finite with |c| > 0
//   theta   atan2f(|n_p x n_g|, n_p . n_g) * (float)(180 / pi), degrees
//   e       |p - g| * sqrtf(1 + x x + y y) over the valid set
//   sums    {n_normal, theta, theta^2, #(theta < 11.25), #(theta < 22.5), #(theta < 30), e, e^2}
//
// Per-pixel terms are individually rounded fp32 operations, accumulated in double.  The walk: a sample is
// cut into tiles of 64 columns x kGeomRows rows; tile t goes to wave t % 4 of block (t / 4) % nb, tiles in
// increasing order.  A wave walks its tile's rows top to bottom with one pixel per lane, carries the two
// rows above in registers, takes the horizontal neighbours from lanes -1 / +1 and re-loads the halo column
// of the strip in lanes 0 and 63, so a pixel is fetched from memory once per tile that touches it (rows:
// (kGeomRows + 2) / kGeomRows, columns: 66 / 64).  There is one loader (4-byte, coalesced over the 64
// lanes), so aligned and unaligned tensors run the same code; nb depends on H and W alone; no atomics:
// lanes are added with a fixed xor butterfly, waves and blocks in index order.  A sample's row is the
// same bits on every run, in whichever batch it arrives, from aligned or unaligned tensors.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace cad {
namespace {

constexpr int kGeomThreads = 256;
constexpr int kGeomWaves = kGeomThreads / 64;
constexpr int kGeomRows = 16;
constexpr int kGeomSums = 8;

template <int ND>
struct GeomPx {
    float d[ND];
    bool v;
};
template <int ND>
struct GeomRow {
    GeomPx<ND> c, l, r;   // the lane's pixel, its left and its right neighbour
};

template <int ND>
__device__ __forceinline__ GeomPx<ND> geom_none() {
    GeomPx<ND> p;
    for (int k = 0; k < ND; ++k) p.d[k] = 0.f;
    p.v = false;
    return p;
}

// Row `row` of the strip whose lane 0 is column col - lane.  Must be reached by all lanes of the wave.
// load(row, col) is only called inside the image.
template <int ND, class Load>
__device__ __forceinline__ GeomRow<ND> geom_load_row(int row, int col, int H, int W, Load&& load) {
    const int lane = threadIdx.x & 63;
    const bool in = row >= 0 && row < H;
    GeomRow<ND> R;
    R.c = (in && col < W) ? load(row, col) : geom_none<ND>();
    for (int k = 0; k < ND; ++k) {
        R.l.d[k] = __shfl_up(R.c.d[k], 1);
        R.r.d[k] = __shfl_down(R.c.d[k], 1);
    }
    const int v = R.c.v ? 1 : 0;
    R.l.v = __shfl_up(v, 1) != 0;
    R.r.v = __shfl_down(v, 1) != 0;
    if (lane == 0) R.l = (in && col >= 1 && col - 1 < W) ? load(row, col - 1) : geom_none<ND>();
    if (lane == 63) R.r = (in && col + 1 < W) ? load(row, col + 1) : geom_none<ND>();
    return R;
}

// The walk described at the top: emit(row, col, centre, left, right, up, down) once per pixel of the image.
template <int ND, class Load, class Emit>
__device__ __forceinline__ void geom_walk(int H, int W, int nb, Load&& load, Emit&& emit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nstrips = (W + 63) / 64, nbands = (H + kGeomRows - 1) / kGeomRows;
    const int ntiles = nstrips * nbands;
    for (int t = blockIdx.x * kGeomWaves + wave; t < ntiles; t += nb * kGeomWaves) {
        const int band = t / nstrips, strip = t - band * nstrips;
        const int col = strip * 64 + lane;
        const int r0 = band * kGeomRows, r1 = min(H, r0 + kGeomRows);
        GeomRow<ND> up = geom_load_row<ND>(r0 - 1, col, H, W, load);
        GeomRow<ND> cen = geom_load_row<ND>(r0, col, H, W, load);
        for (int row = r0; row < r1; ++row) {
            const GeomRow<ND> dn = geom_load_row<ND>(row + 1, col, H, W, load);
            if (col < W) emit(row, col, cen.c, cen.l, cen.r, up.c, dn.c);
            up = cen;
            cen = dn;
        }
    }
}

struct GeomCam {
    float fx, fy, cx, cy;
};
__device__ __forceinline__ GeomCam geom_cam(const float* __restrict__ K, int b) {
    const float* Kb = K + (int64_t)b * 9;
    GeomCam c;
    c.fx = Kb[0];
    c.cx = Kb[2];
    c.fy = Kb[4];
    c.cy = Kb[5];
    return c;
}

// n = -c / |c| of the closed form; false when c is not finite or |c| == 0
__device__ __forceinline__ bool geom_normal(float dl, float dr, float du, float dd, float x, float y, const GeomCam& k,
                                            float (&n)[3]) {
#pragma clang fp contract(off)
    const float a = dr - dl;
    const float A = (dr + dl) / k.fx;
    const float b = dd - du;
    const float B = (dd + du) / k.fy;
    const float c0 = -(a * B);
    const float c1 = -(A * b);
    const float t1 = A * B;
    const float t2 = (x * a) * B;
    const float t3 = (y * A) * b;
    const float c2 = (t1 + t2) + t3;
    const float len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    if (!(__builtin_isfinite(len) && len > 0.f)) return false;
    n[0] = -c0 / len;
    n[1] = -c1 / len;
    n[2] = -c2 / len;
    return true;
}

__device__ __forceinline__ float geom_theta(const float (&p)[3], const float (&g)[3]) {
#pragma clang fp contract(off)
    const float x0 = p[1] * g[2] - p[2] * g[1];
    const float x1 = p[2] * g[0] - p[0] * g[2];
    const float x2 = p[0] * g[1] - p[1] * g[0];
    const float s = sqrtf((x0 * x0 + x1 * x1) + x2 * x2);
    const float c = (p[0] * g[0] + p[1] * g[1]) + p[2] * g[2];
    return atan2f(s, c) * 57.29577951308232f;
}

// grid (nb, B), 256 threads.  part: [B][nb][8]; theta / nvalid: [B][HW] (every pixel is written).
// align: the evaluator's [rows][2] table (row base + b) or null.
__global__ __launch_bounds__(kGeomThreads) void k_geom_partials(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const uint8_t* __restrict__ mask, const float* __restrict__ K,
                                                                int H, int W, float lo, float hi, int clamp_pred,
                                                                const float* __restrict__ align, int64_t base,
                                                                float* __restrict__ theta, uint8_t* __restrict__ nvalid,
                                                                double* __restrict__ part, int nb) {
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    float as = 1.f, at = 0.f;
    if (align) {
        as = align[(base + b) * 2];
        at = align[(base + b) * 2 + 1];
    }
    const GeomCam cam = geom_cam(K, b);
    const float* ps = pred + (int64_t)b * HW;
    const float* gs = gt + (int64_t)b * HW;
    const uint8_t* ms = mask ? mask + (int64_t)b * HW : nullptr;
    float* ts = theta + (int64_t)b * HW;
    uint8_t* vs = nvalid + (int64_t)b * HW;
    double acc[kGeomSums];
    for (int k = 0; k < kGeomSums; ++k) acc[k] = 0.0;

    const auto load = [&](int row, int col) {
#pragma clang fp contract(off)
        const int i = row * W + col;   // H * W < 2^31 (checked by the host)
        GeomPx<2> px;
        float pr = ps[i];
        if (align) {
            const float m = as * pr;   // eval_kernels.hip's align_pred
            pr = m + at;
        }
        px.d[0] = clamp_pred ? fminf(fmaxf(pr, lo), hi) : pr;
        px.d[1] = gs[i];
        px.v = px.d[1] > lo && px.d[1] < hi && (ms ? ms[i] != 0 : true);
        return px;
    };
    const auto emit = [&](int row, int col, const GeomPx<2>& c, const GeomPx<2>& l, const GeomPx<2>& r, const GeomPx<2>& u,
                          const GeomPx<2>& d) {
#pragma clang fp contract(off)
        const int i = row * W + col;
        const float x = ((float)col - cam.cx) / cam.fx;
        const float y = ((float)row - cam.cy) / cam.fy;
        if (c.v) {
            const float e = fabsf(c.d[0] - c.d[1]) * sqrtf((1.0f + x * x) + y * y);
            acc[6] += (double)e;
            acc[7] += (double)(e * e);
        }
        bool nv = c.v && l.v && r.v && u.v && d.v;
        float th = 0.f;
        if (nv) {
            float np[3], ng[3];
            nv = geom_normal(l.d[0], r.d[0], u.d[0], d.d[0], x, y, cam, np) &&
                 geom_normal(l.d[1], r.d[1], u.d[1], d.d[1], x, y, cam, ng);
            if (nv) {
                th = geom_theta(np, ng);
                acc[0] += 1.0;
                acc[1] += (double)th;
                acc[2] += (double)(th * th);
                acc[3] += th < 11.25f ? 1.0 : 0.0;
                acc[4] += th < 22.5f ? 1.0 : 0.0;
                acc[5] += th < 30.0f ? 1.0 : 0.0;
            }
        }
        ts[i] = th;
        vs[i] = nv ? 1 : 0;
    };
    geom_walk<2>(H, W, nb, load, emit);

    __shared__ double red[kGeomWaves][kGeomSums];
    for (int k = 0; k < kGeomSums; ++k) {
        double s = acc[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kGeomSums)
        part[((int64_t)b * nb + blockIdx.x) * kGeomSums + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// grid (B), 64 threads: row base + b of the table = the sample's nb partial rows added in index order
__global__ __launch_bounds__(64) void k_geom_final(const double* __restrict__ part, int nb, double* __restrict__ table,
                                                   int64_t base) {
    const int b = blockIdx.x;
    if (threadIdx.x >= kGeomSums) return;
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[((int64_t)b * nb + i) * kGeomSums + threadIdx.x];
    table[(base + b) * kGeomSums + threadIdx.x] = s;
}

struct NormalsArgs {
    const float* depth;
    const float* K;
    const uint8_t* mask;   // or null
    int H, W, nb;
    float lo, hi;          // valid: isfinite(d) && lo < d < hi && mask != 0
    float* normals;        // (B,3,H,W), or null
    uint8_t* valid;        // (B,H,W), or null
    uint8_t* rgb;          // RGB8 HWC pane, or null
    int64_t row_stride, col_off, image_stride;
    unsigned invalid;      // r | g << 8 | b << 16
};

__device__ __forceinline__ unsigned geom_u8(float t) {
#pragma clang fp contract(off)
    return (unsigned)rintf(fminf(fmaxf(t, 0.f), 1.f) * 255.0f);
}

// grid (nb, B), 256 threads
__global__ __launch_bounds__(kGeomThreads) void k_depth_normals(NormalsArgs a) {
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)a.H * a.W;
    const GeomCam cam = geom_cam(a.K, b);
    const float* ds = a.depth + (int64_t)b * HW;
    const uint8_t* ms = a.mask ? a.mask + (int64_t)b * HW : nullptr;
    const auto load = [&](int row, int col) {
        const int i = row * a.W + col;
        GeomPx<1> px;
        px.d[0] = ds[i];
        px.v = __builtin_isfinite(px.d[0]) && px.d[0] > a.lo && px.d[0] < a.hi && (ms ? ms[i] != 0 : true);
        return px;
    };
    const auto emit = [&](int row, int col, const GeomPx<1>& c, const GeomPx<1>& l, const GeomPx<1>& r, const GeomPx<1>& u,
                          const GeomPx<1>& d) {
#pragma clang fp contract(off)
        const int i = row * a.W + col;
        const float x = ((float)col - cam.cx) / cam.fx;
        const float y = ((float)row - cam.cy) / cam.fy;
        float n[3] = {0.f, 0.f, 0.f};
        bool nv = c.v && l.v && r.v && u.v && d.v;
        if (nv) nv = geom_normal(l.d[0], r.d[0], u.d[0], d.d[0], x, y, cam, n);
        if (!nv) n[0] = n[1] = n[2] = 0.f;
        if (a.normals) {
            float* o = a.normals + (int64_t)b * 3 * HW + i;
            o[0] = n[0];
            o[HW] = n[1];
            o[2 * HW] = n[2];
        }
        if (a.valid) a.valid[(int64_t)b * HW + i] = nv ? 1 : 0;
        if (a.rgb) {
            unsigned c3 = a.invalid;
            if (nv)
                c3 = geom_u8((n[0] + 1.0f) / 2.0f) | geom_u8((1.0f - n[1]) / 2.0f) << 8 | geom_u8((1.0f - n[2]) / 2.0f) << 16;
            uint8_t* o = a.rgb + ((int64_t)b * a.image_stride + (int64_t)row * a.row_stride + a.col_off + col) * 3;
            o[0] = (uint8_t)(c3 & 255u);
            o[1] = (uint8_t)((c3 >> 8) & 255u);
            o[2] = (uint8_t)((c3 >> 16) & 255u);
        }
    };
    geom_walk<1>(a.H, a.W, a.nb, load, emit);
}

}  // namespace

int eval_geom_blocks(int H, int W) {
    const int64_t tiles = (int64_t)((W + 63) / 64) * ((H + kGeomRows - 1) / kGeomRows);
    return (int)std::max<int64_t>(1, std::min<int64_t>(128, (tiles + kGeomWaves - 1) / kGeomWaves));
}

void eval_geom_update(const float* pred, const float* gt, const uint8_t* mask, const float* K, int B, int H, int W,
                      float min_depth, float max_depth, int clamp_pred, const float* align, int64_t base, float* theta,
                      uint8_t* nvalid, double* part, int nb, double* table, const EvalAlignWs& ws, int nb_select, float* med2,
                      hipStream_t st) {
    const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
    CAD_NO_ALIAS("eval_geom_update",
                 {aview(theta, 1, n, 0, n, 4, "theta map"), aview(nvalid, 1, n, 0, n, 1, "normal-valid map"),
                  aview(part, 1, (int64_t)B * nb * kGeomSums, 0, (int64_t)B * nb * kGeomSums, 8, "geometry partials"),
                  aview(table + base * kGeomSums, 1, (int64_t)B * kGeomSums, 0, (int64_t)B * kGeomSums, 8, "geometry rows")},
                 {aview(pred, 1, n, 0, n, 4, "pred"), aview(gt, 1, n, 0, n, 4, "gt"),
                  aview(mask, 1, mask ? n : 0, 0, mask ? n : 0, 1, "mask"), aview(K, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "K")});
    hipLaunchKernelGGL(k_geom_partials, dim3(nb, B), dim3(kGeomThreads), 0, st, pred, gt, mask, K, H, W, min_depth, max_depth,
                       clamp_pred, align, base, theta, nvalid, part, nb);
    hipLaunchKernelGGL(k_geom_final, dim3(B), dim3(64), 0, st, part, nb, table, base);
    // the normal-valid set is a subset of the valid set: med_pred of the select is the median of theta
    eval_valid_medians(theta, gt, nvalid, B, HW, min_depth, max_depth, ws, nb_select, med2 + base * 2, st);
}

void depth_normals(const float* depth, const float* K, const uint8_t* mask, int B, int H, int W, float lo, float hi,
                   float* normals, uint8_t* valid, uint8_t* rgb, int64_t row_stride, int64_t col_off, int64_t image_stride,
                   const uint8_t invalid[3], hipStream_t st) {
    const int64_t n = (int64_t)B * H * W;
    const int64_t span = rgb ? ((int64_t)(B - 1) * image_stride + (int64_t)(H - 1) * row_stride + col_off + W) * 3 : 0;
    CAD_NO_ALIAS("depth_normals",
                 {aview(normals, 1, normals ? 3 * n : 0, 0, normals ? 3 * n : 0, 4, "normals"),
                  aview(valid, 1, valid ? n : 0, 0, valid ? n : 0, 1, "valid map"), aview(rgb, 1, span, 0, span, 1, "rgb pane")},
                 {aview(depth, 1, n, 0, n, 4, "depth"), aview(mask, 1, mask ? n : 0, 0, mask ? n : 0, 1, "mask"),
                  aview(K, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "K")});
    NormalsArgs a;
    a.depth = depth; a.K = K; a.mask = mask;
    a.H = H; a.W = W; a.nb = eval_geom_blocks(H, W);
    a.lo = lo; a.hi = hi;
    a.normals = normals; a.valid = valid; a.rgb = rgb;
    a.row_stride = row_stride; a.col_off = col_off; a.image_stride = image_stride;
    a.invalid = invalid ? ((unsigned)invalid[0] | (unsigned)invalid[1] << 8 | (unsigned)invalid[2] << 16) : 0u;
    hipLaunchKernelGGL(k_depth_normals, dim3(a.nb, B), dim3(kGeomThreads), 0, st, a);
}

}  // namespace cad
