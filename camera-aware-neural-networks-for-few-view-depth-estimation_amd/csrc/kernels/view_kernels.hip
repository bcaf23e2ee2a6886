// Virtual cameras (cad.h, "virtual cameras"; no reference counterpart): the image and the ground-truth depth
// a camera with other intrinsics K', or rotated about its centre by R (P' = R P), would have recorded.
// Neither change has parallax, so both follow exactly from the recorded sample.
//
// Conventions: pixel centres at integer coordinates, depth is Z along the optical axis, x right, y down,
// z forward, skew ignored.  Per output pixel (u', v'):
//
//   d' = ((u' - cx') / fx', (v' - cy') / fy', 1)        d = R^T d'
//   u  = (fx d.x) / d.z + cx                            v = (fy d.y) / d.z + cy
//   rgb    bilinear between floor and floor + 1 of (u, v) clamped to [0, W-1] x [0, H-1] (edge replicate);
//          0 where d.z <= 0 or a coordinate is not finite
//   depth  nearest, iu = floor(u + 0.5), iv = floor(v + 0.5):  Z' = Z(iv, iu) / d.z  where 0 <= iu < W,
//          0 <= iv < H, d.z > 0, Z(iv, iu) finite and positive [and mask(iv, iu) != 0]; 0 (a hole) otherwise
//   valid  that predicate
//
// A sample with R == I and K' == K (fx, fy, cx, cy bit for bit) is copied: rgb and depth keep their bits,
// no arithmetic touches them (valid is still the predicate at the pixel itself).  With R == I alone d.z is
// (0 dx + 0 dy) + 1 == 1, so Z' keeps the bits of the sampled Z.
//
// Every fp32 operation of the coordinates is written out under fp contract(off) in the order above (sums
// left to right), divisions are the correctly rounded ones, so a fp32 restatement gives the same bits.
//
// One pass writes rgb, depth and valid: grid (min(1024, ceil(HW / 256)), B) x 256 threads, a thread walks
// pixels p, p + grid, ... with p consecutive along x, so the 17 bytes per pixel it writes (3 + 1 floats and a
// byte) are coalesced 4-byte and 1-byte stores.  The gathers (4 taps x 3 planes, one depth and one mask
// tap) are plain vector loads: neighbouring lanes read neighbouring source pixels under any smooth view, the
// compulsory traffic is the 16 (17) bytes per source pixel once, the rest is served by L2.  Plane offsets are
// 64-bit.  Nothing here is worth LDS: no value is shared between lanes in a pattern known before the view is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>

#include "kernels.hpp"

namespace cad {
namespace {

constexpr int kViewThreads = 256;
constexpr int kViewMaxBlocks = 1024;

struct ViewCam {
    float fx, fy, cx, cy;
};
__device__ __forceinline__ ViewCam view_cam(const float* __restrict__ K, int b) {
    const float* Kb = K + (int64_t)b * 9;
    ViewCam c;
    c.fx = Kb[0];
    c.cx = Kb[2];
    c.fy = Kb[4];
    c.cy = Kb[5];
    return c;
}

// K' of one view for every sample (one thread per sample); R is the view's, the same for all of them.
// Entries of K other than fx, fy, cx, cy are carried over.
__global__ void k_view_resolve(ViewParams v, const float* __restrict__ K, int B, int H, int W, float* __restrict__ K_new,
                               float* __restrict__ R) {
    // (the product and the sum of cx', cy' are rounded one by one: __fmul_rn / __fadd_rn are inline functions over
    // the plain operators and get contracted, the pragma binds the operators written in its scope)
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* Kb = K + (int64_t)b * 9;
    float* Kn = K_new + (int64_t)b * 9;
    for (int i = 0; i < 9; ++i) Kn[i] = Kb[i];
    const float sx = v.shift_x * (float)W, sy = v.shift_y * (float)H;
    Kn[0] = v.zoom_x * Kb[0];
    Kn[4] = v.zoom_y * Kb[4];
    Kn[2] = Kb[2] + sx;
    Kn[5] = Kb[5] + sy;
    for (int i = 0; i < 9; ++i) R[(int64_t)b * 9 + i] = v.R[i];
}

__device__ __forceinline__ bool view_depth_ok(float z) { return z > 0.f && z <= 3.402823466e38f; }   // finite, positive

__global__ void __launch_bounds__(kViewThreads)
k_camera_view(const float* __restrict__ rgb, const float* __restrict__ depth, const uint8_t* __restrict__ mask,
              const float* __restrict__ K, const float* __restrict__ K_new, const float* __restrict__ R, int H, int W,
              float* __restrict__ rgb_out, float* __restrict__ depth_out, uint8_t* __restrict__ valid_out) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    const ViewCam k = view_cam(K, b), kn = view_cam(K_new, b);
    float r[9];
    for (int i = 0; i < 9; ++i) r[i] = R[(int64_t)b * 9 + i];
    const bool rot = !(r[0] == 1.f && r[1] == 0.f && r[2] == 0.f && r[3] == 0.f && r[4] == 1.f && r[5] == 0.f && r[6] == 0.f &&
                       r[7] == 0.f && r[8] == 1.f);
    const bool same_k = __float_as_uint(k.fx) == __float_as_uint(kn.fx) && __float_as_uint(k.fy) == __float_as_uint(kn.fy) &&
                        __float_as_uint(k.cx) == __float_as_uint(kn.cx) && __float_as_uint(k.cy) == __float_as_uint(kn.cy);
    const float* src = rgb + (int64_t)b * 3 * HW;
    const float* dsrc = depth + (int64_t)b * HW;
    const uint8_t* msrc = mask ? mask + (int64_t)b * HW : nullptr;
    float* out = rgb_out + (int64_t)b * 3 * HW;
    float* dout = depth_out + (int64_t)b * HW;
    uint8_t* vout = valid_out ? valid_out + (int64_t)b * HW : nullptr;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    if (!rot && same_k) {   // the identity view: a copy (uniform over the block)
        for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += step) {
            out[p] = src[p];
            out[HW + p] = src[HW + p];
            out[2 * HW + p] = src[2 * HW + p];
            const float z = dsrc[p];
            dout[p] = z;
            if (vout) vout[p] = (view_depth_ok(z) && (!msrc || msrc[p] != 0)) ? 1 : 0;
        }
        return;
    }
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += step) {
        const int yo = (int)((uint32_t)p / (uint32_t)W), xo = (int)p - yo * W;   // p < H W < 2^31 (the C ABI checks)
        const float dx = ((float)xo - kn.cx) / kn.fx;
        const float dy = ((float)yo - kn.cy) / kn.fy;
        const float ex = (r[0] * dx + r[3] * dy) + r[6];
        const float ey = (r[1] * dx + r[4] * dy) + r[7];
        const float ez = (r[2] * dx + r[5] * dy) + r[8];
        const float u = (k.fx * ex) / ez + k.cx;
        const float v = (k.fy * ey) / ez + k.cy;
        const bool front = ez > 0.f;
        const bool finite = fabsf(u) <= 3.402823466e38f && fabsf(v) <= 3.402823466e38f;   // false for NaN
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, z = 0.f;
        bool ok = false;
        if (front && finite) {
            const float uc = fminf(fmaxf(u, 0.f), wmax), vc = fminf(fmaxf(v, 0.f), hmax);
            const float fu = floorf(uc), fv = floorf(vc);
            const int x0 = (int)fu, y0 = (int)fv;
            const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
            const float lx1 = uc - fu, lx0 = 1.f - lx1, ly1 = vc - fv, ly0 = 1.f - ly1;
            const int64_t o00 = (int64_t)y0 * W + x0, o01 = (int64_t)y0 * W + x1, o10 = (int64_t)y1 * W + x0,
                          o11 = (int64_t)y1 * W + x1;
            float c[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float* pl = src + ch * HW;
                const float t0 = pl[o00] * lx0 + pl[o01] * lx1;
                const float t1 = pl[o10] * lx0 + pl[o11] * lx1;
                c[ch] = t0 * ly0 + t1 * ly1;
            }
            c0 = c[0];
            c1 = c[1];
            c2 = c[2];
            // nearest depth: the range test in float, so that a far-off coordinate never reaches the cast
            const float nu = floorf(u + 0.5f), nv = floorf(v + 0.5f);
            if (nu >= 0.f && nu < (float)W && nv >= 0.f && nv < (float)H) {
                const int64_t o = (int64_t)(int)nv * W + (int)nu;
                const float zs = dsrc[o];
                if (view_depth_ok(zs) && (!msrc || msrc[o] != 0)) {
                    ok = true;
                    z = zs / ez;
                }
            }
        }
        out[p] = c0;
        out[HW + p] = c1;
        out[2 * HW + p] = c2;
        dout[p] = z;
        if (vout) vout[p] = ok ? 1 : 0;
    }
}

}  // namespace

void view_resolve(const ViewParams& v, const float* K, int B, int H, int W, float* K_new, float* R, hipStream_t st) {
    CAD_NO_ALIAS("view_resolve", {aview(K_new, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "K_new"), aview(R, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "R")},
                 {aview(K, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "K")});
    CAD_NO_ALIAS("view_resolve", {aview(K_new, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "K_new")},
                 {aview(R, 1, (int64_t)B * 9, 0, (int64_t)B * 9, 4, "R")});
    hipLaunchKernelGGL(k_view_resolve, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, v, K, B, H, W, K_new, R);
}

void camera_view(const float* rgb, const float* depth, const uint8_t* mask, const float* K, const float* K_new, const float* R,
                 int B, int H, int W, float* rgb_out, float* depth_out, uint8_t* valid_out, hipStream_t st) {
    const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW, k9 = (int64_t)B * 9;
    CAD_NO_ALIAS("camera_view",
                 {aview(rgb_out, 1, 3 * n, 0, 3 * n, 4, "rgb_out"), aview(depth_out, 1, n, 0, n, 4, "depth_out"),
                  aview(valid_out, 1, n, 0, n, 1, "valid_out")},
                 {aview(rgb, 1, 3 * n, 0, 3 * n, 4, "rgb"), aview(depth, 1, n, 0, n, 4, "depth"), aview(mask, 1, n, 0, n, 1, "mask"),
                  aview(K, 1, k9, 0, k9, 4, "K"), aview(K_new, 1, k9, 0, k9, 4, "K_new"), aview(R, 1, k9, 0, k9, 4, "R")});
    // the outputs among themselves: every thread writes all three at its own pixel
    CAD_NO_ALIAS("camera_view", {aview(rgb_out, 1, 3 * n, 0, 3 * n, 4, "rgb_out")},
                 {aview(depth_out, 1, n, 0, n, 4, "depth_out"), aview(valid_out, 1, n, 0, n, 1, "valid_out")});
    CAD_NO_ALIAS("camera_view", {aview(depth_out, 1, n, 0, n, 4, "depth_out")}, {aview(valid_out, 1, n, 0, n, 1, "valid_out")});
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(kViewMaxBlocks, (HW + kViewThreads - 1) / kViewThreads)),
                    (unsigned)B);
    hipLaunchKernelGGL(k_camera_view, grid, dim3(kViewThreads), 0, st, rgb, depth, mask, K, K_new, R, H, W, rgb_out, depth_out,
                       valid_out);
}

}  // namespace cad
