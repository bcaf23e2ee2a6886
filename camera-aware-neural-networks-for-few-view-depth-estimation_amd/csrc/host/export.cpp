// Inference export behind include/cad/cad.h: the cad_exporter handle over csrc/kernels/export_kernels.hip
// (depth renders, 16-bit depth, point clouds; DepthVisualizer, src/visualization/depth_viz.h:23-148), the flip
// helpers of test-time augmentation, and the host side of the files: the integer colour tables, a PNG
// encoder (zlib deflate over adaptively filtered scanlines; the decoder is dataset.cpp's) and the PLY writer.
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/cad/cad.h"
#include "../kernels/kernels.hpp"

namespace cad {
void set_last_error(const std::string& msg);   // cad_api.cpp (cad_last_error)
}

namespace {

struct XError : std::runtime_error {
    cad_status st;
    XError(cad_status s, const std::string& m) : std::runtime_error(m), st(s) {}
};
#define XCHK(expr)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            throw XError(e_ == hipErrorOutOfMemory ? CAD_ERR_OOM : CAD_ERR_HIP,                 \
                         std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)
void need(bool c, const std::string& m) {
    if (!c) throw XError(CAD_ERR_INVALID, m);
}
template <class F>
cad_status xguard(F&& f) {
    try {
        f();
        return CAD_OK;
    } catch (const XError& e) {
        cad::set_last_error(e.what());
        return e.st;
    } catch (const std::exception& e) {
        cad::set_last_error(e.what());
        return CAD_ERR_INVALID;
    }
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

int clamp255(int v) { return std::min(255, std::max(0, v)); }

bool builtin_lut(int id, uint8_t* out) {
    for (int i = 0; i < 256; ++i) {
        int r, g, b;
        switch (id) {
            case CAD_CMAP_GRAY: r = g = b = i; break;
            case CAD_CMAP_JET:
                r = 383 - std::abs(4 * i - 765);
                g = 383 - std::abs(4 * i - 510);
                b = 383 - std::abs(4 * i - 255);
                break;
            case CAD_CMAP_HOT:
                r = 8 * i / 3;
                g = 8 * std::max(i - 96, 0) / 3;
                b = std::max(0, 4 * (i - 191) - 1);
                break;
            default: return false;
        }
        out[3 * i] = (uint8_t)clamp255(r);
        out[3 * i + 1] = (uint8_t)clamp255(g);
        out[3 * i + 2] = (uint8_t)clamp255(b);
    }
    return true;
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- PNG ----
void put32(std::vector<uint8_t>& v, uint32_t x) {
    for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
void put_chunk(std::vector<uint8_t>& png, const char type[4], const uint8_t* data, size_t len) {
    put32(png, (uint32_t)len);
    const size_t at = png.size();
    png.insert(png.end(), type, type + 4);
    if (len) png.insert(png.end(), data, data + len);
    put32(png, (uint32_t)crc32(0L, png.data() + at, (uInt)(len + 4)));
}
int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
}
int64_t png_bound(int h, int w, int channels, int bits) {
    const size_t raw = ((size_t)w * channels * bits / 8 + 1) * (size_t)h;
    return (int64_t)(8 + 25 + 12 + compressBound((uLong)raw) + 12);
}

}  // namespace

struct cad_exporter {
    int device = 0, Bmax = 0, H = 0, W = 0;
    char* mem = nullptr;        // one allocation, carved below
    float* table = nullptr;     // [Bmax][2] range table
    float* part = nullptr;      // range partials
    int* tilecnt = nullptr;     // [Bmax][tiles at stride 1]
    int* tileoff = nullptr;
    uint8_t* luts = nullptr;    // [4][768]: gray, jet, hot, custom
};

extern "C" {

cad_status cad_colormap_lut(const char* name, uint8_t* out768) {
    return xguard([&] {
        need(name && out768, "null argument");
        const std::string n = name;
        const int id = n == "gray" ? CAD_CMAP_GRAY : n == "jet" ? CAD_CMAP_JET : n == "hot" ? CAD_CMAP_HOT : -1;
        need(id >= 0, "unknown colormap '" + n + "': expected gray, jet or hot");
        builtin_lut(id, out768);
    });
}

cad_status cad_exporter_create(int max_batch, int H, int W, int device, cad_exporter** out) {
    return xguard([&] {
        need(out != nullptr, "null output handle");
        need(max_batch > 0, "exporter max_batch must be positive");
        need(H > 0 && W > 0, "exporter H and W must be positive");
        need((int64_t)H * W <= (int64_t(1) << 30), "exporter images hold at most 2^30 pixels");
        XCHK(hipSetDevice(device));
        auto e = std::make_unique<cad_exporter>();
        e->device = device; e->Bmax = max_batch; e->H = H; e->W = W;
        const size_t tiles = (size_t)max_batch * cad::export_point_tiles(H, W, 1);
        const size_t tb = up256(sizeof(float) * 2 * max_batch);
        const size_t pb = up256(sizeof(float) * 2 * std::max<size_t>(2048, max_batch));
        const size_t cb = up256(sizeof(int) * tiles);
        const size_t lb = up256(4 * 768);
        XCHK(hipMalloc((void**)&e->mem, tb + pb + 2 * cb + lb));
        e->table = reinterpret_cast<float*>(e->mem);
        e->part = reinterpret_cast<float*>(e->mem + tb);
        e->tilecnt = reinterpret_cast<int*>(e->mem + tb + pb);
        e->tileoff = reinterpret_cast<int*>(e->mem + tb + pb + cb);
        e->luts = reinterpret_cast<uint8_t*>(e->mem + tb + pb + 2 * cb);
        uint8_t host[4 * 768];
        for (int id = 0; id < 3; ++id) builtin_lut(id, host + 768 * id);
        builtin_lut(CAD_CMAP_GRAY, host + 768 * CAD_CMAP_CUSTOM);   // until cad_exporter_set_lut
        hipError_t err = hipMemset(e->mem, 0, tb + pb + 2 * cb);
        if (err == hipSuccess) err = hipMemcpy(e->luts, host, sizeof(host), hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            (void)hipFree(e->mem);
            XCHK(err);
        }
        *out = e.release();
    });
}

void cad_exporter_destroy(cad_exporter* e) {
    if (!e) return;
    (void)hipFree(e->mem);
    delete e;
}

cad_status cad_exporter_set_lut(cad_exporter* e, const uint8_t* lut768) {
    return xguard([&] {
        need(e && lut768, "null argument");
        XCHK(hipSetDevice(e->device));
        XCHK(hipMemcpy(e->luts + 768 * CAD_CMAP_CUSTOM, lut768, 768, hipMemcpyHostToDevice));
    });
}

cad_status cad_exporter_range(cad_exporter* e, const float* depth, const float* sub, const uint8_t* mask, int B, float* out,
                              void* stream) {
    return xguard([&] {
        need(e && depth, "null argument");
        need(B >= 1 && B <= e->Bmax, "batch exceeds the exporter's max_batch");
        XCHK(hipSetDevice(e->device));
        cad::export_range(depth, sub, mask, B, (int64_t)e->H * e->W, e->part, e->table, out, S(stream));
        XCHK(hipGetLastError());
    });
}

namespace {
struct Pane {
    int64_t row_stride, col_off, image_stride;
};
Pane pane_of(const cad_exporter* e, const cad_render_opts* o) {
    Pane p;
    p.row_stride = o->row_stride ? o->row_stride : e->W;
    p.col_off = o->col_offset;
    need(p.col_off >= 0 && p.row_stride >= p.col_off + e->W, "render: the pane does not fit in a destination row");
    p.image_stride = o->image_stride ? o->image_stride : (int64_t)e->H * p.row_stride;
    need(p.image_stride >= ((int64_t)e->H - 1) * p.row_stride + e->W, "render: image_stride is smaller than an image");
    return p;
}
}  // namespace

cad_status cad_exporter_render(cad_exporter* e, const float* depth, const float* sub, const uint8_t* mask, int B,
                               const cad_render_opts* opts, uint8_t* rgb_out, uint16_t* u16_out, void* stream) {
    return xguard([&] {
        need(e && depth && opts, "null argument");
        need(rgb_out || u16_out, "render: no output requested");
        need(B >= 1 && B <= e->Bmax, "batch exceeds the exporter's max_batch");
        need(opts->colormap >= CAD_CMAP_GRAY && opts->colormap <= CAD_CMAP_CUSTOM, "render: unknown colormap");
        need((reinterpret_cast<uintptr_t>(u16_out) & 1) == 0, "render: u16_out must be 2-byte aligned");
        Pane p{e->W, 0, (int64_t)e->H * e->W};
        if (rgb_out) p = pane_of(e, opts);
        XCHK(hipSetDevice(e->device));
        cad::export_render(depth, sub, mask, B, e->H, e->W, opts->fixed_range ? nullptr : e->table, opts->lo, opts->hi,
                           e->luts + 768 * opts->colormap, opts->invalid, rgb_out, p.row_stride, p.col_off, p.image_stride,
                           u16_out, opts->units_per_metre, S(stream));
        XCHK(hipGetLastError());
    });
}

cad_status cad_exporter_image(cad_exporter* e, const float* rgb, int B, const cad_render_opts* opts, uint8_t* rgb_out,
                              void* stream) {
    return xguard([&] {
        need(e && rgb && opts && rgb_out, "null argument");
        need(B >= 1 && B <= e->Bmax, "batch exceeds the exporter's max_batch");
        const Pane p = pane_of(e, opts);
        XCHK(hipSetDevice(e->device));
        cad::export_image(rgb, B, e->H, e->W, rgb_out, p.row_stride, p.col_off, p.image_stride, S(stream));
        XCHK(hipGetLastError());
    });
}

cad_status cad_exporter_normals(cad_exporter* e, const float* depth, const float* K, const uint8_t* mask, int B,
                                const cad_render_opts* opts, uint8_t* rgb_out, void* stream) {
    return xguard([&] {
        need(e && depth && K && opts && rgb_out, "null argument");
        need(B >= 1 && B <= e->Bmax, "batch exceeds the exporter's max_batch");
        const Pane p = pane_of(e, opts);
        XCHK(hipSetDevice(e->device));
        cad::depth_normals(depth, K, mask, B, e->H, e->W, 0.f, __builtin_inff(), nullptr, nullptr, rgb_out, p.row_stride,
                           p.col_off, p.image_stride, opts->invalid, S(stream));
        XCHK(hipGetLastError());
    });
}

cad_status cad_exporter_points(cad_exporter* e, const float* depth, const float* K, const float* rgb, const uint8_t* mask,
                               int B, int stride, float min_depth, float max_depth, void* records, int32_t* counts,
                               void* stream) {
    return xguard([&] {
        need(stride >= 1, "points: stride must be at least 1");
        need(e && depth && K && records && counts, "null argument");
        need(B >= 1 && B <= e->Bmax, "batch exceeds the exporter's max_batch");
        need(min_depth < max_depth, "points: min_depth must be below max_depth");
        need((reinterpret_cast<uintptr_t>(records) & 15) == 0, "points: records must be 16-byte aligned");
        XCHK(hipSetDevice(e->device));
        cad::export_points(depth, K, rgb, mask, B, e->H, e->W, stride, min_depth, max_depth, e->tilecnt, e->tileoff, records,
                           counts, S(stream));
        XCHK(hipGetLastError());
    });
}

namespace {
void flip_check(const float* b, const float* out, int64_t planes, int H, int W) {
    need(b && out, "null argument");
    need(planes >= 1 && H >= 1 && W >= 1, "flip: planes, H and W must be positive");
    need(planes * H <= (int64_t(1) << 31) / W - 1, "flip: planes * H * W must be below 2^31");
    const int64_t n = planes * H * W;
    need(out + n <= b || b + n <= out, "flip: out must not overlap the mirrored input");
}
}  // namespace

cad_status cad_hflip(const float* in, float* out, int64_t planes, int H, int W, void* stream) {
    return xguard([&] {
        flip_check(in, out, planes, H, W);
        cad::export_flip(nullptr, in, out, planes * H, W, S(stream));
        XCHK(hipGetLastError());
    });
}

cad_status cad_flip_mean(const float* a, const float* b, float* out, int64_t planes, int H, int W, void* stream) {
    return xguard([&] {
        need(a != nullptr, "null argument");
        flip_check(b, out, planes, H, W);
        const int64_t n = planes * H * W;
        need(out == a || out + n <= a || a + n <= out, "flip_mean: out may be a itself but must not overlap it otherwise");
        cad::export_flip(a, b, out, planes * H, W, S(stream));
        XCHK(hipGetLastError());
    });
}

cad_status cad_png_encode(const void* pixels, int h, int w, int channels, int bits, uint8_t* out, int64_t cap, int64_t* size) {
    return xguard([&] {
        need(channels == 1 || channels == 3, "png: channels must be 1 (gray) or 3 (RGB)");
        need(bits == 8 || bits == 16, "png: bits must be 8 or 16");
        need(h > 0 && w > 0 && h <= (1 << 16) && w <= (1 << 16), "png: bad dimensions");
        need(size != nullptr, "null argument");
        if (!out) {
            *size = png_bound(h, w, channels, bits);
            return;
        }
        need(pixels != nullptr, "null argument");
        const int bpp = channels * bits / 8;
        const size_t stride = (size_t)w * bpp;
        // scanlines in file byte order (16-bit: big-endian)
        std::vector<uint8_t> img(stride * (size_t)h);
        if (bits == 8) {
            std::memcpy(img.data(), pixels, img.size());
        } else {
            const uint16_t* src = static_cast<const uint16_t*>(pixels);
            for (size_t i = 0; i < img.size() / 2; ++i) {
                img[2 * i] = (uint8_t)(src[i] >> 8);
                img[2 * i + 1] = (uint8_t)(src[i] & 255);
            }
        }
        // per row the filter with the smallest sum of absolute residuals (the PNG specification's heuristic)
        std::vector<uint8_t> raw((stride + 1) * (size_t)h), cand(stride);
        for (int y = 0; y < h; ++y) {
            const uint8_t* cur = img.data() + (size_t)y * stride;
            const uint8_t* up = y ? cur - stride : nullptr;
            uint8_t* dst = raw.data() + (size_t)y * (stride + 1);
            uint64_t best = ~uint64_t(0);
            for (int ft = 0; ft < 5; ++ft) {
                uint64_t cost = 0;
                for (size_t i = 0; i < stride; ++i) {
                    const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0;
                    const int c = (up && i >= (size_t)bpp) ? up[i - bpp] : 0;
                    const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, c);
                    const uint8_t r = (uint8_t)(cur[i] - pred);
                    cand[i] = r;
                    cost += r < 128 ? r : 256 - r;
                }
                if (cost < best) {
                    best = cost;
                    dst[0] = (uint8_t)ft;
                    std::memcpy(dst + 1, cand.data(), stride);
                }
            }
        }
        std::vector<uint8_t> z(compressBound((uLong)raw.size()));
        uLongf zl = (uLongf)z.size();
        need(compress2(z.data(), &zl, raw.data(), (uLong)raw.size(), 6) == Z_OK, "png: deflate failed");
        std::vector<uint8_t> png = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
        std::vector<uint8_t> ihdr;
        put32(ihdr, (uint32_t)w);
        put32(ihdr, (uint32_t)h);
        ihdr.push_back((uint8_t)bits);
        ihdr.push_back(channels == 1 ? 0 : 2);   // colour type: gray / RGB
        ihdr.insert(ihdr.end(), {0, 0, 0});      // deflate, adaptive filtering, no interlace
        put_chunk(png, "IHDR", ihdr.data(), ihdr.size());
        put_chunk(png, "IDAT", z.data(), zl);
        put_chunk(png, "IEND", nullptr, 0);
        need((int64_t)png.size() <= cap, "png: output buffer too small");
        std::memcpy(out, png.data(), png.size());
        *size = (int64_t)png.size();
    });
}

cad_status cad_ply_write(const char* path, const void* records, int64_t n) {
    return xguard([&] {
        need(path && n >= 0 && (records || n == 0), "bad arguments");
        FILE* f = std::fopen(path, "wb");
        need(f != nullptr, std::string("cannot write ") + path);
        std::shared_ptr<FILE> hold(f, [](FILE* p) { std::fclose(p); });
        const std::string head = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) +
                                 "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                                 "property uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n";
        bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
        if (n) ok = ok && std::fwrite(records, 16, (size_t)n, f) == (size_t)n;
        need(ok && std::fflush(f) == 0, std::string("write failed: ") + path);
    });
}

}  // extern "C"
