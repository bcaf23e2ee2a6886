// cad::Exporter — RAII handle of a cad_exporter (include/cad/cad.h, "inference export"): depth renders
// into RGB8 panes, 16-bit depth and point clouds on the device, for build/predict.  After the reference's
// DepthVisualizer (src/visualization/depth_viz.h:23-148, depth_visualizer.h), which works on the host.
// Every call is asynchronous on `stream`, allocates nothing and never synchronises.
#pragma once
#include <string>

#include "cad.hpp"

namespace cad {

inline int colormap_id(const std::string& name) {
    if (name == "gray") return CAD_CMAP_GRAY;
    if (name == "jet") return CAD_CMAP_JET;
    if (name == "hot") return CAD_CMAP_HOT;
    throw std::runtime_error("unknown colormap '" + name + "': expected jet, hot or gray");
}

class Exporter {
public:
    Exporter(int max_batch, int H, int W, int device = 0) : H_(H), W_(W) {
        check(cad_exporter_create(max_batch, H, W, device, &h_), "cad_exporter_create");
    }
    ~Exporter() { cad_exporter_destroy(h_); }
    Exporter(const Exporter&) = delete;
    Exporter& operator=(const Exporter&) = delete;

    // a pane of a panel: RGB8 HWC rows of row_stride pixels, this pane's first column at col_offset
    struct Pane {
        uint8_t* rgb = nullptr;
        int64_t row_stride = 0, col_offset = 0;
    };
    // (min, max) per image into the exporter's table (and `out`, device B x 2 floats, when given)
    void range(const float* depth, const float* sub, int B, float* out = nullptr, void* stream = nullptr) {
        check(cad_exporter_range(h_, depth, sub, nullptr, B, out, stream), "cad_exporter_range");
    }
    // colourise with the range table's (lo, hi) of each image (the last range()), or fixed lo / hi
    void color(const float* depth, const float* sub, int B, int colormap, const Pane& pane, const float* lo_hi = nullptr,
               void* stream = nullptr) {
        cad_render_opts o = opts(pane);
        o.colormap = colormap;
        if (lo_hi) { o.fixed_range = 1; o.lo = lo_hi[0]; o.hi = lo_hi[1]; }
        check(cad_exporter_render(h_, depth, sub, nullptr, B, &o, pane.rgb, nullptr, stream), "cad_exporter_render");
    }
    void depth16(const float* depth, int B, uint16_t* out, float units_per_metre = 1000.0f, void* stream = nullptr) {
        cad_render_opts o = opts(Pane{});
        o.units_per_metre = units_per_metre;
        check(cad_exporter_render(h_, depth, nullptr, nullptr, B, &o, nullptr, out, stream), "cad_exporter_render");
    }
    void image(const float* rgb, int B, const Pane& pane, void* stream = nullptr) {
        const cad_render_opts o = opts(pane);
        check(cad_exporter_image(h_, rgb, B, &o, pane.rgb, stream), "cad_exporter_image");
    }
    // surface normals of depth from K (B,3,3) as colours: a frontal wall is (128, 128, 255); pixels without a
    // valid five-point stencil, the border included, are black
    void normals(const float* depth, const float* K, int B, const Pane& pane, void* stream = nullptr) {
        const cad_render_opts o = opts(pane);
        check(cad_exporter_normals(h_, depth, K, nullptr, B, &o, pane.rgb, stream), "cad_exporter_normals");
    }
    // createComparisonViz's strip rgb | gt | pred | |pred - gt| of n samples into `panel` (device, n x H x 4W RGB8):
    // gt and pred in gt's range with `colormap`, the error pane in its own range with the hot table
    // (build/predict's <stem>_panel.png and the trainers' predictions/sample_<i> panels)
    void comparison_panel(const float* rgb, const float* gt, const float* pred, int n, int colormap, uint8_t* panel,
                          void* stream = nullptr) {
        const int64_t W = W_;
        image(rgb, n, Pane{panel, 4 * W, 0}, stream);
        range(gt, nullptr, n, nullptr, stream);
        color(gt, nullptr, n, colormap, Pane{panel, 4 * W, W}, nullptr, stream);
        color(pred, nullptr, n, colormap, Pane{panel, 4 * W, 2 * W}, nullptr, stream);
        range(pred, gt, n, nullptr, stream);
        color(pred, gt, n, CAD_CMAP_HOT, Pane{panel, 4 * W, 3 * W}, nullptr, stream);
    }
    int64_t point_capacity(int stride) const { return (int64_t)((H_ + stride - 1) / stride) * ((W_ + stride - 1) / stride); }
    void points(const float* depth, const float* K, const float* rgb, int B, int stride, float min_depth, float max_depth,
                void* records, int32_t* counts, void* stream = nullptr) {
        check(cad_exporter_points(h_, depth, K, rgb, nullptr, B, stride, min_depth, max_depth, records, counts, stream),
              "cad_exporter_points");
    }
    cad_exporter* handle() const { return h_; }

private:
    static cad_render_opts opts(const Pane& p) {
        cad_render_opts o{};
        o.row_stride = p.row_stride;
        o.col_offset = p.col_offset;
        o.units_per_metre = 1000.0f;
        return o;
    }
    cad_exporter* h_ = nullptr;
    int H_, W_;
};

}  // namespace cad
