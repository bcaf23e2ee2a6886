// build/predict — inference and export with a trained checkpoint: images (or dataset samples) in, depth maps
// out, as 16-bit depth PNGs, colourised renders, point clouds, raw arrays and comparison panels.  On
// libcad_hip.so through include/cad/exporter.hpp; the renders follow the reference's DepthVisualizer
// (src/visualization/depth_viz.h:23-148: createComparisonViz's strip, normalizeDepth, applyColormap).
//
//   build/predict -c <final_model.pt | .cadckpt> -g <train_config.yaml> [-o results/predict]
//      -i img.jpg [img2.png ...] [--intrinsics fx,fy,cx,cy | --intrinsics-file intrinsics.txt]
//    | --split val|train --indices 0,3,7 [--data-dir D]
//      [--depth-png] [--color-png] [--ply] [--ply-stride S] [--npy] [--panel] [--normals]
//      [--colormap jet|hot|gray] [--range lo,hi] [--flip-tta] [--gpu N] [--dry-run]
//
// The model and the dataset come from the training YAML, the keys and code paths of build/evaluate.  File
// inputs are decoded on the host (JPEG or PNG), uploaded as uint8 and resized to the model's H x W by the
// device batcher, which scales K with them (--intrinsics is given for the file's own resolution; an
// intrinsics file holds the nine values of K, row-major); outputs are at the model's resolution and the
// PLY and the normals use the scaled K.  Conditioned and geometry models, --ply and --normals need intrinsics.  Dataset samples carry
// ground truth: --panel writes rgb | gt | pred | |pred - gt|, gt and pred in gt's range, the error pane in
// its own range with the hot table, every pane rendered on the device into one buffer.
// Per image: <stem>_depth.png (16-bit, millimetres), <stem>_color.png, <stem>.ply, <stem>.npy,
// <stem>_panel.png, <stem>_normal.png (the predicted surface normals from the depth and K, cad.h
// cad_exporter_normals: a wall facing the camera is (128, 128, 255)); predictions.csv holds name, height, width, min, max, points, forward_ms.  Without an
// output flag the depth and colour PNGs are written.  --flip-tta averages the prediction with the mirrored
// prediction of the mirrored image (K' = K with cx' = W - 1 - cx).  Any exception prints "Error: <what>" and
// exits 1, like build/train.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/cad/cad.hpp"
#include "../../../include/cad/evaluator.hpp"
#include "../../../include/cad/exporter.hpp"
#include "../host/yaml_lite.hpp"
#include "cli_common.hpp"

namespace fs = std::filesystem;
using namespace camera_aware_depth;
using namespace cad_cli;

namespace {

struct Args {
    std::string checkpoint, config, output = "results/predict", data_dir, split, colormap = "jet", intrinsics_file;
    std::vector<std::string> inputs;
    std::vector<int64_t> indices;
    std::vector<float> intrinsics, range;   // fx, fy, cx, cy; lo, hi
    bool depth_png = false, color_png = false, ply = false, npy = false, panel = false, normals = false, flip_tta = false, dry_run = false, fused_forward = false;
    int ply_stride = 1, gpu = 0;
};

void usage() {
    std::cout << "predict - Depth maps, renders and point clouds from a trained model (MI355X)\n"
                 "  -c, --checkpoint arg  Path to model checkpoint (.pt torch::save archive or .cadckpt)\n"
                 "  -g, --config arg      Path to the training config YAML\n"
                 "  -o, --output arg      Output directory (default: results/predict)\n"
                 "  -i, --input args      Image files (.jpg, .png)\n"
                 "      --intrinsics arg  fx,fy,cx,cy of the input files\n"
                 "      --intrinsics-file arg  File with the nine values of K, row-major\n"
                 "      --split arg       val or train: predict dataset samples instead of files\n"
                 "      --indices arg     Comma-separated sample indices of the split\n"
                 "      --data-dir arg    Data directory (overrides the config)\n"
                 "      --depth-png       16-bit depth PNG in millimetres\n"
                 "      --color-png       Colourised depth PNG\n"
                 "      --ply             Coloured point cloud (binary PLY)\n"
                 "      --ply-stride arg  Keep every S-th pixel of every S-th row (default: 1)\n"
                 "      --npy             Raw fp32 depth\n"
                 "      --panel           rgb | gt | pred | error strip (dataset samples)\n"
                 "      --normals         Surface-normal PNG from the predicted depth and K (needs intrinsics)\n"
                 "      --colormap arg    jet, hot or gray (default: jet)\n"
                 "      --range lo,hi     Fixed range of the colourised PNG (default: each image's own)\n"
                 "      --flip-tta        Average with the mirrored prediction of the mirrored image\n"
                 "      --fused-forward   Fused eval forward: BatchNorm, ReLU and FiLM in the convolutions' epilogues\n"
                 "                        (the U-Net families; the same outputs, fewer passes over memory)\n"
                 "      --gpu arg         GPU ID (default: 0)\n"
                 "      --dry-run         Print the plan and exit; no GPU use\n"
                 "  -h, --help            Print help\n";
}

template <class T>
std::vector<T> split_numbers(const std::string& s, const std::string& what) {
    std::vector<T> out;
    std::stringstream ss(s);
    for (std::string cell; std::getline(ss, cell, ',');) {
        try {
            size_t used = 0;
            const double v = std::stod(cell, &used);
            if (used != cell.size()) throw std::invalid_argument(cell);
            out.push_back((T)v);
        } catch (const std::exception&) {
            throw std::runtime_error(what + " '" + s + "': expected comma-separated numbers");
        }
    }
    return out;
}

Args parse_args(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i], v;
        auto eq = k.find('=');
        if (k.rfind("--", 0) == 0 && eq != std::string::npos) { v = k.substr(eq + 1); k = k.substr(0, eq); }
        auto next = [&]() -> std::string {
            if (!v.empty()) return v;
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + k);
            return argv[++i];
        };
        if (k == "-h" || k == "--help") { usage(); std::exit(0); }
        else if (k == "-c" || k == "--checkpoint") a.checkpoint = next();
        else if (k == "-g" || k == "--config") a.config = next();
        else if (k == "-o" || k == "--output") a.output = next();
        else if (k == "-i" || k == "--input") {
            a.inputs.push_back(next());
            while (i + 1 < argc && argv[i + 1][0] != '-') a.inputs.push_back(argv[++i]);
        } else if (k == "--intrinsics") a.intrinsics = split_numbers<float>(next(), "--intrinsics");
        else if (k == "--intrinsics-file") a.intrinsics_file = next();
        else if (k == "--split") a.split = next();
        else if (k == "--indices") a.indices = split_numbers<int64_t>(next(), "--indices");
        else if (k == "--data-dir") a.data_dir = next();
        else if (k == "--depth-png") a.depth_png = true;
        else if (k == "--color-png") a.color_png = true;
        else if (k == "--ply") a.ply = true;
        else if (k == "--ply-stride") a.ply_stride = std::stoi(next());
        else if (k == "--npy") a.npy = true;
        else if (k == "--panel") a.panel = true;
        else if (k == "--normals") a.normals = true;
        else if (k == "--colormap") a.colormap = next();
        else if (k == "--range") a.range = split_numbers<float>(next(), "--range");
        else if (k == "--flip-tta") a.flip_tta = true;
        else if (k == "--fused-forward") a.fused_forward = true;
        else if (k == "--gpu") a.gpu = std::stoi(next());
        else if (k == "--dry-run") a.dry_run = true;
        else throw std::runtime_error("unknown option " + k);
    }
    return a;
}

std::string lower_ext(const std::string& path) {
    std::string e = fs::path(path).extension().string();
    std::transform(e.begin(), e.end(), e.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    return e;
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Cannot open " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a JPEG or PNG file as RGB8 (gray replicated, alpha dropped, 16-bit reduced to its high byte: the loader's rule)
std::vector<uint8_t> decode_rgb8(const std::string& path, int* h, int* w) {
    const std::vector<uint8_t> bytes = slurp(path);
    const std::string ext = lower_ext(path);
    int ch = 0, bits = 8;
    std::vector<uint8_t> raw;
    if (ext == ".png") {
        cad::check(cad_png_decode(bytes.data(), (int64_t)bytes.size(), nullptr, 0, h, w, &ch, &bits), path.c_str());
        raw.resize((size_t)*h * *w * ch * (bits / 8));
        cad::check(cad_png_decode(bytes.data(), (int64_t)bytes.size(), raw.data(), (int64_t)raw.size(), h, w, &ch, &bits),
                   path.c_str());
    } else {
        cad::check(cad_jpeg_decode(bytes.data(), (int64_t)bytes.size(), nullptr, 0, h, w, &ch), path.c_str());
        raw.resize((size_t)*h * *w * ch);
        cad::check(cad_jpeg_decode(bytes.data(), (int64_t)bytes.size(), raw.data(), (int64_t)raw.size(), h, w, &ch), path.c_str());
    }
    std::vector<uint8_t> rgb((size_t)*h * *w * 3);
    const uint16_t* wide = reinterpret_cast<const uint16_t*>(raw.data());
    for (size_t i = 0; i < (size_t)*h * *w; ++i)
        for (int q = 0; q < 3; ++q) {
            const size_t s = i * ch + (ch >= 3 ? q : 0);
            rgb[i * 3 + q] = bits == 16 ? (uint8_t)(wide[s] >> 8) : raw[s];
        }
    return rgb;
}

// device memory through the C ABI
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(int device, int64_t bytes) { cad::check(cad_malloc(device, std::max<int64_t>(bytes, 16), &p), "cad_malloc"); }
    ~DevBuf() { cad_free(p); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }
    template <class T> T* as() const { return static_cast<T*>(p); }
    void upload(const void* host, int64_t bytes) { cad::check(cad_memcpy(p, host, bytes, 0, nullptr), "cad_memcpy h2d"); }
    template <class T> std::vector<T> host(int64_t count, int64_t first = 0) const {
        std::vector<T> h((size_t)count);
        if (count) cad::check(cad_memcpy(h.data(), as<T>() + first, count * (int64_t)sizeof(T), 1, nullptr), "cad_memcpy d2h");
        return h;
    }
};

void write_png(const std::string& path, const void* pixels, int h, int w, int channels, int bits) {
    int64_t size = 0;
    cad::check(cad_png_encode(pixels, h, w, channels, bits, nullptr, 0, &size), "cad_png_encode");
    std::vector<uint8_t> buf((size_t)size);
    cad::check(cad_png_encode(pixels, h, w, channels, bits, buf.data(), size, &size), "cad_png_encode");
    std::ofstream f(path, std::ios::binary);
    if (!f || !f.write((const char*)buf.data(), (std::streamsize)size)) throw std::runtime_error("cannot write " + path);
}

std::string json_list(const std::vector<std::string>& v, bool quote) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + (quote ? "\"" + v[i] + "\"" : v[i]);
    return s + "]";
}

int run(Args a) {
    if (a.checkpoint.empty() || a.config.empty()) throw std::runtime_error("--checkpoint and --config are required");
    if (!fs::exists(a.checkpoint)) throw std::runtime_error("Cannot open checkpoint: " + a.checkpoint);
    const bool pt = ends_with(a.checkpoint, ".pt");
    if (!pt && !ends_with(a.checkpoint, ".cadckpt"))
        throw std::runtime_error("checkpoint '" + a.checkpoint + "': expected a .pt or .cadckpt file");
    Config c = load_config(yaml_lite::load_file(a.config));
    if (!a.data_dir.empty()) c.data_dir = a.data_dir;
    const bool geo = c.architecture == "geometry_aware";
    if (geo && pt) throw std::runtime_error("geometry_aware checkpoints are .cadckpt files");
    if (geo && a.fused_forward)
        throw std::runtime_error("--fused-forward: model.architecture 'geometry_aware' has no fused eval forward (the "
                                 "U-Net families baseline_unet, intrinsics_unet, intrinsics_attention_unet, ray_film_unet do)");
    const int cmap = cad::colormap_id(a.colormap);
    if (!a.range.empty() && a.range.size() != 2) throw std::runtime_error("--range takes lo,hi");
    if (a.ply_stride < 1) throw std::runtime_error("--ply-stride must be at least 1");
    const bool files = !a.inputs.empty();
    if (files == !a.split.empty()) throw std::runtime_error("give either input files (-i) or --split with --indices");
    if (!(a.depth_png || a.color_png || a.ply || a.npy || a.panel || a.normals)) a.depth_png = a.color_png = true;

    bool have_K = false;
    float Kfile[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1};
    const bool real = c.dataset != "synthetic";
    if (files) {
        for (const auto& p : a.inputs) {
            const std::string e = lower_ext(p);
            if (e != ".jpg" && e != ".jpeg" && e != ".png") throw std::runtime_error("input '" + p + "': expected a .jpg or .png file");
            if (!fs::exists(p)) throw std::runtime_error("Cannot open " + p);
        }
        if (!a.intrinsics.empty() && !a.intrinsics_file.empty()) throw std::runtime_error("give --intrinsics or --intrinsics-file, not both");
        if (!a.intrinsics.empty()) {
            if (a.intrinsics.size() != 4) throw std::runtime_error("--intrinsics takes fx,fy,cx,cy");
            Kfile[0] = a.intrinsics[0]; Kfile[4] = a.intrinsics[1]; Kfile[2] = a.intrinsics[2]; Kfile[5] = a.intrinsics[3];
            have_K = true;
        } else if (!a.intrinsics_file.empty()) {
            std::ifstream f(a.intrinsics_file);
            if (!f) throw std::runtime_error("Cannot open " + a.intrinsics_file);
            for (float& v : Kfile)
                if (!(f >> v)) throw std::runtime_error(a.intrinsics_file + ": expected the nine values of K");
            have_K = true;
        }
        if (!have_K && (geo || c.architecture != "baseline_unet"))
            throw std::runtime_error("model " + c.architecture + " is conditioned on the camera: give --intrinsics fx,fy,cx,cy or --intrinsics-file");
        if (!have_K && a.ply) throw std::runtime_error("--ply needs the camera: give --intrinsics fx,fy,cx,cy or --intrinsics-file");
        if (!have_K && a.normals)
            throw std::runtime_error("--normals needs the camera: give --intrinsics fx,fy,cx,cy or --intrinsics-file");
        if (a.panel) throw std::runtime_error("--panel compares with ground truth: use --split and --indices");
    } else {
        if (a.split != "val" && a.split != "train") throw std::runtime_error("--split '" + a.split + "': expected val or train");
        if (a.indices.empty()) throw std::runtime_error("--split needs --indices");
        if (!a.intrinsics.empty() || !a.intrinsics_file.empty()) throw std::runtime_error("dataset samples carry their own intrinsics");
        int64_t ns = a.split == "val" ? c.n_val : c.n_train;
        if (real) {
            std::vector<const char*> sens;
            for (const auto& x : c.sensor_types) sens.push_back(x.c_str());
            cad_dataset* d = nullptr;
            cad::check(cad_dataset_open(c.manifest_path.c_str(), sens.empty() ? nullptr : sens.data(), (int)sens.size(), &d),
                       "SunRGBDLoader");
            ns = cad_dataset_size(d);
            cad_dataset_destroy(d);
            if (a.split == "val") ns = std::min<int64_t>(500, ns);
        }
        for (int64_t i : a.indices)
            if (i < 0 || i >= ns)
                throw std::runtime_error("index " + std::to_string(i) + " is outside the " + a.split + " split (" + std::to_string(ns) + " samples)");
        have_K = true;
    }
    std::vector<std::string> outputs;
    for (const auto& kv : {std::make_pair(a.depth_png, "depth_png"), std::make_pair(a.color_png, "color_png"), std::make_pair(a.ply, "ply"),
                           std::make_pair(a.npy, "npy"), std::make_pair(a.panel, "panel"), std::make_pair(a.normals, "normals")})
        if (kv.first) outputs.push_back(kv.second);
    const int64_t n_in = files ? (int64_t)a.inputs.size() : (int64_t)a.indices.size();
    if (a.dry_run) {
        std::vector<std::string> idx;
        for (int64_t i : a.indices) idx.push_back(std::to_string(i));
        std::cout << "{\"checkpoint\": \"" << a.checkpoint << "\", \"format\": \"" << (pt ? "torch" : "cadckpt")
                  << "\", \"architecture\": \"" << c.architecture << "\", \"init_features\": " << c.init_features
                  << ", \"max_depth\": " << c.max_depth << ", \"source\": \"" << (files ? "files" : a.split) << "\", \"dataset\": \""
                  << (files ? "" : real ? c.manifest_path : "synthetic") << "\", \"inputs\": " << n_in << ", \"indices\": "
                  << json_list(idx, false) << ", \"height\": " << c.height << ", \"width\": " << c.width << ", \"device\": " << a.gpu
                  << ", \"output\": \"" << a.output << "\", \"outputs\": " << json_list(outputs, true) << ", \"colormap\": \""
                  << a.colormap << "\", \"range\": "
                  << (a.range.empty() ? std::string("null") : "[" + std::to_string(a.range[0]) + ", " + std::to_string(a.range[1]) + "]")
                  << ", \"ply_stride\": " << a.ply_stride << ", \"flip_tta\": " << (a.flip_tta ? "true" : "false")
                  << ", \"intrinsics\": " << (have_K ? "true" : "false") << ", \"forward\": \""
                  << (a.fused_forward ? "fused" : "two-pass") << "\"}" << std::endl;
        return 0;
    }

    int ndev = 0;
    cad::check(cad_device_count(&ndev), "device query");
    if (a.gpu < 0 || a.gpu >= ndev) throw std::runtime_error("GPU " + std::to_string(a.gpu) + " not available");
    cad::check(cad_set_device(a.gpu), "set device");
    fs::create_directories(a.output);
    const int H = c.height, W = c.width, dev = a.gpu;
    const int B = files ? 1 : (int)std::min<int64_t>(c.batch_size, n_in);
    const int64_t HW = (int64_t)H * W;

    // the model, as build/evaluate builds and loads it
    const cad::Workspace ws{B, H, W, dev};
    std::shared_ptr<BaselineUNetImpl> unet;
    std::shared_ptr<GeometryAwareNetworkImpl> gnet;
    if (geo) {
        if (c.variant == "lightweight") gnet = std::make_shared<LightweightGeometryNetworkImpl>(3, c.init_features, 4, c.max_depth, ws);
        else gnet = std::make_shared<GeometryAwareNetworkImpl>(3, c.init_features, 4, c.max_depth, c.use_pcl, c.use_attention, ws);
        load_model_state(a.checkpoint, *gnet);
        gnet->eval();
    } else {
        if (c.architecture == "intrinsics_unet") unet = std::make_shared<IntrinsicsConditionedUNetImpl>(3, c.init_features, 4, c.max_depth, ws);
        else if (c.architecture == "intrinsics_attention_unet") unet = std::make_shared<IntrinsicsAttentionUNetImpl>(3, c.init_features, 4, c.max_depth, ws);
        else if (c.architecture == "ray_film_unet") unet = std::make_shared<RayConditionedUNetImpl>(3, c.init_features, 4, c.max_depth, ws);
        else unet = std::make_shared<BaselineUNetImpl>(3, c.init_features, c.max_depth, ws);
        if (pt) load(*unet, a.checkpoint);
        else load_model_state(a.checkpoint, *unet);
        unet->eval();
        unet->fused_eval(a.fused_forward);
    }
    DeviceTensor rgb = DeviceTensor::empty({B, 3, H, W}, dev), gt = DeviceTensor::empty({B, 1, H, W}, dev),
                 K = DeviceTensor::empty({B, 3, 3}, dev), pred = DeviceTensor::empty({B, 1, H, W}, dev),
                 cam = DeviceTensor::empty({B, 4}, dev), rays, rgb_f, pred_f, K_f;
    if (geo) rays = DeviceTensor::empty({B, 3, H, W}, dev);
    if (a.flip_tta) {
        rgb_f = DeviceTensor::empty({B, 3, H, W}, dev);
        pred_f = DeviceTensor::empty({B, 1, H, W}, dev);
        K_f = DeviceTensor::empty({B, 3, 3}, dev);
    }
    const auto forward = [&](const DeviceTensor& x, const DeviceTensor& k, DeviceTensor& out, int n) {
        if (geo) {
            cad::check(cad_ray_directions(k.data, n, H, W, rays.data, nullptr), "rays");
            cad::check(cad_camera_from_K(k.data, n, cam.data, nullptr), "camera_from_K");
            cad::check(cad_geonet_forward(gnet->handle(), x.data, rays.data, cam.data, out.data, n, nullptr), "forward");
        } else if (cad_unet_model(unet->handle()) != CAD_MODEL_BASELINE) {
            cad::check(cad_camera_from_K(k.data, n, cam.data, nullptr), "camera_from_K");
            cad::check(cad_unet_forward_cam(unet->handle(), x.data, cam.data, out.data, n, nullptr), "forward");
        } else {
            cad::check(cad_unet_forward(unet->handle(), x.data, out.data, n, nullptr), "forward");
        }
    };

    // export workspace, sized once
    cad::Exporter ex(B, H, W, dev);
    const int64_t cap = ex.point_capacity(a.ply_stride);
    DevBuf range_d(dev, sizeof(float) * 2 * B), u16_d(dev, a.depth_png ? 2 * B * HW : 0), color_d(dev, a.color_png ? 3 * B * HW : 0),
        panel_d(dev, a.panel ? 12 * B * HW : 0), rec_d(dev, a.ply ? 16 * B * cap : 0), cnt_d(dev, sizeof(int32_t) * B),
        normal_d(dev, a.normals ? 3 * B * HW : 0);
    cad_event *t0 = nullptr, *t1 = nullptr;
    cad::check(cad_event_create(&t0), "event");
    cad::check(cad_event_create(&t1), "event");
    std::shared_ptr<cad_event> g0(t0, cad_event_destroy), g1(t1, cad_event_destroy);

    std::ofstream csv(a.output + "/predictions.csv");
    if (!csv) throw std::runtime_error("cannot write " + a.output + "/predictions.csv");
    csv << "name,height,width,min,max,points,forward_ms\n" << std::setprecision(9);

    // one batch: rgb / gt / K hold n samples
    const auto process = [&](const std::vector<std::string>& names, int n) {
        cad::check(cad_event_record(t0, nullptr), "event");
        forward(rgb, K, pred, n);
        if (a.flip_tta) {
            std::vector<float> kh((size_t)n * 9);
            cad::check(cad_memcpy(kh.data(), K.data, (int64_t)kh.size() * 4, 1, nullptr), "cad_memcpy d2h");
            for (int i = 0; i < n; ++i) kh[(size_t)i * 9 + 2] = (float)(W - 1) - kh[(size_t)i * 9 + 2];   // applyHorizontalFlip
            cad::check(cad_memcpy(K_f.data, kh.data(), (int64_t)kh.size() * 4, 0, nullptr), "cad_memcpy h2d");
            cad::check(cad_hflip(rgb.data, rgb_f.data, (int64_t)n * 3, H, W, nullptr), "cad_hflip");
            forward(rgb_f, K_f, pred_f, n);
            cad::check(cad_flip_mean(pred.data, pred_f.data, pred.data, n, H, W, nullptr), "cad_flip_mean");
        }
        cad::check(cad_event_record(t1, nullptr), "event");
        ex.range(pred.data, nullptr, n, range_d.as<float>());
        if (a.depth_png) ex.depth16(pred.data, n, u16_d.as<uint16_t>());
        if (a.color_png) ex.color(pred.data, nullptr, n, cmap, cad::Exporter::Pane{color_d.as<uint8_t>(), 0, 0}, a.range.empty() ? nullptr : a.range.data());
        if (a.ply) ex.points(pred.data, K.data, rgb.data, n, a.ply_stride, 0.1f, c.max_depth, rec_d.p, cnt_d.as<int32_t>());
        if (a.normals) ex.normals(pred.data, K.data, n, cad::Exporter::Pane{normal_d.as<uint8_t>(), 0, 0});
        if (a.panel) ex.comparison_panel(rgb.data, gt.data, pred.data, n, cmap, panel_d.as<uint8_t>());   // createComparisonViz
        float ms = 0.f;
        cad::check(cad_event_elapsed_ms(t0, t1, &ms), "event");
        // the copies below are synchronous on the default stream, after everything above
        const std::vector<float> lo_hi = range_d.host<float>(2 * n);
        std::vector<int32_t> counts((size_t)n, 0);
        if (a.ply) counts = cnt_d.host<int32_t>(n);
        std::vector<float> ph;
        if (a.npy) {
            ph.resize((size_t)n * HW);
            cad::check(cad_memcpy(ph.data(), pred.data, (int64_t)ph.size() * 4, 1, nullptr), "cad_memcpy d2h");
        }
        for (int i = 0; i < n; ++i) {
            const std::string stem = a.output + "/" + names[(size_t)i];
            if (a.depth_png) write_png(stem + "_depth.png", u16_d.host<uint16_t>(HW, i * HW).data(), H, W, 1, 16);
            if (a.color_png) write_png(stem + "_color.png", color_d.host<uint8_t>(3 * HW, 3 * i * HW).data(), H, W, 3, 8);
            if (a.panel) write_png(stem + "_panel.png", panel_d.host<uint8_t>(12 * HW, 12 * i * HW).data(), H, 4 * W, 3, 8);
            if (a.normals) write_png(stem + "_normal.png", normal_d.host<uint8_t>(3 * HW, 3 * i * HW).data(), H, W, 3, 8);
            if (a.npy) write_npy(stem + ".npy", ph.data() + (size_t)i * HW, H, W);
            if (a.ply) {
                const std::vector<uint8_t> rec = rec_d.host<uint8_t>(16 * (int64_t)counts[(size_t)i], 16 * i * cap);
                cad::check(cad_ply_write((stem + ".ply").c_str(), rec.data(), counts[(size_t)i]), "cad_ply_write");
            }
            csv << names[(size_t)i] << "," << H << "," << W << "," << lo_hi[2 * (size_t)i] << "," << lo_hi[2 * (size_t)i + 1] << ","
                << (a.ply ? std::to_string(counts[(size_t)i]) : std::string("0")) << "," << ms / n << "\n";
        }
    };

    std::cout << "Predicting " << n_in << (files ? " image" : " " + a.split + " sample") << (n_in == 1 ? "" : "s") << " with " << a.checkpoint
              << " (" << c.architecture << ", f=" << c.init_features << ") at " << H << "x" << W << ", MI355X device " << a.gpu
              << (a.flip_tta ? ", flip TTA" : "") << "\n";
    if (files) {
        cad_batcher* bt = nullptr;
        cad::check(cad_batcher_create(1, H, W, dev, &bt), "cad_batcher_create");
        std::shared_ptr<cad_batcher> hold(bt, cad_batcher_destroy);
        DevBuf nodepth(dev, 16);
        const uint16_t zero = 0;
        nodepth.upload(&zero, 2);
        for (const auto& path : a.inputs) {
            int h0 = 0, w0 = 0;
            const std::vector<uint8_t> img = decode_rgb8(path, &h0, &w0);
            DevBuf img_d(dev, (int64_t)img.size());
            img_d.upload(img.data(), (int64_t)img.size());
            cad_sample s{};
            s.rgb = img_d.as<uint8_t>(); s.depth = nodepth.as<uint16_t>();
            s.h0 = h0; s.w0 = w0; s.dh0 = 1; s.dw0 = 1; s.depth_scale = 1.0f / 1000.0f;
            if (have_K) std::copy(Kfile, Kfile + 9, s.K);
            else { s.K[0] = s.K[4] = (float)w0; s.K[2] = 0.5f * w0; s.K[5] = 0.5f * h0; s.K[8] = 1.f; }   // unused by the baseline model
            cad::check(cad_batcher_assemble(bt, &s, 1, rgb.data, gt.data, K.data, nullptr), "cad_batcher_assemble");
            process({fs::path(path).stem().string()}, 1);
            cad::check(cad_stream_synchronize(nullptr), "synchronize");   // img_d is freed next
        }
    } else {
        std::shared_ptr<SunRGBDLoader> loader;
        if (real) {
            loader = std::make_shared<SunRGBDLoader>(c.data_dir, c.manifest_path, a.split == "val" ? "test" : "train");
            if (!c.sensor_types.empty()) loader->filterBySensorType(c.sensor_types);
        } else {
            const int64_t ns = a.split == "val" ? c.n_val : c.n_train;
            loader = SunRGBDLoader::synthetic(ns, H, W, (uint32_t)c.seed + (a.split == "val" ? 1u : 0u));
        }
        loader->setTargetDimensions(H, W);
        cad_loader* ring = loader->ring(B, dev, false);
        cad::check(cad_loader_start_epoch(ring, a.indices.data(), n_in), "predict");
        for (int64_t first = 0;;) {
            const int n = cad_loader_next(ring, rgb.data, gt.data, K.data, nullptr);
            if (n < 0) throw std::runtime_error(std::string("data loader: ") + cad_last_error());
            if (n == 0) break;
            std::vector<std::string> names;
            for (int i = 0; i < n; ++i) names.push_back(a.split + "_" + std::to_string(a.indices[(size_t)(first + i)]));
            process(names, n);
            first += n;
        }
    }
    csv.close();
    if (unet) {
        int nf = 0, nt = 0;
        unet->fused_eval_convs(&nf, &nt);
        std::cout << "Forward mode: " << (a.fused_forward ? "fused eval forward" : "two-pass eval forward") << ", fused " << nf
                  << " of " << nt << " convolutions\n";
    }
    std::cout << "Results saved to: " << a.output << "\n";
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(parse_args(argc, argv));
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
}
