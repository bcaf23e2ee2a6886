// What build/evaluate and build/predict share: the keys of the training YAML that describe the model and the
// data (the ones train_main.cpp's load_config reads), and the .npy writer of a depth map.
#pragma once
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../host/yaml_lite.hpp"

namespace cad_cli {

struct Config {   // the keys of train_main.cpp's load_config that evaluation needs
    int batch_size = 8, init_features = 64, height = 240, width = 320, seed = 42, n_train = 64, n_val = 16;
    float max_depth = 10.0f;
    std::string architecture = "baseline_unet", variant = "full", dataset = "sunrgbd", data_dir = "./data/sunrgbd",
                manifest_path = "./data/sunrgbd_manifest.json";
    bool use_pcl = true, use_attention = true;
    std::vector<std::string> sensor_types;
};

inline Config load_config(const yaml_lite::Node& y) {
    Config c;
    if (auto& t = y["training"]) c.batch_size = t["batch_size"].as<int>(8);
    if (auto& e = y["experiment"]) c.seed = e["seed"].as<int>(42);
    if (auto& m = y["model"]) {
        c.init_features = m["init_features"].as<int>(64);
        c.max_depth = m["max_depth"].as<float>(10.0f);
        c.architecture = m["architecture"].as<std::string>("baseline_unet");
        c.variant = m["variant"].as<std::string>("full");
        c.use_pcl = m["use_pcl"].as<bool>(true);
        c.use_attention = m["use_attention"].as<bool>(true);
        // intrinsics_unet builds the FiLM-only model whatever use_attention says (existing configs and
        // checkpoints keep their meaning); intrinsics_attention_unet is the reference's IntrinsicsAttentionUNet
        if (c.architecture != "baseline_unet" && c.architecture != "intrinsics_unet" &&
            c.architecture != "intrinsics_attention_unet" && c.architecture != "ray_film_unet" &&
            c.architecture != "geometry_aware")
            throw std::runtime_error("model.architecture '" + c.architecture +
                                     "': this CLI evaluates baseline_unet, intrinsics_unet, intrinsics_attention_unet, "
                                     "ray_film_unet or geometry_aware");
        if (c.architecture == "geometry_aware" && c.variant != "full" && c.variant != "lightweight")
            throw std::runtime_error("model.variant '" + c.variant + "': expected full or lightweight");
    }
    if (auto& d = y["data"]) {
        c.height = d["input_height"].as<int>(240);
        c.width = d["input_width"].as<int>(320);
        c.dataset = d["dataset_name"].as<std::string>("sunrgbd");
        c.n_train = d["num_train_samples"].as<int>(64);
        c.n_val = d["num_val_samples"].as<int>(16);
        c.manifest_path = d["manifest_path"].as<std::string>("./data/sunrgbd_manifest.json");
        c.data_dir = d["data_dir"].as<std::string>("./data/sunrgbd");
        c.sensor_types = d["sensor_types"].as<std::vector<std::string>>({});
    }
    if (c.batch_size < 1) throw std::runtime_error("training.batch_size must be positive");
    return c;
}

inline bool ends_with(const std::string& s, const std::string& suf) {
    return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

inline void write_npy(const std::string& path, const float* data, int H, int W) {
    std::string head = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(H) + ", " + std::to_string(W) +
                       "), }";
    while ((10 + head.size() + 1) % 64 != 0) head += ' ';
    head += '\n';
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write " + path);
    const unsigned char pre[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    const uint16_t hl = (uint16_t)head.size();
    f.write((const char*)pre, 8);
    f.write((const char*)&hl, 2);
    f.write(head.data(), (std::streamsize)head.size());
    f.write((const char*)data, (std::streamsize)sizeof(float) * H * W);
}

}  // namespace cad_cli
