// trainer.hpp — header-only C++ drop-in for the reference's training driver, over cad.hpp / cad.h.
//
//   camera_aware_depth::AugmentationConfig          src/data/sunrgbd_loader.h:31-46
//   camera_aware_depth::SunRGBDLoader               src/data/sunrgbd_loader.h:60-128, sunrgbd_loader.cpp:13-78
//   camera_aware_depth::TensorBoardTrainerEnhanced  src/training/tensorboard_trainer_enhanced.h:35-700
//
// Same class names, Config / ValidationMetrics fields, constructor and train(train, val) as the
// reference; the step is the reference's (zero_grad, forward, forwardWithIntrinsics, backward,
// clip_grad_norm_, Adam.step, enhanced.h:287-304) on the MI355X through libcad.  Batches come from the
// loader's prefetch ring (cad_loader: decode threads, pinned double-buffered upload, device resize and
// augmentation) instead of getBatch + torch::stack.  Deliberate differences:
//   * TensorBoard event files are written natively (cad_tb_* in cad.h, no Python subprocess) under
//     <tensorboard_dir>/<experiment_name>: every scalar (also kept as <log_dir>/tensorboard_scalars.csv), the
//     custom-scalars layout, the hparams sub-run and the model/architecture text at the start of train(),
//     weights/* and gradients/* histograms every histogram_interval epochs, predictions/sample_<i> panels
//     (rgb | gt | pred | error) every viz_interval epochs.  Histograms cover every element of a tensor from one
//     device pass over the slab (the reference samples at most 10 000 strided values per tensor on the host),
//     and gradients/norm|max|min come from that pass's statistics.  GeometryTrainer writes the same records
//     (cad_geonet_histograms over its slab), and no CSV, as before;
//   * with a distributed::Communicator the step is data-parallel (the reference is single-device):
//     rank r trains its batch_size-slice of every global batch, gradients are SUM-all-reduced in
//     buckets overlapped with the backward and clipped as the mean; rank 0 validates, logs and saves;
//   * logLossComponents reads sample 0 without augmentation (the reference's getSample(0) draws from
//     the augmentation rng);
//   * Config::recipe_declared (off by default) runs the recipe the reference declares in TrainingConfig / Trainer
//     (src/training/trainer.h:24-92, :262-316, :388-431, :461-467) and never executes: Adam / AdamW / SGD, a
//     per-epoch learning rate (warmup, step or cosine: cad_lr_at), checkImprovement on a monitored validation
//     metric with best_model.*, early stopping, save_best_only and keep_last_n checkpoints — and, ours, an
//     exponential moving average of the weights that validation, panels and <checkpoint>_ema.pt use.  With it off
//     every file, record and line of output is what it was.
#ifndef CAD_TRAINER_HPP
#define CAD_TRAINER_HPP

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <ctime>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <sstream>
#include <thread>

#include "cad.hpp"
#include "exporter.hpp"

namespace camera_aware_depth {

// sunrgbd_loader.h:31-46.  augmentSample ignores saturation / hue (and the configs' random_gamma): they reach the
// batcher only when `declared` is set (build/train: data.augmentation.mode: declared; cad.h, cad_sample).
struct AugmentationConfig {
    bool enable_random_crop = true;
    float crop_scale_min = 0.7f;
    float crop_scale_max = 1.0f;
    bool enable_horizontal_flip = true;
    float horizontal_flip_prob = 0.5f;
    bool enable_color_jitter = true;
    float brightness_delta = 0.2f;
    float contrast_delta = 0.2f;
    float saturation_delta = 0.2f;
    float hue_delta = 0.1f;
    int random_seed = 42;
    bool enable_random_gamma = false;
    float gamma_min = 0.8f;
    float gamma_max = 1.2f;
    bool declared = false;   // honour saturation_delta / hue_delta / random gamma
};

// SUN RGB-D samples from the JSON manifest (valid entries of the allowed sensor types with an
// intrinsics.txt, paths relative to the working directory — data_dir and split are kept but unused,
// as in the reference), resized to the target dimensions (default 480x640, :21-22).
class SunRGBDLoader {
public:
    SunRGBDLoader(const std::string& data_dir, const std::string& manifest_path, const std::string& split)
        : data_dir_(data_dir), manifest_(manifest_path), split_(split) {
        open();
    }
    // n procedurally generated samples of height x width (the synthetic dataset; no files)
    static std::shared_ptr<SunRGBDLoader> synthetic(int64_t n, int height, int width, uint32_t seed = 0) {
        std::shared_ptr<SunRGBDLoader> L(new SunRGBDLoader());
        cad_dataset* d = nullptr;
        cad::check(cad_dataset_synthetic(n, height, width, seed, &d), "synthetic dataset");
        L->ds_.reset(d, cad_dataset_destroy);
        L->h_ = height;
        L->w_ = width;
        return L;
    }
    size_t size() const { return (size_t)cad_dataset_size(ds_.get()); }
    // sample i's manifest sensor_type ("synthetic" for the synthetic dataset)
    std::string sensor(int64_t i) const {
        const char* s = cad_dataset_sensor(ds_.get(), i);
        if (!s) throw std::runtime_error("SunRGBDLoader::sensor: no sample " + std::to_string(i));
        return s;
    }
    void enableAugmentation(const AugmentationConfig& c) { aug_ = c; augment_ = true; rings_.clear(); }
    void disableAugmentation() { augment_ = false; rings_.clear(); }
    bool augmentation_enabled() const { return augment_; }
    void setTargetDimensions(int height, int width) { h_ = height; w_ = width; rings_.clear(); }
    int target_height() const { return h_; }
    int target_width() const { return w_; }
    void filterBySensorType(const std::vector<std::string>& sensor_types) {
        if (manifest_.empty()) throw std::runtime_error("filterBySensorType: the synthetic dataset has no sensors");
        sensors_ = sensor_types;
        open();
    }
    const std::string& manifest_path() const { return manifest_; }
    cad_dataset* handle() const { return ds_.get(); }
    // what the augmented rings' sampler is created from (seed: augmentation().random_seed)
    const AugmentationConfig& augmentation() const { return aug_; }
    cad_aug_config aug_config() const {
        cad_aug_config ac{};
        ac.enable_random_crop = aug_.enable_random_crop;
        ac.crop_scale_min = aug_.crop_scale_min;
        ac.crop_scale_max = aug_.crop_scale_max;
        ac.enable_horizontal_flip = aug_.enable_horizontal_flip;
        ac.horizontal_flip_prob = aug_.horizontal_flip_prob;
        ac.enable_color_jitter = aug_.enable_color_jitter;
        ac.brightness_delta = aug_.brightness_delta;
        ac.contrast_delta = aug_.contrast_delta;
        if (aug_.declared) {
            ac.saturation_delta = aug_.saturation_delta;
            ac.hue_delta = aug_.hue_delta;
            ac.enable_random_gamma = aug_.enable_random_gamma;
            ac.gamma_min = aug_.gamma_min;
            ac.gamma_max = aug_.gamma_max;
        }
        return ac;
    }

    // The batch pipeline behind getBatch: a prefetch ring of `batch`-sample batches on `device`
    // (augmented when augmentation is enabled and `augment`), created on first use.
    cad_loader* ring(int batch, int device, bool augment) {
        const bool aug = augment && augment_;
        const auto key = std::make_tuple(batch, device, aug);
        for (auto& r : rings_)
            if (r.first == key) return r.second.get();
        const cad_aug_config ac = aug_config();
        const int threads = (int)std::max(2u, std::min(8u, std::thread::hardware_concurrency()));
        cad_loader* L = nullptr;
        cad::check(cad_loader_create(ds_.get(), batch, h_, w_, aug ? &ac : nullptr, (uint32_t)aug_.random_seed, threads,
                                     2, device, &L),
                   "SunRGBDLoader");
        rings_.emplace_back(key, std::shared_ptr<cad_loader>(L, cad_loader_destroy));
        return L;
    }

private:
    SunRGBDLoader() = default;
    void open() {
        std::vector<const char*> s;
        for (const auto& x : sensors_) s.push_back(x.c_str());
        cad_dataset* d = nullptr;
        cad::check(cad_dataset_open(manifest_.c_str(), s.empty() ? nullptr : s.data(), (int)s.size(), &d), "SunRGBDLoader");
        ds_.reset(d, cad_dataset_destroy);
        rings_.clear();
    }
    std::string data_dir_, manifest_, split_;
    std::vector<std::string> sensors_;
    std::shared_ptr<cad_dataset> ds_;
    int h_ = 480, w_ = 640;
    bool augment_ = false;
    AugmentationConfig aug_{};
    std::vector<std::pair<std::tuple<int, int, bool>, std::shared_ptr<cad_loader>>> rings_;
};

// RAII cad_tb_writer: the event file of one run (cad.h, "TensorBoard event files").  What the reference sends
// to scripts/tensorboard_writer.py through tensorboard_logger_v2.h, written by the library itself.
class EventWriter {
public:
    explicit EventWriter(const std::string& logdir) { cad::check(cad_tb_open(logdir.c_str(), &w_), "cad_tb_open"); }
    ~EventWriter() { cad_tb_close(w_); }
    EventWriter(const EventWriter&) = delete;
    EventWriter& operator=(const EventWriter&) = delete;
    std::string path() const { return cad_tb_path(w_); }
    void flush() { cad::check(cad_tb_flush(w_), "cad_tb_flush"); }
    void scalar(const std::string& tag, float v, int64_t step) { cad::check(cad_tb_scalar(w_, tag.c_str(), v, step), "cad_tb_scalar"); }
    void text(const std::string& tag, const std::string& body, int64_t step = 0) {
        cad::check(cad_tb_text(w_, tag.c_str(), step, body.c_str()), "cad_tb_text");
    }
    // the reference's layout (tensorboard_trainer_enhanced.h, the tags of its own event files)
    void reference_layout() {
        static const char* const rows[][3] = {
            {"Training", "Loss", "loss/train"}, {"Training", "Loss", "loss/val"},
            {"Training", "Loss Components", "loss_components/si_loss"}, {"Training", "Loss Components", "loss_components/grad_loss"},
            {"Training", "Loss Components", "loss_components/smooth_loss"},
            {"Training", "Loss Components", "loss_components/reproj_loss"}, {"Training", "Learning Rate", "training/lr"},
            {"Metrics", "Relative Error", "metrics/abs_rel"}, {"Metrics", "Relative Error", "metrics/sq_rel"},
            {"Metrics", "RMSE", "metrics/rmse"}, {"Metrics", "RMSE", "metrics/rmse_log"}, {"Metrics", "Accuracy", "metrics/a1"},
            {"Metrics", "Accuracy", "metrics/a2"}, {"Metrics", "Accuracy", "metrics/a3"}, {"Model", "Gradients", "gradients/norm"},
            {"Model", "Gradients", "gradients/max"}, {"Model", "Gradients", "gradients/min"}, {"Model", "Weights", "weights/norm"},
            {"Model", "Weights", "weights/sparsity"}};
        constexpr int n = (int)(sizeof rows / sizeof rows[0]);
        const char *cat[n], *chart[n], *tag[n];
        for (int i = 0; i < n; ++i) { cat[i] = rows[i][0]; chart[i] = rows[i][1]; tag[i] = rows[i][2]; }
        cad::check(cad_tb_custom_scalars(w_, cat, chart, tag, n), "cad_tb_custom_scalars");
    }
    // logHyperparameters (:576-592): the sub-run with metric hparams/training = 0
    void hparams(float lr, int batch_size, float weight_decay, float grad_clip_value, int num_epochs) {
        const char* names[5] = {"learning_rate", "batch_size", "weight_decay", "grad_clip_value", "num_epochs"};
        const double values[5] = {(double)lr, (double)batch_size, (double)weight_decay, (double)grad_clip_value, (double)num_epochs};
        const char* metric = "hparams/training";
        const float zero = 0.f;
        cad::check(cad_tb_hparams(w_, names, values, 5, &metric, &zero, 1, nullptr), "cad_tb_hparams");
    }
    // logModelArchitecture (:593-615)
    void architecture(int64_t total, int64_t trainable) {
        std::stringstream a;
        a << "# Model Architecture\n\n```\nTotal parameters: " << total << "\nTrainable parameters: " << trainable << "\n```\n";
        text("model/architecture", a.str(), 0);
    }
    // one row of cad_hist_read: make_histogram's trimming, then the record
    void histogram(const std::string& tag, int64_t step, const double* row, const uint32_t* counts) {
        if (edges_.empty()) {
            edges_.resize(CAD_HIST_BINS + 1);
            cad_tb_default_bins(edges_.data(), (int)edges_.size());
            lim_.resize(CAD_HIST_BINS + 1);
            buc_.resize(CAD_HIST_BINS + 1);
        }
        int n = 0;
        cad::check(cad_tb_trim_histogram(counts, CAD_HIST_BINS, edges_.data(), lim_.data(), buc_.data(), &n), "trim");
        const double stats[5] = {row[1], row[2], row[0], row[3], row[4]};   // min, max, num, sum, sum_squares
        cad::check(cad_tb_histogram(w_, tag.c_str(), step, stats, lim_.data(), buc_.data(), n), "cad_tb_histogram");
    }
    // an RGB8 image (h x w x 3, host) as a PNG image summary
    void image(const std::string& tag, int64_t step, const uint8_t* rgb, int h, int w) {
        int64_t cap = 0, size = 0;
        cad::check(cad_png_encode(rgb, h, w, 3, 8, nullptr, 0, &cap), "cad_png_encode");
        png_.resize((size_t)cap);
        cad::check(cad_png_encode(rgb, h, w, 3, 8, png_.data(), cap, &size), "cad_png_encode");
        cad::check(cad_tb_image(w_, tag.c_str(), step, h, w, 3, png_.data(), size), "cad_tb_image");
    }

private:
    cad_tb_writer* w_ = nullptr;
    std::vector<double> edges_, lim_, buc_;
    std::vector<uint8_t> png_;
};

// predictions/sample_<i>: the exporter's rgb | gt | pred | error strip of one sample (composed on the device, as
// build/predict's _panel.png), encoded and written as an image summary at step = epoch (visualizeResults, :444-470)
class PanelLogger {
public:
    PanelLogger(int H, int W, int device) : H_(H), W_(W), ex_(1, H, W, device), host_((size_t)12 * H * W) {
        void* p = nullptr;
        cad::check(cad_malloc(device, (int64_t)host_.size(), &p), "panel buffer");
        dev_ = static_cast<uint8_t*>(p);
    }
    ~PanelLogger() { cad_free(dev_); }
    PanelLogger(const PanelLogger&) = delete;
    PanelLogger& operator=(const PanelLogger&) = delete;
    bool fits(int H, int W) const { return H == H_ && W == W_; }
    // visualizeResults (:444-470): the first `ns` samples of the loader's unaugmented batch-1 ring, one at a time;
    // next() fetches a sample into the trainer's buffers, forward() returns its prediction (device, H x W)
    template <class Next, class Forward>
    static void run(std::unique_ptr<PanelLogger>& self, EventWriter& ev, SunRGBDLoader& L, int device, int num_samples,
                    int64_t epoch, const float* rgb, const float* gt, Next&& next, Forward&& forward) {
        const int64_t ns = std::min<int64_t>(num_samples, (int64_t)L.size());
        if (ns <= 0) return;
        const int H = L.target_height(), W = L.target_width();
        if (!self || !self->fits(H, W)) self = std::make_unique<PanelLogger>(H, W, device);
        cad_loader* ring = L.ring(1, device, false);
        cad::check(cad_loader_start_epoch(ring, nullptr, ns), "visualization");
        for (int64_t i = 0; i < ns; ++i) {
            next(ring);
            self->log(ev, (int)i, epoch, rgb, gt, forward());
        }
    }
    void log(EventWriter& ev, int sample, int64_t epoch, const float* rgb, const float* gt, const float* pred) {
        ex_.comparison_panel(rgb, gt, pred, 1, CAD_CMAP_JET, dev_);
        cad::check(cad_memcpy(host_.data(), dev_, (int64_t)host_.size(), 1, nullptr), "panel d2h");
        ev.image("predictions/sample_" + std::to_string(sample), epoch, host_.data(), H_, 4 * W_);
    }

private:
    int H_, W_;
    cad::Exporter ex_;
    uint8_t* dev_ = nullptr;
    std::vector<uint8_t> host_;
};

// logWeightHistograms / logGradientStatistics (:506-555) for any network with a cad_*_histograms pass: weights/* and
// gradients/* histograms of every parameter tensor (all elements, not the reference's 10 000 strided samples) into
// `ev` when given, and the gradient pass's statistics as the reference's three scalars: norm = sqrt(sum of the
// tensors' sum_squares), max starts at 0, min at FLT_MAX.  run(which, &hist) is the model's pass, name(i) the
// i-th named_parameters() name.
struct GradientStats {
    double norm = 0.0;
    float max = 0.f, min = std::numeric_limits<float>::max();
};
template <class Run, class Name>
inline GradientStats log_histograms(EventWriter* ev, int num_params, int64_t epoch, Run&& run, Name&& name) {
    std::vector<double> stats((size_t)num_params * CAD_HIST_STATS);
    std::vector<uint32_t> counts(ev ? (size_t)num_params * CAD_HIST_BINS : 0);
    GradientStats g;
    double sq = 0.0;
    for (int which = ev ? 0 : 1; which < 2; ++which) {
        cad_hist* hh = nullptr;
        cad::check(run(which, &hh), "histogram pass");
        cad::check(cad_hist_read(hh, stats.data(), ev ? counts.data() : nullptr), "cad_hist_read");
        for (int i = 0; i < num_params; ++i) {
            const double* r = &stats[(size_t)i * CAD_HIST_STATS];   // num, min, max, sum, sum_squares, nonfinite
            if (ev) {
                std::string tag = std::string(which ? "gradients/" : "weights/") + name(i);
                std::replace(tag.begin(), tag.end(), '.', '/');
                ev->histogram(tag, epoch, r, &counts[(size_t)i * CAD_HIST_BINS]);
            }
            if (which == 1) {
                sq += r[4];
                if (r[0] > 0) { g.max = std::max(g.max, (float)r[2]); g.min = std::min(g.min, (float)r[1]); }
            }
        }
    }
    g.norm = std::sqrt(sq);
    return g;
}

// The declared recipe's bookkeeping across epochs (TrainingState, trainer.h:97-110): the best monitored metric
// so far and the validations since it last improved.  best starts at +inf (lower is better) or -inf.
struct RecipeProgress {
    float best_metric = std::numeric_limits<float>::infinity();
    int32_t epochs_without_improvement = 0;
    // checkImprovement (trainer.h:461-467): strictly better than best -/+ min_delta; updates the state
    bool improved(float current, bool lower_is_better, float min_delta) {
        const bool better = lower_is_better ? current < best_metric - min_delta : current > best_metric + min_delta;
        if (better) {
            best_metric = current;
            epochs_without_improvement = 0;
        } else {
            ++epochs_without_improvement;
        }
        return better;
    }
};

// a float32 with the nine significant digits that read back to the same float32
inline std::string float_text(float v) {
    std::ostringstream o;
    o << std::setprecision(std::numeric_limits<float>::max_digits10) << v;
    return o.str();
}

// .cadckpt: named parameters and buffers (reference layout) + the Adam state the reference never
// saves (moments, step count) — a full resume.  torch::save archives (.pt) carry the weights only.
// With the declared recipe the optimizer section is tagged instead ("RCPE": rule, hyper-parameters, step count
// and the rule's state slabs), followed by "EMA_" (decay and the averaged slab, when one is kept) and "BEST"
// (RecipeProgress); the learning rate is a function of the epoch and is not stored.  Files of the reference
// recipe carry none of these and are byte for byte what they were.
// the tensor block every .cadckpt starts with: the model's named parameters, then its named buffers
template <class Model>
inline void write_checkpoint_tensors(std::ostream& f, const Model& m) {
    auto ts = m.named_parameters();
    auto bs = m.named_buffers();
    ts.insert(ts.end(), bs.begin(), bs.end());
    f.write("CADCKPT1", 8);
    const int32_t n = (int32_t)ts.size();
    f.write((const char*)&n, 4);
    for (auto& t : ts) {
        const int32_t ln = (int32_t)t.name.size(), nd = (int32_t)t.shape.size();
        f.write((const char*)&ln, 4);
        f.write(t.name.data(), ln);
        f.write((const char*)&nd, 4);
        f.write((const char*)t.shape.data(), 8 * nd);
        f.write((const char*)t.value.data(), 4 * (int64_t)t.value.size());
    }
}

inline void save_training_state(const std::string& path, BaselineUNetImpl& m, optim::Adam& opt) {
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write checkpoint " + path);
    write_checkpoint_tensors(f, m);
    float *mp, *vp;
    int64_t nflat;
    cad::check(cad_unet_flat(m.handle(), nullptr, nullptr, &nflat), "flat");
    cad::check(cad_adam_state(opt.handle(), &mp, &vp), "adam_state");
    std::vector<float> buf((size_t)nflat);
    const int64_t step = opt.step_count();
    f.write("ADAM", 4);
    f.write((const char*)&step, 8);
    f.write((const char*)&nflat, 8);
    for (float* src : {mp, vp}) {
        cad::check(cad_memcpy(buf.data(), src, 4 * nflat, 1, nullptr), "d2h");
        f.write((const char*)buf.data(), 4 * nflat);
    }
}

// host-side writers / readers of the declared recipe's sections (no device: the slabs arrive as host arrays)
struct RecipeSections {
    int32_t rule = CAD_OPTIM_ADAM;
    float hyper[5] = {0.9f, 0.999f, 1e-8f, 0.f, 0.f};   // beta1, beta2, eps, weight_decay, momentum
    int64_t step = 0, nflat = 0;
    std::vector<std::vector<float>> slabs;   // m [, v]
    float ema_decay = 0.f;
    std::vector<float> ema;                  // empty: none
    bool have_progress = false;
    RecipeProgress progress;
    bool have_rule = false;                  // an "RCPE" section was read
    bool reference_adam = false;             // an "ADAM" section (reference recipe) was read instead
};
inline void write_recipe_sections(std::ostream& f, const RecipeSections& s) {
    f.write("RCPE", 4);
    f.write((const char*)&s.rule, 4);
    f.write((const char*)s.hyper, sizeof s.hyper);
    f.write((const char*)&s.step, 8);
    f.write((const char*)&s.nflat, 8);
    const int32_t ns = (int32_t)s.slabs.size();
    f.write((const char*)&ns, 4);
    for (auto& v : s.slabs) f.write((const char*)v.data(), 4 * s.nflat);
    if (!s.ema.empty()) {
        f.write("EMA_", 4);
        f.write((const char*)&s.ema_decay, 4);
        f.write((const char*)&s.nflat, 8);
        f.write((const char*)s.ema.data(), 4 * s.nflat);
    }
    f.write("BEST", 4);
    f.write((const char*)&s.progress.best_metric, 4);
    f.write((const char*)&s.progress.epochs_without_improvement, 4);
}
// reads every section after the tensor block until the end of the file; an "ADAM" section is kept as two slabs
inline RecipeSections read_recipe_sections(std::istream& f, const std::string& path) {
    RecipeSections s;
    char tag[4];
    auto slab = [&](std::vector<float>& v, int64_t n) {
        if (n < 0 || n > (int64_t)1 << 34) throw std::runtime_error("corrupt section size in " + path);
        v.resize((size_t)n);
        f.read((char*)v.data(), 4 * n);
    };
    while (f.read(tag, 4)) {
        if (std::memcmp(tag, "ADAM", 4) == 0) {
            s.reference_adam = true;
            f.read((char*)&s.step, 8);
            f.read((char*)&s.nflat, 8);
            s.slabs.resize(2);
            for (auto& v : s.slabs) slab(v, s.nflat);
        } else if (std::memcmp(tag, "RCPE", 4) == 0) {
            s.have_rule = true;
            int32_t ns = 0;
            f.read((char*)&s.rule, 4);
            f.read((char*)s.hyper, sizeof s.hyper);
            f.read((char*)&s.step, 8);
            f.read((char*)&s.nflat, 8);
            f.read((char*)&ns, 4);
            if (!f || ns < 1 || ns > 2) throw std::runtime_error("corrupt optimizer section in " + path);
            s.slabs.resize((size_t)ns);
            for (auto& v : s.slabs) slab(v, s.nflat);
        } else if (std::memcmp(tag, "EMA_", 4) == 0) {
            int64_t n = 0;
            f.read((char*)&s.ema_decay, 4);
            f.read((char*)&n, 8);
            slab(s.ema, n);
        } else if (std::memcmp(tag, "BEST", 4) == 0) {
            s.have_progress = true;
            f.read((char*)&s.progress.best_metric, 4);
            f.read((char*)&s.progress.epochs_without_improvement, 4);
        } else {
            throw std::runtime_error("unknown section '" + std::string(tag, 4) + "' in " + path);
        }
        if (!f) throw std::runtime_error("truncated section '" + std::string(tag, 4) + "' in " + path);
    }
    return s;
}

inline void save_training_state(const std::string& path, BaselineUNetImpl& m, optim::Optimizer& opt,
                                const RecipeProgress& progress) {
    std::ofstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot write checkpoint " + path);
    write_checkpoint_tensors(f, m);
    RecipeSections s;
    const cad_optim_opts& o = opt.options();
    s.rule = o.rule;
    const float hyper[5] = {o.beta1, o.beta2, o.eps, o.weight_decay, o.momentum};
    std::memcpy(s.hyper, hyper, sizeof hyper);
    s.step = opt.step_count();
    cad::check(cad_unet_flat(m.handle(), nullptr, nullptr, &s.nflat), "flat");
    float *mp = nullptr, *vp = nullptr, *ep = nullptr;
    cad::check(cad_optim_state(opt.handle(), &mp, &vp, &ep), "optim_state");
    auto fetch = [&](float* src) {
        std::vector<float> v((size_t)s.nflat);
        cad::check(cad_memcpy(v.data(), src, 4 * s.nflat, 1, nullptr), "d2h");
        return v;
    };
    s.slabs.push_back(fetch(mp));
    if (vp) s.slabs.push_back(fetch(vp));
    if (ep) {
        s.ema_decay = o.ema_decay;
        s.ema = fetch(ep);
    }
    s.progress = progress;
    write_recipe_sections(f, s);
}

// opens a .cadckpt and loads its tensor block into the model; the stream is left at the first section
inline std::ifstream load_checkpoint_tensors(const std::string& path, BaselineUNetImpl& m) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Cannot open checkpoint: " + path);
    char magic[8];
    f.read(magic, 8);
    if (!f || std::memcmp(magic, "CADCKPT1", 8) != 0) throw std::runtime_error("not a .cadckpt file: " + path);
    int32_t n;
    f.read((char*)&n, 4);
    std::vector<NamedTensor> ts((size_t)std::max(0, n));
    for (auto& t : ts) {
        int32_t ln, nd;
        f.read((char*)&ln, 4);
        t.name.resize((size_t)ln);
        f.read(&t.name[0], ln);
        f.read((char*)&nd, 4);
        t.shape.resize((size_t)nd);
        f.read((char*)t.shape.data(), 8 * nd);
        int64_t cnt = 1;
        for (auto s : t.shape) cnt *= s;
        t.value.resize((size_t)cnt);
        f.read((char*)t.value.data(), 4 * cnt);
    }
    if (f) {
        const std::string why = attention_checkpoint_mismatch(m, has_attention_tensors(ts), path);
        if (!why.empty()) throw std::runtime_error(why);
    }
    if (!f || m.load(ts) != n) throw std::runtime_error("checkpoint does not match the model: " + path);
    return f;
}

inline void load_training_state(const std::string& path, BaselineUNetImpl& m, optim::Adam& opt) {
    std::ifstream f = load_checkpoint_tensors(path, m);
    char tag[4];
    if (!f.read(tag, 4)) return;
    if (std::memcmp(tag, "RCPE", 4) == 0)
        throw std::runtime_error("checkpoint " + path + " was written by the declared recipe: resume it with "
                                 "optimization.recipe: declared (--recipe declared)");
    if (std::memcmp(tag, "ADAM", 4) == 0) {
        int64_t step, nflat, mine;
        f.read((char*)&step, 8);
        f.read((char*)&nflat, 8);
        float *mp, *vp;
        cad::check(cad_unet_flat(m.handle(), nullptr, nullptr, &mine), "flat");
        if (nflat != mine) throw std::runtime_error("optimizer state size mismatch in " + path);
        cad::check(cad_adam_state(opt.handle(), &mp, &vp), "adam_state");
        std::vector<float> buf((size_t)nflat);
        for (float* dst : {mp, vp}) {
            f.read((char*)buf.data(), 4 * nflat);
            cad::check(cad_memcpy(dst, buf.data(), 4 * nflat, 0, nullptr), "h2d");
        }
        cad::check(cad_adam_set_step_count(opt.handle(), step), "set_step");
    }
}

// Resume under the declared recipe: the rule must be the one the file was written by (a reference-recipe file
// counts as "adam"); its state slabs, step count, EMA and progress are restored.  A file without an average
// (or a run without one) restarts the average from the loaded weights.  The hyper-parameters the file records
// (betas, eps, weight_decay, momentum, the EMA decay) are a record only: like the learning rate, the resuming
// run's config decides them, so a run may be continued with, say, another weight decay.
inline void load_training_state(const std::string& path, BaselineUNetImpl& m, optim::Optimizer& opt, RecipeProgress& progress) {
    std::ifstream f = load_checkpoint_tensors(path, m);
    const RecipeSections s = read_recipe_sections(f, path);
    const int mine = opt.rule(), theirs = s.have_rule ? s.rule : CAD_OPTIM_ADAM;
    if ((s.have_rule || s.reference_adam) && theirs != mine)
        throw std::runtime_error("checkpoint " + path + " was written by optimizer '" + optim::Optimizer::rule_name(theirs) +
                                 (s.reference_adam ? "' (reference recipe)" : "'") + " but this run declares '" +
                                 optim::Optimizer::rule_name(mine) + "'");
    float *mp = nullptr, *vp = nullptr, *ep = nullptr;
    cad::check(cad_optim_state(opt.handle(), &mp, &vp, &ep), "optim_state");
    int64_t nflat = 0;
    cad::check(cad_unet_flat(m.handle(), nullptr, nullptr, &nflat), "flat");
    if (!s.slabs.empty()) {
        if (s.nflat != nflat || (int)s.slabs.size() != (vp ? 2 : 1))
            throw std::runtime_error("optimizer state size mismatch in " + path);
        cad::check(cad_memcpy(mp, s.slabs[0].data(), 4 * nflat, 0, nullptr), "h2d");
        if (vp) cad::check(cad_memcpy(vp, s.slabs[1].data(), 4 * nflat, 0, nullptr), "h2d");
        opt.set_step_count(s.step);
    }
    if (ep) {
        if ((int64_t)s.ema.size() == nflat) cad::check(cad_memcpy(ep, s.ema.data(), 4 * nflat, 0, nullptr), "h2d");
        else opt.attach_ema(opt.options().ema_decay);
    }
    if (s.have_progress) progress = s.progress;
}

class TensorBoardTrainerEnhanced {
public:
    struct Config {   // enhanced.h:37-63
        int num_epochs = 50;
        int batch_size = 8;
        float learning_rate = 1e-4f;
        float weight_decay = 1e-5f;
        bool use_grad_clip = true;
        float grad_clip_value = 1.0f;
        int val_interval = 10;
        int log_interval = 10;
        int save_interval = 5;
        int viz_interval = 1;
        int num_viz_samples = 4;
        int histogram_interval = 5;
        int profiler_interval = 0;
        std::string checkpoint_dir = "./checkpoints";
        std::string log_dir = "./logs";
        std::string tensorboard_dir = "./runs";
        std::string experiment_name = "experiment";
        int device = 0;              // torch::Device: the MI355X ordinal
        bool tensorboard = true;     // event files under <tensorboard_dir>/<experiment_name> + <log_dir>/tensorboard_scalars.csv
        bool save_optimizer = true;  // also write <name>_epoch_N.cadckpt next to each .pt
        int64_t bucket_elems = 25 << 18;   // data-parallel gradient buckets (25 MB)
        // The declared recipe (TrainingConfig, trainer.h:24-92; the epoch loop :262-316).  Off by default: the
        // trainers then run the reference's Adam at a constant rate and ignore every field below.
        bool recipe_declared = false;
        std::string optimizer = "adam";      // adam | adamw | sgd
        std::string lr_scheduler = "none";   // none | step | cosine (cad_lr_at)
        int lr_step_size = 30;
        float lr_gamma = 0.1f;
        int lr_warmup_epochs = 0;
        float lr_min = 0.f;
        float momentum = 0.9f;               // SGD
        float adam_betas[2] = {0.9f, 0.999f};
        float adam_eps = 1e-8f;
        bool use_early_stopping = false;
        int early_stop_patience = 20;        // validations without improvement
        float early_stop_min_delta = 0.f;
        std::string metric_to_monitor = "abs_rel";   // abs_rel sq_rel rmse rmse_log a1|delta_1.25 a2 a3 loss
        bool metric_lower_is_better = true;
        bool save_best_only = false;         // no periodic checkpoints (best_model.* and final_model.* only)
        int keep_last_n_checkpoints = 0;     // newest epoch checkpoints kept; 0 keeps all
        float ema_decay = 0.f;               // > 0: exponential moving average of the weights (U-Net family)
        // Independent of the recipe: the model's eval-mode forwards (validation, the prediction panels) run the
        // fused eval forward (BaselineUNetImpl::fused_eval; the train steps ignore it).  U-Net family only
        bool fused_eval = false;
    };

    // ---- the declared recipe's pieces shared with GeometryTrainer ----
    static cad_optim_opts optimOptions(const Config& c) {
        return cad_optim_opts{optim::Optimizer::rule_of(c.optimizer), c.learning_rate, c.adam_betas[0], c.adam_betas[1],
                              c.adam_eps, c.weight_decay, c.momentum, c.ema_decay};
    }
    // the rate of 1-based `epoch` (cad_lr_at); throws for plateau / unknown schedulers, naming the value
    static float learningRateAt(const Config& c, int epoch) {
        cad_lr_opts o{c.learning_rate, c.lr_scheduler.c_str(), c.lr_step_size, c.lr_gamma, c.lr_warmup_epochs, c.lr_min};
        float lr = 0.f;
        cad::check(cad_lr_at(&o, epoch - 1, c.num_epochs, &lr), "optimization");
        return lr;
    }
    // start-up checks of a declared recipe (before any training work)
    static void checkRecipe(const Config& c, bool data_parallel) {
        if (!c.recipe_declared) return;
        optim::Optimizer::rule_of(c.optimizer);
        learningRateAt(c, 1);
        static const char* const known[] = {"abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "delta_1.25", "a2", "a3", "loss"};
        if (std::find(std::begin(known), std::end(known), c.metric_to_monitor) == std::end(known))
            throw std::runtime_error("validation.primary_metric '" + c.metric_to_monitor + "': expected abs_rel, sq_rel, "
                                     "rmse, rmse_log, a1 (delta_1.25), a2, a3 or loss");
        if (c.ema_decay < 0.f || c.ema_decay >= 1.f) throw std::runtime_error("ema.decay must be in [0, 1)");
        if (c.use_early_stopping && data_parallel)
            throw std::runtime_error("early stopping with hardware.distributed: true needs a stop coordinated across "
                                     "ranks, which is not built: turn one of them off");
    }
    // keeps the keep_last_n highest epochs that have <experiment>_epoch_N.* files (.pt, .cadckpt, _ema.pt) and
    // deletes the files of every other epoch, whatever save_interval spaced them by; never best_* / final_*
    static void pruneCheckpoints(const Config& c) {
        if (c.keep_last_n_checkpoints <= 0) return;
        const std::string prefix = c.experiment_name + "_epoch_";
        std::error_code ec;
        std::vector<std::pair<long, std::filesystem::path>> files;   // (epoch, file)
        std::vector<long> epochs;
        for (auto& e : std::filesystem::directory_iterator(c.checkpoint_dir, ec)) {
            const std::string name = e.path().filename().string();
            if (name.compare(0, prefix.size(), prefix) != 0) continue;
            char* end = nullptr;
            const long n = std::strtol(name.c_str() + prefix.size(), &end, 10);
            if (end == name.c_str() + prefix.size() || (*end != '.' && *end != '_')) continue;
            files.emplace_back(n, e.path());
            epochs.push_back(n);
        }
        std::sort(epochs.begin(), epochs.end());
        epochs.erase(std::unique(epochs.begin(), epochs.end()), epochs.end());
        if ((int)epochs.size() <= c.keep_last_n_checkpoints) return;
        const long oldest_kept = epochs[epochs.size() - (size_t)c.keep_last_n_checkpoints];
        for (auto& f : files)
            if (f.first < oldest_kept) std::filesystem::remove(f.second, ec);
    }

    struct ValidationMetrics {   // enhanced.h:65-74
        float loss = 0.0f, abs_rel = 0.0f, sq_rel = 0.0f, rmse = 0.0f, rmse_log = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    };
    // val_metrics[config_.metric_to_monitor] (trainer.h:281)
    static float monitoredMetric(const Config& c, const ValidationMetrics& v) {
        const std::string& k = c.metric_to_monitor;
        return k == "loss" ? v.loss : k == "sq_rel" ? v.sq_rel : k == "rmse" ? v.rmse : k == "rmse_log" ? v.rmse_log
             : (k == "a1" || k == "delta_1.25") ? v.a1 : k == "a2" ? v.a2 : k == "a3" ? v.a3 : v.abs_rel;
    }
    // the validation scalars of an epoch (:196-208), in the reference's order; shared with GeometryTrainer
    template <class Scalar>
    static void validationScalars(Scalar&& scalar, const ValidationMetrics& v) {
        scalar("loss/val", v.loss);
        scalar("metrics/abs_rel", v.abs_rel);
        scalar("metrics/sq_rel", v.sq_rel);
        scalar("metrics/rmse", v.rmse);
        scalar("metrics/rmse_log", v.rmse_log);
        scalar("metrics/a1", v.a1);
        scalar("metrics/a2", v.a2);
        scalar("metrics/a3", v.a3);
    }

    // model and model_impl are the same network (the reference passes the Module and its Impl)
    TensorBoardTrainerEnhanced(std::shared_ptr<BaselineUNetImpl> model, std::shared_ptr<BaselineUNetImpl> model_impl,
                               std::shared_ptr<CombinedDepthLoss> loss_fn, const Config& config,
                               std::shared_ptr<distributed::Communicator> comm = nullptr)
        : model_(model_impl ? model_impl : model), loss_fn_(std::move(loss_fn)), config_(config), comm_(std::move(comm)) {
        if (!model_ || !loss_fn_) throw std::runtime_error("TensorBoardTrainerEnhanced: model and loss are required");
        rank_ = comm_ ? comm_->rank() : 0;
        world_ = comm_ ? comm_->size() : 1;
        lr_ = config_.learning_rate;
        checkRecipe(config_, comm_ != nullptr);
        if (config_.fused_eval) model_->fused_eval(true);
        if (config_.recipe_declared) {
            recipe_ = std::make_shared<optim::Optimizer>(*model_, optimOptions(config_));
            progress_.best_metric = config_.metric_lower_is_better ? INFINITY : -INFINITY;
        } else {
            optimizer_ = std::make_shared<optim::Adam>(*model_, config_.learning_rate, config_.weight_decay);
        }
        if (lead()) {
            std::filesystem::create_directories(config_.checkpoint_dir);
            std::filesystem::create_directories(config_.log_dir);
            train_log_.open(config_.log_dir + "/training.log", std::ios::app);
            metrics_csv_.open(config_.log_dir + "/metrics.csv", std::ios::app);
            if (metrics_csv_.tellp() == 0)   // :111-115
                metrics_csv_ << "epoch,step,train_loss,val_loss,abs_rel,sq_rel,rmse,rmse_log,a1,a2,a3,learning_rate,time_elapsed\n";
            if (config_.tensorboard) {
                tb_.open(config_.log_dir + "/tensorboard_scalars.csv", std::ios::app);
                if (tb_.tellp() == 0) tb_ << "tag,step,value\n";
                // a new run or a resume opens a new event file (never appends); other ranks write nothing
                events_ = std::make_unique<EventWriter>(config_.tensorboard_dir + "/" + config_.experiment_name);
            }
        }
        if (comm_) comm_->broadcast_parameters(*model_, 0);   // identical replicas
        if (comm_ && ema()) recipe_->attach_ema(config_.ema_decay);   // the average starts from the broadcast weights
    }
    const EventWriter* events() const { return events_.get(); }

    // the reference recipe's Adam (a declared recipe has recipe_optimizer() instead)
    optim::Adam& optimizer() {
        if (!optimizer_) throw std::runtime_error("optimizer(): the declared recipe runs recipe_optimizer()");
        return *optimizer_;
    }
    optim::Optimizer* recipe_optimizer() { return recipe_.get(); }
    int64_t optimizer_step_count() const { return recipe_ ? recipe_->step_count() : optimizer_->step_count(); }
    const RecipeProgress& progress() const { return progress_; }
    int64_t global_step() const { return global_step_; }
    // resume: parameters, BN buffers and the optimizer state (.cadckpt; with a declared recipe also the EMA and
    // the best-metric bookkeeping), or the weights of a torch::save archive (.pt: ours or the reference's; the
    // optimizer and the average start fresh)
    void loadCheckpoint(const std::string& path) {
        const bool pt = path.size() >= 3 && path.compare(path.size() - 3, 3, ".pt") == 0;
        if (pt) load(*model_, path);
        else if (recipe_) load_training_state(path, *model_, *recipe_, progress_);
        else load_training_state(path, *model_, *optimizer_);
        if (comm_) comm_->broadcast_parameters(*model_, 0);
        if (pt && ema()) recipe_->attach_ema(config_.ema_decay);
    }
    void saveTrainingState(const std::string& path) {
        if (recipe_) save_training_state(path, *model_, *recipe_, progress_);
        else save_training_state(path, *model_, *optimizer_);
    }

    // enhanced.h:142-240.  Epochs continue after a resumed optimizer step count (whole epochs done).
    void train(std::shared_ptr<SunRGBDLoader> train_loader, std::shared_ptr<SunRGBDLoader> val_loader = nullptr) {
        if (!train_loader) throw std::runtime_error("train: no training loader");
        const int nb = steps_per_epoch(train_loader->size());
        if (nb < 1) throw std::runtime_error("fewer training samples than one global batch");
        logMessage("=== Starting Training (MI355X) ===");
        logMessage("Train samples: " + std::to_string(train_loader->size()));
        if (val_loader) logMessage("Val samples: " + std::to_string(val_loader->size()));
        logMessage("Batch size: " + std::to_string(config_.batch_size) +
                   (world_ > 1 ? " per rank x " + std::to_string(world_) + " ranks" : std::string()));
        logMessage("Epochs: " + std::to_string(config_.num_epochs));
        if (tb_) {   // logHyperparameters / logModelArchitecture (:576-615)
            tb_ << "hparams/learning_rate,0," << config_.learning_rate << "\nhparams/batch_size,0," << config_.batch_size
                << "\nhparams/weight_decay,0," << config_.weight_decay << "\nhparams/grad_clip_value,0,"
                << config_.grad_clip_value << "\nhparams/num_epochs,0," << config_.num_epochs
                << "\nmodel/total_parameters,0," << model_->count_parameters() << "\n";
        }
        if (events_) {
            events_->reference_layout();
            events_->hparams(config_.learning_rate, config_.batch_size, config_.weight_decay, config_.grad_clip_value, config_.num_epochs);
            events_->architecture(model_->count_parameters(), model_->count_parameters());
            events_->flush();
        }
        const auto t0 = std::chrono::steady_clock::now();
        global_step_ = optimizer_step_count() / nb * nb;
        bool stop = false;
        for (int epoch = 1 + (int)(optimizer_step_count() / nb); epoch <= config_.num_epochs && !stop; ++epoch) {
            const auto te = std::chrono::steady_clock::now();
            if (lead()) std::cout << "\n" << std::string(60, '=') << "\nEpoch " << epoch << "/" << config_.num_epochs << "\n";
            if (recipe_) {   // warmup / scheduler (trainer.h:266-269, :305-308): the epoch's rate, a function of the epoch
                lr_ = learningRateAt(config_, epoch);
                recipe_->set_lr(lr_);
            }
            const float train_loss = trainEpoch(*train_loader, nb, (int)global_step_, epoch);
            if (lead()) {
                scalar("loss/train", train_loss, epoch);
                scalar("training/learning_rate", lr_, epoch);
                logLossComponents(*train_loader, epoch);
                scalar("training/epoch_time_seconds",
                       (double)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - te).count(),
                       epoch);
            }
            ValidationMetrics vm;
            bool best = false;   // this epoch's validation improved: best_model.* holds this epoch's checkpoint
            if (lead() && val_loader && config_.val_interval > 0 && epoch % config_.val_interval == 0) {
                if (ema()) recipe_->ema_swap();   // the averaged weights are what is validated and monitored
                vm = validateEpoch(*val_loader, epoch);
                if (ema()) recipe_->ema_swap();
                validationScalars([&](const char* tag, double v) { scalar(tag, v, epoch); }, vm);
                if (recipe_) {   // trainer.h:280-301
                    best = progress_.improved(monitoredMetric(config_, vm), config_.metric_lower_is_better,
                                              config_.early_stop_min_delta);
                    if (config_.use_early_stopping && progress_.epochs_without_improvement >= config_.early_stop_patience) {
                        logMessage("Early stopping triggered after " + std::to_string(epoch) + " epochs");
                        stop = true;   // the epoch's records are still written; final_model.* follows
                    }
                }
            }
            if (lead() && config_.histogram_interval > 0 && epoch % config_.histogram_interval == 0)
                logGradientStatistics(epoch);
            if (lead() && events_ && config_.viz_interval > 0 && epoch % config_.viz_interval == 0)
                visualizeResults(*train_loader, epoch);
            const bool due = lead() && config_.save_interval > 0 && epoch % config_.save_interval == 0 &&
                             !(recipe_ && config_.save_best_only);   // trainer.h:311
            if (due) saveCheckpoint(epoch);
            if (best) saveBestModel(epoch, due);
            if (due && recipe_) pruneCheckpoints(config_);
            const long total = (long)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0).count();
            if (lead()) {
                logEpochMetrics(epoch, (int)global_step_, train_loss, vm, total);
                scalar("training/total_time_seconds", (double)total, epoch);
                if (events_) events_->flush();
            }
            global_step_ += nb;   // :233
        }
        if (lead()) {
            saveModel(config_.checkpoint_dir + "/final_model");   // production_trainer.h:323-330
            logMessage("=== Training Complete ===");
        }
        events_.reset();   // closed at the end of train() (and by the destructor)
    }

    // per-rank batches of an epoch: global batch bi = samples [bi*B*world, (bi+1)*B*world); with more
    // than one rank the last partial global batch is dropped (every replica steps together)
    int steps_per_epoch(size_t n) const {
        const int64_t B = config_.batch_size;
        return world_ > 1 ? (int)((int64_t)n / (B * world_)) : (int)(((int64_t)n + B - 1) / B);
    }

private:
    bool lead() const { return rank_ == 0; }
    bool ema() const { return recipe_ && recipe_->has_ema(); }
    bool conditioned() const { return cad_unet_model(model_->handle()) != CAD_MODEL_BASELINE; }

    void ensure_buffers(const SunRGBDLoader& L) {
        const int B = config_.batch_size, H = L.target_height(), W = L.target_width();
        if (rgb_.numel() == (int64_t)B * 3 * H * W) return;
        const int d = config_.device;
        rgb_ = DeviceTensor::empty({B, 3, H, W}, d);
        gt_ = DeviceTensor::empty({B, 1, H, W}, d);
        K_ = DeviceTensor::empty({B, 3, 3}, d);
        pred_ = DeviceTensor::empty({B, 1, H, W}, d);
        cam_ = DeviceTensor::empty({B, 4}, d);
    }
    int next(cad_loader* ring, int expect) {
        const int n = cad_loader_next(ring, rgb_.data, gt_.data, K_.data, nullptr);
        if (n < 0) throw std::runtime_error(std::string("data loader: ") + cad_last_error());
        if (expect >= 0 && n != expect)
            throw std::runtime_error("data loader: batch of " + std::to_string(n) + ", expected " + std::to_string(expect));
        for (DeviceTensor* t : {&rgb_, &gt_, &K_, &pred_, &cam_}) t->shape[0] = n;
        return n;
    }
    // model_impl_->forward(rgb) (baseline) / forward(rgb, intrinsics) (the FiLM models, camera from K)
    void forward() {
        const int n = (int)rgb_.size(0);
        if (conditioned()) {
            cad::check(cad_camera_from_K(K_.data, n, cam_.data, nullptr), "camera_from_K");
            cad::check(cad_unet_forward_cam(model_->handle(), rgb_.data, cam_.data, pred_.data, n, nullptr), "forward");
        } else {
            model_->forward_into(rgb_, pred_);
        }
    }

    float trainEpoch(SunRGBDLoader& L, int nb, int global_step, int epoch) {   // :257-334
        (void)epoch;
        ensure_buffers(L);
        model_->train();
        const int B = config_.batch_size;
        const int64_t n = (int64_t)L.size();
        std::vector<int64_t> order;   // this rank's samples, in step order
        for (int bi = 0; bi < nb; ++bi) {
            const int64_t first = (int64_t)bi * B * world_ + (int64_t)rank_ * B;
            for (int64_t j = first; j < std::min<int64_t>(first + B, n); ++j) order.push_back(j);
        }
        cad_loader* ring = L.ring(B, config_.device, true);
        cad::check(cad_loader_start_epoch(ring, order.data(), (int64_t)order.size()), "start epoch");
        double total = 0.0;
        int64_t seen = 0;
        for (int bi = 0; bi < nb; ++bi) {
            const int64_t first = (int64_t)bi * B * world_ + (int64_t)rank_ * B;
            const int bs = (int)std::min<int64_t>(B, n - first);
            next(ring, bs);
            forward();   // (zero_grad: every backward overwrites the gradient slab)
            DeviceTensor l = loss_fn_->forwardWithIntrinsics(pred_, gt_, rgb_, K_);
            if (comm_) comm_->backward_allreduce(*model_, loss_fn_->dpred(), config_.bucket_elems);
            else model_->backward(loss_fn_->dpred());
            // clip_grad_norm_ on the mean gradient (the SUM all-reduce's 1/world folded in)
            double gnorm = 0.0;
            if (config_.use_grad_clip) gnorm = clip_grad_norm_(*model_, config_.grad_clip_value, nullptr, 1.0 / world_);
            else cad::check(cad_clip_grad_norm(model_->handle(), INFINITY, 1.f / world_, nullptr), "prescale");
            if (recipe_) recipe_->step();
            else optimizer_->step();
            if (comm_) comm_->allreduce(l.data, 5);   // the logged loss: mean over replicas
            const float lv = l.to_host()[0] / world_;   // loss.item<float>() (:307)
            if (!std::isfinite(lv)) throw std::runtime_error("non-finite loss at step " + std::to_string(global_step + bi));
            total += (double)lv * bs * world_;
            seen += (int64_t)bs * world_;
            if (lead() && (bi + 1) % std::max(1, config_.log_interval) == 0) {   // :313-319
                scalar("batch_loss/train", lv, global_step + bi);
                if (!config_.use_grad_clip) gnorm = clip_grad_norm_(*model_, INFINITY);   // computeGradientNorm
                scalar("training/gradient_norm", gnorm, global_step + bi);
            }
            if (lead() && ((bi + 1) % std::max(1, config_.log_interval) == 0 || bi == nb - 1)) {
                std::cout << "\r  [" << std::setw(3) << (100 * (bi + 1) / nb) << "%] Batch " << (bi + 1) << "/" << nb
                          << " | Loss: " << std::fixed << std::setprecision(4) << lv;
                if (recipe_) std::cout << " | LR: " << float_text(lr_);
                std::cout << std::flush;
            }
        }
        if (lead()) std::cout << std::endl;
        return (float)(total / std::max<int64_t>(1, seen));
    }

    // validateEpoch (:339-395): the first min(500, size) samples one at a time in eval mode; loss and
    // computeDepthMetrics averaged per sample
    ValidationMetrics validateEpoch(SunRGBDLoader& L, int epoch) {
        (void)epoch;
        ensure_buffers(L);
        model_->eval();
        ValidationMetrics m;
        const int64_t ns = std::min<int64_t>(500, (int64_t)L.size());
        cad_loader* ring = L.ring(1, config_.device, false);
        cad::check(cad_loader_start_epoch(ring, nullptr, ns), "validation");
        int count = 0;
        for (int64_t i = 0; i < ns; ++i) {
            next(ring, 1);
            forward();
            DeviceTensor l = loss_fn_->forwardWithIntrinsics(pred_, gt_, rgb_, K_);
            const DepthMetrics s = computeDepthMetrics(pred_, gt_);
            m.loss += l.to_host()[0];
            m.abs_rel += s.abs_rel; m.sq_rel += s.sq_rel; m.rmse += s.rmse; m.rmse_log += s.rmse_log;
            m.a1 += s.a1; m.a2 += s.a2; m.a3 += s.a3;
            ++count;
        }
        if (count)
            for (float* p : {&m.loss, &m.abs_rel, &m.sq_rel, &m.rmse, &m.rmse_log, &m.a1, &m.a2, &m.a3}) *p /= count;
        model_->train();
        return m;
    }

    void logLossComponents(SunRGBDLoader& L, int epoch) {   // :475-501
        if (!tb_ || L.size() == 0) return;
        ensure_buffers(L);
        model_->eval();
        cad_loader* ring = L.ring(1, config_.device, false);
        cad::check(cad_loader_start_epoch(ring, nullptr, 1), "loss components");
        next(ring, 1);
        forward();
        auto c = loss_fn_->getComponentsWithIntrinsics(pred_, gt_, rgb_, K_);
        for (const char* k : {"si_loss", "grad_loss", "smooth_loss", "reproj_loss"})
            scalar(std::string("loss_components/") + k, c[k], epoch);
        model_->train();
    }

    // weights/* and gradients/* histograms from the device pass (log_histograms), and gradients/norm|max|min
    // from its statistics instead of a host copy of every gradient
    void logGradientStatistics(int epoch) {
        if (!tb_) return;
        cad_unet* h = model_->handle();
        const GradientStats g = log_histograms(
            events_.get(), cad_unet_num_params(h), epoch, [&](int which, cad_hist** hh) { return cad_unet_histograms(h, which, nullptr, hh); },
            [&](int i) {
                const char* name = nullptr;
                cad::check(cad_unet_tensor_info(h, 0, i, &name, nullptr, nullptr), "tensor_info");
                return std::string(name);
            });
        scalar("gradients/norm", g.norm, epoch);
        scalar("gradients/max", g.max, epoch);
        scalar("gradients/min", g.min, epoch);
    }

    // predictions/sample_<i> panels (PanelLogger::run); train mode is restored after them
    void visualizeResults(SunRGBDLoader& L, int epoch) {
        ensure_buffers(L);
        model_->eval();
        if (ema()) recipe_->ema_swap();   // the panels show the averaged model, as validation scores it
        PanelLogger::run(panels_, *events_, L, config_.device, config_.num_viz_samples, epoch, rgb_.data, gt_.data,
                         [&](cad_loader* ring) { next(ring, 1); }, [&] { forward(); return (const float*)pred_.data; });
        if (ema()) recipe_->ema_swap();
        model_->train();
    }

    void logEpochMetrics(int epoch, int step, float train_loss, const ValidationMetrics& v, long elapsed) {   // :620-651
        std::stringstream ss;
        ss << "Epoch " << epoch << " | Train Loss: " << std::fixed << std::setprecision(4) << train_loss;
        if (v.loss > 0)
            ss << " | Val Loss: " << v.loss << " | abs_rel: " << v.abs_rel << " | rmse: " << v.rmse
               << " | a1: " << std::setprecision(3) << v.a1;
        ss << " | Time: " << elapsed << "s";
        logMessage(ss.str());
        metrics_csv_ << epoch << "," << step << "," << train_loss << "," << v.loss << "," << v.abs_rel << "," << v.sq_rel
                     << "," << v.rmse << "," << v.rmse_log << "," << v.a1 << "," << v.a2 << "," << v.a3 << ",";
        if (recipe_) metrics_csv_ << float_text(lr_);   // the epoch's scheduled rate, digits that read back exactly
        else metrics_csv_ << config_.learning_rate;
        metrics_csv_ << "," << elapsed << "\n";
        metrics_csv_.flush();
    }

    std::string checkpointStem(int epoch) const {
        return config_.checkpoint_dir + "/" + config_.experiment_name + "_epoch_" + std::to_string(epoch);
    }
    void saveCheckpoint(int epoch) {   // :656-662: torch::save(model_, <dir>/<experiment>_epoch_N.pt)
        saveModel(checkpointStem(epoch));
        logMessage("Checkpoint saved: " + checkpointStem(epoch) + ".pt");
    }
    // best_model.*: copies of this epoch's checkpoint files when one was just written (the same files byte for
    // byte), else written on their own.  Only the files this run writes; a sibling an earlier run left is removed.
    void saveBestModel(int epoch, bool checkpoint_written) {
        namespace fs = std::filesystem;
        const std::string best = config_.checkpoint_dir + "/best_model";
        if (!checkpoint_written) saveModel(best);
        const std::pair<const char*, bool> files[] = {{".pt", true}, {".cadckpt", config_.save_optimizer}, {"_ema.pt", ema()}};
        for (const auto& [suffix, written] : files) {
            if (!written) fs::remove(best + suffix);
            else if (checkpoint_written) fs::copy_file(checkpointStem(epoch) + suffix, best + suffix, fs::copy_options::overwrite_existing);
        }
        logMessage("Best model saved: " + best + ".pt (epoch " + std::to_string(epoch) + ", " + config_.metric_to_monitor +
                   " " + std::to_string(progress_.best_metric) + ")");
    }
    // <stem>.pt (the raw weights), <stem>.cadckpt (save_optimizer) and, with an EMA, <stem>_ema.pt: the averaged
    // weights with the live BatchNorm buffers, an archive build/evaluate and build/predict load like any other
    void saveModel(const std::string& stem) {
        save(*model_, stem + ".pt");
        if (config_.save_optimizer) saveTrainingState(stem + ".cadckpt");
        if (ema()) {
            recipe_->ema_swap();
            save(*model_, stem + "_ema.pt");
            recipe_->ema_swap();
        }
    }

    void scalar(const std::string& tag, double v, int64_t step) {
        if (tb_) tb_ << tag << "," << step << "," << v << "\n";
        if (events_) events_->scalar(tag, (float)v, step);
    }
    void logMessage(const std::string& msg) {   // :667-682
        if (!lead()) return;
        const std::time_t t = std::time(nullptr);
        std::stringstream ts;
        ts << "[" << std::put_time(std::localtime(&t), "%Y-%m-%d %H:%M:%S") << "] " << msg;
        std::cout << ts.str() << std::endl;
        if (train_log_.is_open()) {
            train_log_ << ts.str() << "\n";
            train_log_.flush();
        }
    }

    std::shared_ptr<BaselineUNetImpl> model_;
    std::shared_ptr<CombinedDepthLoss> loss_fn_;
    std::shared_ptr<optim::Adam> optimizer_;       // the reference recipe
    std::shared_ptr<optim::Optimizer> recipe_;     // the declared recipe (exactly one of the two exists)
    RecipeProgress progress_;
    float lr_ = 0.f;                               // the rate in force: config.learning_rate, or the epoch's schedule
    Config config_;
    std::shared_ptr<distributed::Communicator> comm_;
    int rank_ = 0, world_ = 1;
    int64_t global_step_ = 0;
    std::ofstream train_log_, metrics_csv_, tb_;
    std::unique_ptr<EventWriter> events_;   // lead rank with config.tensorboard only
    std::unique_ptr<PanelLogger> panels_;
    DeviceTensor rgb_, gt_, K_, pred_, cam_;
};

// The same training loop (enhanced.h:142-240, 257-395) for the geometry-aware networks
// (geometry_aware_network.h: GeometryAwareNetworkImpl / LightweightGeometryNetworkImpl), fed the
// loader's batch as the reference's forward takes it: rgb, RayDirectionComputer's rays (a18) and the
// (B,4) intrinsics (a15).  Single process; the Adam moments live in the model; checkpoints are
// <exp>_epoch_N.cadckpt / final_model.cadckpt (named parameters and buffers, reference layout).
class GeometryTrainer {
public:
    using Config = TensorBoardTrainerEnhanced::Config;
    GeometryTrainer(std::shared_ptr<GeometryAwareNetworkImpl> model, std::shared_ptr<CombinedDepthLoss> loss_fn,
                    const Config& config)
        : model_(std::move(model)), loss_fn_(std::move(loss_fn)), config_(config) {
        if (!model_ || !loss_fn_) throw std::runtime_error("GeometryTrainer: model and loss are required");
        TensorBoardTrainerEnhanced::checkRecipe(config_, false);
        if (config_.recipe_declared && config_.ema_decay != 0.f)
            throw std::runtime_error("ema: the weight average is built for the U-Net family only; turn ema off for "
                                     "the geometry-aware networks");
        if (config_.fused_eval)
            throw std::runtime_error("fused_eval: the fused eval forward is built for the U-Net family only; turn it off "
                                     "for the geometry-aware networks");
        lr_ = config_.learning_rate;
        progress_.best_metric = config_.metric_lower_is_better ? INFINITY : -INFINITY;
        std::filesystem::create_directories(config_.checkpoint_dir);
        std::filesystem::create_directories(config_.log_dir);
        log_.open(config_.log_dir + "/training.log", std::ios::app);
        metrics_csv_.open(config_.log_dir + "/metrics.csv", std::ios::app);
        if (metrics_csv_.tellp() == 0)
            metrics_csv_ << "epoch,step,train_loss,val_loss,abs_rel,sq_rel,rmse,rmse_log,a1,a2,a3,learning_rate,time_elapsed\n";
        if (config_.tensorboard) events_ = std::make_unique<EventWriter>(config_.tensorboard_dir + "/" + config_.experiment_name);
    }

    void train(std::shared_ptr<SunRGBDLoader> train_loader, std::shared_ptr<SunRGBDLoader> val_loader = nullptr) {
        if (!train_loader) throw std::runtime_error("train: no training loader");
        const int B = config_.batch_size;
        const int nb = (int)(((int64_t)train_loader->size() + B - 1) / B);
        if (nb < 1) throw std::runtime_error("no training samples");
        msg("=== Starting Training (MI355X, geometry-aware network) ===");
        msg("Train samples: " + std::to_string(train_loader->size()) + ", batch size " + std::to_string(B) +
            ", epochs " + std::to_string(config_.num_epochs));
        if (events_) {
            events_->reference_layout();
            events_->hparams(config_.learning_rate, config_.batch_size, config_.weight_decay, config_.grad_clip_value, config_.num_epochs);
            events_->architecture(model_->count_parameters(), model_->count_parameters());
            events_->flush();
        }
        const auto t0 = std::chrono::steady_clock::now();
        int64_t step = 0;
        const bool declared = config_.recipe_declared;
        bool stop = false;
        for (int epoch = 1; epoch <= config_.num_epochs && !stop; ++epoch) {
            std::cout << "\n" << std::string(60, '=') << "\nEpoch " << epoch << "/" << config_.num_epochs << "\n";
            if (declared) lr_ = TensorBoardTrainerEnhanced::learningRateAt(config_, epoch);
            const float tl = trainEpoch(*train_loader, nb, step);
            TensorBoardTrainerEnhanced::ValidationMetrics vm;
            scalar("loss/train", tl, epoch);
            scalar("training/learning_rate", lr_, epoch);
            if (val_loader && config_.val_interval > 0 && epoch % config_.val_interval == 0) {
                vm = validate(*val_loader);
                TensorBoardTrainerEnhanced::validationScalars([&](const char* tag, double v) { scalar(tag, v, epoch); }, vm);
                if (declared) {   // trainer.h:280-301, as TensorBoardTrainerEnhanced::train
                    if (progress_.improved(TensorBoardTrainerEnhanced::monitoredMetric(config_, vm),
                                           config_.metric_lower_is_better, config_.early_stop_min_delta))
                        save(config_.checkpoint_dir + "/best_model.cadckpt");
                    if (config_.use_early_stopping && progress_.epochs_without_improvement >= config_.early_stop_patience) {
                        msg("Early stopping triggered after " + std::to_string(epoch) + " epochs");
                        stop = true;
                    }
                }
            }
            if (config_.histogram_interval > 0 && epoch % config_.histogram_interval == 0) logGradientStatistics(epoch);
            if (events_ && config_.viz_interval > 0 && epoch % config_.viz_interval == 0) visualize(*train_loader, epoch);
            if (config_.save_interval > 0 && epoch % config_.save_interval == 0 && !(declared && config_.save_best_only)) {
                save(config_.checkpoint_dir + "/" + config_.experiment_name + "_epoch_" + std::to_string(epoch) +
                     ".cadckpt");
                if (declared) TensorBoardTrainerEnhanced::pruneCheckpoints(config_);
            }
            const long el = (long)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::steady_clock::now() - t0).count();
            std::stringstream ss;
            ss << "Epoch " << epoch << " | Train Loss: " << std::fixed << std::setprecision(4) << tl;
            if (vm.loss > 0) ss << " | Val Loss: " << vm.loss << " | abs_rel: " << vm.abs_rel << " | rmse: " << vm.rmse;
            msg(ss.str());
            metrics_csv_ << epoch << "," << step << "," << tl << "," << vm.loss << "," << vm.abs_rel << "," << vm.sq_rel
                         << "," << vm.rmse << "," << vm.rmse_log << "," << vm.a1 << "," << vm.a2 << "," << vm.a3 << ",";
            if (declared) metrics_csv_ << float_text(lr_);
            else metrics_csv_ << config_.learning_rate;
            metrics_csv_ << "," << el << "\n";
            metrics_csv_.flush();
            scalar("training/total_time_seconds", (double)el, epoch);
            if (events_) events_->flush();
            step += nb;
        }
        save(config_.checkpoint_dir + "/final_model.cadckpt");
        msg("=== Training Complete ===");
        events_.reset();
    }

    // named parameters and buffers in the .cadckpt layout (no optimizer section)
    void save(const std::string& path) {
        std::ofstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("cannot write checkpoint " + path);
        write_checkpoint_tensors(f, *model_);
        msg("Checkpoint saved: " + path);
    }

private:
    void ensure(const SunRGBDLoader& L) {
        const int B = config_.batch_size, H = L.target_height(), W = L.target_width(), d = config_.device;
        if (rgb_.numel() == (int64_t)B * 3 * H * W) return;
        rgb_ = DeviceTensor::empty({B, 3, H, W}, d);
        gt_ = DeviceTensor::empty({B, 1, H, W}, d);
        K_ = DeviceTensor::empty({B, 3, 3}, d);
        rays_ = DeviceTensor::empty({B, 3, H, W}, d);
        cam_ = DeviceTensor::empty({B, 4}, d);
    }
    int next(cad_loader* ring) {
        const int n = cad_loader_next(ring, rgb_.data, gt_.data, K_.data, nullptr);
        if (n < 0) throw std::runtime_error(std::string("data loader: ") + cad_last_error());
        for (DeviceTensor* t : {&rgb_, &gt_, &K_, &rays_, &cam_}) t->shape[0] = n;
        const int H = (int)rgb_.size(2), W = (int)rgb_.size(3);
        cad::check(cad_ray_directions(K_.data, n, H, W, rays_.data, nullptr), "rays");   // a18
        cad::check(cad_camera_from_K(K_.data, n, cam_.data, nullptr), "camera_from_K");  // a15
        return n;
    }
    float trainEpoch(SunRGBDLoader& L, int nb, int64_t step0) {
        ensure(L);
        model_->train();
        cad_loader* ring = L.ring(config_.batch_size, config_.device, true);
        cad::check(cad_loader_start_epoch(ring, nullptr, (int64_t)L.size()), "start epoch");
        double total = 0.0;
        int64_t seen = 0;
        for (int bi = 0; bi < nb; ++bi) {
            const int n = next(ring);
            DeviceTensor pred = model_->forward(rgb_, rays_, cam_);
            DeviceTensor l = loss_fn_->forwardWithIntrinsics(pred, gt_, rgb_, K_);
            model_->backward(loss_fn_->dpred());
            model_->clip_grad_norm_(config_.use_grad_clip ? config_.grad_clip_value : INFINITY);
            if (config_.recipe_declared) {
                cad_optim_opts o = TensorBoardTrainerEnhanced::optimOptions(config_);
                o.lr = lr_;
                model_->optim_step(o);
            } else {
                model_->adam_step(config_.learning_rate, config_.weight_decay);
            }
            const float lv = l.to_host()[0];
            if (!std::isfinite(lv)) throw std::runtime_error("non-finite loss at step " + std::to_string(step0 + bi));
            total += (double)lv * n;
            seen += n;
            if ((bi + 1) % std::max(1, config_.log_interval) == 0) scalar("batch_loss/train", lv, step0 + bi);
            if ((bi + 1) % std::max(1, config_.log_interval) == 0 || bi == nb - 1)
                std::cout << "\r  [" << std::setw(3) << (100 * (bi + 1) / nb) << "%] Batch " << (bi + 1) << "/" << nb
                          << " | Loss: " << std::fixed << std::setprecision(4) << lv << std::flush;
        }
        std::cout << std::endl;
        return (float)(total / std::max<int64_t>(1, seen));
    }
    TensorBoardTrainerEnhanced::ValidationMetrics validate(SunRGBDLoader& L) {
        ensure(L);
        model_->eval();
        TensorBoardTrainerEnhanced::ValidationMetrics m;
        const int64_t ns = std::min<int64_t>(500, (int64_t)L.size());
        cad_loader* ring = L.ring(1, config_.device, false);
        cad::check(cad_loader_start_epoch(ring, nullptr, ns), "validation");
        int count = 0;
        for (int64_t i = 0; i < ns; ++i) {
            next(ring);
            DeviceTensor pred = model_->forward(rgb_, rays_, cam_);
            DeviceTensor l = loss_fn_->forwardWithIntrinsics(pred, gt_, rgb_, K_);
            const DepthMetrics s = computeDepthMetrics(pred, gt_);
            m.loss += l.to_host()[0];
            m.abs_rel += s.abs_rel; m.sq_rel += s.sq_rel; m.rmse += s.rmse; m.rmse_log += s.rmse_log;
            m.a1 += s.a1; m.a2 += s.a2; m.a3 += s.a3;
            ++count;
        }
        if (count)
            for (float* p : {&m.loss, &m.abs_rel, &m.sq_rel, &m.rmse, &m.rmse_log, &m.a1, &m.a2, &m.a3}) *p /= count;
        model_->train();
        return m;
    }
    // the panels of TensorBoardTrainerEnhanced::visualizeResults, with this family's forward
    void visualize(SunRGBDLoader& L, int epoch) {
        ensure(L);
        model_->eval();
        DeviceTensor pred;
        PanelLogger::run(panels_, *events_, L, config_.device, config_.num_viz_samples, epoch, rgb_.data, gt_.data,
                         [&](cad_loader* ring) { next(ring); },
                         [&] { pred = model_->forward(rgb_, rays_, cam_); return (const float*)pred.data; });
        model_->train();
    }
    // weights/*, gradients/* and gradients/norm|max|min as TensorBoardTrainerEnhanced::logGradientStatistics
    void logGradientStatistics(int epoch) {
        if (!events_) return;
        cad_geonet* h = model_->handle();
        const GradientStats g = log_histograms(
            events_.get(), cad_geonet_num_tensors(h, 0), epoch,
            [&](int which, cad_hist** hh) { return cad_geonet_histograms(h, which, nullptr, hh); },
            [&](int i) {
                const char* name = nullptr;
                cad::check(cad_geonet_tensor_info(h, 0, i, &name, nullptr, nullptr), "tensor_info");
                return std::string(name);
            });
        scalar("gradients/norm", g.norm, epoch);
        scalar("gradients/max", g.max, epoch);
        scalar("gradients/min", g.min, epoch);
    }
    void scalar(const std::string& tag, double v, int64_t step) {
        if (events_) events_->scalar(tag, (float)v, step);
    }
    void msg(const std::string& s) {
        std::cout << s << std::endl;
        if (log_.is_open()) { log_ << s << "\n"; log_.flush(); }
    }

    std::shared_ptr<GeometryAwareNetworkImpl> model_;
    std::shared_ptr<CombinedDepthLoss> loss_fn_;
    Config config_;
    RecipeProgress progress_;   // the declared recipe's best metric / validations without improvement
    float lr_ = 0.f;            // the rate in force: config.learning_rate, or the epoch's schedule
    std::ofstream log_, metrics_csv_;
    std::unique_ptr<EventWriter> events_;   // config.tensorboard only
    std::unique_ptr<PanelLogger> panels_;
    DeviceTensor rgb_, gt_, K_, rays_, cam_;
};

}  // namespace camera_aware_depth

#endif  // CAD_TRAINER_HPP
