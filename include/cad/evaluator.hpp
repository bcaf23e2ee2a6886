// evaluator.hpp — header-only C++ drop-in for the reference's offline evaluation, over cad.hpp / cad.h.
//
//   camera_aware_depth::DepthMetricsFull    DepthMetrics            src/evaluation/depth_metrics.h:28-254
//   camera_aware_depth::MetricsAccumulator  MetricsAccumulator      depth_metrics.h:259-304
//   camera_aware_depth::formatMetrics       formatMetrics           depth_metrics.h:309-333
//   camera_aware_depth::ModelEvaluator      Evaluator               src/evaluation/evaluator.h
//
// (cad.hpp's DepthMetrics struct is the trainer's seven-number computeDepthMetrics result; the evaluation
// class therefore carries the name DepthMetricsFull.)  Everything is built on the device-resident
// cad_evaluator: predictions are scored where they are produced, the twelve sums per sample stay on the
// device, and one copy at the end brings them to the host.
#ifndef CAD_EVALUATOR_HPP
#define CAD_EVALUATOR_HPP

#include <cstring>
#include <fstream>
#include <functional>
#include <iomanip>
#include <sstream>
#include <type_traits>

#include "cad.hpp"
#include "trainer.hpp"

namespace camera_aware_depth {

using MetricMap = std::map<std::string, float>;

// DepthMetrics::compute's keys in cad.h's metric order
inline const std::array<const char*, CAD_EVAL_METRICS>& metricKeys() {
    static const std::array<const char*, CAD_EVAL_METRICS> k = {
        "abs_rel", "sq_rel", "rmse", "rmse_log", "mae", "log10", "delta_1.25", "delta_1.25^2", "delta_1.25^3",
        "num_valid_pixels", "mean_pred_depth", "mean_gt_depth"};
    return k;
}
inline MetricMap metricMap(const float* v) {
    MetricMap m;
    for (int k = 0; k < CAD_EVAL_METRICS; ++k) m[metricKeys()[(size_t)k]] = v[k];
    return m;
}

// per-sample scale alignment of the prediction before the metrics (cad_eval_align of cad.h; the reference
// has no counterpart)
enum class Alignment { None = CAD_ALIGN_NONE, Median = CAD_ALIGN_MEDIAN, LogMean = CAD_ALIGN_LOG_MEAN,
                       ScaleShift = CAD_ALIGN_SCALE_SHIFT };
inline const char* alignmentName(Alignment a) {
    switch (a) {
        case Alignment::Median: return "median";
        case Alignment::LogMean: return "log_mean";
        case Alignment::ScaleShift: return "scale_shift";
        default: return "none";
    }
}
inline bool parseAlignment(const std::string& s, Alignment* out) {
    for (Alignment a : {Alignment::None, Alignment::Median, Alignment::LogMean, Alignment::ScaleShift})
        if (s == alignmentName(a)) {
            *out = a;
            return true;
        }
    return false;
}

// Stratified evaluation (cad.h, "stratified evaluation"): the per-pixel axes and one axis's result
enum class StrataAxis { Depth = CAD_STRATA_DEPTH, Angle = CAD_STRATA_ANGLE };
struct StrataResult {
    int bins = 0;                            // 0: the axis was off
    std::vector<float> edges;                // bins + 1: metres, or degrees ending at 90
    std::vector<double> sums;                // count x bins x 12
    std::vector<float> per_sample;           // count x bins x 12 metrics, metricKeys() order
    std::vector<cad_eval_summary> summary;   // per bin, over the samples with a valid pixel in it
};
// cad_strata_config of two cut lists (empty: that axis is off); more than 15 cuts throw, naming the count
inline cad_strata_config strataConfig(const std::vector<float>& depth_cuts, const std::vector<float>& angle_cuts_deg) {
    cad_strata_config c{};
    const auto fill = [](const char* what, const std::vector<float>& v, int* n, float* out) {
        if (v.size() > (size_t)CAD_STRATA_MAX_BINS - 1)
            throw std::runtime_error(std::string(what) + " cuts: " + std::to_string(v.size()) + " given, at most " +
                                     std::to_string(CAD_STRATA_MAX_BINS - 1));
        *n = (int)v.size();
        for (size_t j = 0; j < v.size(); ++j) out[j] = v[j];
    };
    fill("depth", depth_cuts, &c.n_depth_cuts, c.depth_cuts);
    fill("angle", angle_cuts_deg, &c.n_angle_cuts, c.angle_cuts_deg);
    return c;
}

// Geometric evaluation (cad.h, "geometric evaluation"): the surface-normal and 3-D point metrics of a run
inline const std::vector<const char*>& geometryKeys() {
    static const std::vector<const char*> k = {"normal_mean", "normal_median", "normal_rmse", "normal_11.25", "normal_22.5",
                                               "normal_30", "num_normal_pixels", "point_mae", "point_rmse"};
    return k;
}
struct GeometryResult {
    bool on = false;                 // false: geometry was off, everything below is empty
    std::vector<double> sums;        // count x 8
    std::vector<float> medians;      // count: median theta of each sample
    std::vector<float> per_sample;   // count x 9 metrics, geometryKeys() order
    cad_geom_summary summary{};      // the normal columns over the samples with a normal-valid pixel
};

// RAII handle of a cad_evaluator
class MetricsTable {
public:
    MetricsTable(int64_t capacity, int max_batch, int H, int W, float min_depth = 0.1f, float max_depth = 10.0f,
                 bool clamp_pred = true, int device = 0, Alignment align = Alignment::None) {
        const cad_eval_config c{min_depth, max_depth, clamp_pred ? 1 : 0};
        cad::check(cad_evaluator_create(capacity, max_batch, H, W, &c, device, &h_), "cad_evaluator_create");
        if (align != Alignment::None && cad_evaluator_set_alignment(h_, (int)align) != CAD_OK) {
            const std::string why = cad_last_error();
            cad_evaluator_destroy(h_);
            throw std::runtime_error("cad_evaluator_set_alignment: " + why);
        }
    }
    ~MetricsTable() { cad_evaluator_destroy(h_); }
    MetricsTable(const MetricsTable&) = delete;
    MetricsTable& operator=(const MetricsTable&) = delete;
    // asynchronous on `stream`: no allocation, no host synchronisation
    void update(const DeviceTensor& pred, const DeviceTensor& gt, const uint8_t* mask = nullptr, void* stream = nullptr) {
        cad::check(cad_evaluator_update(h_, pred.data, gt.data, mask, (int)pred.size(0), stream), "cad_evaluator_update");
    }
    // the form with the batch's K (B,3,3): required while the angle strata are on
    void update(const DeviceTensor& pred, const DeviceTensor& gt, const uint8_t* mask, const DeviceTensor& K, void* stream = nullptr) {
        cad::check(cad_evaluator_update_k(h_, pred.data, gt.data, mask, K.data, (int)pred.size(0), stream), "cad_evaluator_update_k");
    }
    // allowed only while count() == 0; allocates the strata table, so that update still allocates nothing
    void setStrata(const std::vector<float>& depth_cuts, const std::vector<float>& angle_cuts_deg) {
        const cad_strata_config c = strataConfig(depth_cuts, angle_cuts_deg);
        cad::check(cad_evaluator_set_strata(h_, &c), "cad_evaluator_set_strata");
        depth_cuts_ = depth_cuts;
        angle_cuts_ = angle_cuts_deg;
    }
    // allowed only while count() == 0; allocates the geometry table, maps and workspace, so that update still
    // allocates nothing.  While on, update needs the batch's K.
    void setGeometry(bool on) { cad::check(cad_evaluator_set_geometry(h_, on ? 1 : 0), "cad_evaluator_set_geometry"); }
    bool geometryOn() const { return cad_evaluator_get_geometry(h_) != 0; }
    // the eight geometry sums per sample (count x 8); one synchronous copy on `stream`
    std::vector<double> geometrySums(void* stream = nullptr) {
        std::vector<double> s((size_t)count() * CAD_GEOM_SUMS);
        cad::check(cad_evaluator_geom_sums(h_, s.data(), stream), "cad_evaluator_geom_sums");
        return s;
    }
    // sums, medians, per-sample metrics and summary; synchronous copies on `stream` (on == false: geometry off)
    GeometryResult geometry(void* stream = nullptr) {
        GeometryResult r;
        r.on = geometryOn();
        if (!r.on) return r;
        r.sums = geometrySums(stream);
        r.medians.assign((size_t)count(), 0.f);
        r.per_sample.assign((size_t)count() * CAD_GEOM_METRICS, 0.f);
        cad::check(cad_evaluator_geom_medians(h_, r.medians.data(), stream), "cad_evaluator_geom_medians");
        const std::vector<double> total = sums(stream);
        cad::check(cad_eval_geom_finish(r.sums.data(), r.medians.data(), total.data(), count(), r.per_sample.data(), &r.summary),
                   "cad_eval_geom_finish");
        return r;
    }
    int strataBins(StrataAxis axis) const { return cad_evaluator_strata_bins(h_, (int)axis); }
    // one axis's sums, metrics and per-bin summaries; one synchronous copy on `stream` (bins == 0: axis off)
    StrataResult strata(StrataAxis axis, float lo, float hi, void* stream = nullptr) {
        StrataResult r;
        r.bins = strataBins(axis);
        if (r.bins == 0) return r;
        const std::vector<float>& cuts = axis == StrataAxis::Depth ? depth_cuts_ : angle_cuts_;
        r.edges.push_back(lo);
        r.edges.insert(r.edges.end(), cuts.begin(), cuts.end());
        r.edges.push_back(hi);
        const size_t n = (size_t)count() * (size_t)r.bins * CAD_EVAL_METRICS;
        r.sums.assign(n, 0.0);
        r.per_sample.assign(n, 0.f);
        r.summary.resize((size_t)r.bins);
        cad::check(cad_evaluator_strata_sums(h_, (int)axis, r.sums.data(), stream), "cad_evaluator_strata_sums");
        cad::check(cad_eval_strata_finish(r.sums.data(), count(), r.bins, r.per_sample.data(), r.summary.data()),
                   "cad_eval_strata_finish");
        return r;
    }
    // the table's twelve sums per sample (count x 12); one synchronous copy on `stream`
    std::vector<double> sums(void* stream = nullptr) {
        std::vector<double> s((size_t)count() * CAD_EVAL_METRICS);
        cad::check(cad_evaluator_sums(h_, s.data(), stream), "cad_evaluator_sums");
        return s;
    }
    void reset() { cad::check(cad_evaluator_reset(h_), "cad_evaluator_reset"); }
    int64_t count() const { return cad_evaluator_count(h_); }
    // per-sample metrics (count x 12, metricKeys() order) and the summary; one synchronous copy
    std::vector<float> metrics(cad_eval_summary* summary = nullptr) {
        std::vector<float> per((size_t)count() * CAD_EVAL_METRICS);
        cad::check(cad_evaluator_metrics(h_, per.data(), summary), "cad_evaluator_metrics");
        return per;
    }
    // allowed only while count() == 0
    void setAlignment(Alignment a) { cad::check(cad_evaluator_set_alignment(h_, (int)a), "cad_evaluator_set_alignment"); }
    Alignment alignmentMode() const { return (Alignment)cad_evaluator_get_alignment(h_); }
    // per-sample (scale, shift), count x 2, and (nullable) whether the mode's own formula gave the row
    // (0 where a fallback applied); synchronous copies on the stream of the caller's updates
    std::vector<float> alignment(std::vector<uint8_t>* aligned = nullptr, void* stream = nullptr) {
        std::vector<float> st((size_t)count() * 2);
        cad::check(cad_evaluator_alignment(h_, st.data(), stream), "cad_evaluator_alignment");
        if (aligned) {
            aligned->assign((size_t)count(), 0);
            cad::check(cad_evaluator_aligned(h_, aligned->data(), stream), "cad_evaluator_aligned");
        }
        return st;
    }
    cad_evaluator* handle() const { return h_; }

private:
    cad_evaluator* h_ = nullptr;
    std::vector<float> depth_cuts_, angle_cuts_;
};

struct DepthMetricsFull {
    // compute (depth_metrics.h:40-88): the metrics over all valid pixels of the batch
    static MetricMap compute(const DeviceTensor& pred, const DeviceTensor& gt,
                             const std::optional<cad::DeviceMask>& valid_mask = std::nullopt, float min_depth = 0.1f,
                             float max_depth = 10.0f) {
        cad_eval_summary s;
        table(pred, gt, valid_mask, min_depth, max_depth, &s);
        return metricMap(s.pooled);
    }
    // computePerSample (:93-117)
    static std::vector<MetricMap> computePerSample(const DeviceTensor& pred, const DeviceTensor& gt,
                                                   const std::optional<cad::DeviceMask>& valid_mask = std::nullopt,
                                                   float min_depth = 0.1f, float max_depth = 10.0f) {
        const std::vector<float> per = table(pred, gt, valid_mask, min_depth, max_depth, nullptr);
        std::vector<MetricMap> out;
        for (size_t i = 0; i < per.size(); i += CAD_EVAL_METRICS) out.push_back(metricMap(per.data() + i));
        return out;
    }
    // average (:122-141)
    static MetricMap average(const std::vector<MetricMap>& metrics_list) {
        if (metrics_list.empty()) return getZeroMetrics();
        MetricMap avg;
        for (const auto& kv : metrics_list[0]) {
            float sum = 0.0f;
            for (const auto& m : metrics_list) sum += m.at(kv.first);
            avg[kv.first] = sum / metrics_list.size();
        }
        return avg;
    }
    static MetricMap getZeroMetrics() {   // :238-253
        const float z[CAD_EVAL_METRICS] = {0};
        return metricMap(z);
    }

private:
    static std::vector<float> table(const DeviceTensor& pred, const DeviceTensor& gt,
                                    const std::optional<cad::DeviceMask>& mask, float min_depth, float max_depth,
                                    cad_eval_summary* s) {
        if (pred.numel() != gt.numel() || pred.dim() < 3) throw std::runtime_error("DepthMetrics: pred and gt must match");
        if (mask && mask->numel() != pred.numel()) throw std::runtime_error("DepthMetrics: valid_mask must match pred");
        const int B = (int)pred.size(0);
        MetricsTable t(B, B, (int)pred.size(-2), (int)pred.size(-1), min_depth, max_depth, true, pred.device);
        t.update(pred, gt, mask ? mask->data : nullptr);
        return t.metrics(s);
    }
};

class MetricsAccumulator {   // depth_metrics.h:259-304
public:
    void update(const MetricMap& metrics) {
        for (const auto& kv : metrics) running_sum_[kv.first] += kv.second;
        count_++;
    }
    MetricMap average() const {
        MetricMap avg;
        if (count_ == 0) return avg;
        for (const auto& kv : running_sum_) avg[kv.first] = kv.second / count_;
        return avg;
    }
    void reset() {
        running_sum_.clear();
        count_ = 0;
    }
    int64_t count() const { return count_; }

private:
    MetricMap running_sum_;
    int64_t count_ = 0;
};

inline std::string formatMetrics(const MetricMap& m) {   // depth_metrics.h:309-333
    std::stringstream ss;
    ss << std::fixed << std::setprecision(4);
    ss << "Error Metrics:\n";
    ss << "  AbsRel:  " << m.at("abs_rel") << "\n";
    ss << "  RMSE:    " << m.at("rmse") << "\n";
    ss << "  RMSElog: " << m.at("rmse_log") << "\n";
    ss << "  MAE:     " << m.at("mae") << "\n";
    ss << "\nAccuracy Metrics (%):\n";
    ss << "  δ < 1.25:    " << (m.at("delta_1.25") * 100.0f) << "%\n";
    ss << "  δ < 1.25²:   " << (m.at("delta_1.25^2") * 100.0f) << "%\n";
    ss << "  δ < 1.25³:   " << (m.at("delta_1.25^3") * 100.0f) << "%\n";
    ss << "\nStatistics:\n";
    ss << "  Valid pixels: " << static_cast<int>(m.at("num_valid_pixels")) << "\n";
    ss << "  Mean pred:    " << m.at("mean_pred_depth") << "m\n";
    ss << "  Mean GT:      " << m.at("mean_gt_depth") << "m\n";
    return ss.str();
}

// the tensors of a .cadckpt file (trainer.hpp: named parameters and buffers in the reference layout; a
// trailing optimizer section is ignored) into a model with load(std::vector<NamedTensor>)
template <class Model>
inline void load_model_state(const std::string& path, Model& m) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Cannot open checkpoint: " + path);
    char magic[8];
    f.read(magic, 8);
    if (!f || std::memcmp(magic, "CADCKPT1", 8) != 0) throw std::runtime_error("not a .cadckpt file: " + path);
    int32_t n = 0;
    f.read((char*)&n, 4);
    if (!f || n < 0 || n > (1 << 20)) throw std::runtime_error("corrupt checkpoint: " + path);
    std::vector<NamedTensor> ts((size_t)n);
    for (auto& t : ts) {
        int32_t ln = 0, nd = 0;
        f.read((char*)&ln, 4);
        if (!f || ln < 0 || ln > 4096) throw std::runtime_error("corrupt checkpoint: " + path);
        t.name.resize((size_t)ln);
        f.read(&t.name[0], ln);
        f.read((char*)&nd, 4);
        if (!f || nd < 0 || nd > 8) throw std::runtime_error("corrupt checkpoint: " + path);
        t.shape.resize((size_t)nd);
        f.read((char*)t.shape.data(), 8 * nd);
        int64_t cnt = 1;
        for (auto s : t.shape) cnt *= s;
        if (!f || cnt < 0 || cnt > (int64_t(1) << 32)) throw std::runtime_error("corrupt checkpoint: " + path);
        t.value.resize((size_t)cnt);
        f.read((char*)t.value.data(), 4 * cnt);
    }
    if constexpr (std::is_base_of<BaselineUNetImpl, Model>::value) {
        if (f) {
            const std::string why = attention_checkpoint_mismatch(m, has_attention_tensors(ts), path);
            if (!why.empty()) throw std::runtime_error(why);
        }
    }
    if (!f || m.load(ts) != n) throw std::runtime_error("checkpoint does not match the model: " + path);
}

// Camera sweep (cad.h, "virtual cameras"): a labelled view, and what one view's pass over the loader gives
struct NamedView {
    std::string label;   // such as "zoom:1.5"
    cad_view view{1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.f};
};
struct ViewResult {
    std::string label;
    cad_view view{};
    std::vector<float> per_sample;   // count x 12, metricKeys() order
    MetricMap mean_metrics, std_metrics, median_metrics, min_metrics, max_metrics, pooled_metrics;
    std::vector<float> alignment;    // count x 2 (scale, shift)
    std::vector<uint8_t> aligned;    // count
    double valid_share = 0.0;        // the view's valid pixels over the main pass's
};

struct EvaluationConfig {
    float min_depth = 0.1f;
    float max_depth = 10.0f;
    bool clamp_pred = true;
    Alignment align = Alignment::None;   // per-sample scale alignment before the metrics
    int batch_size = 8;
    int device = 0;
    int64_t max_samples = -1;   // -1: the whole loader
    // stratified evaluation (cad.h): cuts in metres / in degrees off the optical axis (empty: axis off), and
    // whether the result carries each sample's sensor
    std::vector<float> depth_cuts, angle_cuts_deg;
    bool by_sensor = false;
    bool geometry = false;   // surface-normal and 3-D point metrics from each batch's K (cad.h, "geometric evaluation")
    // camera sweep: after the main pass over a batch each view is applied to it on the device, forwarded and
    // scored into a table of its own (same range, clamp and align; no strata, no geometry).
    // view_intrinsics_true == false: the model is given the sample's own K, the data is still the warped one.
    std::vector<NamedView> views;
    bool view_intrinsics_true = true;
    // called after each batch's update with (index of its first sample, predictions (n,1,H,W), n).  A
    // callback that copies to the host synchronises; without one the loop never does.
    std::function<void(int64_t, const DeviceTensor&, int)> on_batch;
};

struct EvaluationResult {
    std::vector<MetricMap> sample_results;
    std::vector<float> per_sample;   // count x 12, metricKeys() order
    Alignment align = Alignment::None;
    std::vector<float> alignment;    // count x 2 (scale, shift); (1, 0) rows without alignment
    std::vector<uint8_t> aligned;    // count; 0 where a fallback gave the row (all 0 without alignment)
    MetricMap mean_metrics, std_metrics, median_metrics, min_metrics, max_metrics, pooled_metrics;
    double forward_ms_per_image = 0.0;   // HIP events around the whole loop / samples
    int64_t num_parameters = 0;
    StrataResult depth_strata, angle_strata;   // bins == 0 unless EvaluationConfig asked for the axis
    std::vector<double> sums;                  // count x 12, filled with by_sensor or strata
    std::vector<std::string> sensors;          // one per sample, filled with by_sensor
    GeometryResult geometry;                   // on == false unless EvaluationConfig asked for it
    std::vector<ViewResult> views;             // one per EvaluationConfig::views, in its order
};

class ModelEvaluator {
public:
    // BaselineUNetImpl and the camera-conditioned U-Nets derived from it (forward(x, intrinsics) from K)
    ModelEvaluator(std::shared_ptr<BaselineUNetImpl> model, const EvaluationConfig& config) : config_(config) {
        if (!model) throw std::runtime_error("ModelEvaluator: no model");
        num_parameters_ = model->count_parameters();
        set_mode_ = [model](bool train) { model->train(train); };
        get_mode_ = [model] { return model->is_training(); };
        forward_ = [model, this](int n) {
            if (cad_unet_model(model->handle()) != CAD_MODEL_BASELINE) {
                cad::check(cad_camera_from_K(in_K_->data, n, cam_.data, nullptr), "camera_from_K");
                cad::check(cad_unet_forward_cam(model->handle(), in_rgb_->data, cam_.data, pred_.data, n, nullptr), "forward");
            } else {
                cad::check(cad_unet_forward(model->handle(), in_rgb_->data, pred_.data, n, nullptr), "forward");
            }
        };
    }
    // the geometry-aware networks: forward(rgb, rays(K), intrinsics(K)), as GeometryTrainer feeds them
    ModelEvaluator(std::shared_ptr<GeometryAwareNetworkImpl> model, const EvaluationConfig& config) : config_(config) {
        if (!model) throw std::runtime_error("ModelEvaluator: no model");
        num_parameters_ = model->count_parameters();
        set_mode_ = [model](bool train) { model->train(train); };
        get_mode_ = [model] { return model->is_training(); };
        forward_ = [model, this](int n) {
            const int H = (int)rgb_.size(2), W = (int)rgb_.size(3);
            if (rays_.numel() == 0) rays_ = DeviceTensor::empty({config_.batch_size, 3, H, W}, config_.device);
            cad::check(cad_ray_directions(in_K_->data, n, H, W, rays_.data, nullptr), "rays");
            cad::check(cad_camera_from_K(in_K_->data, n, cam_.data, nullptr), "camera_from_K");
            cad::check(cad_geonet_forward(model->handle(), in_rgb_->data, rays_.data, cam_.data, pred_.data, n, nullptr),
                       "forward");
        };
    }

    ModelEvaluator(const ModelEvaluator&) = delete;
    ModelEvaluator& operator=(const ModelEvaluator&) = delete;

    // Eval-mode forwards over the loader's samples in order, batch by batch, each batch scored on the
    // device; the model's previous train / eval mode is restored.  With EvaluationConfig::views each batch is
    // still decoded once: after the unchanged main pass over it, every view is applied to it (cad_camera_view
    // into the view buffers), forwarded and scored into that view's own table.  forward_ms_per_image then sums
    // one event pair per batch around the main pass alone.
    EvaluationResult evaluate(SunRGBDLoader& L) {
        const bool restore_training = get_mode_();
        const int B = config_.batch_size, H = L.target_height(), W = L.target_width(), d = config_.device;
        int64_t ns = (int64_t)L.size();
        if (config_.max_samples >= 0) ns = std::min(ns, config_.max_samples);
        if (ns <= 0) throw std::runtime_error("ModelEvaluator: no samples");
        rgb_ = DeviceTensor::empty({B, 3, H, W}, d);
        gt_ = DeviceTensor::empty({B, 1, H, W}, d);
        K_ = DeviceTensor::empty({B, 3, 3}, d);
        pred_ = DeviceTensor::empty({B, 1, H, W}, d);
        cam_ = DeviceTensor::empty({B, 4}, d);
        rays_ = DeviceTensor();
        MetricsTable table(ns, B, H, W, config_.min_depth, config_.max_depth, config_.clamp_pred, d, config_.align);
        const bool strata = !config_.depth_cuts.empty() || !config_.angle_cuts_deg.empty();
        if (strata) table.setStrata(config_.depth_cuts, config_.angle_cuts_deg);
        if (config_.geometry) table.setGeometry(true);
        const bool with_k = strata || config_.geometry;
        const size_t nv = config_.views.size();
        for (const NamedView& v : config_.views) cad::check(cad_view_check(&v.view), ("view " + v.label).c_str());
        std::vector<std::unique_ptr<MetricsTable>> vtables;
        std::vector<std::pair<std::shared_ptr<cad_event>, std::shared_ptr<cad_event>>> spans;
        if (nv) {
            vrgb_ = DeviceTensor::empty({B, 3, H, W}, d);
            vgt_ = DeviceTensor::empty({B, 1, H, W}, d);
            vK_ = DeviceTensor::empty({B, 3, 3}, d);
            vR_ = DeviceTensor::empty({B, 3, 3}, d);
            for (size_t v = 0; v < nv; ++v)
                vtables.push_back(std::make_unique<MetricsTable>(ns, B, H, W, config_.min_depth, config_.max_depth,
                                                                 config_.clamp_pred, d, config_.align));
            for (int64_t i = 0; i < (ns + B - 1) / B; ++i) {   // created up front: the loop allocates nothing
                cad_event *a = nullptr, *z = nullptr;
                cad::check(cad_event_create(&a), "event");
                std::shared_ptr<cad_event> ga(a, cad_event_destroy);
                cad::check(cad_event_create(&z), "event");
                spans.emplace_back(ga, std::shared_ptr<cad_event>(z, cad_event_destroy));
            }
        }
        in_rgb_ = &rgb_;
        in_K_ = &K_;
        cad_loader* ring = L.ring(B, d, false);
        cad::check(cad_loader_start_epoch(ring, nullptr, ns), "evaluation");
        cad_event *t0 = nullptr, *t1 = nullptr;
        cad::check(cad_event_create(&t0), "event");
        cad::check(cad_event_create(&t1), "event");
        std::shared_ptr<cad_event> g0(t0, cad_event_destroy), g1(t1, cad_event_destroy);
        set_mode_(false);
        EvaluationResult r;
        try {
            cad::check(cad_event_record(t0, nullptr), "event");
            size_t batch = 0;   // after the loop: the number of batches
            for (int64_t first = 0;; ++batch) {
                const int n = cad_loader_next(ring, rgb_.data, gt_.data, K_.data, nullptr);
                if (n < 0) throw std::runtime_error(std::string("data loader: ") + cad_last_error());
                if (n == 0) break;   // the loader's end of epoch: the loop's only host-visible event
                for (DeviceTensor* t : {&rgb_, &gt_, &K_, &pred_, &cam_}) t->shape[0] = n;
                if (nv) {
                    if (batch >= spans.size()) throw std::runtime_error("ModelEvaluator: the loader gave more batches than planned");
                    cad::check(cad_event_record(spans[batch].first.get(), nullptr), "event");
                }
                forward_(n);
                if (with_k) table.update(pred_, gt_, nullptr, K_);
                else table.update(pred_, gt_);
                if (nv) cad::check(cad_event_record(spans[batch].second.get(), nullptr), "event");
                if (config_.on_batch) config_.on_batch(first, pred_, n);
                for (size_t v = 0; v < nv; ++v) {
                    for (DeviceTensor* t : {&vrgb_, &vgt_, &vK_, &vR_}) t->shape[0] = n;
                    cad::check(cad_view_resolve(&config_.views[v].view, K_.data, n, H, W, vK_.data, vR_.data, nullptr), "cad_view_resolve");
                    cad::check(cad_camera_view(rgb_.data, gt_.data, nullptr, K_.data, vK_.data, vR_.data, n, H, W, vrgb_.data,
                                               vgt_.data, nullptr, nullptr),
                               "cad_camera_view");
                    in_rgb_ = &vrgb_;
                    in_K_ = config_.view_intrinsics_true ? &vK_ : &K_;
                    forward_(n);
                    in_rgb_ = &rgb_;
                    in_K_ = &K_;
                    vtables[v]->update(pred_, vgt_);
                }
                first += n;
            }
            cad::check(cad_event_record(t1, nullptr), "event");
            const size_t batch_count = batch;
            cad_eval_summary s;
            r.per_sample = table.metrics(&s);
            r.align = config_.align;
            r.alignment = table.alignment(&r.aligned);
            if (strata) {
                r.depth_strata = table.strata(StrataAxis::Depth, config_.min_depth, config_.max_depth);
                r.angle_strata = table.strata(StrataAxis::Angle, 0.f, 90.f);
            }
            if (strata || config_.by_sensor) r.sums = table.sums();
            if (config_.geometry) r.geometry = table.geometry();
            if (config_.by_sensor)
                for (int64_t i = 0; i < table.count(); ++i) r.sensors.push_back(L.sensor(i));
            float ms = 0.f;
            if (nv) {
                for (size_t i = 0; i < batch_count; ++i) {
                    float part = 0.f;
                    cad::check(cad_event_elapsed_ms(spans[i].first.get(), spans[i].second.get(), &part), "event");
                    ms += part;
                }
            } else {
                cad::check(cad_event_elapsed_ms(t0, t1, &ms), "event");
            }
            if (nv) {
                double main_valid = 0.0;
                const std::vector<double> ms_sums = table.sums();
                for (size_t i = 0; i < ms_sums.size(); i += CAD_EVAL_METRICS) main_valid += ms_sums[i];
                for (size_t v = 0; v < nv; ++v) {
                    ViewResult vr;
                    vr.label = config_.views[v].label;
                    vr.view = config_.views[v].view;
                    cad_eval_summary vs;
                    vr.per_sample = vtables[v]->metrics(&vs);
                    vr.alignment = vtables[v]->alignment(&vr.aligned);
                    vr.mean_metrics = metricMap(vs.mean);
                    vr.std_metrics = metricMap(vs.std);
                    vr.median_metrics = metricMap(vs.median);
                    vr.min_metrics = metricMap(vs.min);
                    vr.max_metrics = metricMap(vs.max);
                    vr.pooled_metrics = metricMap(vs.pooled);
                    double valid = 0.0;
                    const std::vector<double> vsums = vtables[v]->sums();
                    for (size_t i = 0; i < vsums.size(); i += CAD_EVAL_METRICS) valid += vsums[i];
                    vr.valid_share = main_valid > 0 ? valid / main_valid : 0.0;
                    r.views.push_back(std::move(vr));
                }
            }
            r.forward_ms_per_image = (double)ms / (double)std::max<int64_t>(1, table.count());
            for (size_t i = 0; i < r.per_sample.size(); i += CAD_EVAL_METRICS)
                r.sample_results.push_back(metricMap(r.per_sample.data() + i));
            r.mean_metrics = metricMap(s.mean);
            r.std_metrics = metricMap(s.std);
            r.median_metrics = metricMap(s.median);
            r.min_metrics = metricMap(s.min);
            r.max_metrics = metricMap(s.max);
            r.pooled_metrics = metricMap(s.pooled);
            r.num_parameters = num_parameters_;
        } catch (...) {
            set_mode_(restore_training);
            throw;
        }
        set_mode_(restore_training);
        return r;
    }

private:
    EvaluationConfig config_;
    int64_t num_parameters_ = 0;
    std::function<void(bool)> set_mode_;
    std::function<bool()> get_mode_;
    std::function<void(int)> forward_;
    DeviceTensor rgb_, gt_, K_, pred_, cam_, rays_;
    DeviceTensor vrgb_, vgt_, vK_, vR_;                    // one view of the current batch
    const DeviceTensor *in_rgb_ = &rgb_, *in_K_ = &K_;     // what forward_ reads: the batch, or a view of it
};

}  // namespace camera_aware_depth

#endif  // CAD_EVALUATOR_HPP
