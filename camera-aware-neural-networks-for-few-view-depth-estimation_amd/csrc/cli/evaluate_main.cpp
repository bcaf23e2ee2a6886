// build/evaluate — offline evaluation of a trained checkpoint, after the reference's evaluate target
// (src/evaluation/evaluate_main.cpp:283-297 flags, :214-278 report), which does not build there; on
// libcad_hip.so through include/cad/evaluator.hpp (ModelEvaluator over the device-resident metrics table).
//
//   build/evaluate -c <final_model.pt | .cadckpt> -g <train_config.yaml> [-o results/eval] [--data-dir D]
//                  [--split val|train] [--save-predictions] [--gpu 0] [--dry-run]
//                  [--align none|median|log_mean|scale_shift]
//                  [--depth-bins 1,2,3,5] [--angle-bins 10,20,30] [--by-sensor] [--geometry]
//                  [--camera-sweep zoom:0.7,1.5]... [--view-intrinsics true|source]
//   build/evaluate --compare A/per_sample.csv B/per_sample.csv [--metric abs_rel] [--seed 42]
//   build/evaluate --compare A/per_sample_strata.csv B/per_sample_strata.csv --stratum depth:2 [--metric abs_rel]
//   build/evaluate --compare A/per_sample_camera.csv B/per_sample_camera.csv --view zoom:1.5 [--metric abs_rel]
//
// The model (model.architecture, init_features, max_depth, variant, use_pcl, use_attention), the data
// section and training.batch_size come from the training YAML, the keys build/train reads; the synthetic
// dataset works as it does for training (val: num_val_samples generated with seed + 1, the trainer's
// validation split; train: num_train_samples with the seed).  On the manifest, val takes the first
// min(500, size) samples like validateEpoch and train all of them, both without augmentation.
// Writes summary.csv, per_sample.csv, report.txt (the reference's report without its timing block, whose
// per-image numbers need host timing around each forward) and, with --save-predictions, pred_<index>.npy
// (fp32, H x W).  --align scores scale * pred + shift with a per-sample scale (median ratio, log mean or
// least squares, computed on the device; cad.h "scale-aligned evaluation"): per_sample.csv then gains the
// trailing columns scale, shift, aligned (0 where a fallback applied) and report.txt names the mode;
// pred_<index>.npy stays the raw prediction, and with none every file is as without the flag.
// --depth-bins / --angle-bins (cuts in metres / in degrees off the optical axis; cad.h "stratified
// evaluation") add strata_depth.csv / strata_angle.csv (one row per bin: stratum, lo, hi, num_samples = the
// samples with a valid pixel in the bin, pixel_share, then summary.csv's metric columns), per_sample_strata.csv
// (long form: index, axis, bin, the twelve metrics; rows without a valid pixel are left out) and a report
// section per axis; --by-sensor adds strata_sensor.csv (the per-sample rows grouped by the manifest's
// sensor_type) and a trailing sensor column in per_sample.csv.  Without these options every file is as before.
// --geometry (cad.h "geometric evaluation") adds summary_geometry.csv (one row per statistic over the nine
// geometry columns), per_sample_geometry.csv (index, the nine metrics; --compare reads it like per_sample.csv)
// and a "Geometric metrics" report section: the surface-normal angular error and the 3-D point error of the
// aligned, clamped prediction, from each sample's K.  The strata files are unaffected by it.
// --camera-sweep AXIS:v1,v2,... (repeatable; axes zoom, zoom_x, zoom_y, shift_x, shift_y, yaw, pitch, roll; cad.h
// "virtual cameras") scores the model under virtual cameras: each value is one view with every other field
// neutral, applied on the device to every batch after its unchanged main pass, forwarded and scored into a table
// of its own.  It adds camera_sweep.csv (one row per view: axis, value, num_samples, valid_share = the view's
// valid pixels over the main pass's, then summary.csv's metric columns), per_sample_camera.csv (long form: axis,
// value, index, the twelve metrics, scale, shift, aligned) and a "Camera Sweep" report section appended after
// the report's closing rule; every other file keeps its bytes.  --view-intrinsics source gives the model the
// sample's own K while the data is the warped one.  Strata and geometry are not computed per view.  --compare
// with --view axis:value pairs the samples of that view in two per_sample_camera.csv files.
// --compare with --stratum axis:bin pairs the samples present in that stratum in both long-form files.  Any
// exception prints "Error: <what>" and exits 1, like build/train.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/cad/cad.hpp"
#include "../../../include/cad/eval_stats.hpp"
#include "../../../include/cad/evaluator.hpp"
#include "../host/yaml_lite.hpp"
#include "cli_common.hpp"

namespace fs = std::filesystem;
using namespace camera_aware_depth;
using namespace cad_cli;

namespace {

std::string cut_str(float v) {
    std::ostringstream o;
    o << std::setprecision(7) << v;   // the shortest form that tells two fp32 cuts apart in practice (0.1, not 0.100000001)
    return o.str();
}

struct Args {
    std::string checkpoint, config, output = "results/eval", data_dir, split = "val", metric = "abs_rel";
    Alignment align = Alignment::None;
    std::vector<std::string> compare;
    int gpu = 0;
    uint32_t seed = 42;
    bool save_predictions = false, dry_run = false, by_sensor = false, geometry = false;
    bool fused_forward = false;                  // --fused-forward
    std::vector<float> depth_bins, angle_bins;   // cuts; empty: the option was not given
    std::string stratum;                         // --compare: "depth:2"
    std::vector<NamedView> views;                // --camera-sweep, in command-line order
    bool view_intrinsics_true = true;            // --view-intrinsics
    std::string view;                            // --compare: "zoom:1.5"
};

void usage() {
    std::cout << "evaluate - Evaluate a trained depth estimation model (MI355X)\n"
                 "  -c, --checkpoint arg  Path to model checkpoint (.pt torch::save archive or .cadckpt)\n"
                 "  -g, --config arg      Path to the training config YAML\n"
                 "  -o, --output arg      Output directory for results (default: results/eval)\n"
                 "      --data-dir arg    Data directory (overrides the config)\n"
                 "      --split arg       val or train (default: val)\n"
                 "      --save-predictions  Save every depth prediction as pred_<index>.npy\n"
                 "      --gpu arg         GPU ID (default: 0)\n"
                 "      --dry-run         Print the evaluation plan and exit; no GPU use\n"
                 "      --align arg       Per-sample scale alignment before the metrics: none, median,\n"
                 "                        log_mean or scale_shift (default: none)\n"
                 "      --depth-bins arg  Ascending depth cuts in metres, e.g. 1,2,3,5: metrics per depth range\n"
                 "      --angle-bins arg  Ascending cuts in degrees off the optical axis, e.g. 10,20,30\n"
                 "      --by-sensor       Metrics per manifest sensor_type\n"
                 "      --geometry        Surface-normal angular error and 3-D point error from each sample's K\n"
                 "                        (over the whole image: per-stratum geometry is not computed)\n"
                 "      --camera-sweep arg  AXIS:v1,v2,...: score the model under virtual cameras, one per value; axes\n"
                 "                        zoom, zoom_x, zoom_y, shift_x, shift_y (image widths / heights), yaw, pitch,\n"
                 "                        roll (degrees).  May be repeated\n"
                 "      --view-intrinsics arg  true: the model is given each view's K' (default); source: the\n"
                 "                        sample's own K\n"
                 "      --fused-forward   Fused eval forward: BatchNorm, ReLU and FiLM in the convolutions' epilogues\n"
                 "                        (the U-Net families; the same metrics, fewer passes over memory)\n"
                 "      --compare A B     Paired comparison of two per_sample.csv files (no GPU use)\n"
                 "      --stratum arg     With --compare on two per_sample_strata.csv files: axis:bin, e.g. depth:2\n"
                 "      --view arg        With --compare on two per_sample_camera.csv files: axis:value, e.g. zoom:1.5\n"
                 "      --metric arg      Column compared by --compare (default: abs_rel)\n"
                 "      --seed arg        Bootstrap seed of --compare (default: 42)\n"
                 "  -h, --help            Print help\n";
}

// "1,2,3,5" -> cuts: at least one and at most 15 finite numbers, strictly ascending (the range is checked
// once the config is read)
std::vector<float> parse_cuts(const std::string& opt, const std::string& list) {
    std::vector<float> out;
    std::string cell;
    std::stringstream ls(list);
    while (std::getline(ls, cell, ',')) {
        size_t used = 0;
        float v = 0.f;
        try {
            v = std::stof(cell, &used);
        } catch (const std::exception&) {
            used = 0;
        }
        if (cell.empty() || used != cell.size() || !std::isfinite(v))
            throw std::runtime_error(opt + " '" + list + "': '" + cell + "' is not a number");
        if (!out.empty() && !(out.back() < v))
            throw std::runtime_error(opt + " '" + list + "': the cuts must be strictly ascending (" + cell + " follows " +
                                     cut_str(out.back()) + ")");
        out.push_back(v);
    }
    if (out.empty() || (!list.empty() && list.back() == ',')) throw std::runtime_error(opt + " '" + list + "': expected a list of cuts such as 1,2,3");
    if (out.size() > (size_t)CAD_STRATA_MAX_BINS - 1)
        throw std::runtime_error(opt + " '" + list + "': " + std::to_string(out.size()) + " cuts, at most " +
                                 std::to_string(CAD_STRATA_MAX_BINS - 1));
    return out;
}
void check_cut_range(const std::string& opt, const std::vector<float>& cuts, float lo, float hi, const char* unit) {
    for (float v : cuts)
        if (!(v > lo && v < hi))
            throw std::runtime_error(opt + ": cut " + cut_str(v) + " is not strictly inside (" + cut_str(lo) + ", " + cut_str(hi) +
                                     ") " + unit);
}

// "zoom:0.7,1.5" -> one view per value, every other field neutral; refused values fail here, on the host
const char* const kSweepAxes[] = {"zoom", "zoom_x", "zoom_y", "shift_x", "shift_y", "yaw", "pitch", "roll"};
void parse_sweep(const std::string& opt, const std::string& spec, std::vector<NamedView>* views) {
    const auto colon = spec.find(':');
    const std::string axis = spec.substr(0, colon);
    int ax = -1;
    for (int i = 0; i < 8; ++i)
        if (axis == kSweepAxes[i]) ax = i;
    if (colon == std::string::npos || ax < 0)
        throw std::runtime_error(opt + " '" + spec + "': expected AXIS:v1,v2,... with AXIS one of zoom, zoom_x, zoom_y, shift_x, "
                                 "shift_y, yaw, pitch, roll" + (colon == std::string::npos ? "" : " (not '" + axis + "')"));
    const std::string list = spec.substr(colon + 1);
    std::string cell;
    size_t count = 0;
    for (std::stringstream ls(list); std::getline(ls, cell, ','); ++count) {
        size_t used = 0;
        float v = 0.f;
        try {
            v = std::stof(cell, &used);
        } catch (const std::exception&) {
            used = 0;
        }
        if (cell.empty() || used != cell.size()) throw std::runtime_error(opt + " '" + spec + "': '" + cell + "' is not a number");
        NamedView nv;
        float* const field[8] = {nullptr,           &nv.view.zoom_x,  &nv.view.zoom_y,    &nv.view.shift_x,
                                 &nv.view.shift_y,  &nv.view.yaw_deg, &nv.view.pitch_deg, &nv.view.roll_deg};
        if (ax == 0) nv.view.zoom_x = nv.view.zoom_y = v;
        else *field[ax] = v;
        nv.label = axis + ":" + cut_str(v);
        if (cad_view_check(&nv.view) != CAD_OK) throw std::runtime_error(opt + " '" + spec + "': " + cad_last_error());
        for (const NamedView& o : *views)
            if (o.label == nv.label) throw std::runtime_error(opt + " '" + spec + "': the view " + nv.label + " is given twice");
        views->push_back(nv);
    }
    if (count == 0 || list.back() == ',') throw std::runtime_error(opt + " '" + spec + "': expected a list of values such as " + axis + ":0.7,1.5");
}

Args parse_args(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i], v;
        auto eq = k.find('=');
        const bool has_eq = k.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_eq) { v = k.substr(eq + 1); k = k.substr(0, eq); }
        auto next = [&]() -> std::string {
            if (!v.empty() || (has_eq && (k == "--depth-bins" || k == "--angle-bins" || k == "--camera-sweep"))) return v;
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + k);
            return argv[++i];
        };
        if (k == "-h" || k == "--help") { usage(); std::exit(0); }
        else if (k == "-c" || k == "--checkpoint") a.checkpoint = next();
        else if (k == "-g" || k == "--config") a.config = next();
        else if (k == "-o" || k == "--output") a.output = next();
        else if (k == "--data-dir") a.data_dir = next();
        else if (k == "--split") a.split = next();
        else if (k == "--save-predictions") a.save_predictions = true;
        else if (k == "--gpu") a.gpu = std::stoi(next());
        else if (k == "--dry-run") a.dry_run = true;
        else if (k == "--align") {
            const std::string m = next();
            if (!parseAlignment(m, &a.align))
                throw std::runtime_error("--align '" + m + "': expected none, median, log_mean or scale_shift");
        } else if (k == "--depth-bins") a.depth_bins = parse_cuts(k, next());
        else if (k == "--angle-bins") a.angle_bins = parse_cuts(k, next());
        else if (k == "--by-sensor") a.by_sensor = true;
        else if (k == "--geometry") a.geometry = true;
        else if (k == "--fused-forward") a.fused_forward = true;
        else if (k == "--camera-sweep") parse_sweep(k, next(), &a.views);
        else if (k == "--view-intrinsics") {
            const std::string m = next();
            if (m != "true" && m != "source") throw std::runtime_error("--view-intrinsics '" + m + "': expected true or source");
            a.view_intrinsics_true = m == "true";
        } else if (k == "--view") a.view = next();
        else if (k == "--stratum") a.stratum = next();
        else if (k == "--metric") a.metric = next();
        else if (k == "--seed") a.seed = (uint32_t)std::stoul(next());
        else if (k == "--compare") {
            a.compare.push_back(next());
            if (i + 1 >= argc) throw std::runtime_error("--compare takes two per_sample.csv files");
            a.compare.push_back(argv[++i]);
        } else throw std::runtime_error("unknown option " + k);
    }
    return a;
}

// ---- --compare: two per_sample.csv files, paired by their index column ----
struct Column {
    std::vector<long long> index;
    std::vector<double> value;
};
Column read_column(const std::string& path, const std::string& metric) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("Cannot open " + path);
    std::string line, cell;
    if (!std::getline(f, line)) throw std::runtime_error(path + " is empty");
    int col = -1, n = 0;
    std::string names;
    for (std::stringstream hs(line); std::getline(hs, cell, ','); ++n) {
        if (n == 0 && cell != "index") throw std::runtime_error(path + ": the first column must be index");
        if (cell == metric) col = n;
        if (n >= 1) names += (n > 1 ? ", " : "") + cell;
    }
    if (col < 1) throw std::runtime_error(path + " has no column '" + metric + "' (its columns: " + names + ")");
    Column c;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::stringstream ls(line);
        for (int i = 0; std::getline(ls, cell, ','); ++i) {
            if (i == 0) c.index.push_back(std::stoll(cell));
            if (i == col) c.value.push_back(std::stod(cell));
        }
        if (c.index.size() != c.value.size()) throw std::runtime_error(path + ": short row '" + line + "'");
    }
    return c;
}

// the rows of one stratum of a per_sample_strata.csv (index, axis, bin, metrics...)
Column read_stratum_column(const std::string& path, const std::string& metric, const std::string& axis, long long bin) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("Cannot open " + path);
    std::string line, cell;
    if (!std::getline(f, line)) throw std::runtime_error(path + " is empty");
    int col = -1, n = 0;
    std::string names;
    for (std::stringstream hs(line); std::getline(hs, cell, ','); ++n) {
        static const char* head[3] = {"index", "axis", "bin"};
        if (n < 3 && cell != head[n])
            throw std::runtime_error(path + ": the first columns must be index,axis,bin (a per_sample_strata.csv file)");
        if (n >= 3 && cell == metric) col = n;
        if (n >= 3) names += (n > 3 ? ", " : "") + cell;
    }
    if (col < 3) throw std::runtime_error(path + " has no column '" + metric + "' (its columns: " + names + ")");
    Column c;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::vector<std::string> cells;
        for (std::stringstream ls(line); std::getline(ls, cell, ',');) cells.push_back(cell);
        if ((int)cells.size() <= col) throw std::runtime_error(path + ": short row '" + line + "'");
        if (cells[1] != axis || std::stoll(cells[2]) != bin) continue;
        c.index.push_back(std::stoll(cells[0]));
        c.value.push_back(std::stod(cells[(size_t)col]));
    }
    return c;
}

// the rows of one view of a per_sample_camera.csv (axis, value, index, metrics...)
Column read_view_column(const std::string& path, const std::string& metric, const std::string& axis, float value) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("Cannot open " + path);
    std::string line, cell;
    if (!std::getline(f, line)) throw std::runtime_error(path + " is empty");
    int col = -1, n = 0;
    std::string names;
    for (std::stringstream hs(line); std::getline(hs, cell, ','); ++n) {
        static const char* head[3] = {"axis", "value", "index"};
        if (n < 3 && cell != head[n])
            throw std::runtime_error(path + ": the first columns must be axis,value,index (a per_sample_camera.csv file)");
        if (n >= 3 && cell == metric) col = n;
        if (n >= 3) names += (n > 3 ? ", " : "") + cell;
    }
    if (col < 3) throw std::runtime_error(path + " has no column '" + metric + "' (its columns: " + names + ")");
    Column c;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::vector<std::string> cells;
        for (std::stringstream ls(line); std::getline(ls, cell, ',');) cells.push_back(cell);
        if ((int)cells.size() <= col) throw std::runtime_error(path + ": short row '" + line + "'");
        if (cells[0] != axis || std::stof(cells[1]) != value) continue;
        c.index.push_back(std::stoll(cells[2]));
        c.value.push_back(std::stod(cells[(size_t)col]));
    }
    return c;
}

int compare_view(const Args& a) {
    const auto colon = a.view.find(':');
    const std::string axis = a.view.substr(0, colon);
    bool known = false;
    for (const char* k : kSweepAxes) known = known || axis == k;
    float value = 0.f;
    size_t used = 0;
    if (colon != std::string::npos) {
        try {
            value = std::stof(a.view.substr(colon + 1), &used);
        } catch (const std::exception&) {
            used = 0;
        }
    }
    if (!known || colon == std::string::npos || used == 0 || used != a.view.size() - colon - 1)
        throw std::runtime_error("--view '" + a.view + "': expected axis:value such as zoom:1.5");
    const Column x = read_view_column(a.compare[0], a.metric, axis, value), y = read_view_column(a.compare[1], a.metric, axis, value);
    for (const auto* c : {&x, &y})
        if (c->index.empty())
            throw std::runtime_error("the view " + a.view + " is not in " + (c == &x ? a.compare[0] : a.compare[1]));
    if (x.index.size() != y.index.size())
        throw std::runtime_error("the files hold " + std::to_string(x.index.size()) + " and " + std::to_string(y.index.size()) +
                                 " samples of view " + a.view + ": a paired comparison needs the same samples");
    if (x.index != y.index) throw std::runtime_error("the sample indices of view " + a.view + " do not match in the two files");
    if (x.value.size() < 2) throw std::runtime_error("a paired comparison needs at least two samples in view " + a.view);
    std::cout << eval_stats::compare_models(x.value, y.value, a.compare[0], a.compare[1], a.metric + " [" + a.view + "]", a.seed);
    return 0;
}

int compare_stratum(const Args& a) {
    const auto colon = a.stratum.find(':');
    const std::string axis = a.stratum.substr(0, colon);
    long long bin = -1;
    size_t used = 0;
    if (colon != std::string::npos) {
        try {
            bin = std::stoll(a.stratum.substr(colon + 1), &used);
        } catch (const std::exception&) {
            bin = -1;
        }
    }
    if ((axis != "depth" && axis != "angle") || bin < 0 || bin >= CAD_STRATA_MAX_BINS || used != a.stratum.size() - colon - 1)
        throw std::runtime_error("--stratum '" + a.stratum + "': expected depth:<bin> or angle:<bin>");
    const Column x = read_stratum_column(a.compare[0], a.metric, axis, bin), y = read_stratum_column(a.compare[1], a.metric, axis, bin);
    std::map<long long, double> ym;
    for (size_t i = 0; i < y.index.size(); ++i) ym[y.index[i]] = y.value[i];
    std::vector<double> xv, yv;
    size_t only_x = 0;
    for (size_t i = 0; i < x.index.size(); ++i) {
        const auto it = ym.find(x.index[i]);
        if (it == ym.end()) {
            ++only_x;
            continue;
        }
        xv.push_back(x.value[i]);
        yv.push_back(it->second);
    }
    const size_t only_y = y.index.size() - xv.size();
    if (only_x + only_y > 0)
        throw std::runtime_error(std::to_string(only_x + only_y) + " samples are present in stratum " + a.stratum +
                                 " of only one file (" + std::to_string(only_x) + " only in " + a.compare[0] + ", " +
                                 std::to_string(only_y) + " only in " + a.compare[1] + "): a paired comparison needs the same samples");
    if (xv.size() < 2) throw std::runtime_error("a paired comparison needs at least two samples in stratum " + a.stratum);
    std::cout << eval_stats::compare_models(xv, yv, a.compare[0], a.compare[1], a.metric + " [" + a.stratum + "]", a.seed);
    return 0;
}

int compare(const Args& a) {
    if (!a.stratum.empty() && !a.view.empty()) throw std::runtime_error("--stratum and --view cannot be combined");
    if (!a.view.empty()) return compare_view(a);
    if (!a.stratum.empty()) return compare_stratum(a);
    const Column x = read_column(a.compare[0], a.metric), y = read_column(a.compare[1], a.metric);
    if (x.index.size() != y.index.size())
        throw std::runtime_error("the files hold " + std::to_string(x.index.size()) + " and " +
                                 std::to_string(y.index.size()) + " samples: a paired comparison needs the same samples");
    if (x.index != y.index) throw std::runtime_error("the sample indices of the two files do not match");
    if (x.value.size() < 2) throw std::runtime_error("a paired comparison needs at least two samples");
    std::cout << eval_stats::compare_models(x.value, y.value, a.compare[0], a.compare[1], a.metric, a.seed);
    return 0;
}

// ---- outputs ----
struct StratumRow {
    std::string name, lo, hi;
    cad_eval_summary s;
    double pixels = 0.0;
};

// the sensor strata: the per-sample rows grouped by sensor (first appearance order), each group finished
// like the whole table (a sample without a valid pixel counts as twelve zeros)
std::vector<StratumRow> sensor_strata(const EvaluationResult& r) {
    std::vector<std::string> names;
    for (const auto& s : r.sensors)
        if (std::find(names.begin(), names.end(), s) == names.end()) names.push_back(s);
    std::vector<StratumRow> rows;
    for (const auto& name : names) {
        std::vector<double> sums;
        StratumRow row;
        row.name = name;
        for (size_t i = 0; i < r.sensors.size(); ++i)
            if (r.sensors[i] == name) {
                sums.insert(sums.end(), r.sums.begin() + (long)(i * CAD_EVAL_METRICS), r.sums.begin() + (long)((i + 1) * CAD_EVAL_METRICS));
                row.pixels += r.sums[i * CAD_EVAL_METRICS];
            }
        cad::check(cad_eval_finish(sums.data(), (int64_t)(sums.size() / CAD_EVAL_METRICS), nullptr, &row.s), "cad_eval_finish");
        rows.push_back(row);
    }
    return rows;
}

std::vector<StratumRow> axis_strata(const StrataResult& st) {
    std::vector<StratumRow> rows;
    const size_t n = st.bins ? st.sums.size() / ((size_t)st.bins * CAD_EVAL_METRICS) : 0;
    for (int b = 0; b < st.bins; ++b) {
        StratumRow row;
        row.name = std::to_string(b);
        row.lo = cut_str(st.edges[(size_t)b]);
        row.hi = cut_str(st.edges[(size_t)b + 1]);
        row.s = st.summary[(size_t)b];
        for (size_t i = 0; i < n; ++i) row.pixels += st.sums[(i * (size_t)st.bins + (size_t)b) * CAD_EVAL_METRICS];
        rows.push_back(row);
    }
    return rows;
}

void write_strata_csv(const std::string& path, const std::vector<StratumRow>& rows, double total_pixels) {
    std::ofstream f(path);
    if (!f) throw std::runtime_error("cannot write " + path);
    f << "stratum,lo,hi,num_samples,pixel_share";
    for (const char* k : metricKeys())
        for (const char* s : {"mean", "std", "median", "pooled"}) f << "," << k << "_" << s;
    f << "\n" << std::setprecision(9);
    for (const auto& row : rows) {
        f << row.name << "," << row.lo << "," << row.hi << "," << row.s.count << ","
          << (total_pixels > 0 ? row.pixels / total_pixels : 0.0);
        for (int k = 0; k < CAD_EVAL_METRICS; ++k)
            for (const float* m : {row.s.mean, row.s.std, row.s.median, row.s.pooled}) f << "," << m[k];
        f << "\n";
    }
}

void report_strata(std::ostream& rep, const std::string& rule, const char* title, const char* unit,
                   const std::vector<StratumRow>& rows, double total_pixels) {
    rep << rule << "\n" << title << "\n" << rule << "\n\n";
    rep << std::fixed << std::setprecision(4);
    for (const auto& row : rows) {
        rep << "  " << row.name;
        if (!row.lo.empty()) rep << " [" << row.lo << ", " << row.hi << ") " << unit;
        rep << ": " << row.s.count << " samples, " << (total_pixels > 0 ? 100.0 * row.pixels / total_pixels : 0.0)
            << "% of the valid pixels\n";
        rep << "    AbsRel:   " << row.s.mean[0] << " ± " << row.s.std[0] << "\n";
        rep << "    RMSE:     " << row.s.mean[2] << " ± " << row.s.std[2] << "\n";
        rep << "    δ < 1.25: " << row.s.mean[6] << " ± " << row.s.std[6] << "\n";
    }
    rep << "\n";
}

// --geometry: summary_geometry.csv, per_sample_geometry.csv and the report section
void write_geometry(const Args& a, const GeometryResult& g, std::ostream& rep, const std::string& rule) {
    const auto& keys = geometryKeys();
    const size_t n = g.medians.size();
    {
        std::ofstream f(a.output + "/per_sample_geometry.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/per_sample_geometry.csv");
        f << "index";
        for (const char* k : keys) f << "," << k;
        f << "\n" << std::setprecision(9);
        for (size_t i = 0; i < n; ++i) {
            f << i;
            for (int k = 0; k < CAD_GEOM_METRICS; ++k) f << "," << g.per_sample[i * CAD_GEOM_METRICS + (size_t)k];
            f << "\n";
        }
    }
    const cad_geom_summary& s = g.summary;
    {
        std::ofstream f(a.output + "/summary_geometry.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/summary_geometry.csv");
        f << "statistic";
        for (const char* k : keys) f << "," << k;
        f << "\n" << std::setprecision(9);
        const std::pair<const char*, const float*> rows[] = {{"mean", s.mean}, {"std", s.std}, {"median", s.median},
                                                             {"min", s.min},   {"max", s.max}, {"pooled", s.pooled}};
        for (const auto& row : rows) {
            f << row.first;
            for (int k = 0; k < CAD_GEOM_METRICS; ++k) {
                f << ",";
                if (!std::isnan(row.second[k])) f << row.second[k];   // the pooled median is not defined: empty
            }
            f << "\n";
        }
    }
    rep << rule << "\n                     Geometric Metrics\n" << rule << "\n\n";
    rep << std::fixed << std::setprecision(4);
    rep << "Surface normals (degrees, " << s.count_normal << " of " << s.count << " samples with a normal-valid pixel):\n";
    rep << "  Mean:      " << s.mean[0] << " ± " << s.std[0] << "\n";
    rep << "  Median:    " << s.mean[1] << " ± " << s.std[1] << "\n";
    rep << "  RMSE:      " << s.mean[2] << " ± " << s.std[2] << "\n";
    rep << "  < 11.25°:  " << s.mean[3] << " ± " << s.std[3] << "\n";
    rep << "  < 22.5°:   " << s.mean[4] << " ± " << s.std[4] << "\n";
    rep << "  < 30°:     " << s.mean[5] << " ± " << s.std[5] << "\n";
    rep << "3-D points (metres, " << s.count_point << " of " << s.count << " samples with a valid pixel):\n";
    rep << "  MAE:       " << s.mean[7] << " ± " << s.std[7] << "\n";
    rep << "  RMSE:      " << s.mean[8] << " ± " << s.std[8] << "\n\n";
}

// --camera-sweep: camera_sweep.csv, per_sample_camera.csv and the report section (after the report's closing rule)
void write_camera_sweep(const Args& a, const EvaluationResult& r, std::ostream& rep, const std::string& bar, const std::string& rule) {
    const auto& keys = metricKeys();
    const auto split = [](const std::string& label) {
        const auto colon = label.find(':');
        return std::make_pair(label.substr(0, colon), label.substr(colon + 1));
    };
    {
        std::ofstream f(a.output + "/camera_sweep.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/camera_sweep.csv");
        f << "axis,value,num_samples,valid_share";
        for (const char* k : keys)
            for (const char* s : {"mean", "std", "median", "pooled"}) f << "," << k << "_" << s;
        f << "\n" << std::setprecision(9);
        for (const ViewResult& v : r.views) {
            const auto av = split(v.label);
            f << av.first << "," << av.second << "," << v.per_sample.size() / CAD_EVAL_METRICS << "," << v.valid_share;
            for (const char* k : keys)
                for (const MetricMap* m : {&v.mean_metrics, &v.std_metrics, &v.median_metrics, &v.pooled_metrics}) f << "," << m->at(k);
            f << "\n";
        }
    }
    {
        std::ofstream f(a.output + "/per_sample_camera.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/per_sample_camera.csv");
        f << "axis,value,index";
        for (const char* k : keys) f << "," << k;
        f << ",scale,shift,aligned\n" << std::setprecision(9);
        for (const ViewResult& v : r.views) {
            const auto av = split(v.label);
            for (size_t i = 0; i < v.per_sample.size() / CAD_EVAL_METRICS; ++i) {
                f << av.first << "," << av.second << "," << i;
                for (int k = 0; k < CAD_EVAL_METRICS; ++k) f << "," << v.per_sample[i * CAD_EVAL_METRICS + (size_t)k];
                f << "," << v.alignment[2 * i] << "," << v.alignment[2 * i + 1] << "," << (int)v.aligned[i] << "\n";
            }
        }
    }
    rep << rule << "\n                       Camera Sweep\n" << rule << "\n\n";
    rep << "Virtual cameras, warped on the device; the model is given "
        << (a.view_intrinsics_true ? "each view's K'" : "the sample's own K (--view-intrinsics source)") << ".\n";
    rep << "Means over the samples; valid: the view's valid pixels over the unwarped run's.\n";
    rep << std::fixed << std::setprecision(4);
    std::vector<std::string> axes;
    for (const ViewResult& v : r.views)
        if (std::find(axes.begin(), axes.end(), split(v.label).first) == axes.end()) axes.push_back(split(v.label).first);
    const auto row = [&](const std::string& name, float abs_rel, float rmse, float a1, double share) {
        rep << "  " << std::left << std::setw(12) << name << std::right << std::setw(10) << abs_rel << std::setw(10) << rmse
            << std::setw(10) << a1 << std::setw(9) << 100.0 * share << "%\n";
    };
    for (const std::string& axis : axes) {
        rep << "\n  " << std::left << std::setw(12) << axis << std::right << std::setw(10) << "AbsRel" << std::setw(10) << "RMSE"
            << std::setw(11) << "δ < 1.25" << std::setw(10) << "valid" << "\n";
        row("(unwarped)", r.mean_metrics.at("abs_rel"), r.mean_metrics.at("rmse"), r.mean_metrics.at("delta_1.25"), 1.0);
        for (const ViewResult& v : r.views)
            if (split(v.label).first == axis)
                row(split(v.label).second, v.mean_metrics.at("abs_rel"), v.mean_metrics.at("rmse"), v.mean_metrics.at("delta_1.25"),
                    v.valid_share);
    }
    rep << "\n" << bar << "\n";
}

void write_outputs(const Args& a, const Config& c, const EvaluationResult& r) {
    const auto& keys = metricKeys();
    const bool al = a.align != Alignment::None;
    {
        std::ofstream f(a.output + "/per_sample.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/per_sample.csv");
        f << "index";
        for (const char* k : keys) f << "," << k;
        if (al) f << ",scale,shift,aligned";
        if (a.by_sensor) f << ",sensor";
        f << "\n" << std::setprecision(9);
        for (size_t i = 0; i < r.sample_results.size(); ++i) {
            f << i;
            for (int k = 0; k < CAD_EVAL_METRICS; ++k) f << "," << r.per_sample[i * CAD_EVAL_METRICS + (size_t)k];
            if (al) f << "," << r.alignment[2 * i] << "," << r.alignment[2 * i + 1] << "," << (int)r.aligned[i];
            if (a.by_sensor) f << "," << r.sensors[i];
            f << "\n";
        }
    }
    {
        std::ofstream f(a.output + "/summary.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/summary.csv");
        f << "num_samples";
        for (const char* k : keys)
            for (const char* s : {"mean", "std", "median", "pooled"}) f << "," << k << "_" << s;
        f << "\n" << std::setprecision(9) << r.sample_results.size();
        for (const char* k : keys)
            for (const MetricMap* m : {&r.mean_metrics, &r.std_metrics, &r.median_metrics, &r.pooled_metrics}) f << "," << m->at(k);
        f << "\n";
    }
    std::ofstream rep(a.output + "/report.txt");
    if (!rep) throw std::runtime_error("cannot write " + a.output + "/report.txt");
    const std::time_t now = std::time(nullptr);
    const std::string bar(65, '='), rule(65, '-');
    rep << bar << "\n                  Model Evaluation Report\n" << bar << "\n\n";
    rep << "Checkpoint: " << a.checkpoint << "\n";
    rep << "Model Type: " << c.architecture << (c.architecture == "geometry_aware" ? "/" + c.variant : std::string()) << "\n";
    rep << "Parameters: " << r.num_parameters << "\n";
    rep << "Test Samples: " << r.sample_results.size() << " (" << a.split << ")\n";
    rep << "Evaluation Date: " << std::put_time(std::localtime(&now), "%Y-%m-%d %H:%M:%S") << "\n";
    if (al) {
        std::vector<double> sc;
        int64_t fallbacks = 0;
        for (size_t i = 0; i < r.aligned.size(); ++i) {
            sc.push_back((double)r.alignment[2 * i]);
            fallbacks += r.aligned[i] ? 0 : 1;
        }
        rep << "Alignment: " << alignmentName(a.align) << " (per sample; metrics score scale * pred + shift), scale "
            << std::fixed << std::setprecision(4) << eval_stats::mean(sc) << " ± " << eval_stats::stddev(sc, 0) << ", "
            << fallbacks << " fallback" << (fallbacks == 1 ? "" : "s") << "\n";
        rep.unsetf(std::ios::floatfield);
        rep << std::setprecision(6);
    }
    rep << "\n";
    rep << rule << "\n                    Performance Metrics\n" << rule << "\n\n";
    rep << std::fixed << std::setprecision(4);
    const auto pm = [&](const char* label, const char* k) {
        rep << label << r.mean_metrics.at(k) << " ± " << r.std_metrics.at(k) << "\n";
    };
    rep << "Lower is better:\n";
    pm("  AbsRel:   ", "abs_rel");
    pm("  SqRel:    ", "sq_rel");
    pm("  RMSE:     ", "rmse");
    pm("  RMSElog:  ", "rmse_log");
    pm("  MAE:      ", "mae");
    pm("  Log10:    ", "log10");
    rep << "\nHigher is better (Accuracy thresholds):\n";
    pm("  δ < 1.25:    ", "delta_1.25");
    pm("  δ < 1.25²:   ", "delta_1.25^2");
    pm("  δ < 1.25³:   ", "delta_1.25^3");
    rep << "\n" << rule << "\n                   Inference Performance\n" << rule << "\n\n";
    rep << "  Mean Time:   " << r.forward_ms_per_image << " ms per image (device time of the whole loop, batch "
        << c.batch_size << ")\n";
    rep << "  FPS:         " << (r.forward_ms_per_image > 0 ? 1000.0 / r.forward_ms_per_image : 0.0) << "\n\n";
    rep << rule << "\n                     Median Metrics\n" << rule << "\n\n";
    rep << "  AbsRel:   " << r.median_metrics.at("abs_rel") << "\n";
    rep << "  RMSE:     " << r.median_metrics.at("rmse") << "\n";
    rep << "  RMSElog:  " << r.median_metrics.at("rmse_log") << "\n";
    rep << "  δ < 1.25: " << r.median_metrics.at("delta_1.25") << "\n\n";
    rep << rule << "\n              Pooled Over All Valid Pixels\n" << rule << "\n\n";
    rep << formatMetrics(r.pooled_metrics) << "\n";
    double total_pixels = 0.0;
    for (size_t i = 0; i < r.sums.size(); i += CAD_EVAL_METRICS) total_pixels += r.sums[i];
    if (r.depth_strata.bins) {
        const auto rows = axis_strata(r.depth_strata);
        write_strata_csv(a.output + "/strata_depth.csv", rows, total_pixels);
        report_strata(rep, rule, "                  Metrics By Depth Range", "m", rows, total_pixels);
    }
    if (r.angle_strata.bins) {
        const auto rows = axis_strata(r.angle_strata);
        write_strata_csv(a.output + "/strata_angle.csv", rows, total_pixels);
        report_strata(rep, rule, "           Metrics By Ray Angle Off The Optical Axis", "degrees", rows, total_pixels);
    }
    if (a.by_sensor) {
        const auto rows = sensor_strata(r);
        write_strata_csv(a.output + "/strata_sensor.csv", rows, total_pixels);
        report_strata(rep, rule, "                     Metrics By Sensor", "", rows, total_pixels);
    }
    if (r.depth_strata.bins || r.angle_strata.bins) {
        std::ofstream f(a.output + "/per_sample_strata.csv");
        if (!f) throw std::runtime_error("cannot write " + a.output + "/per_sample_strata.csv");
        f << "index,axis,bin";
        for (const char* k : keys) f << "," << k;
        f << "\n" << std::setprecision(9);
        for (size_t i = 0; i < r.sample_results.size(); ++i)
            for (const auto* st : {&r.depth_strata, &r.angle_strata})
                for (int b = 0; b < st->bins; ++b) {
                    const size_t at = (i * (size_t)st->bins + (size_t)b) * CAD_EVAL_METRICS;
                    if (!(st->sums[at] > 0)) continue;
                    f << i << "," << (st == &r.depth_strata ? "depth" : "angle") << "," << b;
                    for (int k = 0; k < CAD_EVAL_METRICS; ++k) f << "," << st->per_sample[at + (size_t)k];
                    f << "\n";
                }
    }
    if (r.geometry.on) write_geometry(a, r.geometry, rep, rule);
    rep << bar << "\n";
    if (!r.views.empty()) write_camera_sweep(a, r, rep, bar, rule);
}

int run(const Args& a) {
    if (!a.compare.empty()) return compare(a);
    if (a.checkpoint.empty() || a.config.empty()) throw std::runtime_error("--checkpoint and --config are required");
    if (a.split != "val" && a.split != "train") throw std::runtime_error("--split '" + a.split + "': expected val or train");
    if (!fs::exists(a.checkpoint)) throw std::runtime_error("Cannot open checkpoint: " + a.checkpoint);
    const bool pt = ends_with(a.checkpoint, ".pt");
    if (!pt && !ends_with(a.checkpoint, ".cadckpt"))
        throw std::runtime_error("checkpoint '" + a.checkpoint + "': expected a .pt or .cadckpt file");
    Config c = load_config(yaml_lite::load_file(a.config));
    if (!a.data_dir.empty()) c.data_dir = a.data_dir;
    check_cut_range("--depth-bins", a.depth_bins, EvaluationConfig().min_depth, c.max_depth, "metres");
    check_cut_range("--angle-bins", a.angle_bins, 0.f, 90.f, "degrees");
    const bool geo = c.architecture == "geometry_aware";
    if (geo && pt) throw std::runtime_error("geometry_aware checkpoints are .cadckpt files");
    if (geo && a.fused_forward)
        throw std::runtime_error("--fused-forward: model.architecture 'geometry_aware' has no fused eval forward (the "
                                 "U-Net families baseline_unet, intrinsics_unet, intrinsics_attention_unet, ray_film_unet do)");
    const bool real = c.dataset != "synthetic";
    int64_t ns = a.split == "val" ? c.n_val : c.n_train;
    if (real) {   // the sample count, read on the host before any GPU call
        std::vector<const char*> sens;
        for (const auto& x : c.sensor_types) sens.push_back(x.c_str());
        cad_dataset* d = nullptr;
        cad::check(cad_dataset_open(c.manifest_path.c_str(), sens.empty() ? nullptr : sens.data(), (int)sens.size(), &d),
                   "SunRGBDLoader");
        ns = cad_dataset_size(d);
        cad_dataset_destroy(d);
        if (a.split == "val") ns = std::min<int64_t>(500, ns);
    }
    if (ns <= 0) throw std::runtime_error("no samples to evaluate in the " + a.split + " split");
    if (a.dry_run) {
        std::cout << "{\"checkpoint\": \"" << a.checkpoint << "\", \"format\": \"" << (pt ? "torch" : "cadckpt")
                  << "\", \"architecture\": \"" << c.architecture << "\", \"init_features\": " << c.init_features
                  << ", \"max_depth\": " << c.max_depth << ", \"dataset\": \"" << (real ? c.manifest_path : "synthetic")
                  << "\", \"split\": \"" << a.split << "\", \"samples\": " << ns << ", \"batch_size\": " << c.batch_size
                  << ", \"batches\": " << (ns + c.batch_size - 1) / c.batch_size << ", \"height\": " << c.height
                  << ", \"width\": " << c.width << ", \"device\": " << a.gpu << ", \"output\": \"" << a.output
                  << "\", \"save_predictions\": " << (a.save_predictions ? "true" : "false") << ", \"align\": \""
                  << alignmentName(a.align) << "\"";
        const auto list = [](const char* key, const std::vector<float>& v) {
            if (v.empty()) return;
            std::cout << ", \"" << key << "\": [";
            for (size_t j = 0; j < v.size(); ++j) std::cout << (j ? ", " : "") << cut_str(v[j]);
            std::cout << "]";
        };
        list("depth_bins", a.depth_bins);
        list("angle_bins", a.angle_bins);
        if (a.by_sensor) std::cout << ", \"by_sensor\": true";
        if (a.geometry) std::cout << ", \"geometry\": true";
        // (how many convolutions fuse is the handle's to say: cad_unet_fused_eval_convs after a forward)
        std::cout << ", \"forward\": \"" << (a.fused_forward ? "fused" : "two-pass") << "\"";
        if (!a.views.empty()) {
            std::cout << ", \"camera_sweep\": [";
            for (size_t j = 0; j < a.views.size(); ++j) std::cout << (j ? ", " : "") << "\"" << a.views[j].label << "\"";
            std::cout << "], \"view_intrinsics\": \"" << (a.view_intrinsics_true ? "true" : "source") << "\"";
        }
        std::cout << "}" << std::endl;
        return 0;
    }
    int ndev = 0;
    cad::check(cad_device_count(&ndev), "device query");
    if (a.gpu < 0 || a.gpu >= ndev) throw std::runtime_error("GPU " + std::to_string(a.gpu) + " not available");
    cad::check(cad_set_device(a.gpu), "set device");
    fs::create_directories(a.output);

    std::shared_ptr<SunRGBDLoader> loader;
    if (real) {
        loader = std::make_shared<SunRGBDLoader>(c.data_dir, c.manifest_path, a.split == "val" ? "test" : "train");
        if (!c.sensor_types.empty()) loader->filterBySensorType(c.sensor_types);
    } else {
        loader = SunRGBDLoader::synthetic(ns, c.height, c.width, (uint32_t)c.seed + (a.split == "val" ? 1u : 0u));
    }
    loader->setTargetDimensions(c.height, c.width);

    EvaluationConfig ec;
    ec.max_depth = c.max_depth;
    ec.batch_size = c.batch_size;
    ec.device = a.gpu;
    ec.max_samples = ns;
    ec.align = a.align;
    ec.depth_cuts = a.depth_bins;
    ec.angle_cuts_deg = a.angle_bins;
    ec.by_sensor = a.by_sensor;
    ec.geometry = a.geometry;
    ec.views = a.views;
    ec.view_intrinsics_true = a.view_intrinsics_true;
    if (a.save_predictions)
        ec.on_batch = [&](int64_t first, const DeviceTensor& pred, int n) {
            const std::vector<float> h = pred.to_host();
            const int64_t hw = (int64_t)c.height * c.width;
            for (int i = 0; i < n; ++i)
                write_npy(a.output + "/pred_" + std::to_string(first + i) + ".npy", h.data() + i * hw, c.height, c.width);
        };
    const cad::Workspace ws{c.batch_size, c.height, c.width, a.gpu};
    std::unique_ptr<ModelEvaluator> ev;
    std::shared_ptr<BaselineUNetImpl> unet;   // the U-Net families: the fused eval forward's switch and count
    if (geo) {
        std::shared_ptr<GeometryAwareNetworkImpl> m;
        if (c.variant == "lightweight") m = std::make_shared<LightweightGeometryNetworkImpl>(3, c.init_features, 4, c.max_depth, ws);
        else m = std::make_shared<GeometryAwareNetworkImpl>(3, c.init_features, 4, c.max_depth, c.use_pcl, c.use_attention, ws);
        load_model_state(a.checkpoint, *m);
        ev = std::make_unique<ModelEvaluator>(m, ec);
    } else {
        std::shared_ptr<BaselineUNetImpl> m;
        if (c.architecture == "intrinsics_unet") m = std::make_shared<IntrinsicsConditionedUNetImpl>(3, c.init_features, 4, c.max_depth, ws);
        else if (c.architecture == "intrinsics_attention_unet") m = std::make_shared<IntrinsicsAttentionUNetImpl>(3, c.init_features, 4, c.max_depth, ws);
        else if (c.architecture == "ray_film_unet") m = std::make_shared<RayConditionedUNetImpl>(3, c.init_features, 4, c.max_depth, ws);
        else m = std::make_shared<BaselineUNetImpl>(3, c.init_features, c.max_depth, ws);
        if (pt) load(*m, a.checkpoint);
        else load_model_state(a.checkpoint, *m);
        m->fused_eval(a.fused_forward);
        unet = m;
        ev = std::make_unique<ModelEvaluator>(m, ec);
    }
    std::cout << "Evaluating " << a.checkpoint << " (" << c.architecture << ", f=" << c.init_features << ") on " << ns << " "
              << a.split << " samples" << (real ? " of " + c.manifest_path : std::string(" (synthetic)")) << ", batch "
              << c.batch_size << ", MI355X device " << a.gpu
              << (a.align != Alignment::None ? std::string(", alignment ") + alignmentName(a.align) : std::string()) << "\n";
    const EvaluationResult r = ev->evaluate(*loader);
    write_outputs(a, c, r);
    if (unet) {
        int nf = 0, nt = 0;
        unet->fused_eval_convs(&nf, &nt);
        std::cout << "Forward mode: " << (a.fused_forward ? "fused eval forward" : "two-pass eval forward") << ", fused " << nf
                  << " of " << nt << " convolutions\n";
    }
    std::cout << "\nMean over " << r.sample_results.size() << " samples:\n" << formatMetrics(r.mean_metrics) << "\nForward: "
              << std::fixed << std::setprecision(3) << r.forward_ms_per_image << " ms per image, " << r.num_parameters
              << " parameters\nResults saved to: " << a.output << "\n";
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
