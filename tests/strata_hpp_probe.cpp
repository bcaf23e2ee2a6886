// Compile-and-link probe of the stratified-evaluation surface of include/cad/evaluator.hpp (never run on a
// device by the CPU tests: with an argument it only exercises the host-only entry points).
#include <cstdio>

#include "cad/evaluator.hpp"

using namespace camera_aware_depth;

int main(int argc, char** argv) {
    if (argc > 1) {   // host only: the struct conversion and the angle thresholds
        const cad_strata_config c = strataConfig({1.f, 2.f, 3.f, 5.f}, {10.f, 20.f, 30.f});
        float t[3];
        if (cad_strata_angle_thresholds(c.angle_cuts_deg, c.n_angle_cuts, t) != CAD_OK) return 1;
        std::printf("%d %d %.9g %.9g %.9g\n", c.n_depth_cuts, c.n_angle_cuts, t[0], t[1], t[2]);
        try {
            strataConfig(std::vector<float>(16, 1.f), {});
        } catch (const std::exception& e) {
            std::printf("%s\n", e.what());
            return 0;
        }
        return 1;
    }
    MetricsTable table(4, 2, 16, 16);
    table.setStrata({1.f, 2.f, 3.f, 5.f}, {10.f, 20.f, 30.f});
    DeviceTensor pred = DeviceTensor::empty({2, 1, 16, 16}, 0), gt = DeviceTensor::empty({2, 1, 16, 16}, 0);
    DeviceTensor K = DeviceTensor::empty({2, 3, 3}, 0);
    table.update(pred, gt, nullptr, K);
    const StrataResult d = table.strata(StrataAxis::Depth, 0.1f, 10.f), a = table.strata(StrataAxis::Angle, 0.f, 90.f);
    EvaluationConfig ec;
    ec.depth_cuts = {1.f};
    ec.by_sensor = true;
    EvaluationResult r;
    std::printf("%d %d %d %zu %zu\n", d.bins, a.bins, table.strataBins(StrataAxis::Depth), r.sensors.size(), ec.depth_cuts.size());
    return 0;
}
