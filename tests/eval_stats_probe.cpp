// Prints include/cad/eval_stats.hpp's results for one pair of vectors (tests/test_eval_cpu.py).
//   eval_stats_probe <file: N, then N values of a, then N values of b> <seed>
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "cad/eval_stats.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream f(argv[1]);
    size_t n = 0;
    f >> n;
    std::vector<double> a(n), b(n);
    for (auto& x : a) f >> x;
    for (auto& x : b) f >> x;
    if (!f) return 3;
    namespace es = camera_aware_depth::eval_stats;
    const es::TTest t = es::paired_t_test(a, b);
    const es::Wilcoxon w = es::wilcoxon_signed_rank(a, b);
    const auto ci = es::bootstrap_ci(a, b, (uint32_t)std::strtoul(argv[2], nullptr, 10));
    std::printf("t %.17g\ndf %.17g\nt_p %.17g\nmean_diff %.17g\nW %.17g\nw_p %.17g\nn_nonzero %lld\ncohens_d %.17g\n"
                "ci_lo %.17g\nci_hi %.17g\n",
                t.t, t.df, t.p, t.mean_diff, w.w, w.p, (long long)w.n, es::cohens_d(a, b), ci.first, ci.second);
    return 0;
}
