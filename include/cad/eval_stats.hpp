// eval_stats.hpp — host-only statistics for comparing two models on the same samples (no device, no
// dependency on cad.h).  The reference's StatisticalTester (src/evaluation/statistical_tests.h) offers
// the same four tools; here the t-test's p-value comes from the regularised incomplete beta function
// (the reference approximates Student's t by a normal, :468-500) and the Wilcoxon variance carries the
// tie correction.
//
//   paired_t_test        t, df = N - 1, two-sided p = I_{df/(df+t^2)}(df/2, 1/2)
//   wilcoxon_signed_rank zero differences dropped, average ranks for ties, W = min(W+, W-),
//                        z = (W+ - n(n+1)/4) / sqrt(n(n+1)(2n+1)/24 - sum(t^3 - t)/48), no continuity
//                        correction, two-sided p = erfc(|z| / sqrt 2)
//   cohens_d             mean / sample standard deviation (/ (N-1)) of the paired differences
//   bootstrap_ci         percentile bootstrap CI of the mean difference, std::mt19937(seed)
//   compare_models       one text block with all of the above
#ifndef CAD_EVAL_STATS_HPP
#define CAD_EVAL_STATS_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iomanip>
#include <limits>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace camera_aware_depth {
namespace eval_stats {

// continued fraction of the incomplete beta function (modified Lentz)
inline double betacf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 10000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

// regularised incomplete beta function I_x(a, b)
inline double incomplete_beta(double a, double b, double x) {
    if (!(x > 0.0)) return 0.0;
    if (!(x < 1.0)) return 1.0;
    const double lbt = std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x);
    if (x < (a + 1.0) / (a + b + 2.0)) return std::exp(lbt) * betacf(a, b, x) / a;
    return 1.0 - std::exp(lbt) * betacf(b, a, 1.0 - x) / b;
}

// two-sided p-value of Student's t with df degrees of freedom
inline double student_t_two_sided(double t, double df) {
    if (std::isnan(t)) return std::numeric_limits<double>::quiet_NaN();
    if (std::isinf(t)) return 0.0;
    return incomplete_beta(0.5 * df, 0.5, df / (df + t * t));
}

inline std::vector<double> differences(const std::vector<double>& a, const std::vector<double>& b) {
    if (a.size() != b.size()) throw std::invalid_argument("paired samples differ in length");
    std::vector<double> d(a.size());
    for (size_t i = 0; i < a.size(); ++i) d[i] = a[i] - b[i];
    return d;
}
inline double mean(const std::vector<double>& v) {
    double s = 0.0;
    for (double x : v) s += x;
    return v.empty() ? 0.0 : s / (double)v.size();
}
// standard deviation with divisor N - ddof
inline double stddev(const std::vector<double>& v, int ddof) {
    if ((int64_t)v.size() <= ddof) return 0.0;
    const double m = mean(v);
    double s = 0.0;
    for (double x : v) s += (x - m) * (x - m);
    return std::sqrt(s / (double)((int64_t)v.size() - ddof));
}
inline double median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

struct TTest {
    double t = 0, df = 0, p = 1, mean_diff = 0, std_diff = 0;
};
inline TTest paired_t_test(const std::vector<double>& a, const std::vector<double>& b) {
    const std::vector<double> d = differences(a, b);
    if (d.size() < 2) throw std::invalid_argument("paired t-test needs at least two pairs");
    TTest r;
    r.df = (double)d.size() - 1.0;
    r.mean_diff = mean(d);
    r.std_diff = stddev(d, 1);
    r.t = r.mean_diff / (r.std_diff / std::sqrt((double)d.size()));
    r.p = student_t_two_sided(r.t, r.df);
    return r;
}

struct Wilcoxon {
    double w_plus = 0, w_minus = 0, w = 0, z = 0, p = 1;
    int64_t n = 0;   // non-zero differences
};
inline Wilcoxon wilcoxon_signed_rank(const std::vector<double>& a, const std::vector<double>& b) {
    std::vector<double> d;
    for (double x : differences(a, b))
        if (x != 0.0) d.push_back(x);
    Wilcoxon r;
    r.n = (int64_t)d.size();
    if (d.empty()) return r;
    std::vector<size_t> idx(d.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](size_t i, size_t j) { return std::fabs(d[i]) < std::fabs(d[j]); });
    std::vector<double> rank(d.size());
    double tie = 0.0;
    for (size_t i = 0; i < idx.size();) {
        size_t j = i;
        while (j < idx.size() && std::fabs(d[idx[j]]) == std::fabs(d[idx[i]])) ++j;
        const double avg = 0.5 * ((double)(i + 1) + (double)j);   // ranks i+1 .. j
        for (size_t k = i; k < j; ++k) rank[idx[k]] = avg;
        const double t = (double)(j - i);
        tie += t * t * t - t;
        i = j;
    }
    for (size_t i = 0; i < d.size(); ++i) (d[i] > 0 ? r.w_plus : r.w_minus) += rank[i];
    r.w = std::min(r.w_plus, r.w_minus);
    const double n = (double)r.n;
    const double mu = n * (n + 1.0) / 4.0;
    const double var = n * (n + 1.0) * (2.0 * n + 1.0) / 24.0 - tie / 48.0;
    r.z = (r.w_plus - mu) / std::sqrt(var);
    r.p = std::erfc(std::fabs(r.z) / std::sqrt(2.0));
    return r;
}

inline double cohens_d(const std::vector<double>& a, const std::vector<double>& b) {
    const std::vector<double> d = differences(a, b);
    return mean(d) / stddev(d, 1);
}

// percentile bootstrap of the mean paired difference; indices are drawn as floor(u32 * N / 2^32) from
// std::mt19937 (the engine's output is fixed by the standard, so a seed gives the same interval everywhere)
inline std::pair<double, double> bootstrap_ci(const std::vector<double>& a, const std::vector<double>& b, uint32_t seed,
                                              int resamples = 2000, double confidence = 0.95) {
    const std::vector<double> d = differences(a, b);
    if (d.empty() || resamples < 1) throw std::invalid_argument("bootstrap needs samples");
    std::mt19937 rng(seed);
    std::vector<double> means((size_t)resamples);
    for (auto& m : means) {
        double s = 0.0;
        for (size_t i = 0; i < d.size(); ++i) s += d[(size_t)(((uint64_t)(uint32_t)rng() * (uint64_t)d.size()) >> 32)];
        m = s / (double)d.size();
    }
    std::sort(means.begin(), means.end());
    const double alpha = 0.5 * (1.0 - confidence);
    const auto at = [&](double q) {
        const int64_t i = (int64_t)std::floor(q * (double)(resamples - 1) + 0.5);
        return means[(size_t)std::max<int64_t>(0, std::min<int64_t>(resamples - 1, i))];
    };
    return {at(alpha), at(1.0 - alpha)};
}

inline std::string compare_models(const std::vector<double>& a, const std::vector<double>& b, const std::string& name_a,
                                  const std::string& name_b, const std::string& metric, uint32_t seed = 42) {
    const TTest t = paired_t_test(a, b);
    const Wilcoxon w = wilcoxon_signed_rank(a, b);
    const double d = cohens_d(a, b);
    const auto ci = bootstrap_ci(a, b, seed);
    const double ad = std::fabs(d);
    const char* size = ad < 0.2 ? "negligible" : ad < 0.5 ? "small" : ad < 0.8 ? "medium" : "large";
    std::ostringstream o;
    o << "===========================================================\n"
      << "  Statistical Model Comparison (" << metric << ")\n"
      << "===========================================================\n\n"
      << "Comparing: " << name_a << " vs " << name_b << "\nSample size: " << a.size() << "\n\n"
      << std::fixed << std::setprecision(4) << "Descriptive Statistics:\n"
      << "-----------------------------------------------------------\n"
      << name_a << ":\n  Mean: " << mean(a) << " +/- " << stddev(a, 0) << "\n  Median: " << median(a) << "\n\n"
      << name_b << ":\n  Mean: " << mean(b) << " +/- " << stddev(b, 0) << "\n  Median: " << median(b) << "\n\n"
      << "Effect Size (Cohen's d): " << d << " (" << size << ")\n\n"
      << "Paired t-test:\n-----------------------------------------------------------\n"
      << "Mean difference: " << t.mean_diff << " +/- " << t.std_diff << "\nt-statistic: " << t.t << " (df=" << (int64_t)t.df
      << ")\np-value: " << std::setprecision(6) << t.p << std::setprecision(4) << "\nResult: "
      << (t.p < 0.05 ? "SIGNIFICANT difference (p < 0.05)" : "NOT significant (p >= 0.05)") << "\n\n"
      << "Wilcoxon Signed-Rank Test:\n-----------------------------------------------------------\n"
      << "W+ (sum of positive ranks): " << w.w_plus << "\nW- (sum of negative ranks): " << w.w_minus
      << "\nW statistic: " << w.w << " (n=" << w.n << " non-zero differences, z=" << w.z << ")\np-value: "
      << std::setprecision(6) << w.p << std::setprecision(4) << "\nResult: "
      << (w.p < 0.05 ? "SIGNIFICANT difference (p < 0.05)" : "NOT significant (p >= 0.05)") << "\n\n"
      << "Bootstrap Confidence Interval (95%, seed " << seed << "):\n"
      << "-----------------------------------------------------------\n"
      << "Mean difference: [" << ci.first << ", " << ci.second << "]\n\n"
      << "===========================================================\n"
      << "Conclusion: ";
    if (t.p < 0.05 && w.p < 0.05)
        o << (t.mean_diff < 0 ? name_a : name_b) << " has the lower " << metric << " (both tests significant)\n";
    else if (t.p < 0.05 || w.p < 0.05)
        o << "the tests disagree; the difference is not established\n";
    else
        o << "no significant difference between " << name_a << " and " << name_b << "\n";
    o << "===========================================================\n";
    return o.str();
}

}  // namespace eval_stats
}  // namespace camera_aware_depth

#endif  // CAD_EVAL_STATS_HPP
