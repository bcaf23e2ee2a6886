// Scale alignment of the offline evaluation: the closed forms and fallbacks that turn a sample's
// statistics or medians into (scale, shift).  One inline function for the device solve kernel
// (eval_align_kernels.hip) and the host entry point cad_eval_solve_alignment, so both run the same code.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define CAD_HD __host__ __device__
#else
#define CAD_HD
#endif

namespace cad {

constexpr int kAlignNone = 0, kAlignMedian = 1, kAlignLogMean = 2, kAlignScaleShift = 3;   // cad_eval_align
constexpr int kAlignStats = 7;   // {n, n_pos, sum p, sum g, sum p^2, sum pg, sum(ln g - ln p)}

// st: kAlignStats doubles; med: {med_pred, med_gt} (read for kAlignMedian only).  out2 = {scale, shift},
// each rounded to fp32 once.  Returns 1 when the mode's own formula applied, 0 when a fallback did.
CAD_HD inline int eval_solve_alignment(int mode, const double* st, const float* med, float* out2) {
#pragma clang fp contract(off)
    out2[0] = 1.0f;
    out2[1] = 0.0f;
    const double n = st[0];
    if (mode == kAlignNone) return 1;
    if (!(n > 0.0)) return 0;
    if (mode == kAlignMedian) {
        if (!(med[0] > 0.0f)) return 0;
        out2[0] = med[1] / med[0];
        return 1;
    }
    if (mode == kAlignLogMean) {
        if (!(st[1] > 0.0)) return 0;
        out2[0] = (float)exp(st[6] / st[1]);
        return 1;
    }
    const double sp = st[2], sg = st[3], spp = st[4], spg = st[5];
    const double det = n * spp - sp * sp;
    if (det > 0.0) {
        const double s = (n * spg - sp * sg) / det;
        out2[0] = (float)s;
        out2[1] = (float)((sg - s * sp) / n);
        return 1;
    }
    if (spp > 0.0) out2[0] = (float)(spg / spp);   // scale only
    return 0;
}

}  // namespace cad
