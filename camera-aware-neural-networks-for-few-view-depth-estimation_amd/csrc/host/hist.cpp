// cad_hist: the handle of the device histogram pass (kernels/hist_kernels.hip) — the segment and chunk tables,
// the bucket edges as fp32 order keys, and the output buffers, all built once at create time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/cad/cad.h"
#include "../kernels/kernels.hpp"

namespace cad {
void set_last_error(const std::string& msg);   // cad_api.cpp (cad_last_error)
}

static_assert(CAD_HIST_BINS == cad::kHistBins && CAD_HIST_STATS == cad::kHistStats, "cad.h and kernels.hpp disagree");

namespace {

struct HError : std::runtime_error {
    cad_status st;
    HError(cad_status s, const std::string& m) : std::runtime_error(m), st(s) {}
};
#define HCHK(expr)                                                                              \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            throw HError(e_ == hipErrorOutOfMemory ? CAD_ERR_OOM : CAD_ERR_HIP,                 \
                         std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)
void need(bool c, const std::string& m) {
    if (!c) throw HError(CAD_ERR_INVALID, m);
}
template <class F>
cad_status hguard(F&& f) {
    try {
        f();
        return CAD_OK;
    } catch (const HError& e) {
        cad::set_last_error(e.what());
        return e.st;
    } catch (const std::exception& e) {
        cad::set_last_error(e.what());
        return CAD_ERR_INVALID;
    }
}

unsigned order_key(float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
// smallest fp32 >= e / largest fp32 <= e, for a finite double inside the fp32 range
float f32_not_below(double e) {
    float f = (float)e;   // round to nearest
    if ((double)f < e) f = std::nextafterf(f, INFINITY);
    if (f == 0.f) f = 0.f;   // +0.0: the kernel counts -0.0 as 0.0
    return f;
}
float f32_not_above(double e) {
    float f = (float)e;
    if ((double)f > e) f = std::nextafterf(f, -INFINITY);
    return f;
}

}  // namespace

struct cad_hist {
    int device = 0, nseg = 0, nchunks = 0;
    int64_t span = 0;
    unsigned key_hi = 0;
    void* base = nullptr;   // one allocation: out (stats, bins), part, segs, chunks, ukey
    double *stats = nullptr, *part = nullptr;
    unsigned *bins = nullptr, *ukey = nullptr;
    cad::HistSegment* segs = nullptr;
    cad::HistChunk* chunks = nullptr;
    std::vector<char> host;   // staging of cad_hist_read's single copy
    size_t out_bytes = 0;
};

extern "C" {

cad_status cad_hist_create(const cad_hist_segment* segments, int nseg, int device, cad_hist** out) {
    return hguard([&] {
        need(segments && out && nseg > 0, "hist: null argument or no segment");
        std::vector<cad::HistSegment> segs(nseg);
        std::vector<cad::HistChunk> chunks;
        int64_t span = 0;
        for (int s = 0; s < nseg; ++s) {
            const cad_hist_segment& g = segments[s];
            need(g.offset >= 0 && g.count >= 0 && g.count < (int64_t(1) << 32), "hist: segment offset / count out of range");
            need(g.period >= 1 && g.period < (int64_t(1) << 30) && g.keep >= 1 && g.keep <= g.period,
                 "hist: segment needs 1 <= keep <= period < 2^30");
            need((g.inner_period == 0 && g.inner_keep == 0) ||
                     (g.inner_period >= 1 && g.inner_period <= g.period && g.inner_keep >= 1 && g.inner_keep <= g.inner_period),
                 "hist: segment needs inner_period = inner_keep = 0 or 1 <= inner_keep <= inner_period <= period");
            segs[s] = cad::HistSegment{g.offset, g.count, g.period, g.keep, g.inner_period, g.inner_keep, (int)chunks.size(), 0};
            for (int64_t a = 0; a < g.count; a += cad::kHistChunk)
                chunks.push_back(cad::HistChunk{a, s, (int)std::min<int64_t>(cad::kHistChunk, g.count - a)});
            segs[s].nchunks = (int)chunks.size() - segs[s].first_chunk;
            span = std::max(span, g.offset + g.count);
            need(chunks.size() < (size_t(1) << 30), "hist: too many chunks");
        }
        std::vector<double> edges(cad::kHistBins + 1);
        need(cad_tb_default_bins(edges.data(), (int)edges.size()) == cad::kHistBins + 1, "hist: bucket table size");
        std::vector<unsigned> ukey(edges.size());
        for (size_t k = 0; k < edges.size(); ++k) ukey[k] = order_key(f32_not_below(edges[k]));
        for (size_t k = 1; k < ukey.size(); ++k) need(ukey[k] > ukey[k - 1], "hist: bucket edges collapse in fp32");

        HCHK(hipSetDevice(device));
        auto h = std::make_unique<cad_hist>();
        h->device = device; h->nseg = nseg; h->nchunks = (int)chunks.size(); h->span = span;
        h->key_hi = order_key(f32_not_above(edges.back()));
        const auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
        const size_t stats_b = sizeof(double) * cad::kHistStats * (size_t)nseg, bins_b = sizeof(unsigned) * cad::kHistBins * (size_t)nseg;
        h->out_bytes = stats_b + bins_b;
        const size_t o_part = up(h->out_bytes), o_segs = o_part + up(sizeof(double) * cad::kHistStats * std::max<size_t>(chunks.size(), 1)),
                     o_chunks = o_segs + up(sizeof(cad::HistSegment) * segs.size()),
                     o_ukey = o_chunks + up(sizeof(cad::HistChunk) * std::max<size_t>(chunks.size(), 1)),
                     total = o_ukey + up(sizeof(unsigned) * ukey.size());
        HCHK(hipMalloc(&h->base, total));
        char* b = static_cast<char*>(h->base);
        h->stats = reinterpret_cast<double*>(b);
        h->bins = reinterpret_cast<unsigned*>(b + stats_b);
        h->part = reinterpret_cast<double*>(b + o_part);
        h->segs = reinterpret_cast<cad::HistSegment*>(b + o_segs);
        h->chunks = reinterpret_cast<cad::HistChunk*>(b + o_chunks);
        h->ukey = reinterpret_cast<unsigned*>(b + o_ukey);
        hipError_t e = hipMemset(h->base, 0, total);
        if (e == hipSuccess) e = hipMemcpy(h->segs, segs.data(), sizeof(cad::HistSegment) * segs.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !chunks.empty())
            e = hipMemcpy(h->chunks, chunks.data(), sizeof(cad::HistChunk) * chunks.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(h->ukey, ukey.data(), sizeof(unsigned) * ukey.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(h->base);
            throw HError(CAD_ERR_HIP, std::string("hist: table upload: ") + hipGetErrorString(e));
        }
        h->host.resize(h->out_bytes);
        *out = h.release();
    });
}

void cad_hist_destroy(cad_hist* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->base);
    delete h;
}

int cad_hist_num_segments(const cad_hist* h) { return h ? h->nseg : 0; }

cad_status cad_hist_run(cad_hist* h, const float* base, void* stream) {
    return hguard([&] {
        need(h && base, "hist: null argument");
        need((reinterpret_cast<uintptr_t>(base) & 3u) == 0, "hist: base is not 4-byte aligned");
        HCHK(hipSetDevice(h->device));
        cad::hist_run(base, h->segs, h->nseg, h->chunks, h->nchunks, h->ukey, h->key_hi, h->stats, h->bins, h->part, h->span,
                      reinterpret_cast<hipStream_t>(stream));
        HCHK(hipGetLastError());
    });
}

cad_status cad_hist_read(cad_hist* h, double* stats, uint32_t* counts) {
    return hguard([&] {
        need(h != nullptr, "hist: null handle");
        HCHK(hipSetDevice(h->device));
        HCHK(hipDeviceSynchronize());
        HCHK(hipMemcpy(h->host.data(), h->stats, h->out_bytes, hipMemcpyDeviceToHost));
        const size_t stats_b = sizeof(double) * cad::kHistStats * (size_t)h->nseg;
        if (stats) std::memcpy(stats, h->host.data(), stats_b);
        if (counts) std::memcpy(counts, h->host.data() + stats_b, h->out_bytes - stats_b);
    });
}

}  // extern "C"
