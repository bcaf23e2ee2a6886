// TensorBoard event files, written natively (cad_tb_* in cad.h; host only, no device call).
//
// The reference reaches TensorBoard through a Python subprocess (tensorboard_logger_v2.h ->
// scripts/tensorboard_writer.py -> torch.utils.tensorboard).  This file writes the same bytes: the record
// framing with masked CRC-32C and the protobuf wire encoding of Event / Summary and of the text,
// custom_scalars and hparams plugin messages, by hand — no protobuf library, nothing generated from .proto
// files.  tests/golden/tfevents holds two files the reference's run left; every record kind they contain is
// reproduced byte for byte (tests/test_tfevents_cpu.py), wall_time aside.
//
//   Event            wall_time = 1 (double), step = 2 (varint, left out when 0), file_version = 3,
//                    summary = 5, source_metadata = 10 {writer = 1}
//   Summary          value = 1 (repeated)
//   Summary.Value    tag = 1, simple_value = 2 (float), image = 4, histo = 5, tensor = 8, metadata = 9
//   Summary.Image    height = 1, width = 2, colorspace = 3, encoded_image_string = 4
//   HistogramProto   min = 1, max = 2, num = 3, sum = 4, sum_squares = 5, bucket_limit = 6, bucket = 7 (packed)
//   SummaryMetadata  plugin_data = 1 {plugin_name = 1, content = 2}
//   TensorProto      dtype = 1 (DT_STRING = 7), tensor_shape = 2 {dim = 2 {size = 1}}, string_val = 8
//   custom scalars   Layout {category = 2 {title = 1, chart = 2 {title = 1, multiline = 2 {tag = 1}}}}
//   hparams          HParamsPluginData {experiment = 2 {hparam_infos = 4 {name = 1, type = 4},
//                    metric_infos = 5 {name = 1 {tag = 2}}}, session_start_info = 3 {hparams = 1 map<string,
//                    Value {number_value = 2}>}, session_end_info = 4 {status = 1}}
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/cad/cad.h"

namespace cad {
void set_last_error(const std::string& msg);   // cad_api.cpp (cad_last_error)
}

namespace {

template <class F>
cad_status tguard(F&& f) {
    try {
        f();
        return CAD_OK;
    } catch (const std::exception& e) {
        cad::set_last_error(e.what());
        return CAD_ERR_INVALID;
    }
}
void need(bool c, const std::string& m) {
    if (!c) throw std::invalid_argument(m);
}

// ---------------- CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), table driven ----------------
struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            t[i] = c;
        }
    }
};
uint32_t crc32c(const void* data, size_t n) {
    static const CrcTable tab;
    const uint8_t* p = static_cast<const uint8_t*>(data);
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = tab.t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xA282EAD8u; }

// ---------------- protobuf wire format ----------------
using Buf = std::string;
void put_varint(Buf& b, uint64_t v) {
    while (v >= 0x80) {
        b.push_back((char)((v & 0x7F) | 0x80));
        v >>= 7;
    }
    b.push_back((char)v);
}
void put_key(Buf& b, int field, int wire) { put_varint(b, ((uint64_t)field << 3) | (uint64_t)wire); }
void put_fixed(Buf& b, const void* p, size_t n) {   // little-endian host
    if (n) b.append(static_cast<const char*>(p), n);
}
void put_double(Buf& b, int field, double v) {
    put_key(b, field, 1);
    put_fixed(b, &v, 8);
}
void put_float(Buf& b, int field, float v) {
    put_key(b, field, 5);
    put_fixed(b, &v, 4);
}
void put_int(Buf& b, int field, uint64_t v) {
    put_key(b, field, 0);
    put_varint(b, v);
}
void put_bytes(Buf& b, int field, const void* p, size_t n) {
    put_key(b, field, 2);
    put_varint(b, n);
    put_fixed(b, p, n);
}
void put_msg(Buf& b, int field, const Buf& m) { put_bytes(b, field, m.data(), m.size()); }
void put_str(Buf& b, int field, const std::string& s) { put_bytes(b, field, s.data(), s.size()); }

double now_seconds() {
    timeval tv;
    gettimeofday(&tv, nullptr);
    return (double)tv.tv_sec + 1e-6 * (double)tv.tv_usec;
}

Buf plugin_metadata(const std::string& plugin, const Buf* content) {
    Buf pd;
    put_str(pd, 1, plugin);
    if (content) put_msg(pd, 2, *content);
    Buf md;
    put_msg(md, 1, pd);
    return md;
}

Buf string_tensor(const std::string& s, bool scalar_shape) {
    Buf t;
    put_int(t, 1, 7);   // DT_STRING
    Buf shape;
    if (!scalar_shape) {
        Buf dim;
        put_int(dim, 1, 1);
        put_msg(shape, 2, dim);
    }
    put_msg(t, 2, shape);
    put_str(t, 8, s);
    return t;
}

void mkdirs(const std::string& path) {
    std::string cur;
    for (size_t i = 0; i <= path.size(); ++i) {
        if (i == path.size() || path[i] == '/') {
            if (!cur.empty() && ::mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST)
                throw std::runtime_error("cannot create directory " + cur + ": " + std::strerror(errno));
        }
        if (i < path.size()) cur.push_back(path[i]);
    }
}

std::atomic<int> g_writer_uid{0};   // the trailing .<k> of the file name: no two writers of a process share a file

struct EventFile {
    FILE* fh = nullptr;
    std::string path;

    void open(const std::string& dir) {
        need(!dir.empty(), "event directory is empty");
        mkdirs(dir);
        char host[256] = "localhost";
        (void)gethostname(host, sizeof host - 1);
        host[sizeof host - 1] = 0;
        const double t = now_seconds();
        for (;;) {   // never append to a file that exists (a resume in the same second by a recycled pid)
            path = dir + "/events.out.tfevents." + std::to_string((long long)t) + "." + host + "." +
                   std::to_string((long long)getpid()) + "." + std::to_string(g_writer_uid.fetch_add(1));
            struct stat sb;
            if (::stat(path.c_str(), &sb) != 0) break;
        }
        fh = std::fopen(path.c_str(), "wb");
        if (!fh) throw std::runtime_error("cannot open " + path + ": " + std::strerror(errno));
        Buf ev;
        put_double(ev, 1, t);
        put_str(ev, 3, "brain.Event:2");
        Buf src;
        put_str(src, 1, "tensorboard.summary.writer.event_file_writer");
        put_msg(ev, 10, src);
        record(ev);
        flush();
    }
    void record(const Buf& payload) {
        need(fh != nullptr, "event file is closed");
        const uint64_t len = payload.size();
        uint8_t head[12];
        std::memcpy(head, &len, 8);
        const uint32_t hc = mask_crc(crc32c(head, 8));
        std::memcpy(head + 8, &hc, 4);
        const uint32_t pc = mask_crc(crc32c(payload.data(), payload.size()));
        if (std::fwrite(head, 1, 12, fh) != 12 || std::fwrite(payload.data(), 1, payload.size(), fh) != payload.size() ||
            std::fwrite(&pc, 1, 4, fh) != 4)
            throw std::runtime_error("write to " + path + " failed: " + std::strerror(errno));
    }
    // Event{wall_time, step, summary{value}}
    void value(int64_t step, const Buf& val) {
        Buf ev;
        put_double(ev, 1, now_seconds());
        if (step != 0) put_int(ev, 2, (uint64_t)step);
        Buf summary;
        put_msg(summary, 1, val);
        put_msg(ev, 5, summary);
        record(ev);
    }
    void scalar(const std::string& tag, float v, int64_t step) {
        Buf val;
        put_str(val, 1, tag);
        put_float(val, 2, v);
        value(step, val);
    }
    void flush() {
        if (fh && std::fflush(fh) != 0) throw std::runtime_error("flush of " + path + " failed");
    }
    void close() {
        if (fh) std::fclose(fh);
        fh = nullptr;
    }
};

}  // namespace

struct cad_tb_writer {
    std::string logdir;
    EventFile main, sub;
};

extern "C" {

uint32_t cad_crc32c(const void* data, int64_t size) { return crc32c(data, size > 0 ? (size_t)size : 0); }
uint32_t cad_crc32c_masked(const void* data, int64_t size) { return mask_crc(cad_crc32c(data, size)); }

cad_status cad_tb_open(const char* logdir, cad_tb_writer** out) {
    return tguard([&] {
        need(logdir && out, "null argument");
        auto* w = new cad_tb_writer();
        try {
            w->logdir = logdir;
            while (w->logdir.size() > 1 && w->logdir.back() == '/') w->logdir.pop_back();
            w->main.open(w->logdir);
        } catch (...) {
            delete w;
            throw;
        }
        *out = w;
    });
}

void cad_tb_close(cad_tb_writer* w) {
    if (!w) return;
    w->main.close();
    w->sub.close();
    delete w;
}

cad_status cad_tb_flush(cad_tb_writer* w) {
    return tguard([&] {
        need(w != nullptr, "null writer");
        w->main.flush();
        w->sub.flush();
    });
}

const char* cad_tb_path(const cad_tb_writer* w) { return w ? w->main.path.c_str() : ""; }
const char* cad_tb_hparams_path(const cad_tb_writer* w) { return w ? w->sub.path.c_str() : ""; }

cad_status cad_tb_scalar(cad_tb_writer* w, const char* tag, float value, int64_t step) {
    return tguard([&] {
        need(w && tag, "null argument");
        w->main.scalar(tag, value, step);
    });
}

cad_status cad_tb_histogram(cad_tb_writer* w, const char* tag, int64_t step, const double stats[5], const double* limits,
                            const double* buckets, int n) {
    return tguard([&] {
        need(w && tag && stats && n >= 0 && (n == 0 || (limits && buckets)), "bad histogram arguments");
        Buf h;
        for (int k = 0; k < 5; ++k) put_double(h, k + 1, stats[k]);
        put_bytes(h, 6, limits, sizeof(double) * (size_t)n);
        put_bytes(h, 7, buckets, sizeof(double) * (size_t)n);
        Buf val;
        put_str(val, 1, tag);
        put_msg(val, 5, h);
        w->main.value(step, val);
    });
}

cad_status cad_tb_image(cad_tb_writer* w, const char* tag, int64_t step, int height, int width, int colorspace,
                        const void* png, int64_t bytes) {
    return tguard([&] {
        need(w && tag && png && bytes > 0 && height > 0 && width > 0 && colorspace >= 1 && colorspace <= 4,
             "bad image arguments");
        Buf im;
        put_int(im, 1, (uint64_t)height);
        put_int(im, 2, (uint64_t)width);
        put_int(im, 3, (uint64_t)colorspace);
        put_bytes(im, 4, png, (size_t)bytes);
        Buf val;
        put_str(val, 1, tag);
        put_msg(val, 4, im);
        w->main.value(step, val);
    });
}

cad_status cad_tb_text(cad_tb_writer* w, const char* tag, int64_t step, const char* text) {
    return tguard([&] {
        need(w && tag && text, "null argument");
        Buf val;
        put_str(val, 1, std::string(tag) + "/text_summary");
        put_msg(val, 8, string_tensor(text, false));
        put_msg(val, 9, plugin_metadata("text", nullptr));
        w->main.value(step, val);
    });
}

cad_status cad_tb_custom_scalars(cad_tb_writer* w, const char* const* categories, const char* const* charts,
                                 const char* const* tags, int n) {
    return tguard([&] {
        need(w && n >= 0 && (n == 0 || (categories && charts && tags)), "bad layout arguments");
        for (int i = 0; i < n; ++i) need(categories[i] && charts[i] && tags[i], "null layout entry");
        Buf layout;
        int i = 0;
        while (i < n) {
            const std::string cat = categories[i];
            Buf cmsg;
            put_str(cmsg, 1, cat);
            while (i < n && cat == categories[i]) {
                const std::string chart = charts[i];
                Buf multi;
                while (i < n && cat == categories[i] && chart == charts[i]) put_str(multi, 1, tags[i++]);
                Buf ch;
                put_str(ch, 1, chart);
                put_msg(ch, 2, multi);
                put_msg(cmsg, 2, ch);
            }
            put_msg(layout, 2, cmsg);
        }
        Buf val;
        put_str(val, 1, "custom_scalars__config__");
        put_msg(val, 8, string_tensor(layout, true));
        put_msg(val, 9, plugin_metadata("custom_scalars", nullptr));
        w->main.value(0, val);
    });
}

cad_status cad_tb_hparams(cad_tb_writer* w, const char* const* names, const double* values, int n,
                          const char* const* metric_tags, const float* metric_values, int nmetrics, const char* subdir) {
    return tguard([&] {
        need(w && n >= 0 && nmetrics >= 0 && (n == 0 || (names && values)) && (nmetrics == 0 || (metric_tags && metric_values)),
             "bad hparams arguments");
        need(w->sub.fh == nullptr, "this writer already has a hyper-parameter sub-run");
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) {
            need(names[i] != nullptr, "null hparam name");
            order[i] = i;
        }
        std::sort(order.begin(), order.end(), [&](int a, int b) { return std::strcmp(names[a], names[b]) < 0; });
        std::string sd;
        if (subdir && *subdir) sd = subdir;
        else {
            char buf[64];
            std::snprintf(buf, sizeof buf, "%.6f", now_seconds());
            sd = buf;
        }
        need(sd.find('/') == std::string::npos, "hparams sub-run name must not contain '/'");
        w->sub.open(w->logdir + "/" + sd);

        Buf exp;   // Experiment
        for (int i : order) {
            Buf info;
            put_str(info, 1, names[i]);
            put_int(info, 4, 3);   // DATA_TYPE_FLOAT64
            put_msg(exp, 4, info);
        }
        for (int m = 0; m < nmetrics; ++m) {
            need(metric_tags[m] != nullptr, "null metric tag");
            Buf name, mi;
            put_str(name, 2, metric_tags[m]);
            put_msg(mi, 1, name);
            put_msg(exp, 5, mi);
        }
        Buf start;   // SessionStartInfo
        for (int i : order) {
            Buf v, entry;
            put_double(v, 2, values[i]);
            put_str(entry, 1, names[i]);
            put_msg(entry, 2, v);
            put_msg(start, 1, entry);
        }
        Buf end;     // SessionEndInfo{status = STATUS_SUCCESS}
        put_int(end, 1, 1);
        const struct { const char* tag; int field; const Buf* msg; } recs[3] = {
            {"_hparams_/experiment", 2, &exp}, {"_hparams_/session_start_info", 3, &start},
            {"_hparams_/session_end_info", 4, &end}};
        for (const auto& r : recs) {
            Buf content;
            put_msg(content, r.field, *r.msg);
            Buf val;
            put_str(val, 1, r.tag);
            put_msg(val, 9, plugin_metadata("hparams", &content));
            w->sub.value(0, val);
        }
        for (int m = 0; m < nmetrics; ++m) w->sub.scalar(metric_tags[m], metric_values[m], 0);
        w->sub.flush();
    });
}

int cad_tb_default_bins(double* edges, int cap) {
    std::vector<double> pos;
    double v = 1e-12;
    while (v < 1e20) {
        pos.push_back(v);
        v *= 1.1;
    }
    const int n = 2 * (int)pos.size() + 1;
    if (edges) {
        for (int i = 0; i < n && i < cap; ++i) {
            const int m = (int)pos.size();
            edges[i] = i < m ? -pos[m - 1 - i] : i == m ? 0.0 : pos[i - m - 1];
        }
    }
    return n;
}

cad_status cad_tb_trim_histogram(const uint32_t* counts, int nbins, const double* edges, double* limits, double* buckets,
                                 int* n) {
    return tguard([&] {
        need(counts && edges && limits && buckets && n && nbins > 0, "bad trim arguments");
        int first = -1, last = -1;
        for (int i = 0; i < nbins; ++i)
            if (counts[i]) {
                if (first < 0) first = i;
                last = i;
            }
        if (first < 0) {   // nothing landed in a bucket
            limits[0] = 0.0;
            buckets[0] = 0.0;
            *n = 1;
            return;
        }
        // make_histogram: start = first, end = last + 1; counts[start - 1 : end] (or a 0 in front when start == 0),
        // limits[start : end + 1]
        int k = 0;
        buckets[k] = first > 0 ? (double)counts[first - 1] : 0.0;   // empty by construction
        limits[k++] = edges[first];
        for (int i = first; i <= last; ++i) {
            buckets[k] = (double)counts[i];
            limits[k++] = edges[i + 1];
        }
        *n = k;
    });
}

}  // extern "C"
