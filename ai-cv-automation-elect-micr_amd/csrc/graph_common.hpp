// Shared pieces of the native graph executors.  graph_exec.hip holds the five ABI entries over one Graph; graph_exec_d.hip (graphs D /
// D'), graph_exec_x.hip (graph X) and graph_exec_g.hip (graph G's generator) each hold a layer table, its parameters and a launch
// sequence.  Here: what they share at create time (weight lookup with a typed error, the scope uniquifier, batch-norm folding, upload
// and packing) and at run time (the workspace arena, activation views, the run context, the Graph interface).  Host code only.
#pragma once

#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mfma_common.hpp"

namespace emd {
namespace gx {

struct Packed {   // bf16 hi / lo planes on the device (one allocation, lo behind hi)
    uint16_t* hi = nullptr;
    uint16_t* lo = nullptr;
};

typedef std::map<std::string, std::pair<const float*, long>> WeightMap;

struct CreateError {   // why emd_graph_create failed: the code it returns and the text of emd_last_error(); unset (EMD_OK) = none yet
    int code = EMD_OK;
    std::string text;
    bool set(int c, const std::string& t) {   // returns false, for `return err->set(...)`
        code = c;
        text = t;
        return false;
    }
};

inline bool fetch(const WeightMap& w, const std::string& name, long count, const float** out, CreateError* err) {
    auto it = w.find(name);
    if (it == w.end()) return err->set(EMD_E_INVALID, "emd_graph_create: missing variable " + name);
    if (it->second.second != count)
        return err->set(EMD_E_INVALID, "emd_graph_create: " + name + ": " + std::to_string(it->second.second) + " elements, expected " +
                                           std::to_string(count));
    *out = it->second.first;
    return true;
}

// tf.variable_scope default-name uniquifier: names are counted per enclosing scope (the stack; emdenoise.gan._Scope)
struct Scope {
    std::vector<std::string> stack;
    std::map<std::string, int> counts;
    explicit Scope(const std::string& root) : stack{root} {}
    std::string operator()(const std::string& base) {
        std::string parent = stack[0];
        for (size_t i = 1; i < stack.size(); ++i) parent += "/" + stack[i];
        const int k = counts[parent + "|" + base]++;
        return k == 0 ? parent + "/" + base : parent + "/" + base + "_" + std::to_string(k);
    }
};

template <typename T>
T* upload(std::vector<void*>& allocs, const T* host, size_t n) {
    void* d = nullptr;
    if (hipMalloc(&d, n * sizeof(T) < 16 ? 16 : n * sizeof(T)) != hipSuccess) return nullptr;
    allocs.push_back(d);
    if (hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return static_cast<T*>(d);
}

inline float* upload_f(std::vector<void*>& allocs, const std::vector<double>& v) {
    std::vector<float> f(v.begin(), v.end());
    return upload(allocs, f.data(), f.size());
}

// host weights [taps][a][b] -> packed planes on the device
inline bool pack(std::vector<void*>& allocs, const float* w, int taps, int cin, int cout, int cout_major, Packed* out) {
    const size_t n = emd_packed_weight_elems(taps, cin, cout), npad = (n + 63) / 64 * 64;
    std::vector<uint16_t> both(2 * npad, 0);
    if (emd_pack_weights_bf16(w, taps, cin, cout, cout_major, both.data(), both.data() + npad) != EMD_OK) return false;
    uint16_t* d = upload(allocs, both.data(), both.size());
    if (!d) return false;
    out->hi = d;
    out->lo = d + npad;
    return true;
}

// inference batch norm as y = x * gs + hs (float64)
inline bool bn_affine(const WeightMap& w, const std::string& scope, int C, double eps, std::vector<double>* gs, std::vector<double>* hs,
                      CreateError* err) {
    const float *gamma, *beta, *mean, *var;
    if (!fetch(w, scope + "/gamma", C, &gamma, err) || !fetch(w, scope + "/beta", C, &beta, err) ||
        !fetch(w, scope + "/moving_mean", C, &mean, err) || !fetch(w, scope + "/moving_variance", C, &var, err))
        return false;
    gs->resize(C);
    hs->resize(C);
    for (int c = 0; c < C; ++c) {
        (*gs)[c] = (double)gamma[c] / std::sqrt((double)var[c] + eps);
        (*hs)[c] = (double)beta[c] - (double)mean[c] * (*gs)[c];
    }
    return true;
}

// bias (or NULL), then the batch norms of bn_scopes in order -> one affine y = x * s + t (float64; the operand order is what the
// uploaded bytes depend on)
inline bool fold_affine(const WeightMap& w, const float* bias, const std::vector<std::string>& bn_scopes, int C, double eps,
                        std::vector<double>* s, std::vector<double>* t, CreateError* err) {
    s->assign(C, 1.0);
    t->assign(C, 0.0);
    if (bias)
        for (int c = 0; c < C; ++c) (*t)[c] = bias[c];
    for (const std::string& scope : bn_scopes) {
        std::vector<double> gs, hs;
        if (!bn_affine(w, scope, C, eps, &gs, &hs, err)) return false;
        for (int c = 0; c < C; ++c) {
            (*s)[c] *= gs[c];
            (*t)[c] = (*t)[c] * gs[c] + hs[c];
        }
    }
    return true;
}

// transposed-conv kernel [3][3][Cout][Cin] -> per output phase [taps][Cout][Cin], packed
inline bool pack_deconv_phases(std::vector<void*>& allocs, const float* wt, int cin, int cout, Packed (&phase)[4]) {
    const size_t tap = (size_t)cout * cin;
    for (int ph = 0; ph < 4; ++ph) {
        int ky[4], kx[4];
        const int nt = emd_deconv_phase_taps(ph, ky, kx);
        std::vector<float> sub(nt * tap);
        for (int q = 0; q < nt; ++q) std::memcpy(sub.data() + q * tap, wt + (size_t)(ky[q] * 3 + kx[q]) * tap, sizeof(float) * tap);
        if (!pack(allocs, sub.data(), nt, cin, cout, 1, &phase[ph])) return false;
    }
    return true;
}

struct PhasePtrs {   // the four phases' planes as the transposed-conv entry points take them
    const uint16_t *hi[4], *lo[4];
    explicit PhasePtrs(const Packed (&phase)[4]) {
        for (int ph = 0; ph < 4; ++ph) {
            hi[ph] = phase[ph].hi;
            lo[ph] = phase[ph].lo;
        }
    }
};

// ---- workspace: a first-fit free-list allocator over the caller's buffer; in measuring mode it only tracks the peak
struct Arena {
    unsigned char* base = nullptr;
    size_t cap = 0, peak = 0;
    bool measuring = false;
    std::map<size_t, size_t> live;   // offset -> size
    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        size_t off = 0;
        for (auto& kv : live) {   // ordered by offset: first gap that fits
            if (kv.first - off >= bytes) break;
            off = kv.first + kv.second;
        }
        if (!measuring && off + bytes > cap) return nullptr;
        live[off] = bytes;
        if (off + bytes > peak) peak = off + bytes;
        return measuring ? reinterpret_cast<void*>(off + 4096) : static_cast<void*>(base + off);   // measuring: a fake non-null address
    }
    void release(void* p) {
        if (!p) return;
        const size_t off = measuring ? reinterpret_cast<size_t>(p) - 4096 : static_cast<size_t>(static_cast<unsigned char*>(p) - base);
        live.erase(off);
    }
};

struct T4 {   // an activation: channels [c0, c0 + C) of a [B,H,W,ld] fp32 buffer
    float* buf = nullptr;
    int B = 0, H = 0, W = 0, C = 0, ld = 0, c0 = 0;
    float* ptr() const { return buf + c0; }
    T4 slice(int off, int n) const {
        T4 t = *this;
        t.c0 = c0 + off;
        t.C = n;
        return t;
    }
};

// ---- what every launch sequence runs in: the arena, the stream, dry (plan the workspace, launch nothing) and the first error
struct RunBase {
    Arena* ar;
    hipStream_t st;
    bool dry;
    int rc = EMD_OK;

    void* raw(size_t bytes) {
        void* p = ar->alloc(bytes);
        if (!p && rc == EMD_OK) rc = emd::fail(EMD_E_INVALID, "emd_graph_run: workspace too small");
        return p;
    }
    T4 E(int B, int H, int W, int C) {
        T4 t;
        t.B = B; t.H = H; t.W = W; t.C = C; t.ld = C;
        t.buf = static_cast<float*>(raw((size_t)B * H * W * C * 4));
        return t;
    }
    void release(void* p) { ar->release(p); }
    void release(T4& t) {
        ar->release(t.buf);
        t.buf = nullptr;
    }
    void call(int code) {
        if (code != EMD_OK && rc == EMD_OK) rc = code;
    }
    bool live() const { return !dry && rc == EMD_OK; }
    // a keyed layer table's record; an unknown key is reported (once) and answered with an empty record, so a dry pass still ends
    template <typename P>
    const P& param(const std::map<std::string, P>& table, const std::string& key) {
        static const P none{};
        auto it = table.find(key);
        if (it != table.end()) return it->second;
        if (rc == EMD_OK) {
            emd::set_error("emd_graph_run: no layer %s", key.c_str());
            rc = EMD_E_INVALID;
        }
        return none;
    }
};

// The split32 form of an activation: xs (pitch *ld) where the caller has one, otherwise the fp32 view x converted into a temporary;
// *tmp is what to release after the launch that reads it (NULL where nothing was made)
inline const void* as_split32(RunBase& r, const T4* x, const void* xs, long npix, int cin, int* ld, void** tmp) {
    *tmp = nullptr;
    if (xs) return xs;
    *ld = emd_split32_ld(cin);
    *tmp = r.raw((size_t)npix * *ld * 4);
    if (r.live()) r.call(emd_to_split32_f32(x->ptr(), x->ld, *tmp, *ld, npix, cin, r.st));
    return *tmp;
}

// ---- one native graph: parameters on the device (owned by the handle's allocation list) and a launch sequence
struct Graph {
    virtual ~Graph() = default;
    virtual bool side_ok(int S) const = 0;          // beyond the ABI's own S >= 16, S % 16 == 0
    virtual const char* side_error() const = 0;
    virtual bool has_two_stream_form() const { return false; }   // forward() looks at two_streams: a workspace query plans both forms
    // launches (dry = false) or only plans the workspace (dry = true: ar in measuring mode); returns an EMD_* code
    virtual int forward(Arena* ar, hipStream_t st, bool dry, bool two_streams, const float* in, float* out, int B, int S) = 0;
};

// A create returns NULL with *err set; a failure that left *err unset is a device allocation, an upload or a weight packing
// (the caller gives it EMD_E_ALLOC and "... device allocation or upload failed").  Device memory goes on `allocs` either way.
std::unique_ptr<Graph> d_create(const WeightMap& w, std::vector<void*>& allocs, bool twin, CreateError* err);   // graph_exec_d.hip
std::unique_ptr<Graph> x_create(const WeightMap& w, std::vector<void*>& allocs, CreateError* err);              // graph_exec_x.hip
std::unique_ptr<Graph> g_create(const WeightMap& w, std::vector<void*>& allocs, CreateError* err);              // graph_exec_g.hip

}  // namespace gx
}  // namespace emd
