// graph_exec.hip -- the native graph executor's C ABI: emd_graph_create / _workspace_bytes / _run / _set_two_streams / _destroy
// (last row) over one Graph (graph_common.hpp).  The graphs themselves -- layer table in the reference's variable-creation
// order, folded batch norms, packed weights, launch sequence -- are graph_exec_d.hip (variants 0 / 1: graphs D / D'),
// graph_exec_x.hip (2: graph X) and graph_exec_g.hip (3: graph G's generator).
//
// Ownership: emd_graph_create uploads the prepared parameters into device memory it allocates and emd_graph_destroy frees (the
// one explicit handle of the ABI); activations live in the caller's workspace (emd_graph_workspace_bytes), nothing else is
// allocated, no global state.  A workspace query does not write the handle.
#include "graph_common.hpp"

using emd::gx::Arena;

struct emd_graph {   // the handle behind emd_graph_t
    std::unique_ptr<emd::gx::Graph> g;
    std::vector<void*> allocs;
    bool two_streams = false;   // emd_graph_set_two_streams
};

extern "C" int emd_graph_create(emd_graph** out, int variant, int n_vars, const char* const* names, const float* const* data,
                                const long* counts) {
    EMD_REQUIRE(out && names && data && counts && n_vars > 0, EMD_E_INVALID, "emd_graph_create: null argument");
    EMD_REQUIRE(variant >= 0 && variant <= 3, EMD_E_UNSUPPORTED,
                "emd_graph_create: variant 0 (graph D, machine_learning/denoiser.py), 1 (graph D', misc_py/denoiser-multi-gpu.py, phase=False) , 2 (graph X, misc_py/modified_Xception.py) or 3 (graph G's generator, misc_py/gan-infilling-100.py)");
    *out = nullptr;
    emd::gx::WeightMap w;
    for (int i = 0; i < n_vars; ++i) {
        EMD_REQUIRE(names[i] && data[i] && counts[i] > 0, EMD_E_INVALID, "emd_graph_create: null variable entry");
        w[names[i]] = {data[i], counts[i]};
    }
    emd_graph* g = new emd_graph();
    emd::gx::CreateError err;
    g->g = variant <= 1 ? emd::gx::d_create(w, g->allocs, variant == 1, &err)
                        : variant == 2 ? emd::gx::x_create(w, g->allocs, &err) : emd::gx::g_create(w, g->allocs, &err);
    if (!g->g) {
        if (err.code == EMD_OK) err.set(EMD_E_ALLOC, "emd_graph_create: device allocation or upload failed");
        emd::set_error("%s", err.text.c_str());
        for (void* q : g->allocs) (void)hipFree(q);
        delete g;
        return err.code;
    }
    *out = g;
    return EMD_OK;
}

extern "C" size_t emd_graph_workspace_bytes(emd_graph* g, int B, int S) {
    if (!g || B < 1 || S < 16 || S % 16 || !g->g->side_ok(S)) return 0;
    // the larger of the two launch forms: a size asked for before emd_graph_set_two_streams stays valid after it
    size_t need = 0;
    for (int two = 0; two < (g->g->has_two_stream_form() ? 2 : 1); ++two) {
        Arena ar;
        ar.measuring = true;
        if (g->g->forward(&ar, nullptr, true, two != 0, nullptr, nullptr, B, S) != EMD_OK) return 0;
        need = ar.peak > need ? ar.peak : need;
    }
    return need + 256;
}

extern "C" int emd_graph_run(emd_graph* g, const float* x, float* y, int B, int S, void* workspace, size_t workspace_bytes,
                             emd_stream_t stream) {
    EMD_REQUIRE(g && x && y && workspace, EMD_E_INVALID, "emd_graph_run: null pointer");
    EMD_REQUIRE(B >= 1 && S >= 16 && S % 16 == 0, EMD_E_INVALID, "emd_graph_run: square crops with side a multiple of 16, B >= 1");
    EMD_REQUIRE(x != y, EMD_E_INVALID, "emd_graph_run: the output aliases the input");
    unsigned char* base = static_cast<unsigned char*>(workspace);
    const size_t skew = (256 - (reinterpret_cast<uintptr_t>(base) & 255)) & 255;
    EMD_REQUIRE(workspace_bytes > skew, EMD_E_INVALID, "emd_graph_run: workspace too small");
    EMD_REQUIRE(g->g->side_ok(S), EMD_E_INVALID, g->g->side_error());
    Arena ar;
    ar.base = base + skew;
    ar.cap = workspace_bytes - skew;
    return g->g->forward(&ar, static_cast<hipStream_t>(stream), false, g->two_streams, x, y, B, S);
}

extern "C" int emd_graph_set_two_streams(emd_graph* g, int on) {
    EMD_REQUIRE(g, EMD_E_INVALID, "emd_graph_set_two_streams: null handle");
    g->two_streams = on != 0;
    return EMD_OK;
}

extern "C" void emd_graph_destroy(emd_graph* g) {
    if (!g) return;
    for (void* q : g->allocs) (void)hipFree(q);
    delete g;   // graph D's side streams and events go with it
}
