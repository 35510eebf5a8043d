// batched inference for every net of a population (azg_population_mlp_eval / _device / azg_population_root_eval, include/azgym_eval.h):
// the kernel's instantiations and the C ABI entries (the kernel, its launch and its grid rule: population_eval.cuh)
#include "engine_host.h"
#include "population_eval.cuh"

// Widths up to 256 (padded): NREG as the search keeps this network's hidden->hidden layers (e->nreg: 0 streams them), the instantiations of
// dispatch_rollout; 512 and 1024: the weight-streaming form (any depth, LayerNorm, six inputs, every activation), mlp_eval_kernel's LDS plan.
static hipError_t dispatch_population_eval(azg_engine* e, const PopEval& pe, int* groups, int* resident) {
    const int NR = e->nreg;
    *resident = 0;
    switch (e->HP) {
        case 64: *resident = NR == 1 || NR == 2;
                 return NR == 1 ? population_eval_launch<64, 1>(e, pe, groups) : NR == 2 ? population_eval_launch<64, 2>(e, pe, groups) : population_eval_launch<64, 0>(e, pe, groups);
        case 128: *resident = NR == 1 || NR == 2;
                  return NR == 1 ? population_eval_launch<128, 1>(e, pe, groups) : NR == 2 ? population_eval_launch<128, 2>(e, pe, groups) : population_eval_launch<128, 0>(e, pe, groups);
        case 256: *resident = NR == 1;
                  return NR == 1 ? population_eval_launch<256, 1>(e, pe, groups) : population_eval_launch<256, 0>(e, pe, groups);
        case 512: return population_eval_launch<512, 0>(e, pe, groups);
        case 1024: return population_eval_launch<1024, 0>(e, pe, groups);
    }
    return hipErrorInvalidValue;
}

// the checks both forms share; *go: there is something to launch
static int population_eval_checks(azg_engine* e, const float* obs, size_t n, const azg_eval_info* info, bool* go) {
    *go = false;
    if (!e) return AZG_E_INVALID;
    if (!obs) return fail(e, AZG_E_INVALID, "azg_population_mlp_eval: obs must not be NULL");
    if (info && info->struct_size != (int32_t)sizeof(azg_eval_info)) return fail(e, AZG_E_INVALID, "azg_eval_info size mismatch");
    if (e->n_nets > 65535 || n > ((size_t)1 << 24) / (size_t)e->n_nets)
        return fail(e, AZG_E_INVALID, "azg_population_mlp_eval: too many observations in one call (n_nets * n <= 2^24, n_nets <= 65535)");
    if (!e->mlp_ready) return fail(e, AZG_E_STATE, "azg_population_mlp_eval: every net needs weights (azg_set_weights / azg_set_net_weights)");
    *go = n > 0;
    return AZG_OK;
}

// the launch on e->stream (device pointers), and what it ran as
static int population_eval_run(azg_engine* e, const float* d_obs, size_t n, int32_t shared_obs, float* d_value, float* d_dist, float* d_raw,
                               azg_eval_info* out) {
    PopEval pe;
    pe.obs = d_obs; pe.obs_stride = shared_obs ? 0 : n * (size_t)e->S_obs;
    pe.n = (int)n; pe.S_obs = e->S_obs; pe.nd = e->nd;
    pe.value = d_value; pe.dist = d_dist; pe.raw = d_raw;
    const int tiles = (int)((n + 15) / 16);
    int resident = 0;
    out->tiles = tiles;
    const hipError_t rc = dispatch_population_eval(e, pe, &out->groups, &resident);   // (the grid rule: population_eval_launch)
    if (rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string("population_eval kernel launch: ") + hipGetErrorString(rc));
    out->resident = resident;
    return AZG_OK;
}

static void report(azg_eval_info* info, const azg_eval_info& ran) {
    if (!info) return;
    info->resident = ran.resident; info->groups = ran.groups; info->tiles = ran.tiles;
}

extern "C" int azg_population_mlp_eval(azg_engine* e, const float* obs, size_t n, int32_t shared_obs, float* value, float* dist, float* raw,
                                       azg_eval_info* info) {
    bool go;
    int rc = population_eval_checks(e, obs, n, info, &go);
    if (rc || !go) return rc;
    ON_DEVICE(e);
    const size_t K = e->n_nets, So = e->S_obs, nd = e->nd, rows = K * n;
    const size_t n_obs = (shared_obs ? n : rows) * So;
    const size_t need = n_obs + rows * (1 + nd + 1 + nd);
    if (need > e->peval_floats) {   // scratch of its own (azg_mlp_eval's is not touched), grow-only
        e->peval_mem.clear();
        e->peval_floats = 0;
        if (dalloc(e, e->peval_mem, &e->d_peval, need)) return AZG_E_DEVICE;
        e->peval_floats = need;
    }
    float* d_obs = e->d_peval;
    float* d_v = d_obs + n_obs;
    float* d_d = d_v + rows;
    float* d_r = d_d + rows * nd;
    HIPCHK(e, hipMemcpyAsync(d_obs, obs, n_obs * 4, hipMemcpyHostToDevice, e->stream));
    azg_eval_info ran{};
    rc = population_eval_run(e, d_obs, n, shared_obs, value ? d_v : nullptr, dist ? d_d : nullptr, raw ? d_r : nullptr, &ran);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    D2H(value, d_v, rows * 4);
    D2H(dist, d_d, rows * nd * 4);
    D2H(raw, d_r, rows * (nd + 1) * 4);
    report(info, ran);
    return AZG_OK;
}

extern "C" int azg_population_mlp_eval_device(azg_engine* e, const float* obs, size_t n, int32_t shared_obs, float* value, float* dist,
                                              float* raw, azg_eval_info* info) {
    bool go;
    int rc = population_eval_checks(e, obs, n, info, &go);
    if (rc || !go) return rc;
    ON_DEVICE(e);
    azg_eval_info ran{};
    rc = population_eval_run(e, obs, n, shared_obs, value, dist, raw, &ran);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    report(info, ran);
    return AZG_OK;
}

// azg_root_eval without the population guard: every search form writes the root's value and distribution parameters for every tree of a
// population (results_for_tree: the persistent kernel's epilogue, results_kernel behind the team and per-layer forms), in tree order
extern "C" int azg_population_root_eval(azg_engine* e, float* value, float* dist) {
    if (!e) return AZG_E_INVALID;
    ON_DEVICE(e);
    int rc = launch_results(e);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t B = e->cfg.n_trees;
    D2H(value, e->d_rootV, B * 4);
    D2H(dist, e->d_rootdist, B * e->nd * 4);
    return AZG_OK;
}
