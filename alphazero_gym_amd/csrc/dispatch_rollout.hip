// policy rollouts (azg_policy_rollout, include/azgym_eval.h): the kernel's instantiations, their choice and the C ABI entry
#include <cstring>

#include "engine_host.h"
#include "rollout.cuh"

// widths up to 256 (padded); NREG as the search keeps this network's hidden->hidden layers (e->nreg: 0 streams them)
static hipError_t dispatch_rollout(azg_engine* e, const Rollout& ro) {
    const int NR = e->nreg;
    switch (e->HP) {
        case 64: return NR == 1 ? rollout_launch<64, 1>(e, ro) : NR == 2 ? rollout_launch<64, 2>(e, ro) : rollout_launch<64, 0>(e, ro);
        case 128: return NR == 1 ? rollout_launch<128, 1>(e, ro) : NR == 2 ? rollout_launch<128, 2>(e, ro) : rollout_launch<128, 0>(e, ro);
        case 256: return NR == 1 ? rollout_launch<256, 1>(e, ro) : rollout_launch<256, 0>(e, ro);
    }
    return hipErrorInvalidValue;
}

extern "C" int azg_policy_rollout(azg_engine* e, const azg_rollout_config* c, double* returns, int32_t* lengths, int32_t* terminated,
                                  float* first_value) {
    if (!e) return AZG_E_INVALID;
    if (!c || !returns || !lengths) return fail(e, AZG_E_INVALID, "azg_policy_rollout: cfg, returns and lengths must not be NULL");
    if (c->struct_size != (int32_t)sizeof(azg_rollout_config)) return fail(e, AZG_E_INVALID, "azg_rollout_config size mismatch");
    if (c->episodes_per_net < 1 || c->max_episode_length < 1)
        return fail(e, AZG_E_INVALID, "azg_policy_rollout: episodes_per_net and max_episode_length must be >= 1");
    if (c->action_rule != AZG_ROLLOUT_MODE && c->action_rule != AZG_ROLLOUT_SAMPLE) return fail(e, AZG_E_INVALID, "azg_policy_rollout: unknown action_rule");
    if (!e->mlp_ready) return fail(e, AZG_E_STATE, "azg_policy_rollout: every net needs weights (azg_set_weights / azg_set_net_weights)");
    if (e->HP >= 512)
        return fail(e, AZG_E_UNSUPPORTED, "azg_policy_rollout: networks wider than 256 (padded) are not supported");
    const size_t N = (size_t)e->n_nets * (size_t)c->episodes_per_net;
    if (N > (size_t)1 << 24 || e->n_nets > 65535) return fail(e, AZG_E_INVALID, "azg_policy_rollout: too many episodes in one call");
    ON_DEVICE(e);
    // one block: returns [N] float64 | lengths [N] | terminated [N] | first_value [N]
    const size_t bytes = N * 20;
    if (bytes > e->rollout_bytes) {
        e->rollout_mem.clear();
        e->rollout_bytes = 0;
        if (dalloc(e, e->rollout_mem, &e->d_rollout, bytes)) return AZG_E_DEVICE;
        e->rollout_bytes = bytes;
    }
    Rollout ro;
    ro.G = c->episodes_per_net; ro.max_len = c->max_episode_length; ro.rule = c->action_rule;
    ro.game_id_base = c->game_id_base; ro.episode = c->episode;
    ro.returns = (double*)e->d_rollout;
    ro.lengths = (int*)(e->d_rollout + N * 8);
    ro.terminated = ro.lengths + N;
    ro.first_value = (float*)(ro.terminated + N);
    hipError_t rc = dispatch_rollout(e, ro);
    if (rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string("rollout kernel launch: ") + hipGetErrorString(rc));
    e->rollout_stage.resize(bytes);
    HIPCHK(e, hipMemcpyAsync(e->rollout_stage.data(), e->d_rollout, bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const char* h = e->rollout_stage.data();
    memcpy(returns, h, N * 8);
    memcpy(lengths, h + N * 8, N * 4);
    if (terminated) memcpy(terminated, h + N * 12, N * 4);
    if (first_value) memcpy(first_value, h + N * 16, N * 4);
    return AZG_OK;
}
