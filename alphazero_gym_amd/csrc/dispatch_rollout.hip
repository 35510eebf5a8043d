// policy rollouts (azg_policy_rollout / azg_policy_rollout_ex, include/azgym_eval.h): the group kernel's instantiations, the choice of
// the form and the C ABI entries (the team form's kernel and launches: dispatch_rollout_team.hip)
#include <cstring>

#include "engine_host.h"
#include "rollout.cuh"

// The group form.  Widths up to 256 (padded): NREG as the search keeps this network's hidden->hidden layers (e->nreg: 0 streams them);
// 512 and 1024: the weight-streaming form (any depth, LayerNorm, six inputs, every activation).
// LDS at 1024: two activation buffers 128 KB + the head partials 16 KB + 1.1 KB, mlp_eval_kernel's plan plus a word, of the CU's 160 KB.
static hipError_t dispatch_rollout(azg_engine* e, const Rollout& ro) {
    const int NR = e->nreg;
    switch (e->HP) {
        case 64: return NR == 1 ? rollout_launch<64, 1>(e, ro) : NR == 2 ? rollout_launch<64, 2>(e, ro) : rollout_launch<64, 0>(e, ro);
        case 128: return NR == 1 ? rollout_launch<128, 1>(e, ro) : NR == 2 ? rollout_launch<128, 2>(e, ro) : rollout_launch<128, 0>(e, ro);
        case 256: return NR == 1 ? rollout_launch<256, 1>(e, ro) : rollout_launch<256, 0>(e, ro);
        case 512: return rollout_launch<512, 0>(e, ro);
        case 1024: return rollout_launch<1024, 0>(e, ro);
    }
    return hipErrorInvalidValue;
}

// The one place where a rollout's form is chosen.  Team: a lock-step shaped net (the tile weight layout and the VALU first layer exist
// for it), AZG_LS_TEAM not 0 (the switch that also sends searches to the per-layer launches), and no team rollout of this engine has
// given up before (ro_team_off: the rollouts' own flag -- opt.ls_team stays the search's).  Everything else: group.
static bool rollout_wants_team(const azg_engine* e) {
    return azg_lockstep_shaped(e->HP, e->n_hidden, e->P.layernorm != 0, e->S_obs) && e->opt.ls_team && !e->ro_team_off;
}

// the body of both entries; wide: padded widths >= 512 are served (azg_policy_rollout_ex)
static int policy_rollout(azg_engine* e, const azg_rollout_config* c, double* returns, int32_t* lengths, int32_t* terminated, float* first_value,
                          bool wide, azg_rollout_info* info) {
    if (!e) return AZG_E_INVALID;
    if (!c || !returns || !lengths) return fail(e, AZG_E_INVALID, "azg_policy_rollout: cfg, returns and lengths must not be NULL");
    if (c->struct_size != (int32_t)sizeof(azg_rollout_config)) return fail(e, AZG_E_INVALID, "azg_rollout_config size mismatch");
    if (info && info->struct_size != (int32_t)sizeof(azg_rollout_info)) return fail(e, AZG_E_INVALID, "azg_rollout_info size mismatch");
    if (c->episodes_per_net < 1 || c->max_episode_length < 1)
        return fail(e, AZG_E_INVALID, "azg_policy_rollout: episodes_per_net and max_episode_length must be >= 1");
    if (c->action_rule != AZG_ROLLOUT_MODE && c->action_rule != AZG_ROLLOUT_SAMPLE) return fail(e, AZG_E_INVALID, "azg_policy_rollout: unknown action_rule");
    if (!e->mlp_ready) return fail(e, AZG_E_STATE, "azg_policy_rollout: every net needs weights (azg_set_weights / azg_set_net_weights)");
    if (e->HP >= 512 && !wide)
        return fail(e, AZG_E_UNSUPPORTED, "azg_policy_rollout: networks wider than 256 (padded) are not supported (azg_policy_rollout_ex takes them)");
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
    int form = AZG_ROLLOUT_FORM_GROUP, launches = 0;
    unsigned* abort_word = nullptr;
    if (rollout_wants_team(e)) {
        const hipError_t rc = azg_rollout_team(e, ro, &launches, &abort_word);
        if (rc == hipSuccess) form = AZG_ROLLOUT_FORM_TEAM;
        else if (rc != hipErrorNotReady) return fail(e, AZG_E_DEVICE, std::string("team rollout launch: ") + hipGetErrorString(rc));
    }
    e->rollout_stage.resize(bytes + 4);
    char* h = e->rollout_stage.data();
    unsigned gave_up = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (form == AZG_ROLLOUT_FORM_GROUP) {
            const hipError_t rc = dispatch_rollout(e, ro);
            if (rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string("rollout kernel launch: ") + hipGetErrorString(rc));
            launches += 1;
        } else {
            HIPCHK(e, hipMemcpyAsync(h + bytes, abort_word, 4, hipMemcpyDeviceToHost, e->stream));
        }
        HIPCHK(e, hipMemcpyAsync(h, e->d_rollout, bytes, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (form == AZG_ROLLOUT_FORM_GROUP) break;
        memcpy(&gave_up, h + bytes, 4);
        if (!gave_up) break;
        // a wait of the team kernel timed out (its workgroups were not all resident): every workgroup left and nothing it wrote counts.
        // The whole call is replayed in the group form, which this engine's rollouts take from now on.
        e->ro_team_off = 1;
        e->ro_team_fallbacks += 1;
        form = AZG_ROLLOUT_FORM_GROUP;
    }
    memcpy(returns, h, N * 8);
    memcpy(lengths, h + N * 8, N * 4);
    if (terminated) memcpy(terminated, h + N * 12, N * 4);
    if (first_value) memcpy(first_value, h + N * 16, N * 4);
    if (info) { info->form = form; info->launches = launches; info->team_fallbacks = e->ro_team_fallbacks; }
    return AZG_OK;
}

extern "C" int azg_policy_rollout(azg_engine* e, const azg_rollout_config* c, double* returns, int32_t* lengths, int32_t* terminated,
                                  float* first_value) {
    return policy_rollout(e, c, returns, lengths, terminated, first_value, false, nullptr);
}

extern "C" int azg_policy_rollout_ex(azg_engine* e, const azg_rollout_config* c, double* returns, int32_t* lengths, int32_t* terminated,
                                     float* first_value, azg_rollout_info* info) {
    return policy_rollout(e, c, returns, lengths, terminated, first_value, true, info);
}
