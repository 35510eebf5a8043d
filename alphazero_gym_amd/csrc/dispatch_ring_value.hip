// the replay ring's bootstrap values from the value head (azg_selfplay_refresh_values, include/azgym_refresh.h): the kernel's
// instantiations and the C ABI entry (the kernel, its launch and its grid rule: ring_value.cuh)
#include "engine_host.h"
#include "ring_value.cuh"
#include "../../include/azgym_refresh.h"

// population_eval's instantiations: NREG as the search keeps this network's hidden->hidden layers at widths up to 256 (e->nreg: 0 streams
// them); 512 and 1024: the weight-streaming form
static hipError_t dispatch_ring_value(azg_engine* e, const RingValue& rv, int* groups) {
    const int NR = e->nreg;
    switch (e->HP) {
        case 64: return NR == 1 ? ring_value_launch<64, 1>(e, rv, groups) : NR == 2 ? ring_value_launch<64, 2>(e, rv, groups) : ring_value_launch<64, 0>(e, rv, groups);
        case 128: return NR == 1 ? ring_value_launch<128, 1>(e, rv, groups) : NR == 2 ? ring_value_launch<128, 2>(e, rv, groups) : ring_value_launch<128, 0>(e, rv, groups);
        case 256: return NR == 1 ? ring_value_launch<256, 1>(e, rv, groups) : ring_value_launch<256, 0>(e, rv, groups);
        case 512: return ring_value_launch<512, 0>(e, rv, groups);
        case 1024: return ring_value_launch<1024, 0>(e, rv, groups);
    }
    return hipErrorInvalidValue;
}

extern "C" int azg_selfplay_refresh_values(azg_engine* e, const int32_t* slots, int32_t n_slots) {
    if (!e) return AZG_E_INVALID;
    ReplayRing& r = e->ring;
    // every refusal comes before the staging is touched and before anything is launched
    if (!r.on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!r.tr.on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_transitions has not been called: the stored steps' values were not kept");
    if (!e->mlp_ready) return fail(e, AZG_E_STATE, "azg_selfplay_refresh_values: every net needs weights in the set in use (azg_set_weights / azg_set_net_weights)");
    if (slots && n_slots < 0) return fail(e, AZG_E_INVALID, "azg_selfplay_refresh_values: n_slots must be >= 0");
    for (int32_t i = 0; slots && i < n_slots; ++i)
        if (slots[i] < 0 || slots[i] >= r.steps)
            return fail(e, AZG_E_INVALID, "azg_selfplay_refresh_values: slot " + std::to_string(slots[i]) + " is not a stored step (size_steps " + std::to_string(r.steps) + ")");
    if (e->n_nets > 65535) return fail(e, AZG_E_UNSUPPORTED, "azg_selfplay_refresh_values: n_nets <= 65535");
    const size_t n = slots ? (size_t)n_slots : (size_t)r.steps;
    if (n == 0) return AZG_OK;
    ON_DEVICE(e);
    RingValue rv;
    rv.rows = r.rows; rv.value = r.tr.value; rv.slots = nullptr; rv.n_slots = n;
    rv.B = e->cfg.n_trees; rv.T = e->cfg.n_trees / e->n_nets; rv.row_len = r.row; rv.S_obs = e->S_obs;
    if (slots) {
        ReplayRing::ValueRefresh& st = r.refresh;
        if (st.cap < n) {   // (grow-only: a launch in flight may still read the smaller one, which goes with the next begin)
            int* d = nullptr;
            if (dalloc(e, r.mem, &d, n)) return AZG_E_DEVICE;
            st.d = d; st.cap = n;
        }
        if (!r.slots_copied) HIPCHK(e, hipEventCreateWithFlags(&r.slots_copied, hipEventDisableTiming));
        else HIPCHK(e, hipEventSynchronize(r.slots_copied));   // (the last call's copy has read the host side: it may be rewritten)
        st.h.assign(slots, slots + n);
        HIPCHK(e, hipMemcpyAsync(st.d, st.h.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipEventRecord(r.slots_copied, e->stream));
        rv.slots = st.d;
    }
    int groups = 0;
    const hipError_t rc = dispatch_ring_value(e, rv, &groups);
    if (rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string("ring_value kernel launch: ") + hipGetErrorString(rc));
    return AZG_OK;
}
