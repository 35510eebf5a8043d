// engine_selfplay.hip -- the C ABI's device-resident self-play (azg_selfplay_*, azg_population_selfplay_begin), the reanalysis of its
// replay ring (azgym_reanalyse.h), the ring's n-step return targets (azgym_nstep.h), its prioritised sampling (azgym_priority.h), the
// search rollouts (azgym_search_rollout.h) and the launches of the small kernels after a search: results_kernel, the self-play step,
// the reanalysis' gather and row kernels, the n-step target kernel, the priority, scan and draw kernels and the search rollouts' step
// (aux_kernels.cuh and priority.cuh are compiled in this unit only).
#include <cmath>
#include <cstring>

#include "engine_host.h"
#include "../../include/azgym_reanalyse.h"
#include "../../include/azgym_nstep.h"
#include "../../include/azgym_priority.h"
#include "../../include/azgym_search_rollout.h"
#include "mlp.cuh"
#include "aux_kernels.cuh"
#include "priority.cuh"

int launch_results(azg_engine* e) {
    if (!e->searched) return fail(e, AZG_E_STATE, "no search has run");
    if (e->results_valid) return AZG_OK;
    { int trc = settle_team(e); if (trc) return trc; }
    int B = e->cfg.n_trees;
    hipLaunchKernelGGL(results_kernel, dim3((B + RS_TREES - 1) / RS_TREES), dim3(16 * RS_TREES), 0, e->stream, e->P);
    HIPCHK(e, hipGetLastError());
    e->results_valid = 1;   // (in stream order: whatever reads the buffers is ordered after this launch)
    return AZG_OK;
}

// The final-action rule's settings, as azg_selfplay_config and azg_search_rollout_config carry them: what both refuse
static int act_rule_refusal(azg_engine* e, int final_selection, double temperature, double agent_epsilon) {
    if (final_selection != AZG_FS_MAX_VISIT && final_selection != AZG_FS_MAX_VALUE) return fail(e, AZG_E_INVALID, "unknown final_selection");
    if (!(temperature > 0.0)) return fail(e, AZG_E_INVALID, "temperature must be > 0");
    if (agent_epsilon < 0.0 || agent_epsilon > 1.0) return fail(e, AZG_E_INVALID, "agent_epsilon must be in [0, 1]");
    if (e->cfg.mode == AZG_MODE_DISCRETE && final_selection == AZG_FS_MAX_VALUE && temperature != 1.0)
        return fail(e, AZG_E_UNSUPPORTED, "final_selection max_value on the device supports temperature 1 only");
    return AZG_OK;
}

// Discrete mode with temperature != 1: stable_normalizer (helpers.py:10-27) raises x / max(x) to the temperature: (c / m)^t for every
// pair of a root edge count c and the root's largest count m that can occur, python float pow = libm pow on the host (like check_pw's
// table), at [m (m + 1) / 2 + c].  Empty (and AZG_OK) where the rule needs no table.
static int act_rule_ctab(azg_engine* e, double temperature, std::vector<double>& tab) {
    tab.clear();
    if (e->cfg.mode != AZG_MODE_DISCRETE || temperature == 1.0) return AZG_OK;
    const size_t ns = (size_t)e->cfg.n_sims;
    if (ns > 2048) return fail(e, AZG_E_UNSUPPORTED, "temperature != 1 on the device supports n_sims <= 2048");
    tab.assign((ns + 1) * (ns + 2) / 2, 0.0);
    for (size_t m = 1; m <= ns; ++m)
        for (size_t k = 0; k <= m; ++k) tab[m * (m + 1) / 2 + k] = std::pow((double)k / (double)m, temperature);
    return AZG_OK;
}

extern "C" {

int azg_selfplay_row_len(const azg_engine* e) { return e ? e->S_obs + 3 * e->Kmax + 1 : AZG_E_INVALID; }

// Common body of azg_selfplay_begin_ex and azg_population_selfplay_begin.  A population's games are its trees: net k plays games
// k*T .. k*T+T-1 (global ids tree_id_base + k*T + j), and the self-play kernels work per tree on what the search returned, so the
// steps, rows, ring and stats are those of an engine of one net.
static int selfplay_begin_impl(azg_engine* e, const azg_selfplay_config* c) {
    if (c->struct_size != (int32_t)sizeof(azg_selfplay_config)) return fail(e, AZG_E_INVALID, "azg_selfplay_config size mismatch");
    if (c->max_episode_length < 1 || c->capacity_steps < 1) return fail(e, AZG_E_INVALID, "max_episode_length and capacity_steps must be >= 1");
    if (c->final_selection != AZG_FS_MAX_VISIT && c->final_selection != AZG_FS_MAX_VALUE) return fail(e, AZG_E_INVALID, "unknown final_selection");
    if (c->ring_mode != AZG_RING_STOP && c->ring_mode != AZG_RING_FIFO) return fail(e, AZG_E_INVALID, "unknown ring_mode");
    { int rrc = act_rule_refusal(e, c->final_selection, c->temperature, c->agent_epsilon); if (rrc) return rrc; }
    const bool discrete = e->cfg.mode == AZG_MODE_DISCRETE;
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->sp_mem.clear();
    e->sp_on = 0;
    e->d_sp_states = e->d_sp_states_mem = nullptr;   // (azg_selfplay_keep_states is asked for again after every begin)
    e->sp_tr_on = 0;                                 // (azg_selfplay_keep_transitions too)
    e->d_sp_tr_reward = e->d_sp_tr_value = nullptr; e->d_sp_tr_action = nullptr; e->d_sp_tr_end = nullptr;
    e->sp_prio_on = 0;                               // (azg_selfplay_keep_priorities too)
    e->d_sp_prio_q = e->d_sp_prio_within = e->d_sp_prio_seg = nullptr; e->d_sp_prio_given = nullptr; e->d_sp_prio_slots = nullptr;
    e->d_sp_isw = nullptr; e->d_sp_isw_min = nullptr;
    e->sp_rows_gen += 1; e->sp_prio_gen = -1; e->sp_isw_gen = -1;
    const size_t B = e->cfg.n_trees;
    e->sp_row = e->S_obs + 3 * e->Kmax + 1;
    if (dalloc(e, e->sp_mem, &e->d_sp_t, B) || dalloc(e, e->sp_mem, &e->d_sp_episode, B) || dalloc(e, e->sp_mem, &e->d_sp_fcnt, B) ||
        dalloc(e, e->sp_mem, &e->d_sp_ret, B) || dalloc(e, e->sp_mem, &e->d_sp_fsum, B) ||
        dalloc(e, e->sp_mem, &e->d_sp_rows, (size_t)c->capacity_steps * B * e->sp_row))
        return AZG_E_DEVICE;
    e->d_sp_ctab = nullptr;
    {
        std::vector<double> tab;
        int trc = act_rule_ctab(e, c->temperature, tab);
        if (trc) return trc;
        if (!tab.empty()) {
            if (dalloc(e, e->sp_mem, &e->d_sp_ctab, tab.size())) return AZG_E_DEVICE;
            HIPCHK(e, hipMemcpy(e->d_sp_ctab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        }
    }
    HIPCHK(e, hipMemset(e->d_sp_t, 0, B * 4));
    HIPCHK(e, hipMemset(e->d_sp_episode, 0, B * 4));
    HIPCHK(e, hipMemset(e->d_sp_fcnt, 0, B * 4));
    HIPCHK(e, hipMemset(e->d_sp_ret, 0, B * 8));
    HIPCHK(e, hipMemset(e->d_sp_fsum, 0, B * 8));
    std::vector<double> roots(B * e->S_env);
    azg_synthetic_roots(e, roots.data());
    HIPCHK(e, hipMemcpy(e->d_roots, roots.data(), roots.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemset(e->d_carry, 0, B * 4));
    e->carry_max = discrete ? e->cfg.n_sims : 0;   // a reused root carries its node count as a child: at most n_sims
    e->sp_on = 1; e->sp_max_len = c->max_episode_length; e->sp_det = c->deterministic; e->sp_cap = c->capacity_steps; e->sp_steps = 0;
    e->sp_insert = 0; e->sp_total = 0; e->sp_fs = c->final_selection; e->sp_ring = c->ring_mode; e->sp_agent_eps = c->agent_epsilon;
    e->sp_step_idx = 0;
    return AZG_OK;
}

int azg_selfplay_begin_ex(azg_engine* e, const azg_selfplay_config* c) {
    if (!e || !c) return AZG_E_INVALID;
    if (e->n_nets > 1)
        return fail(e, AZG_E_UNSUPPORTED, "device self-play of a population (azg_set_population > 1) starts with azg_population_selfplay_begin");
    return selfplay_begin_impl(e, c);
}

int azg_population_selfplay_begin(azg_engine* e, const azg_selfplay_config* c) {
    if (!e || !c) return AZG_E_INVALID;
    return selfplay_begin_impl(e, c);
}

int azg_selfplay_begin(azg_engine* e, int32_t max_episode_length, int32_t deterministic, int32_t capacity_steps) {
    azg_selfplay_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = (int32_t)sizeof(c);
    c.max_episode_length = max_episode_length; c.deterministic = deterministic; c.capacity_steps = capacity_steps;
    c.final_selection = AZG_FS_MAX_VISIT; c.ring_mode = AZG_RING_STOP; c.temperature = 1.0; c.agent_epsilon = 0.0;
    return azg_selfplay_begin_ex(e, &c);
}

int azg_selfplay_step(azg_engine* e) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (e->sp_ring == AZG_RING_STOP && e->sp_steps >= e->sp_cap) return fail(e, AZG_E_STATE, "replay ring is full: download and clear the rows");
    // selfplay_kernel (roots with more than 16 children) knows the continuous final-action rule only: a discrete engine has its env's
    // 2 or 3 actions per node (azg_engine_create), so this cannot happen
    if (e->Kmax > 16 && e->cfg.mode != AZG_MODE_CONTINUOUS)
        return fail(e, AZG_E_STATE, "device self-play with more than 16 actions per node supports continuous mode only");
    int rc = azg_search_resident(e);
    if (rc) return rc;
    ON_DEVICE(e);
    rc = settle_team(e);   // (wide networks: the persistent team kernel may have given up)
    if (rc) return rc;
    // ReplayBuffer.store (buffers.py:75-82) for this step's block of n_trees rows
    int slot;
    if (e->sp_steps < e->sp_cap) { slot = e->sp_steps; e->sp_steps += 1; }
    else { slot = e->sp_insert; e->sp_insert = (e->sp_insert + 1) % e->sp_steps; }
    SelfPlay sp;
    sp.max_len = e->sp_max_len; sp.S_obs = e->S_obs;
    sp.rule.deterministic = e->sp_det; sp.rule.final_selection = e->sp_fs; sp.rule.agent_eps = e->sp_agent_eps; sp.rule.ctab = e->d_sp_ctab;
    sp.rule.step_idx = e->sp_step_idx;
    sp.t = e->d_sp_t; sp.episode = e->d_sp_episode; sp.fcnt = e->d_sp_fcnt; sp.ret = e->d_sp_ret; sp.fsum = e->d_sp_fsum;
    sp.rows = e->d_sp_rows + (size_t)slot * e->cfg.n_trees * e->sp_row;
    sp.states = e->d_sp_states ? e->d_sp_states + (size_t)slot * e->cfg.n_trees * e->S_env : nullptr;
    sp.roots = e->d_roots; sp.carry = e->d_carry;
    const int B = e->cfg.n_trees;
    const size_t tr_at = (size_t)slot * B;
    sp.tr_reward = e->sp_tr_on ? e->d_sp_tr_reward + tr_at : nullptr; sp.tr_value = e->sp_tr_on ? e->d_sp_tr_value + tr_at : nullptr;
    sp.tr_action = e->sp_tr_on ? e->d_sp_tr_action + tr_at : nullptr; sp.tr_end = e->sp_tr_on ? e->d_sp_tr_end + tr_at : nullptr;
    e->redo_ok = 0;   // (the step moves the roots on: the search that just ran cannot be re-run for a dump)
    if (e->Kmax <= 16) {
        rc = launch_results(e);   // return_results of this search (a launch only after the lock-step / team kernels)
        if (rc) return rc;
        hipLaunchKernelGGL(selfplay_kernel16, dim3((B + SP_TREES - 1) / SP_TREES), dim3(16 * SP_TREES), 0, e->stream, e->P, sp);
    } else {
        hipLaunchKernelGGL(selfplay_kernel, dim3((B + SPW_THREADS - 1) / SPW_THREADS), dim3(SPW_THREADS), 0, e->stream, e->P, sp);   // (reads the trees)
    }
    HIPCHK(e, hipGetLastError());
    e->sp_total += 1;
    e->sp_step_idx += 1;
    e->sp_rows_gen += 1;
    return AZG_OK;
}

int azg_selfplay_rows(azg_engine* e, float* rows, size_t max_rows, int32_t clear) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t n = (size_t)e->sp_steps * e->cfg.n_trees;
    if (n > max_rows) n = max_rows;
    if (rows && n) HIPCHK(e, hipMemcpy(rows, e->d_sp_rows, n * e->sp_row * 4, hipMemcpyDeviceToHost));
    if (clear) { e->sp_steps = 0; e->sp_insert = 0; e->sp_rows_gen += 1; }   // ReplayBuffer.clear (buffers.py:56-60)
    return (int)n;
}

int azg_selfplay_ring(azg_engine* e, int32_t* size_steps, int32_t* insert_step, int64_t* total_steps) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (size_steps) *size_steps = e->sp_steps;
    if (insert_step) *insert_step = e->sp_insert;
    if (total_steps) *total_steps = e->sp_total;
    return AZG_OK;
}

int azg_selfplay_rows_device(azg_engine* e, void** device_ptr, size_t* capacity_rows, size_t* row_len) {
    if (!e || !device_ptr) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    *device_ptr = e->d_sp_rows;
    if (capacity_rows) *capacity_rows = (size_t)e->sp_cap * e->cfg.n_trees;
    if (row_len) *row_len = (size_t)e->sp_row;
    return AZG_OK;
}

int azg_selfplay_stats(azg_engine* e, double* fsum, int32_t* fcnt, double* env_state) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t B = e->cfg.n_trees;
    D2H(fsum, e->d_sp_fsum, B * 8);
    D2H(fcnt, e->d_sp_fcnt, B * 4);
    D2H(env_state, e->d_roots, B * e->S_env * 8);
    return AZG_OK;
}

// ---- reanalysis (include/azgym_reanalyse.h)

int azg_selfplay_keep_states(azg_engine* e, int32_t on) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (e->sp_steps != 0) return fail(e, AZG_E_STATE, "azg_selfplay_keep_states: the replay ring is not empty (call it right after begin, or after clearing the rows)");
    if (!on) { e->d_sp_states = nullptr; return AZG_OK; }   // (the memory goes with the next begin)
    if (e->d_sp_states) return AZG_OK;
    ON_DEVICE(e);
    const size_t B = e->cfg.n_trees, S = e->S_env;
    if (!e->d_sp_states_mem &&   // (switched off and on again within one begin: the ring is still there)
        (dalloc(e, e->sp_mem, &e->d_sp_states_mem, (size_t)e->sp_cap * B * S) || dalloc(e, e->sp_mem, &e->d_ra_roots, B * S) ||
         dalloc(e, e->sp_mem, &e->d_ra_carry, B) || dalloc(e, e->sp_mem, &e->d_ra_slots, B))) {
        e->d_sp_states_mem = nullptr;
        return AZG_E_DEVICE;
    }
    e->d_sp_states = e->d_sp_states_mem;
    return AZG_OK;
}

int azg_selfplay_states(azg_engine* e, double* states, size_t max_rows) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->d_sp_states) return fail(e, AZG_E_STATE, "azg_selfplay_keep_states has not been called");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t n = (size_t)e->sp_steps * e->cfg.n_trees;
    if (n > max_rows) n = max_rows;
    if (states && n) HIPCHK(e, hipMemcpy(states, e->d_sp_states, n * e->S_env * 8, hipMemcpyDeviceToHost));
    return (int)n;
}

int azg_selfplay_reanalyse(azg_engine* e, const int32_t* slots, int32_t slot, uint32_t search_index) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->d_sp_states) return fail(e, AZG_E_STATE, "azg_selfplay_keep_states has not been called: the stored positions' env states were not kept");
    const int B = e->cfg.n_trees;
    for (int t = 0; t < (slots ? B : 1); ++t) {
        const int s = slots ? slots[t] : slot;
        if (s < 0 || s >= e->sp_steps) return fail(e, AZG_E_INVALID, "azg_selfplay_reanalyse: slot " + std::to_string(s) + " is not a stored step (size_steps " + std::to_string(e->sp_steps) + ")");
    }
    if (e->Kmax > 16 && e->cfg.mode != AZG_MODE_CONTINUOUS)   // (as azg_selfplay_step: cannot happen)
        return fail(e, AZG_E_STATE, "device self-play with more than 16 actions per node supports continuous mode only");
    int rc = search_refusal(e);
    if (rc) return rc;
    ON_DEVICE(e);
    rc = settle_team(e);   // (an abandoned team search is redone on the roots it was started with, before this one's take their place)
    if (rc) return rc;
    Reanalyse ra;
    ra.slots = nullptr; ra.slot = slot; ra.S_obs = e->S_obs;
    ra.states = e->d_sp_states; ra.rows = e->d_sp_rows; ra.roots = e->d_ra_roots; ra.carry = e->d_ra_carry;
    ra.tr_value = e->sp_tr_on ? e->d_sp_tr_value : nullptr;
    if (slots) {
        e->ra_slots.assign(slots, slots + B);
        HIPCHK(e, hipMemcpyAsync(e->d_ra_slots, e->ra_slots.data(), (size_t)B * 4, hipMemcpyHostToDevice, e->stream));
        ra.slots = e->d_ra_slots;
    }
    hipLaunchKernelGGL(reanalyse_gather_kernel, dim3((B + RA_THREADS - 1) / RA_THREADS), dim3(RA_THREADS), 0, e->stream, e->P, ra);
    HIPCHK(e, hipGetLastError());
    // One ordinary search from the staging roots (fresh roots: no carried count) under search_index.  The live games' roots and
    // carried counts are not touched -- the kernels read KParams' pointers -- and the running search index comes back; an abandoned
    // team search is redone while the staging roots are still the engine's.
    const double* const live_roots = e->P.roots;
    const int* const live_carry = e->P.carry;
    const int live_carry_max = e->carry_max;
    const uint32_t idx_now = e->search_idx;
    e->P.roots = e->d_ra_roots; e->P.carry = e->d_ra_carry; e->carry_max = 0; e->search_idx = search_index;
    rc = azg_search_resident(e);
    if (!rc) rc = settle_team(e);
    e->P.roots = live_roots; e->P.carry = live_carry; e->carry_max = live_carry_max; e->search_idx = idx_now;
    if (rc) return rc;
    e->redo_ok = 0;   // (the roots are the live games' again: the search that just ran cannot be re-run for a dump)
    if (e->Kmax <= 16) {
        rc = launch_results(e);
        if (rc) return rc;
        hipLaunchKernelGGL(reanalyse_kernel16, dim3((B + SP_TREES - 1) / SP_TREES), dim3(16 * SP_TREES), 0, e->stream, e->P, ra);
    } else {
        hipLaunchKernelGGL(reanalyse_kernel, dim3((B + SPW_THREADS - 1) / SPW_THREADS), dim3(SPW_THREADS), 0, e->stream, e->P, ra);   // (reads the trees)
    }
    HIPCHK(e, hipGetLastError());
    return AZG_OK;
}

// ---- n-step return targets (include/azgym_nstep.h)

int azg_selfplay_keep_transitions(azg_engine* e, int32_t on) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (e->sp_steps != 0) return fail(e, AZG_E_STATE, "azg_selfplay_keep_transitions: the replay ring is not empty (call it right after begin, or after clearing the rows)");
    if (!on) { e->sp_tr_on = 0; return AZG_OK; }   // (the memory goes with the next begin)
    if (e->sp_tr_on) return AZG_OK;
    ON_DEVICE(e);
    const size_t n = (size_t)e->sp_cap * e->cfg.n_trees;
    if (!e->d_sp_tr_reward &&   // (switched off and on again within one begin: the blocks are still there)
        (dalloc(e, e->sp_mem, &e->d_sp_tr_reward, n) || dalloc(e, e->sp_mem, &e->d_sp_tr_value, n) ||
         dalloc(e, e->sp_mem, &e->d_sp_tr_action, n) || dalloc(e, e->sp_mem, &e->d_sp_tr_end, n))) {
        e->d_sp_tr_reward = nullptr;
        return AZG_E_DEVICE;
    }
    e->sp_tr_on = 1;
    return AZG_OK;
}

int azg_selfplay_transitions(azg_engine* e, double* reward, double* value, float* action, int32_t* end, size_t max_rows) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_tr_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_transitions has not been called");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t n = (size_t)e->sp_steps * e->cfg.n_trees;
    if (n > max_rows) n = max_rows;
    if (n) {
        D2H(reward, e->d_sp_tr_reward, n * 8);
        D2H(value, e->d_sp_tr_value, n * 8);
        D2H(action, e->d_sp_tr_action, n * 4);
        D2H(end, e->d_sp_tr_end, n * 4);
    }
    return (int)n;
}

int azg_selfplay_nstep_targets(azg_engine* e, const azg_nstep_config* c) {
    if (!e) return AZG_E_INVALID;
    if (!c) return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: cfg must not be NULL");
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_tr_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_transitions has not been called: the stored steps' rewards and ends were not kept");
    if (c->struct_size != (int32_t)sizeof(azg_nstep_config)) return fail(e, AZG_E_INVALID, "azg_nstep_config size mismatch");
    if (c->n_step < 0) return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: n_step must be >= 0");
    if (c->flags & ~(int32_t)AZG_NSTEP_SEARCH_GAMMA) return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: unknown flag bits (AZG_NSTEP_SEARCH_GAMMA is the only flag)");
    const bool search_gamma = (c->flags & AZG_NSTEP_SEARCH_GAMMA) != 0;
    if (!search_gamma && !(c->gamma >= 0.0 && std::isfinite(c->gamma)))
        return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: gamma must be finite and >= 0 (or set AZG_NSTEP_SEARCH_GAMMA)");
    if (e->sp_steps == 0) return AZG_OK;
    ON_DEVICE(e);
    NStep ns;
    ns.B = e->cfg.n_trees; ns.T = e->cfg.n_trees / e->n_nets;
    // ReplayBuffer.store's order: while the ring fills, slot 0 holds the oldest step (and the insert index is 0); once it overwrites,
    // the oldest step is the next one to go, at the insert index
    ns.size = e->sp_steps; ns.oldest = e->sp_insert;
    ns.n_step = c->n_step < e->sp_steps ? c->n_step : e->sp_steps;
    ns.row_len = e->sp_row; ns.vcol = e->sp_row - 1;
    ns.gamma = search_gamma ? e->cfg.gamma : c->gamma;
    ns.nets = search_gamma ? e->net_search.rec : nullptr;
    ns.reward = e->d_sp_tr_reward; ns.value = e->d_sp_tr_value; ns.end = e->d_sp_tr_end; ns.rows = e->d_sp_rows;
    const long long rows = (long long)ns.size * ns.B;
    hipLaunchKernelGGL(nstep_targets_kernel, dim3((unsigned)((rows + NS_THREADS - 1) / NS_THREADS)), dim3(NS_THREADS), 0, e->stream, ns);
    HIPCHK(e, hipGetLastError());
    return AZG_OK;
}

// ---- prioritised sampling (include/azgym_priority.h)

int azg_selfplay_keep_priorities(azg_engine* e, int32_t on) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!on) { e->sp_prio_on = 0; e->sp_prio_gen = -1; e->sp_isw_gen = -1; return AZG_OK; }   // (the memory goes with the next begin)
    if (e->sp_prio_on) return AZG_OK;
    const size_t n = (size_t)e->sp_cap * e->cfg.n_trees;
    if (n >= ((size_t)1 << 31)) return fail(e, AZG_E_UNSUPPORTED, "azg_selfplay_keep_priorities: capacity_steps * n_trees must stay below 2^31 rows");
    ON_DEVICE(e);
    // every net's last segment may be partial: at most one segment more per net than the rows fill, and a net has at least one game
    const size_t segs = n / PR_SEG + (size_t)e->cfg.n_trees + 1;
    if (!e->d_sp_prio_q &&   // (switched off and on again within one begin: the blocks are still there)
        (dalloc(e, e->sp_mem, &e->d_sp_prio_q, n) || dalloc(e, e->sp_mem, &e->d_sp_prio_within, n) ||
         dalloc(e, e->sp_mem, &e->d_sp_prio_seg, segs) || dalloc(e, e->sp_mem, &e->d_sp_prio_given, n) ||
         dalloc(e, e->sp_mem, &e->d_sp_prio_slots, (size_t)e->cfg.n_trees))) {
        e->d_sp_prio_q = nullptr;
        return AZG_E_DEVICE;
    }
    e->sp_prio_segs = segs;
    e->sp_prio_on = 1; e->sp_prio_gen = -1;
    return AZG_OK;
}

int azg_selfplay_priorities(azg_engine* e, const azg_priority_config* c) {
    if (!e) return AZG_E_INVALID;
    if (!c) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: cfg must not be NULL");
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_prio_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_priorities has not been called");
    if (c->struct_size != (int32_t)sizeof(azg_priority_config)) return fail(e, AZG_E_INVALID, "azg_priority_config size mismatch");
    if (c->source != AZG_PRIO_VALUE_GAP && c->source != AZG_PRIO_GIVEN) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: unknown source");
    if (c->source == AZG_PRIO_VALUE_GAP && !e->sp_tr_on)
        return fail(e, AZG_E_STATE, "azg_selfplay_priorities: AZG_PRIO_VALUE_GAP needs azg_selfplay_keep_transitions: the stored steps' search values were not kept");
    if (!(c->alpha >= 0.0f && std::isfinite(c->alpha))) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: alpha must be finite and >= 0");
    if (!(c->eps > 0.0f && std::isfinite(c->eps))) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: eps must be finite and > 0");
    const size_t n = (size_t)e->sp_steps * e->cfg.n_trees;
    if (c->source == AZG_PRIO_GIVEN) {
        if (!c->given) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: AZG_PRIO_GIVEN needs the given array");
        for (size_t i = 0; i < n; ++i)
            if (!(c->given[i] >= 0.0f)) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: given[" + std::to_string(i) + "] is negative or NaN");
    }
    e->sp_isw_gen = -1;   // (weights computed from the priorities before these are no longer handed out)
    if (n == 0) { e->sp_prio_gen = e->sp_rows_gen; return AZG_OK; }
    ON_DEVICE(e);
    Priorities pr;
    pr.rows_n = (long long)n; pr.source = c->source;
    pr.row_len = e->sp_row; pr.vcol = e->sp_row - 1;
    pr.alpha = c->alpha; pr.eps = c->eps;
    pr.value = e->d_sp_tr_value; pr.rows = e->d_sp_rows; pr.given = e->d_sp_prio_given; pr.q = e->d_sp_prio_q;
    if (c->source == AZG_PRIO_GIVEN) {
        e->prio_given.assign(c->given, c->given + n);
        HIPCHK(e, hipMemcpyAsync(e->d_sp_prio_given, e->prio_given.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    }
    hipLaunchKernelGGL(priorities_kernel, dim3((unsigned)((n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, e->stream, pr);
    HIPCHK(e, hipGetLastError());
    e->sp_prio_gen = e->sp_rows_gen;
    return AZG_OK;
}

int azg_selfplay_priority_values(azg_engine* e, uint64_t* q, size_t max_rows) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_prio_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_priorities has not been called");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t n = (size_t)e->sp_steps * e->cfg.n_trees;
    if (n > max_rows) n = max_rows;
    if (n) D2H(q, e->d_sp_prio_q, n * 8);
    return (int)n;
}

// What both draws refuse: no begin, no keep_priorities, priorities older than the ring's set of stored rows, an empty ring
static int sample_refusal(azg_engine* e, const char* who) {
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_prio_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_priorities has not been called");
    if (e->sp_prio_gen != e->sp_rows_gen)
        return fail(e, AZG_E_STATE, std::string(who) + ": azg_selfplay_priorities has not run since the ring's stored rows last changed (a step, a clear or a begin)");
    if (e->sp_steps == 0) return fail(e, AZG_E_STATE, std::string(who) + ": the replay ring is empty");
    return AZG_OK;
}

int azg_selfplay_sample_rows(azg_engine* e, const azg_sample_config* c, int32_t* order) {
    if (!e) return AZG_E_INVALID;
    if (!c || !order) return fail(e, AZG_E_INVALID, "azg_selfplay_sample_rows: cfg and order must not be NULL");
    if (c->struct_size != (int32_t)sizeof(azg_sample_config)) return fail(e, AZG_E_INVALID, "azg_sample_config size mismatch");
    if (c->n_order < 1) return fail(e, AZG_E_INVALID, "azg_selfplay_sample_rows: n_order must be >= 1");
    int rc = sample_refusal(e, "azg_selfplay_sample_rows");
    if (rc) return rc;
    const int K = e->n_nets;
    PrioScan ps;
    ps.B = e->cfg.n_trees; ps.T = e->cfg.n_trees / K;
    ps.N = e->sp_steps * ps.T; ps.nseg = (ps.N + PR_SEG - 1) / PR_SEG;
    ps.q = e->d_sp_prio_q; ps.within = e->d_sp_prio_within; ps.seg = e->d_sp_prio_seg;
    if ((size_t)K * ps.nseg > e->sp_prio_segs || K * ps.T != ps.B)   // (the population was changed after keep_priorities)
        return fail(e, AZG_E_STATE, "azg_selfplay_sample_rows: the population changed since azg_selfplay_keep_priorities");
    ON_DEVICE(e);
    const size_t out_n = (size_t)K * c->n_order;
    if (!e->sp_order_buf.reserve(out_n * 4)) return fail(e, AZG_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e->sp_order_buf.last));
    hipLaunchKernelGGL(prio_scan_segments_kernel, dim3(ps.nseg, K), dim3(PR_THREADS), 0, e->stream, ps);
    HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(prio_scan_totals_kernel, dim3(K), dim3(64), 0, e->stream, ps);
    HIPCHK(e, hipGetLastError());
    PrioRows dr;
    dr.ps = ps; dr.n_order = c->n_order; dr.sample_index = c->sample_index; dr.tree_base = (unsigned)e->cfg.tree_id_base;
    dr.seed = e->cfg.seed; dr.order = (int*)e->sp_order_buf.p;
    hipLaunchKernelGGL(prio_draw_rows_kernel, dim3((c->n_order + PR_THREADS - 1) / PR_THREADS, K), dim3(PR_THREADS), 0, e->stream, dr);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(order, dr.order, out_n * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AZG_OK;
}

int azg_selfplay_sample_slots(azg_engine* e, uint32_t sample_index, int32_t* slots) {
    if (!e) return AZG_E_INVALID;
    if (!slots) return fail(e, AZG_E_INVALID, "azg_selfplay_sample_slots: slots must not be NULL");
    int rc = sample_refusal(e, "azg_selfplay_sample_slots");
    if (rc) return rc;
    ON_DEVICE(e);
    const int B = e->cfg.n_trees;
    PrioSlots dr;
    dr.B = B; dr.size = e->sp_steps; dr.sample_index = sample_index; dr.tree_base = (unsigned)e->cfg.tree_id_base;
    dr.seed = e->cfg.seed; dr.q = e->d_sp_prio_q; dr.slots = e->d_sp_prio_slots;
    hipLaunchKernelGGL(prio_draw_slots_kernel, dim3((B + PR_THREADS - 1) / PR_THREADS), dim3(PR_THREADS), 0, e->stream, dr);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(slots, dr.slots, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AZG_OK;
}

// ---- importance-sampling weights of the stored rows (include/azgym_priority.h)

int azg_selfplay_is_weights(azg_engine* e, float beta) {
    if (!e) return AZG_E_INVALID;
    int rc = sample_refusal(e, "azg_selfplay_is_weights");
    if (rc) return rc;
    if (!(beta >= 0.0f && std::isfinite(beta))) return fail(e, AZG_E_INVALID, "azg_selfplay_is_weights: beta must be finite and >= 0");
    const int K = e->n_nets;
    PrioMin pm;
    pm.B = e->cfg.n_trees; pm.T = e->cfg.n_trees / K;
    pm.N = e->sp_steps * pm.T; pm.nseg = (pm.N + PR_SEG - 1) / PR_SEG;
    if ((size_t)K * pm.nseg > e->sp_prio_segs || K * pm.T != pm.B)   // (the population was changed after keep_priorities)
        return fail(e, AZG_E_STATE, "azg_selfplay_is_weights: the population changed since azg_selfplay_keep_priorities");
    ON_DEVICE(e);
    if (!e->d_sp_isw) {   // one block: the minima (uint64) in front of the weights, so a failure leaves nothing behind
        const size_t n_min = e->sp_prio_segs + (size_t)e->cfg.n_trees, n_w = (size_t)e->sp_cap * e->cfg.n_trees;
        unsigned long long* block = nullptr;
        if (dalloc(e, e->sp_mem, &block, n_min + (n_w + 1) / 2)) return AZG_E_DEVICE;
        e->d_sp_isw_min = block; e->d_sp_isw = reinterpret_cast<float*>(block + n_min);
    }
    pm.q = e->d_sp_prio_q; pm.seg_min = e->d_sp_isw_min; pm.net_min = e->d_sp_isw_min + e->sp_prio_segs;
    hipLaunchKernelGGL(prio_min_segments_kernel, dim3(pm.nseg, K), dim3(PR_THREADS), 0, e->stream, pm);
    HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(prio_min_nets_kernel, dim3(K), dim3(64), 0, e->stream, pm);
    HIPCHK(e, hipGetLastError());
    IsWeights iw;
    iw.rows_n = (long long)e->sp_steps * pm.B; iw.B = pm.B; iw.T = pm.T; iw.beta = beta;
    iw.q = e->d_sp_prio_q; iw.net_min = pm.net_min; iw.w = e->d_sp_isw;
    hipLaunchKernelGGL(is_weights_kernel, dim3((unsigned)((iw.rows_n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, e->stream, iw);
    HIPCHK(e, hipGetLastError());
    e->sp_isw_gen = e->sp_rows_gen;
    return AZG_OK;
}

int azg_selfplay_is_weights_device(azg_engine* e, const float** w) {
    if (!e) return AZG_E_INVALID;
    if (!w) return fail(e, AZG_E_INVALID, "azg_selfplay_is_weights_device: w must not be NULL");
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_prio_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_priorities has not been called");
    if (!e->d_sp_isw || e->sp_isw_gen != e->sp_rows_gen)
        return fail(e, AZG_E_STATE, "azg_selfplay_is_weights_device: azg_selfplay_is_weights has not run since the ring's stored rows or their priorities last changed");
    *w = e->d_sp_isw;
    return AZG_OK;
}

int azg_selfplay_is_weight_values(azg_engine* e, float* w, size_t max_rows) {
    if (!e) return AZG_E_INVALID;
    if (!e->sp_on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if (!e->sp_prio_on) return fail(e, AZG_E_STATE, "azg_selfplay_keep_priorities has not been called");
    if (!e->d_sp_isw) return fail(e, AZG_E_STATE, "azg_selfplay_is_weight_values: azg_selfplay_is_weights has not been called");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t n = (size_t)e->sp_steps * e->cfg.n_trees;
    if (n > max_rows) n = max_rows;
    if (n) D2H(w, e->d_sp_isw, n * 4);
    return (int)n;
}

// ---- search rollouts (include/azgym_search_rollout.h)

// The steps of azg_search_rollout, with the evaluation's roots in place of the engine's: one ordinary search per step under search
// index index_base + s, then the step kernel; the count of unfinished games is read every poll_steps steps.
static int search_rollout_steps(azg_engine* e, const azg_search_rollout_config* c, SearchRollout& sr, int* steps, int* polls) {
    const int B = e->cfg.n_trees;
    const long long bound = (long long)c->episodes_per_game * c->max_episode_length;
    for (long long s = 0; s < bound; ++s) {
        e->search_idx = c->index_base + (uint32_t)s;
        int rc = azg_search_resident(e);
        if (!rc) rc = settle_team(e);   // (wide networks: the persistent team kernel may have given up)
        if (rc) return rc;
        sr.rule.step_idx = c->index_base + (uint32_t)s;
        if (e->Kmax <= 16) {
            rc = launch_results(e);
            if (rc) return rc;
            hipLaunchKernelGGL(search_rollout_kernel16, dim3((B + SP_TREES - 1) / SP_TREES), dim3(16 * SP_TREES), 0, e->stream, e->P, sr);
        } else {
            hipLaunchKernelGGL(search_rollout_kernel, dim3((B + SPW_THREADS - 1) / SPW_THREADS), dim3(SPW_THREADS), 0, e->stream, e->P, sr);   // (reads the trees)
        }
        HIPCHK(e, hipGetLastError());
        *steps += 1;
        if ((s + 1) % c->poll_steps == 0 && s + 1 < bound) {
            int left = 0;
            HIPCHK(e, hipMemcpyAsync(&left, sr.unfinished, 4, hipMemcpyDeviceToHost, e->stream));
            HIPCHK(e, hipStreamSynchronize(e->stream));
            *polls += 1;
            if (left == 0) break;
        }
    }
    return AZG_OK;
}

int azg_search_rollout(azg_engine* e, const azg_search_rollout_config* c, double* returns, int32_t* lengths, int32_t* terminated,
                       azg_search_rollout_info* info) {
    if (!e) return AZG_E_INVALID;
    if (!c || !returns || !lengths) return fail(e, AZG_E_INVALID, "azg_search_rollout: cfg, returns and lengths must not be NULL");
    if (c->struct_size != (int32_t)sizeof(azg_search_rollout_config)) return fail(e, AZG_E_INVALID, "azg_search_rollout_config size mismatch");
    if (info && info->struct_size != (int32_t)sizeof(azg_search_rollout_info)) return fail(e, AZG_E_INVALID, "azg_search_rollout_info size mismatch");
    if (c->episodes_per_game < 1 || c->max_episode_length < 1 || c->poll_steps < 1)
        return fail(e, AZG_E_INVALID, "episodes_per_game, max_episode_length and poll_steps must be >= 1");
    if ((long long)c->episodes_per_game * c->max_episode_length > (1LL << 30))
        return fail(e, AZG_E_INVALID, "episodes_per_game * max_episode_length must be at most 2^30 steps");
    int rc = act_rule_refusal(e, c->final_selection, c->temperature, c->agent_epsilon);
    if (rc) return rc;
    std::vector<double> tab;
    rc = act_rule_ctab(e, c->temperature, tab);
    if (rc) return rc;
    if (e->Kmax > 16 && e->cfg.mode != AZG_MODE_CONTINUOUS)   // (as azg_selfplay_step: cannot happen)
        return fail(e, AZG_E_STATE, "search rollouts with more than 16 actions per node support continuous mode only");
    rc = search_refusal(e);
    if (rc) return rc;
    ON_DEVICE(e);
    rc = settle_team(e);   // (an abandoned team search is redone on the roots it was started with, before the evaluation's take their place)
    if (rc) return rc;
    // evaluation state and outputs in one block that only grows: float64 parts first
    const size_t B = e->cfg.n_trees, S = e->S_env, E = c->episodes_per_game;
    const size_t o_roots = 0, o_ret = o_roots + B * S * 8, o_returns = o_ret + B * 8, o_lengths = o_returns + B * E * 8,
                 o_term = o_lengths + B * E * 4, o_carry = o_term + B * E * 4, o_t = o_carry + B * 4, o_ep = o_t + B * 4, o_left = o_ep + B * 4,
                 bytes = o_left + 16;
    if (!e->sr_buf.reserve(bytes)) return fail(e, AZG_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e->sr_buf.last));
    if (!tab.empty()) {
        if (!e->sr_ctab.reserve(tab.size() * 8)) return fail(e, AZG_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e->sr_ctab.last));
        HIPCHK(e, hipMemcpy(e->sr_ctab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    }
    char* const base = (char*)e->sr_buf.p;
    SearchRollout sr;
    sr.max_len = c->max_episode_length; sr.E = (int)E; sr.T = (int)(B / e->n_nets);
    sr.game_id_base = c->game_id_base; sr.episode = c->episode;
    sr.rule.deterministic = c->deterministic; sr.rule.final_selection = c->final_selection; sr.rule.agent_eps = c->agent_epsilon;
    sr.rule.ctab = tab.empty() ? nullptr : (const double*)e->sr_ctab.p; sr.rule.step_idx = c->index_base;
    sr.roots = (double*)(base + o_roots); sr.ret = (double*)(base + o_ret); sr.returns = (double*)(base + o_returns);
    sr.lengths = (int*)(base + o_lengths); sr.terminated = (int*)(base + o_term); sr.carry = (int*)(base + o_carry);
    sr.t = (int*)(base + o_t); sr.ep = (int*)(base + o_ep); sr.unfinished = (int*)(base + o_left);
    hipLaunchKernelGGL(search_rollout_init_kernel, dim3(((int)B + SR_THREADS - 1) / SR_THREADS), dim3(SR_THREADS), 0, e->stream, e->P, sr);
    HIPCHK(e, hipGetLastError());
    // Ordinary searches from the evaluation's roots and carried counts.  The live games' are not touched -- the kernels read KParams'
    // pointers -- and the running search index comes back on every path; an abandoned team search is redone while the evaluation's
    // roots are still the engine's.
    const double* const live_roots = e->P.roots;
    const int* const live_carry = e->P.carry;
    const int live_carry_max = e->carry_max;
    const uint32_t idx_now = e->search_idx;
    e->P.roots = sr.roots; e->P.carry = sr.carry;
    e->carry_max = e->cfg.mode == AZG_MODE_DISCRETE ? e->cfg.n_sims : 0;   // (as self-play: a reused root carries at most n_sims)
    int steps = 0, polls = 0;
    rc = search_rollout_steps(e, c, sr, &steps, &polls);
    e->P.roots = live_roots; e->P.carry = live_carry; e->carry_max = live_carry_max; e->search_idx = idx_now;
    if (steps) e->redo_ok = 0;   // (the roots are the live games' again: the search that just ran cannot be re-run for a dump)
    if (rc) { (void)hipStreamSynchronize(e->stream); return rc; }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(returns, sr.returns, B * E * 8, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(lengths, sr.lengths, B * E * 4, hipMemcpyDeviceToHost));
    D2H(terminated, sr.terminated, B * E * 4);
    if (info) { info->steps = steps; info->polls = polls; }
    return AZG_OK;
}

}  // extern "C"
