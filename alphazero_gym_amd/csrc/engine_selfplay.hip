// engine_selfplay.hip -- the C ABI's device-resident self-play (azg_selfplay_*, azg_population_selfplay_begin), the reanalysis of its
// replay ring (azgym_reanalyse.h), the ring's n-step and lambda-return targets (azgym_nstep.h, azgym_lambda.h), its prioritised sampling (azgym_priority.h), the
// search rollouts (azgym_search_rollout.h) and the launches of the small kernels after a search: results_kernel, the self-play step,
// the reanalysis' gather and row kernels, the n-step and lambda target kernels, the priority, scan, draw and error-maximum kernels and the search rollouts' step
// (aux_kernels.cuh and priority.cuh are compiled in this unit only).  The ring is the engine's one ReplayRing (replay_ring.h); what its
// entry points share stands once, in front of them: their refusals, the row-aligned download, the keep_* calls' allocate-once, the
// per-net partition, the launch after a search and the scoped swap of the engine's roots (reanalysis, search rollouts).
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "engine_host.h"
#include "../../include/azgym_reanalyse.h"
#include "../../include/azgym_nstep.h"
#include "../../include/azgym_lambda.h"
#include "../../include/azgym_priority.h"
#include "../../include/azgym_search_rollout.h"
#include "mlp.cuh"
#include "aux_kernels.cuh"
#include "priority.cuh"
#include "priority_online.cuh"
#include "online_ring.h"

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

// After a search, the kernel that works on its outcome: roots of at most 16 children are read from return_results' arrays (a launch
// of their own only after the lock-step / team kernels), wider roots from the trees
template <typename A>
static int launch_after_search(azg_engine* e, void (*kernel16)(KParams, A), void (*kernel_wide)(KParams, A), const A& a) {
    const int B = e->cfg.n_trees;
    if (e->Kmax <= 16) {
        int rc = launch_results(e);
        if (rc) return rc;
        hipLaunchKernelGGL(kernel16, dim3((B + SP_TREES - 1) / SP_TREES), dim3(16 * SP_TREES), 0, e->stream, e->P, a);
    } else {
        hipLaunchKernelGGL(kernel_wide, dim3((B + SPW_THREADS - 1) / SPW_THREADS), dim3(SPW_THREADS), 0, e->stream, e->P, a);
    }
    HIPCHK(e, hipGetLastError());
    return AZG_OK;
}

// While one lives the engine searches from staging roots with their carried counts, under another search index.  The live games' are
// not touched -- the kernels read KParams' pointers -- and they, carry_max and the running search index come back when the scope ends,
// on every path.  (An abandoned team search is redone inside the scope, while the staging roots are still the engine's.)
struct RootSwap {
    azg_engine* const e;
    const double* const roots; const int* const carry; const int carry_max; const uint32_t search_idx;   // the live values
    RootSwap(azg_engine* e_, const double* r, const int* c, int cmax, uint32_t index)
        : e(e_), roots(e_->P.roots), carry(e_->P.carry), carry_max(e_->carry_max), search_idx(e_->search_idx) {
        e->P.roots = r; e->P.carry = c; e->carry_max = cmax; e->search_idx = index;
    }
    RootSwap(const RootSwap&) = delete;
    ~RootSwap() { e->P.roots = roots; e->P.carry = carry; e->carry_max = carry_max; e->search_idx = search_idx; }
};

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

// ---- what the ring's entry points share

// What a ring entry point refuses first: no engine, no begin, a column of `need` not kept (`why`: what the entry point adds to that)
enum { NEED_STATES = 1, NEED_TRANSITIONS = 2, NEED_PRIORITIES = 4, NEED_ERRORS = 8 };
static int ring_refusal(azg_engine* e, int need = 0, const char* why = "") {
    if (!e) return AZG_E_INVALID;
    const ReplayRing& r = e->ring;
    if (!r.on) return fail(e, AZG_E_STATE, "azg_selfplay_begin has not been called");
    if ((need & NEED_STATES) && !r.states.on) return fail(e, AZG_E_STATE, std::string("azg_selfplay_keep_states has not been called") + why);
    if ((need & NEED_TRANSITIONS) && !r.tr.on) return fail(e, AZG_E_STATE, std::string("azg_selfplay_keep_transitions has not been called") + why);
    if ((need & NEED_PRIORITIES) && !r.prio.on) return fail(e, AZG_E_STATE, std::string("azg_selfplay_keep_priorities has not been called") + why);
    if ((need & NEED_ERRORS) && !r.prio.err_on) return fail(e, AZG_E_STATE, std::string("azg_selfplay_keep_errors has not been called") + why);
    return AZG_OK;
}

// What both draws and the weights refuse: no begin, no keep_priorities, priorities older than the ring's set of stored rows, an empty ring
static int sample_refusal(azg_engine* e, const char* who) {
    if (int rc = ring_refusal(e, NEED_PRIORITIES)) return rc;
    if (e->ring.prio.gen != e->ring.rows_gen)
        return fail(e, AZG_E_STATE, std::string(who) + ": azg_selfplay_priorities has not run since the ring's stored rows last changed (a step, a clear or a begin)");
    if (e->ring.steps == 0) return fail(e, AZG_E_STATE, std::string(who) + ": the replay ring is empty");
    return AZG_OK;
}

// The row-aligned downloads: once the stream is idle, the first n rows of every column that has a destination, n the stored rows or
// max_rows if that is fewer.  Returns n.
struct RingColumn { void* dst; const void* src; size_t row_bytes; };
static int ring_download(azg_engine* e, size_t max_rows, std::initializer_list<RingColumn> columns) {
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t n = e->ring.stored_rows();
    if (n > max_rows) n = max_rows;
    for (const RingColumn& c : columns)
        if (c.dst && n) HIPCHK(e, hipMemcpy(c.dst, c.src, n * c.row_bytes, hipMemcpyDeviceToHost));
    return (int)n;
}

// What the keep_* calls do alike: switched off, the column keeps its memory (it goes with the next begin); switched on, `alloc` (true:
// it failed) fills the column's pointers, *first among them, unless the memory of an earlier switch-on within this begin is still there
template <typename T, typename Alloc>
static int keep_column(azg_engine* e, int32_t on, int* flag, T** first, Alloc alloc) {
    if (!on) { *flag = 0; return AZG_OK; }
    if (*flag) return AZG_OK;
    ON_DEVICE(e);
    if (!*first && alloc()) { *first = nullptr; return AZG_E_DEVICE; }
    *flag = 1;
    return AZG_OK;
}
static int nonempty_ring_refusal(azg_engine* e, const char* who) {   // (keep_states, keep_transitions: a column holds every stored step or none)
    if (e->ring.steps == 0) return AZG_OK;
    return fail(e, AZG_E_STATE, std::string(who) + ": the replay ring is not empty (call it right after begin, or after clearing the rows)");
}

// The stored rows net by net, into the B, T, N and nseg of a PrioScan / PrioMin (priority.cuh).  The refusal cannot fire:
// azg_set_population refuses while self-play is on and a begin drops the priorities, so n_nets is what azg_selfplay_keep_priorities
// saw -- and it divides n_trees, and n_nets * nseg <= capacity * n_trees / PR_SEG + n_nets <= segs, whatever n_nets <= n_trees is.
// It stays as the bound of the scratch the kernels write.
template <typename Part>
static int ring_partition(azg_engine* e, const char* who, Part* p) {
    const int K = e->n_nets;
    p->B = e->cfg.n_trees; p->T = e->cfg.n_trees / K;
    p->N = e->ring.steps * p->T; p->nseg = (p->N + PR_SEG - 1) / PR_SEG;
    if ((size_t)K * p->nseg > e->ring.prio.segs || K * p->T != p->B)
        return fail(e, AZG_E_STATE, std::string(who) + ": the population changed since azg_selfplay_keep_priorities");
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
    if (c->ring_mode != AZG_RING_STOP && c->ring_mode != AZG_RING_FIFO) return fail(e, AZG_E_INVALID, "unknown ring_mode");
    if (int rc = act_rule_refusal(e, c->final_selection, c->temperature, c->agent_epsilon)) return rc;
    const bool discrete = e->cfg.mode == AZG_MODE_DISCRETE;
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    ReplayRing& r = e->ring;
    r.restart();   // (every kept column goes too: the azg_selfplay_keep_* calls are made again after every begin)
    const size_t B = e->cfg.n_trees;
    r.B = (int)B; r.cap = c->capacity_steps; r.row = e->S_obs + 3 * e->Kmax + 1; r.mode = c->ring_mode;
    r.max_len = c->max_episode_length; r.det = c->deterministic; r.fs = c->final_selection; r.agent_eps = c->agent_epsilon;
    if (dalloc(e, r.mem, &r.t, B) || dalloc(e, r.mem, &r.episode, B) || dalloc(e, r.mem, &r.fcnt, B) || dalloc(e, r.mem, &r.ret, B) ||
        dalloc(e, r.mem, &r.fsum, B) || dalloc(e, r.mem, &r.rows, (size_t)r.cap * B * r.row))
        return AZG_E_DEVICE;
    {
        std::vector<double> tab;
        if (int trc = act_rule_ctab(e, c->temperature, tab)) return trc;
        if (!tab.empty()) {
            if (dalloc(e, r.mem, &r.ctab, tab.size())) return AZG_E_DEVICE;
            HIPCHK(e, hipMemcpy(r.ctab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        }
    }
    HIPCHK(e, hipMemset(r.t, 0, B * 4));
    HIPCHK(e, hipMemset(r.episode, 0, B * 4));
    HIPCHK(e, hipMemset(r.fcnt, 0, B * 4));
    HIPCHK(e, hipMemset(r.ret, 0, B * 8));
    HIPCHK(e, hipMemset(r.fsum, 0, B * 8));
    std::vector<double> roots(B * e->S_env);
    azg_synthetic_roots(e, roots.data());
    HIPCHK(e, hipMemcpy(e->d_roots, roots.data(), roots.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemset(e->d_carry, 0, B * 4));
    e->carry_max = discrete ? e->cfg.n_sims : 0;   // a reused root carries its node count as a child: at most n_sims
    r.on = 1;
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
    if (int rc = ring_refusal(e)) return rc;
    ReplayRing& r = e->ring;
    if (r.mode == AZG_RING_STOP && r.steps >= r.cap) return fail(e, AZG_E_STATE, "replay ring is full: download and clear the rows");
    // selfplay_kernel (roots with more than 16 children) knows the continuous final-action rule only: a discrete engine has its env's
    // 2 or 3 actions per node (azg_engine_create), so this cannot happen
    if (e->Kmax > 16 && e->cfg.mode != AZG_MODE_CONTINUOUS)
        return fail(e, AZG_E_STATE, "device self-play with more than 16 actions per node supports continuous mode only");
    int rc = azg_search_resident(e);
    if (rc) return rc;
    ON_DEVICE(e);
    rc = settle_team(e);   // (wide networks: the persistent team kernel may have given up)
    if (rc) return rc;
    const size_t at = (size_t)r.store_slot() * e->cfg.n_trees;   // where this step's block of n_trees rows goes
    SelfPlay sp;
    sp.max_len = r.max_len; sp.S_obs = e->S_obs;
    sp.rule.deterministic = r.det; sp.rule.final_selection = r.fs; sp.rule.agent_eps = r.agent_eps; sp.rule.ctab = r.ctab;
    sp.rule.step_idx = r.step_idx;
    sp.t = r.t; sp.episode = r.episode; sp.fcnt = r.fcnt; sp.ret = r.ret; sp.fsum = r.fsum;
    sp.rows = r.rows + at * r.row;
    sp.states = r.states.on ? r.states.d + at * e->S_env : nullptr;
    sp.roots = e->d_roots; sp.carry = e->d_carry;
    sp.tr_reward = r.tr.on ? r.tr.reward + at : nullptr; sp.tr_value = r.tr.on ? r.tr.value + at : nullptr;
    sp.tr_action = r.tr.on ? r.tr.action + at : nullptr; sp.tr_end = r.tr.on ? r.tr.end + at : nullptr;
    e->redo_ok = 0;   // (the step moves the roots on: the search that just ran cannot be re-run for a dump)
    rc = launch_after_search(e, selfplay_kernel16, selfplay_kernel, sp);
    if (rc) return rc;
    // kept errors (azg_selfplay_keep_errors): the rows of this slot have not been trained on
    if (r.prio.err_on) HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)(r.prio.err + at), (int)PR_ERR_UNSEEN_BITS, (size_t)e->cfg.n_trees, e->stream));
    r.stepped();
    return AZG_OK;
}

int azg_selfplay_rows(azg_engine* e, float* rows, size_t max_rows, int32_t clear) {
    if (int rc = ring_refusal(e)) return rc;
    const int n = ring_download(e, max_rows, {{rows, e->ring.rows, (size_t)e->ring.row * 4}});
    if (n >= 0 && clear) e->ring.clear_rows();
    return n;
}

int azg_selfplay_ring(azg_engine* e, int32_t* size_steps, int32_t* insert_step, int64_t* total_steps) {
    if (int rc = ring_refusal(e)) return rc;
    if (size_steps) *size_steps = e->ring.steps;
    if (insert_step) *insert_step = e->ring.insert;
    if (total_steps) *total_steps = e->ring.total;
    return AZG_OK;
}

int azg_selfplay_rows_device(azg_engine* e, void** device_ptr, size_t* capacity_rows, size_t* row_len) {
    if (!e || !device_ptr) return AZG_E_INVALID;
    if (int rc = ring_refusal(e)) return rc;
    *device_ptr = e->ring.rows;
    if (capacity_rows) *capacity_rows = (size_t)e->ring.cap * e->cfg.n_trees;
    if (row_len) *row_len = (size_t)e->ring.row;
    return AZG_OK;
}

int azg_selfplay_stats(azg_engine* e, double* fsum, int32_t* fcnt, double* env_state) {
    if (int rc = ring_refusal(e)) return rc;
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    size_t B = e->cfg.n_trees;
    D2H(fsum, e->ring.fsum, B * 8);
    D2H(fcnt, e->ring.fcnt, B * 4);
    D2H(env_state, e->d_roots, B * e->S_env * 8);
    return AZG_OK;
}

// ---- reanalysis (include/azgym_reanalyse.h)

int azg_selfplay_keep_states(azg_engine* e, int32_t on) {
    if (int rc = ring_refusal(e)) return rc;
    if (int rc = nonempty_ring_refusal(e, "azg_selfplay_keep_states")) return rc;
    ReplayRing& r = e->ring;
    ReplayRing::States& st = r.states;
    return keep_column(e, on, &st.on, &st.d, [&] {
        const size_t B = e->cfg.n_trees, S = e->S_env;
        return dalloc(e, r.mem, &st.d, (size_t)r.cap * B * S) || dalloc(e, r.mem, &st.roots, B * S) || dalloc(e, r.mem, &st.carry, B) ||
               dalloc(e, r.mem, &st.slots, B);
    });
}

int azg_selfplay_states(azg_engine* e, double* states, size_t max_rows) {
    if (int rc = ring_refusal(e, NEED_STATES)) return rc;
    return ring_download(e, max_rows, {{states, e->ring.states.d, (size_t)e->S_env * 8}});
}

int azg_selfplay_reanalyse(azg_engine* e, const int32_t* slots, int32_t slot, uint32_t search_index) {
    if (int rc = ring_refusal(e, NEED_STATES, ": the stored positions' env states were not kept")) return rc;
    ReplayRing& r = e->ring;
    const int B = e->cfg.n_trees;
    for (int t = 0; t < (slots ? B : 1); ++t) {
        const int s = slots ? slots[t] : slot;
        if (s < 0 || s >= r.steps) return fail(e, AZG_E_INVALID, "azg_selfplay_reanalyse: slot " + std::to_string(s) + " is not a stored step (size_steps " + std::to_string(r.steps) + ")");
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
    ra.states = r.states.d; ra.rows = r.rows; ra.roots = r.states.roots; ra.carry = r.states.carry;
    ra.tr_value = r.tr.on ? r.tr.value : nullptr;
    if (slots) {
        r.states.h_slots.assign(slots, slots + B);
        HIPCHK(e, hipMemcpyAsync(r.states.slots, r.states.h_slots.data(), (size_t)B * 4, hipMemcpyHostToDevice, e->stream));
        ra.slots = r.states.slots;
    }
    hipLaunchKernelGGL(reanalyse_gather_kernel, dim3((B + RA_THREADS - 1) / RA_THREADS), dim3(RA_THREADS), 0, e->stream, e->P, ra);
    HIPCHK(e, hipGetLastError());
    {   // one ordinary search from the staging roots (fresh roots: no carried count) under search_index
        RootSwap staged(e, r.states.roots, r.states.carry, 0, search_index);
        rc = azg_search_resident(e);
        if (!rc) rc = settle_team(e);
    }
    if (rc) return rc;
    e->redo_ok = 0;   // (the roots are the live games' again: the search that just ran cannot be re-run for a dump)
    return launch_after_search(e, reanalyse_kernel16, reanalyse_kernel, ra);
}

// ---- n-step return targets (include/azgym_nstep.h)

int azg_selfplay_keep_transitions(azg_engine* e, int32_t on) {
    if (int rc = ring_refusal(e)) return rc;
    if (int rc = nonempty_ring_refusal(e, "azg_selfplay_keep_transitions")) return rc;
    ReplayRing& r = e->ring;
    ReplayRing::Transitions& tr = r.tr;
    return keep_column(e, on, &tr.on, &tr.reward, [&] {
        const size_t n = (size_t)r.cap * e->cfg.n_trees;
        return dalloc(e, r.mem, &tr.reward, n) || dalloc(e, r.mem, &tr.value, n) || dalloc(e, r.mem, &tr.action, n) || dalloc(e, r.mem, &tr.end, n);
    });
}

int azg_selfplay_transitions(azg_engine* e, double* reward, double* value, float* action, int32_t* end, size_t max_rows) {
    if (int rc = ring_refusal(e, NEED_TRANSITIONS)) return rc;
    const ReplayRing::Transitions& tr = e->ring.tr;
    return ring_download(e, max_rows, {{reward, tr.reward, 8}, {value, tr.value, 8}, {action, tr.action, 4}, {end, tr.end, 4}});
}

int azg_selfplay_nstep_targets(azg_engine* e, const azg_nstep_config* c) {
    if (!e) return AZG_E_INVALID;
    if (!c) return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: cfg must not be NULL");
    if (int rc = ring_refusal(e, NEED_TRANSITIONS, ": the stored steps' rewards and ends were not kept")) return rc;
    if (c->struct_size != (int32_t)sizeof(azg_nstep_config)) return fail(e, AZG_E_INVALID, "azg_nstep_config size mismatch");
    if (c->n_step < 0) return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: n_step must be >= 0");
    if (c->flags & ~(int32_t)AZG_NSTEP_SEARCH_GAMMA) return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: unknown flag bits (AZG_NSTEP_SEARCH_GAMMA is the only flag)");
    const bool search_gamma = (c->flags & AZG_NSTEP_SEARCH_GAMMA) != 0;
    if (!search_gamma && !(c->gamma >= 0.0 && std::isfinite(c->gamma)))
        return fail(e, AZG_E_INVALID, "azg_selfplay_nstep_targets: gamma must be finite and >= 0 (or set AZG_NSTEP_SEARCH_GAMMA)");
    const ReplayRing& r = e->ring;
    if (r.steps == 0) return AZG_OK;
    ON_DEVICE(e);
    NStep ns;
    ns.B = e->cfg.n_trees; ns.T = e->cfg.n_trees / e->n_nets;
    // ReplayBuffer.store's order: while the ring fills, slot 0 holds the oldest step (and the insert index is 0); once it overwrites,
    // the oldest step is the next one to go, at the insert index
    ns.size = r.steps; ns.oldest = r.insert;
    ns.n_step = c->n_step < r.steps ? c->n_step : r.steps;
    ns.row_len = r.row; ns.vcol = r.row - 1;
    ns.gamma = search_gamma ? e->cfg.gamma : c->gamma;
    ns.nets = search_gamma ? e->net_search.rec : nullptr;
    ns.reward = r.tr.reward; ns.value = r.tr.value; ns.end = r.tr.end; ns.rows = r.rows;
    const long long rows = (long long)ns.size * ns.B;
    hipLaunchKernelGGL(nstep_targets_kernel, dim3((unsigned)((rows + NS_THREADS - 1) / NS_THREADS)), dim3(NS_THREADS), 0, e->stream, ns);
    HIPCHK(e, hipGetLastError());
    return AZG_OK;
}

// ---- lambda-return targets (include/azgym_lambda.h)

// Both calls: entry k of `rules` is net k's rule, or rules[0] every net's (one: azg_selfplay_lambda_targets).  Everything is refused
// before the table's host side is touched; then one copy and one launch on the engine's stream.
static int lambda_targets(azg_engine* e, const azg_return_rule* rules, bool one, const char* who_) {
    if (!e) return AZG_E_INVALID;
    const std::string who = who_;
    if (!rules) return fail(e, AZG_E_INVALID, who + ": the rule must not be NULL");
    if (int rc = ring_refusal(e, NEED_TRANSITIONS, ": the stored steps' rewards and ends were not kept")) return rc;
    const int K = e->n_nets;
    for (int k = 0; k < (one ? 1 : K); ++k) {
        const azg_return_rule& c = rules[k];
        const std::string net = one ? who + ": " : who + ": net " + std::to_string(k) + ": ";
        if (k > 0 && c.struct_size != rules[0].struct_size)
            return fail(e, AZG_E_INVALID, who + ": struct_size of net " + std::to_string(k) + " differs from net 0's (it must be equal in every entry)");
        if (c.struct_size != (int32_t)sizeof(azg_return_rule)) return fail(e, AZG_E_INVALID, net + "azg_return_rule size mismatch");
        if (k > 0 && c.flags != rules[0].flags)
            return fail(e, AZG_E_INVALID, who + ": flags of net " + std::to_string(k) + " differs from net 0's (it must be equal in every entry)");
        if (c.n_step < 0) return fail(e, AZG_E_INVALID, net + "n_step must be >= 0");
        if (c.flags & ~(int32_t)AZG_NSTEP_SEARCH_GAMMA) return fail(e, AZG_E_INVALID, net + "unknown flag bits (AZG_NSTEP_SEARCH_GAMMA is the only flag)");
        if (!(c.lambda >= 0.0 && c.lambda <= 1.0)) return fail(e, AZG_E_INVALID, net + "lambda must be in [0, 1]");
        if (!(c.flags & AZG_NSTEP_SEARCH_GAMMA) && !(c.gamma >= 0.0 && std::isfinite(c.gamma)))
            return fail(e, AZG_E_INVALID, net + "gamma must be finite and >= 0 (or set AZG_NSTEP_SEARCH_GAMMA)");
    }
    ReplayRing& r = e->ring;
    if (r.steps == 0) return AZG_OK;
    ON_DEVICE(e);
    const bool search_gamma = (rules[0].flags & AZG_NSTEP_SEARCH_GAMMA) != 0;
    // the search's gammas: per net where a table is set (the host keeps them beside it), azg_config's otherwise
    const bool per_net = search_gamma && e->net_search.rec;
    if (per_net && (int)e->net_search_gamma.size() != K) return fail(e, AZG_E_STATE, who + ": the per-net search table was not set completely (azg_set_net_search failed)");
    ReplayRing::ReturnRules& t = r.rules;
    if (t.n < K) {
        ReturnRuleRec* d = nullptr;
        if (dalloc(e, r.mem, &d, (size_t)K)) return AZG_E_DEVICE;
        t.d = d; t.n = K;
    }
    if (!r.rules_copied) HIPCHK(e, hipEventCreateWithFlags(&r.rules_copied, hipEventDisableTiming));
    else HIPCHK(e, hipEventSynchronize(r.rules_copied));   // (the last call's copy has read the host side: it may be rewritten)
    t.h.resize(K);
    for (int k = 0; k < K; ++k) {
        const azg_return_rule& c = rules[one ? 0 : k];
        ReturnRuleRec& rec = t.h[k];
        rec.n_step = c.n_step < r.steps ? c.n_step : r.steps;   // (a longer window cannot reach further)
        rec.pad = 0;
        rec.lambda = c.lambda; rec.om = 1.0 - c.lambda;
        rec.gamma = !search_gamma ? c.gamma : per_net ? e->net_search_gamma[k] : e->cfg.gamma;
    }
    HIPCHK(e, hipMemcpyAsync(t.d, t.h.data(), (size_t)K * sizeof(ReturnRuleRec), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipEventRecord(r.rules_copied, e->stream));
    LambdaTargets lt;
    lt.B = e->cfg.n_trees; lt.T = e->cfg.n_trees / K;
    lt.size = r.steps; lt.oldest = r.insert;   // (as azg_selfplay_nstep_targets)
    lt.row_len = r.row; lt.vcol = r.row - 1;
    lt.rules = t.d;
    lt.reward = r.tr.reward; lt.value = r.tr.value; lt.end = r.tr.end; lt.rows = r.rows;
    const long long rows = (long long)lt.size * lt.B;
    hipLaunchKernelGGL(lambda_targets_kernel, dim3((unsigned)((rows + NS_THREADS - 1) / NS_THREADS)), dim3(NS_THREADS), 0, e->stream, lt);
    HIPCHK(e, hipGetLastError());
    return AZG_OK;
}

int azg_selfplay_lambda_targets(azg_engine* e, const azg_return_rule* rule) { return lambda_targets(e, rule, true, "azg_selfplay_lambda_targets"); }

int azg_selfplay_lambda_targets_nets(azg_engine* e, const azg_return_rule* rules) { return lambda_targets(e, rules, false, "azg_selfplay_lambda_targets_nets"); }

// ---- prioritised sampling (include/azgym_priority.h)

int azg_selfplay_keep_priorities(azg_engine* e, int32_t on) {   // (at any ring size: the priorities are computed on demand)
    if (int rc = ring_refusal(e)) return rc;
    ReplayRing& r = e->ring;
    ReplayRing::Priorities& p = r.prio;
    if (!on) { p.gen = p.w_gen = -1; p.err_on = 0; }   // (so a switch-on finds gen -1: what was computed before is not handed out)
    const size_t B = e->cfg.n_trees, n = (size_t)r.cap * B;
    if (on && !p.on && n >= ((size_t)1 << 31)) return fail(e, AZG_E_UNSUPPORTED, "azg_selfplay_keep_priorities: capacity_steps * n_trees must stay below 2^31 rows");
    return keep_column(e, on, &p.on, &p.q, [&] {
        // every net's last segment may be partial: at most one segment more per net than the rows fill, and a net has at least one game
        p.segs = n / PR_SEG + B + 1;
        return dalloc(e, r.mem, &p.q, n) || dalloc(e, r.mem, &p.within, n) || dalloc(e, r.mem, &p.seg, p.segs) || dalloc(e, r.mem, &p.given, n) ||
               dalloc(e, r.mem, &p.slots, B);
    });
}

int azg_selfplay_priorities(azg_engine* e, const azg_priority_config* c) {
    if (!e) return AZG_E_INVALID;
    if (!c) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: cfg must not be NULL");
    if (int rc = ring_refusal(e, NEED_PRIORITIES)) return rc;
    ReplayRing& r = e->ring;
    ReplayRing::Priorities& p = r.prio;
    if (c->struct_size != (int32_t)sizeof(azg_priority_config)) return fail(e, AZG_E_INVALID, "azg_priority_config size mismatch");
    if (c->source != AZG_PRIO_VALUE_GAP && c->source != AZG_PRIO_GIVEN) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: unknown source");
    if (c->source == AZG_PRIO_VALUE_GAP && !r.tr.on)
        return fail(e, AZG_E_STATE, "azg_selfplay_priorities: AZG_PRIO_VALUE_GAP needs azg_selfplay_keep_transitions: the stored steps' search values were not kept");
    if (!(c->alpha >= 0.0f && std::isfinite(c->alpha))) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: alpha must be finite and >= 0");
    if (!(c->eps > 0.0f && std::isfinite(c->eps))) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: eps must be finite and > 0");
    const size_t n = r.stored_rows();
    if (c->source == AZG_PRIO_GIVEN) {
        if (!c->given) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: AZG_PRIO_GIVEN needs the given array");
        for (size_t i = 0; i < n; ++i)
            if (!(c->given[i] >= 0.0f)) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities: given[" + std::to_string(i) + "] is negative or NaN");
    }
    p.w_gen = -1;   // (weights computed from the priorities before these are no longer handed out)
    if (n == 0) { p.gen = r.rows_gen; return AZG_OK; }
    ON_DEVICE(e);
    Priorities pr;
    pr.rows_n = (long long)n; pr.source = c->source;
    pr.row_len = r.row; pr.vcol = r.row - 1;
    pr.alpha = c->alpha; pr.eps = c->eps;
    pr.value = r.tr.value; pr.rows = r.rows; pr.given = p.given; pr.q = p.q;
    if (c->source == AZG_PRIO_GIVEN) {
        p.h_given.assign(c->given, c->given + n);
        HIPCHK(e, hipMemcpyAsync(p.given, p.h_given.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    }
    hipLaunchKernelGGL(priorities_kernel, dim3((unsigned)((n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, e->stream, pr);
    HIPCHK(e, hipGetLastError());
    p.gen = r.rows_gen;
    return AZG_OK;
}

int azg_selfplay_priority_values(azg_engine* e, uint64_t* q, size_t max_rows) {
    if (int rc = ring_refusal(e, NEED_PRIORITIES)) return rc;
    return ring_download(e, max_rows, {{q, e->ring.prio.q, 8}});
}

int azg_selfplay_sample_rows(azg_engine* e, const azg_sample_config* c, int32_t* order) {
    if (!e) return AZG_E_INVALID;
    if (!c || !order) return fail(e, AZG_E_INVALID, "azg_selfplay_sample_rows: cfg and order must not be NULL");
    if (c->struct_size != (int32_t)sizeof(azg_sample_config)) return fail(e, AZG_E_INVALID, "azg_sample_config size mismatch");
    if (c->n_order < 1) return fail(e, AZG_E_INVALID, "azg_selfplay_sample_rows: n_order must be >= 1");
    if (int rc = sample_refusal(e, "azg_selfplay_sample_rows")) return rc;
    const int K = e->n_nets;
    PrioScan ps;
    if (int rc = ring_partition(e, "azg_selfplay_sample_rows", &ps)) return rc;
    ps.q = e->ring.prio.q; ps.within = e->ring.prio.within; ps.seg = e->ring.prio.seg;
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
    if (int rc = sample_refusal(e, "azg_selfplay_sample_slots")) return rc;
    ON_DEVICE(e);
    const int B = e->cfg.n_trees;
    PrioSlots dr;
    dr.B = B; dr.size = e->ring.steps; dr.sample_index = sample_index; dr.tree_base = (unsigned)e->cfg.tree_id_base;
    dr.seed = e->cfg.seed; dr.q = e->ring.prio.q; dr.slots = e->ring.prio.slots;
    hipLaunchKernelGGL(prio_draw_slots_kernel, dim3((B + PR_THREADS - 1) / PR_THREADS), dim3(PR_THREADS), 0, e->stream, dr);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(slots, dr.slots, (size_t)B * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AZG_OK;
}

// ---- importance-sampling weights of the stored rows (include/azgym_priority.h)

// the weights' memory, allocated by the first call that needs it (the engine's device is current)
static int ensure_weights(azg_engine* e) {
    ReplayRing& r = e->ring;
    ReplayRing::Priorities& p = r.prio;
    if (p.w) return AZG_OK;
    // one block: the minima (uint64) in front of the weights, so a failure leaves nothing behind
    const size_t n_min = p.segs + (size_t)e->cfg.n_trees, n_w = (size_t)r.cap * e->cfg.n_trees;
    unsigned long long* block = nullptr;
    if (dalloc(e, r.mem, &block, n_min + (n_w + 1) / 2)) return AZG_E_DEVICE;
    p.w_min = block; p.w = reinterpret_cast<float*>(block + n_min);
    return AZG_OK;
}

int azg_selfplay_is_weights(azg_engine* e, float beta) {
    if (int rc = sample_refusal(e, "azg_selfplay_is_weights")) return rc;
    if (!(beta >= 0.0f && std::isfinite(beta))) return fail(e, AZG_E_INVALID, "azg_selfplay_is_weights: beta must be finite and >= 0");
    ReplayRing& r = e->ring;
    ReplayRing::Priorities& p = r.prio;
    const int K = e->n_nets;
    PrioMin pm;
    if (int rc = ring_partition(e, "azg_selfplay_is_weights", &pm)) return rc;
    ON_DEVICE(e);
    if (int rc = ensure_weights(e)) return rc;
    pm.q = p.q; pm.seg_min = p.w_min; pm.net_min = p.w_min + p.segs;
    hipLaunchKernelGGL(prio_min_segments_kernel, dim3(pm.nseg, K), dim3(PR_THREADS), 0, e->stream, pm);
    HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(prio_min_nets_kernel, dim3(K), dim3(64), 0, e->stream, pm);
    HIPCHK(e, hipGetLastError());
    IsWeights iw;
    iw.rows_n = (long long)r.steps * pm.B; iw.B = pm.B; iw.T = pm.T; iw.beta = beta;
    iw.q = p.q; iw.net_min = pm.net_min; iw.w = p.w;
    hipLaunchKernelGGL(is_weights_kernel, dim3((unsigned)((iw.rows_n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, e->stream, iw);
    HIPCHK(e, hipGetLastError());
    p.w_gen = r.rows_gen;
    return AZG_OK;
}

int azg_selfplay_is_weights_device(azg_engine* e, const float** w) {
    if (!e) return AZG_E_INVALID;
    if (!w) return fail(e, AZG_E_INVALID, "azg_selfplay_is_weights_device: w must not be NULL");
    if (int rc = ring_refusal(e, NEED_PRIORITIES)) return rc;
    if (!e->ring.prio.w || e->ring.prio.w_gen != e->ring.rows_gen)
        return fail(e, AZG_E_STATE, "azg_selfplay_is_weights_device: azg_selfplay_is_weights has not run since the ring's stored rows or their priorities last changed");
    *w = e->ring.prio.w;
    return AZG_OK;
}

int azg_selfplay_is_weight_values(azg_engine* e, float* w, size_t max_rows) {
    if (int rc = ring_refusal(e, NEED_PRIORITIES)) return rc;
    if (!e->ring.prio.w) return fail(e, AZG_E_STATE, "azg_selfplay_is_weight_values: azg_selfplay_is_weights has not been called");
    return ring_download(e, max_rows, {{w, e->ring.prio.w, 4}});
}

// ---- priorities fed back from the trainer's value errors (include/azgym_priority.h)

int azg_selfplay_keep_errors(azg_engine* e, int32_t on) {   // (at any ring size, like the priorities it belongs to)
    if (int rc = ring_refusal(e, on ? NEED_PRIORITIES : 0, ": the errors are kept beside the priorities")) return rc;
    ReplayRing& r = e->ring;
    ReplayRing::Priorities& p = r.prio;
    if (!on) { p.err_on = 0; return AZG_OK; }
    if (p.err_on) return AZG_OK;
    ON_DEVICE(e);
    const size_t n = (size_t)r.cap * e->cfg.n_trees;
    if (!p.err) {   // one block: the maxima's bits (int32: per scan segment, then per net) in front of the errors
        const size_t n_max = p.segs + (size_t)e->cfg.n_trees;
        int* block = nullptr;
        if (dalloc(e, r.mem, &block, n_max + n)) return AZG_E_DEVICE;
        p.err_max = block; p.err = reinterpret_cast<float*>(block + n_max);
    }
    HIPCHK(e, hipMemsetD32Async((hipDeviceptr_t)p.err, (int)PR_ERR_UNSEEN_BITS, n, e->stream));
    p.err_on = 1;
    return AZG_OK;
}

int azg_selfplay_errors_device(azg_engine* e, float** err) {
    if (!e) return AZG_E_INVALID;
    if (!err) return fail(e, AZG_E_INVALID, "azg_selfplay_errors_device: err must not be NULL");
    if (int rc = ring_refusal(e, NEED_PRIORITIES | NEED_ERRORS)) return rc;
    *err = e->ring.prio.err;
    return AZG_OK;
}

int azg_selfplay_error_values(azg_engine* e, float* err, size_t max_rows) {
    if (int rc = ring_refusal(e, NEED_PRIORITIES | NEED_ERRORS)) return rc;
    return ring_download(e, max_rows, {{err, e->ring.prio.err, 4}});
}

int azg_selfplay_set_error_values(azg_engine* e, const float* err, size_t n_rows) {
    if (!e) return AZG_E_INVALID;
    if (!err) return fail(e, AZG_E_INVALID, "azg_selfplay_set_error_values: err must not be NULL");
    if (int rc = ring_refusal(e, NEED_PRIORITIES | NEED_ERRORS)) return rc;
    ReplayRing::Priorities& p = e->ring.prio;
    const size_t n = e->ring.stored_rows();
    if (n_rows != n) return fail(e, AZG_E_INVALID, "azg_selfplay_set_error_values: n_rows must be the stored rows (" + std::to_string(n) + ")");
    for (size_t i = 0; i < n; ++i)
        if (!(err[i] >= 0.0f || err[i] == PR_ERR_UNSEEN || err[i] != err[i]))
            return fail(e, AZG_E_INVALID, "azg_selfplay_set_error_values: err[" + std::to_string(i) + "] is neither -1, NaN nor >= 0");
    if (n == 0) return AZG_OK;
    ON_DEVICE(e);
    p.h_err.assign(err, err + n);
    HIPCHK(e, hipMemcpyAsync(p.err, p.h_err.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    return AZG_OK;
}

// What azg_selfplay_priorities_trained refuses, and the online epoch with it (online_ring_check)
static int trained_priorities_refusal(azg_engine* e, const azg_trained_priority_config* c) {
    if (!e) return AZG_E_INVALID;
    if (!c) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities_trained: cfg must not be NULL");
    if (int rc = ring_refusal(e, NEED_PRIORITIES | NEED_ERRORS)) return rc;
    const ReplayRing& r = e->ring;
    if (c->struct_size != (int32_t)sizeof(azg_trained_priority_config)) return fail(e, AZG_E_INVALID, "azg_trained_priority_config size mismatch");
    if (c->unseen != AZG_UNSEEN_MAX && c->unseen != AZG_UNSEEN_VALUE_GAP && c->unseen != AZG_UNSEEN_CONSTANT)
        return fail(e, AZG_E_INVALID, "azg_selfplay_priorities_trained: unknown unseen");
    if (c->unseen == AZG_UNSEEN_VALUE_GAP && !r.tr.on)
        return fail(e, AZG_E_STATE, "azg_selfplay_priorities_trained: AZG_UNSEEN_VALUE_GAP needs azg_selfplay_keep_transitions: the stored steps' search values were not kept");
    if (!(c->alpha >= 0.0f && std::isfinite(c->alpha))) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities_trained: alpha must be finite and >= 0");
    if (!(c->eps > 0.0f && std::isfinite(c->eps))) return fail(e, AZG_E_INVALID, "azg_selfplay_priorities_trained: eps must be finite and > 0");
    if (c->unseen == AZG_UNSEEN_CONSTANT && !(c->unseen_d >= 0.0f && std::isfinite(c->unseen_d)))
        return fail(e, AZG_E_INVALID, "azg_selfplay_priorities_trained: unseen_d must be finite and >= 0");
    return AZG_OK;
}

// The two launches of a net's largest seen error, and the q kernel's arguments, from the partition both share
static void launch_errmax(azg_engine* e, hipStream_t stream, PrioErrMax& pm) {
    ReplayRing::Priorities& p = e->ring.prio;
    pm.err = p.err; pm.seg_max = p.err_max; pm.net_max = p.err_max + p.segs;
    hipLaunchKernelGGL(prio_errmax_segments_kernel, dim3(pm.nseg, e->n_nets), dim3(PR_THREADS), 0, stream, pm);
    hipLaunchKernelGGL(prio_errmax_nets_kernel, dim3(e->n_nets), dim3(64), 0, stream, pm);
}
static PrioritiesTrained trained_args(azg_engine* e, const azg_trained_priority_config& c, int B, int T) {
    const ReplayRing& r = e->ring;
    PrioritiesTrained pr;
    pr.rows_n = (long long)r.stored_rows(); pr.unseen = c.unseen;
    pr.row_len = r.row; pr.vcol = r.row - 1; pr.B = B; pr.T = T;
    pr.alpha = c.alpha; pr.eps = c.eps; pr.unseen_d = c.unseen_d;
    pr.err = r.prio.err; pr.net_max = r.prio.err_max + r.prio.segs; pr.value = r.tr.value; pr.rows = r.rows; pr.q = r.prio.q;
    return pr;
}

int azg_selfplay_priorities_trained(azg_engine* e, const azg_trained_priority_config* c) {
    if (int rc = trained_priorities_refusal(e, c)) return rc;
    ReplayRing& r = e->ring;
    ReplayRing::Priorities& p = r.prio;
    PrioErrMax pm;
    if (int rc = ring_partition(e, "azg_selfplay_priorities_trained", &pm)) return rc;
    const size_t n = r.stored_rows();
    p.w_gen = -1;   // (weights computed from the priorities before these are no longer handed out)
    if (n == 0) { p.gen = r.rows_gen; return AZG_OK; }
    ON_DEVICE(e);
    if (c->unseen == AZG_UNSEEN_MAX) {
        launch_errmax(e, e->stream, pm);
        HIPCHK(e, hipGetLastError());
    }
    const PrioritiesTrained pr = trained_args(e, *c, pm.B, pm.T);
    hipLaunchKernelGGL(priorities_trained_kernel, dim3((unsigned)((n + PR_THREADS - 1) / PR_THREADS)), dim3(PR_THREADS), 0, e->stream, pr);
    HIPCHK(e, hipGetLastError());
    p.gen = r.rows_gen;
    return AZG_OK;
}

// ---- search rollouts (include/azgym_search_rollout.h)

// The steps of azg_search_rollout, with the evaluation's roots in place of the engine's: one ordinary search per step under search
// index index_base + s, then the step kernel; the count of unfinished games is read every poll_steps steps.
static int search_rollout_steps(azg_engine* e, const azg_search_rollout_config* c, SearchRollout& sr, int* steps, int* polls) {
    const long long bound = (long long)c->episodes_per_game * c->max_episode_length;
    for (long long s = 0; s < bound; ++s) {
        e->search_idx = c->index_base + (uint32_t)s;
        int rc = azg_search_resident(e);
        if (!rc) rc = settle_team(e);   // (wide networks: the persistent team kernel may have given up)
        if (rc) return rc;
        sr.rule.step_idx = c->index_base + (uint32_t)s;
        rc = launch_after_search(e, search_rollout_kernel16, search_rollout_kernel, sr);
        if (rc) return rc;
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
    int steps = 0, polls = 0;
    {   // ordinary searches from the evaluation's roots and carried counts (as self-play: a reused root carries at most n_sims)
        RootSwap evaluation(e, sr.roots, sr.carry, e->cfg.mode == AZG_MODE_DISCRETE ? e->cfg.n_sims : 0, c->index_base);
        rc = search_rollout_steps(e, c, sr, &steps, &polls);
    }
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

// ---- the online epoch's side of the ring (online_ring.h; include/azgym_train_online.h)

int online_ring_check(azg_engine* e, const azg_trained_priority_config* prio, float beta, OnlineRingShape* shape) {
    if (int rc = trained_priorities_refusal(e, prio)) return rc;
    if (e->ring.steps == 0) return fail(e, AZG_E_STATE, "azg_trainer_epoch_online: the replay ring is empty");
    if (!(beta >= 0.0f && std::isfinite(beta))) return fail(e, AZG_E_INVALID, "azg_selfplay_is_weights: beta must be finite and >= 0");
    PrioScan ps;
    if (int rc = ring_partition(e, "azg_trainer_epoch_online", &ps)) return rc;
    shape->device_id = e->cfg.device_id; shape->n_nets = e->n_nets;
    shape->obs_dim = e->S_obs; shape->n_actions = e->Kmax;
    shape->err = e->ring.prio.err;
    return AZG_OK;
}

int online_ring_enter(azg_engine* e) {
    ON_DEVICE(e);
    if (int rc = ensure_weights(e)) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->ring.prio.gen = e->ring.rows_gen;
    e->ring.prio.w_gen = -1;
    return AZG_OK;
}

hipError_t online_ring_refresh(azg_engine* e, hipStream_t stream, const azg_trained_priority_config& prio, float beta,
                               uint32_t sample_index, const OnlineStage& stage) {
    const ReplayRing& r = e->ring;
    const ReplayRing::Priorities& p = r.prio;
    const int K = e->n_nets;
    PrioErrMax pm;
    PrioScan ps;
    if (ring_partition(e, "azg_trainer_epoch_online", &ps)) return hipErrorInvalidValue;   // (online_ring_check has passed it)
    pm.B = ps.B; pm.T = ps.T; pm.N = ps.N; pm.nseg = ps.nseg;
    if (prio.unseen == AZG_UNSEEN_MAX) launch_errmax(e, stream, pm);
    ps.q = p.q; ps.within = p.within; ps.seg = p.seg;
    OnlineRefresh on;
    on.pr = trained_args(e, prio, ps.B, ps.T); on.ps = ps; on.seg_min = p.w_min;
    hipLaunchKernelGGL(online_refresh_segments_kernel, dim3(ps.nseg, K), dim3(PR_THREADS), 0, stream, on);
    unsigned long long* net_min = p.w_min + p.segs;
    hipLaunchKernelGGL(online_refresh_nets_kernel, dim3(K), dim3(64), 0, stream, ps, (const pr_u64*)p.w_min, net_min);
    OnlineDraw od;
    od.ps = ps;
    od.g.row_len = r.row; od.g.state_dim = e->S_obs; od.g.A = e->Kmax;
    od.sample_index = sample_index; od.tree_base = (unsigned)e->cfg.tree_id_base; od.seed = e->cfg.seed;
    od.beta = beta; od.n_rows = stage.n_rows; od.net_min = net_min; od.rows = r.rows;
    od.obs = stage.obs; od.actions = stage.actions; od.counts = stage.counts; od.values = stage.values; od.wout = stage.w;
    od.at_out = stage.at; od.drawn = stage.drawn;
    hipLaunchKernelGGL(online_draw_gather_kernel, dim3((stage.n_rows + PR_THREADS / 64 - 1) / (PR_THREADS / 64), K), dim3(PR_THREADS), 0, stream, od);
    return hipGetLastError();
}
