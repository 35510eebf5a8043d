// ls_dispatch.cuh -- host-side launch sequence of the lock-step path (included by dispatch_lockstep.hip and dispatch_mcc_wide.hip).
#pragma once

#include "engine_host.h"
#include "lockstep.cuh"

// The launch sequence of one search: per simulation step a tree kernel, the first layer and one LDS-tiled kernel per hidden->hidden
// layer, all on the engine's stream.  (A captured hipGraph of the sequence ran in the same time as the plain launches: the path is
// not host-bound.  Cutting the batch into pipelines on several streams measured +6 % / +40 % time at config E: removed, HISTORY.md.)
// POP: the kernels' population forms (lockstep.cuh: every tree group and tile pair reads its net's weights).
// NSET: the population forms with the engine's table of per-net MCTS settings -- ls_tree_kernel_nets; the layer kernels read no setting.
// With a table the steps run to its largest per-net budget (azg_engine::net_sims_max <= cfg.n_sims); a tree group whose net has a
// smaller one finishes in the tree launch of its own last step and sits the later ones out (lockstep.cuh: ls_tree_kernel_nets).
template <int ENV, int HP, bool GMM, bool POP, bool NSET = false>
static hipError_t ls_enqueue(azg_engine* e, hipStream_t st) {
    static_assert(!NSET || POP, "per-net settings run the population forms");
    constexpr int NS = HP / 256, NCH = HP / 64;
    const int G = (e->cfg.n_trees + TREES_PER_WG - 1) / TREES_PER_WG;
    const size_t tab_bytes = ((size_t)e->tab_n * 8 + (size_t)(e->cfg.n_sims + 2) * 4 + 15) / 16 * 16;
    const auto tree_launch = [&](int sim) {
        if constexpr (NSET) hipLaunchKernelGGL((ls_tree_kernel_nets<ENV, GMM, NCH, HP>), dim3(G), dim3(256), tab_bytes, st, e->P, e->ls, sim, 0, e->net_search);
        else hipLaunchKernelGGL((ls_tree_kernel<ENV, GMM, NCH, HP, POP>), dim3(G), dim3(256), tab_bytes, st, e->P, e->ls, sim, 0);
    };
    // hidden layers: 32 trees x 64 units per workgroup (two workgroups per CU at 1024 trees x 1024 units)
    auto tkh = ls_hidden_tiled_kernel<HP, false, 2, 4, POP>;
    auto tkl = ls_hidden_tiled_kernel<HP, true, 2, 4, POP>;
    const int TQ = (G + 1) / 2, NU = HP / 64;
    // two stages of A (4 tiles) + B (2 groups); the weights-direct tile stages the activations only (and passes the head chain through
    // the first TG * 64 entries)
    const size_t tiled_bytes = LS_LAYER_WD ? (size_t)2 * 2 * LS_LAYER_KC * 64 * 16 : (size_t)2 * (4 + 2) * LS_KC * 64 * 16;
    static KernelAttrs tkh_attrs, tkl_attrs;
    hipError_t rc = tkh_attrs.set_dyn_lds(e, (const void*)tkh, tiled_bytes);
    if (rc == hipSuccess) rc = tkl_attrs.set_dyn_lds(e, (const void*)tkl, tiled_bytes);
    if (rc != hipSuccess) return rc;
    tree_launch(-2);
    const int n_steps = NSET ? e->net_sims_max : e->cfg.n_sims;
    for (int sim = -1; sim < n_steps; ++sim) {
        hipLaunchKernelGGL((ls_layer0_kernel<HP, POP>), dim3(G * NS), dim3(256), 0, st, e->P, e->ls, 0);
        for (int l = 1; l < e->n_hidden; ++l) {
            auto k = l == e->n_hidden - 1 ? tkl : tkh;
            hipLaunchKernelGGL(k, dim3(TQ * NU), dim3(256), tiled_bytes, st, e->P, e->ls, l, (l - 1) & 1, TQ, 0);
        }
        tree_launch(sim);
    }
    return hipGetLastError();
}

template <int ENV, int HP, bool GMM, bool NSET>
static hipError_t ls_run(azg_engine* e) {
    if (e->opt.ls_team) {
        hipError_t rc;
        if constexpr (NSET) rc = azg_team_search_nets<ENV>(e);
        else rc = azg_team_search<ENV>(e);
        if (rc != hipErrorNotReady) return rc;
    }
    e->last.form = AZG_FORM_PER_LAYER;
    e->last.nets = NSET;
    if constexpr (NSET) return ls_enqueue<ENV, HP, GMM, true, true>(e, e->stream);   // (also an engine of one net: net_T = B)
    else return e->n_nets > 1 ? ls_enqueue<ENV, HP, GMM, true>(e, e->stream) : ls_enqueue<ENV, HP, GMM, false>(e, e->stream);
}

template <int ENV, bool NSET>
static hipError_t lockstep_search(azg_engine* e) {
    constexpr bool CONT = EnvFamily<ENV>::CONT;   // (mixture heads: the continuous family only)
    const bool gmm = CONT && e->P.ncomp >= 2;
    if (e->HP == 512) return gmm ? ls_run<ENV, 512, CONT, NSET>(e) : ls_run<ENV, 512, false, NSET>(e);
    return gmm ? ls_run<ENV, 1024, CONT, NSET>(e) : ls_run<ENV, 1024, false, NSET>(e);
}
template <int ENV>
hipError_t azg_lockstep_search(azg_engine* e) { return lockstep_search<ENV, false>(e); }
// the same with the engine's table of per-net MCTS settings (instantiated by the dispatch_nets_*.hip translation units)
template <int ENV>
hipError_t azg_lockstep_search_nets(azg_engine* e) { return lockstep_search<ENV, true>(e); }
