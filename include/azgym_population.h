/* azgym_population.h -- populations: K agents with networks of their own, searched in one launch (an extension of azgym.h;
 * same ABI version).
 *
 * azg_set_population splits the engine's trees into n_nets nets (n_trees % n_nets == 0, T = n_trees / n_nets): trees
 * k*T .. k*T+T-1 are searched with net k's weights, and their RNG streams are those of global trees tree_id_base + k*T + j, as in
 * an engine without nets (seed and search index stay per engine).  Results, root children and tree dumps keep their order and
 * shapes.  Changing n_nets drops every weight; 1 restores the single-network engine.  All nets share the game, azg_config and the
 * network descriptor; they differ in their weights.
 * With n_nets > 1: azg_set_weights / _device return AZG_E_STATE; azg_search* return AZG_E_STATE until every net has weights;
 * networks wider than 256 (padded: the team / per-layer forms), azg_selfplay_begin*, azg_mlp_eval and azg_root_eval return
 * AZG_E_UNSUPPORTED.  The CPU oracle does not export these: the tests hold a K-net engine against K single-net engines. */
#ifndef AZGYM_POPULATION_H
#define AZGYM_POPULATION_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

int azg_set_population(azg_engine* e, int32_t n_nets);
/* net k's weights (the azg_set_weights blob, host memory); every net must have the same descriptor */
int azg_set_net_weights(azg_engine* e, int32_t net, const azg_mlp_desc* desc, const float* blob, size_t n_floats);

#ifdef __cplusplus
}
#endif
#endif
