/* azgym_refresh.h -- refresh the replay ring's bootstrap values from the value head: one forward pass per stored row instead of the
 * n_sims network evaluations of a reanalysis (azgym_reanalyse.h).  An extension of azgym.h, azgym_nstep.h and azgym_target.h; same ABI
 * version.  A library may lack this symbol.
 *
 * Every n-step / lambda-return target (azgym_nstep.h, azgym_lambda.h) bootstraps from the kept float64 `value` of a stored step
 * (azg_selfplay_keep_transitions), which the self-play step wrote from its search and a reanalysis overwrites from a fresh search.
 * azg_selfplay_refresh_values overwrites it with the value head's output: net k's weights of the weight set in use (LIVE or TARGET,
 * azg_use_weights) on the stored observation of net k's rows, read in the ring where they lie, the float32 value of azg_mlp_eval /
 * azg_population_mlp_eval for that observation bit for bit, widened to float64.  azg_selfplay_nstep_targets / _lambda_targets then turn
 * the fresh values into targets, as they do after a reanalysis; with the TARGET set in use this is MuZero Reanalyse's value target
 * z = r + ... + gamma^m v_target_net(s + m).
 *
 * What the column holds afterwards: the network's value in the units a tree node holds (continuous mode: rewards divided by
 * reward_scale), no longer azg_config.v_target's search value.  A later reanalysis of a row overwrites it again with that search's
 * value.  A window that bootstraps from its own row -- the newest stored step, a time-limit step, n_step = 0 -- gets the net's own
 * value as its target; with the TARGET set in use that is the usual target-network TD target.  The priority
 * (|kept value - V_target| + eps)^alpha (azgym_priority.h) becomes the net's own TD error.
 *
 * Asynchronous: one small copy of `slots` and one launch on the engine's stream, nothing is synchronised (the engine stages `slots`: the
 * caller's array may go when the call returns).  Written: the kept `value` of the rows (slot, every tree) of the listed slots.  Left
 * alone: the rows (V_target included), reward / action / end, the kept states, the priorities, weights and errors and the generation
 * they were computed at (the caller recomputes priorities, as after a reanalysis), the live games, the self-play step index and the
 * running search index, the last search's cached results and the weight set in use.
 *
 * Not provided: a separate bootstrap column that keeps the search value for a row's own target; a blend of old and new values; one
 * slot per game; refreshing the policy targets from the heads; a choice of weight set per net; other ranks' rows. */
#ifndef AZGYM_REFRESH_H
#define AZGYM_REFRESH_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* slots: host array [n_slots] of ring slots in [0, size_steps) (a slot may be listed twice); NULL: every stored slot (n_slots ignored).
 * Refused before anything is launched, the ring untouched: a NULL engine (AZG_E_INVALID); no azg_selfplay_begin or no
 * azg_selfplay_keep_transitions (AZG_E_STATE); a net without weights in the set in use (AZG_E_STATE); slots non-NULL with n_slots < 0
 * (AZG_E_INVALID); a slot outside [0, size_steps) (AZG_E_INVALID).  An empty ring with slots NULL, or n_slots == 0 with a list: AZG_OK,
 * nothing is launched. */
int azg_selfplay_refresh_values(azg_engine* e, const int32_t* slots, int32_t n_slots);

#ifdef __cplusplus
}
#endif
#endif
