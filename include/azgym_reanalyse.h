/* azgym_reanalyse.h -- reanalysis of the device replay ring: search stored positions again with the engine's current weights and
 * overwrite their rows' targets (MuZero's "Reanalyse").  An extension of azgym.h's device self-play; same ABI version.
 *
 * A replay row keeps the float32 observation, which is not the float64 env state a search starts from, so the engine keeps the
 * states itself on request (azg_selfplay_keep_states): one block [n_trees][S_env] per ring slot, written by the self-play step
 * beside the slot's rows.  azg_selfplay_reanalyse is then one ordinary search of the engine -- every width, kernel form, population,
 * per-net settings table and per-net budget: net k's rows are searched by net k -- from those states, plus a kernel that rewrites
 * the rows' target columns.  The CPU oracle does not export these: the expected row is MCTS.return_results of an ordinary oracle
 * search of the kept state under the same search index.
 *
 * What a reanalysis writes: row (slots[t], t)'s actions[Kmax] | counts[Kmax] | Q[Kmax] | V_target columns, exactly what a self-play
 * step would have written for this search (return_results' actions -- discrete: the index as float -- counts and Q, zero beyond
 * n_children; the value target by azg_config.v_target, rounded to float32).  Every row is written by one tree.
 * What it leaves alone: the rows' observation columns and every other row; the live games (roots, carried counts, t, episode, return,
 * finished-episode sums and counts); the self-play step index; the ring's size, insert index and total; the engine's running search
 * index (saved and restored: a self-play run with reanalyses interleaved plays bit-identical games to one without them, given the
 * same weights).
 * Afterwards the reanalysis is simply the last search: azg_results, azg_root_eval and azg_search_info describe it; azg_dump_tree
 * behaves as after azg_selfplay_step (the search cannot be re-run). */
#ifndef AZGYM_REANALYSE_H
#define AZGYM_REANALYSE_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Keep every stored step's env states beside the replay ring: [capacity_steps][n_trees][S_env] float64, slot-aligned with the rows
 * (the state the step's search started from, i.e. what the row's observation was computed from).  on = 1 / 0.  Allowed after
 * azg_*selfplay_begin* while the ring is empty (size_steps == 0), else AZG_E_STATE; the next begin drops it. */
int azg_selfplay_keep_states(azg_engine* e, int32_t on);

/* The kept states of the stored steps, ordered like azg_selfplay_rows ([slot][tree][S_env]); returns the number of rows copied.
 * Synchronises the engine's stream.  AZG_E_STATE without keep_states. */
int azg_selfplay_states(azg_engine* e, double* states, size_t max_rows);

/* Search stored positions again with the engine's CURRENT weights and settings and overwrite their rows' targets.
 *   slots [n_trees] (host) : tree t re-searches the position of ITS OWN game column in ring slot slots[t] and rewrites row
 *                            (slots[t], t); NULL: every tree takes `slot`.
 *   search_index           : the RNG search index this search runs under (what azg_set_search_index sets for a normal search).
 * Tree t's root is the kept state with carried count 0 (a fresh root, as after a reset; continuous searches never carry); its global
 * id stays tree_id_base + t.  Asynchronous like azg_selfplay_step: launches only (wide networks: the team kernel's status is read
 * as azg_selfplay_step reads it).
 * Refusals, before anything is launched and with the ring untouched: no begin or no keep_states: AZG_E_STATE; a slot outside
 * [0, size_steps): AZG_E_INVALID; whatever azg_search_resident refuses (weights not set, a settings table on wide nets without
 * AZG_NET_SEARCH_WIDE), with its code. */
int azg_selfplay_reanalyse(azg_engine* e, const int32_t* slots, int32_t slot, uint32_t search_index);

#ifdef __cplusplus
}
#endif
#endif
