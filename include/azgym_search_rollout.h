/* azgym_search_rollout.h -- search rollouts: whole episodes played under MCTS, on the device, in one call: the return of an agent
 * that acts with its search.  An extension of azgym.h's device self-play; same ABI version.
 *
 * azg_search_rollout lets every game of the engine play episodes_per_game (E) whole episodes: every step is one ordinary search of
 * all trees -- every width, kernel form, population, per-net settings table and per-net budget: net k's games are searched by net k --
 * followed by a kernel that picks the final action by the agents' rule, steps the closed-form env in float64 and keeps the episode's
 * books.  The call works on evaluation state of its own (roots, carried counts, books) and needs no azg_selfplay_begin.  The CPU
 * oracle does not export it: the tests compose the same loop from an ordinary oracle search, its env step and its draws.
 *
 * Start states.  Tree t = k*T + j (net k, game j, T = n_trees / n_nets) plays its i-th episode from
 *   azg_reset_state(seed, game_id_base + j, episode + i, kind): azg_policy_rollout's start states, common to all nets, so that
 *   raw-policy and search returns are over the same states and the nets can be ranked.
 * RNG keys.  The tree's global id for the search's and the rule's draws stays tree_id_base + t: net k has the bits of a one-net engine
 *   with tree_id_base + k*T, its table entry and its budget.  Step s of the call (s = 0, 1, ... over the whole call, not per episode)
 *   is one search of all trees under search index index_base + s, and its AZG_STREAM_ACT draw is keyed with step index_base + s.
 * Carry.  A discrete search carries the picked child's node count into the next step's root, exactly as azg_selfplay_step does; the
 *   carry is dropped at an episode's end; continuous searches never carry.
 * Final action.  The rule of azg_selfplay_config (final_selection, deterministic, temperature, agent_epsilon) with the call's own
 *   settings, independent of a self-play that may be running, and with the same refusals.
 * Episodes.  Rewards are added unscaled, in step order, in float64.  An episode ends when the env says done or after
 *   max_episode_length steps (once when both happen).  After its E-th episode a game is parked: its root becomes the reset state of
 *   episode + E with carried count 0 and nothing of it is written any more; its tree is still searched -- the batch is fixed -- and
 *   the result is ignored.
 * Early end.  The step kernel counts the unfinished games down on the device; the host reads that count every poll_steps steps and
 *   stops at 0.  The hard bound is E * max_episode_length steps.  The outputs do not depend on poll_steps (info.steps does).
 *
 * Outputs are host arrays [n_trees][E]: returns (float64), lengths, terminated (1: the env said done; 0: cut at the length limit;
 * may be NULL).  The call uses the engine's stream and is complete on return.
 *
 * What it leaves alone: the live games (roots, carried counts, t, episode, return, finished-episode sums and counts), the replay ring
 * with its books and kept states, the self-play step index and the engine's running search index (saved and restored on every exit
 * path): a self-play run with search rollouts interleaved plays bit-identical games to one without them, given the same weights.
 * Afterwards the call's last search is simply the last search: azg_results, azg_root_eval and azg_search_info describe it;
 * azg_dump_tree behaves as after azg_selfplay_step (the search cannot be re-run).
 *
 * Errors, before anything is launched and with nothing written: NULL e / cfg / returns / lengths, a struct_size mismatch (cfg, or
 * a given info), episodes_per_game / max_episode_length / poll_steps < 1, an unknown final_selection, temperature <= 0, agent_epsilon
 * outside [0, 1]: AZG_E_INVALID; discrete mode with final_selection max_value and temperature != 1, or with temperature != 1 and
 * n_sims > 2048: AZG_E_UNSUPPORTED; whatever azg_search_resident refuses (weights not set, a settings table on wide nets without
 * AZG_NET_SEARCH_WIDE), with its code.  info (may be NULL) is written on success only. */
#ifndef AZGYM_SEARCH_ROLLOUT_H
#define AZGYM_SEARCH_ROLLOUT_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct azg_search_rollout_config {
    int32_t struct_size;            /* sizeof(azg_search_rollout_config), checked */
    int32_t episodes_per_game;      /* E >= 1 */
    int32_t max_episode_length;     /* >= 1 */
    int32_t final_selection;        /* AZG_FS_* */
    int32_t deterministic;          /* discrete: arg-max pi (1) or sampled (0) */
    int32_t poll_steps;             /* >= 1: the host looks at the device's count of unfinished games every poll_steps steps */
    uint32_t game_id_base, episode; /* start states, as azg_rollout_config */
    uint32_t index_base;            /* step s of the call searches under RNG search index index_base + s */
    double temperature, agent_epsilon;
} azg_search_rollout_config;

typedef struct azg_search_rollout_info {
    int32_t struct_size;            /* sizeof(azg_search_rollout_info), checked */
    int32_t steps;                  /* searches run */
    int32_t polls;                  /* times the host read the count of unfinished games */
} azg_search_rollout_info;

int azg_search_rollout(azg_engine* e, const azg_search_rollout_config* cfg, double* returns /* [n_trees][E] */, int32_t* lengths,
                       int32_t* terminated /* may be NULL */, azg_search_rollout_info* info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif
