/* azgym_eval.h -- policy rollouts: whole episodes played by the network alone, no tree; and batched inference for every net of a
 * population (azg_population_mlp_eval, below).  An extension of azgym.h; same ABI version.
 *
 * azg_policy_rollout plays episodes_per_net (G) episodes per net of the engine in ONE kernel launch, from reset to their end: the
 * raw policy's return, the number the reference's users read off a deployed net.  Game j of EVERY net starts at
 * azg_reset_state(seed, game_id_base + j, episode, kind) -- common random numbers: the nets' returns are over the same start
 * states and can be ranked; another `episode` gives a fresh set.  Every step evaluates the net on the game's observation with the
 * search's own arithmetic (the head outputs are azg_mlp_eval's `raw`, bit for bit), turns them into an action by action_rule,
 * steps the closed-form env in float64 and adds the reward (unscaled, as the env pays it) to the game's return, in step order.
 * An episode ends when the env says done or after max_episode_length steps.
 *
 * action_rule
 *   AZG_ROLLOUT_MODE    discrete head: arg-max logit, lowest index on ties.  Normal head: bound * tanh(mu) (the squashing function
 *                       the search samples with, at noise 0).  Mixture head: the component with the largest log-coefficient
 *                       (lowest index on ties), then as the Normal head.
 *   AZG_ROLLOUT_SAMPLE  discrete head: inverse CDF in float64 over the float32 softmax in index order (first a with
 *                       u < p_0 + .. + p_a, else the last action), u = (word 0 + 0.5) / 2^32 of the AZG_STREAM_ACT draw keyed
 *                       (seed, game id, step t).  Normal head: bound * tanh(mu + sigma * eps), eps the search's Normal draw keyed
 *                       (seed, game id, t, 0).  Mixture head: the component by inverse CDF with the third word of that same draw
 *                       (the search's widening rule), then eps as for the Normal head.
 *
 * Outputs are host arrays [n_nets][G]: returns (float64), lengths, terminated (1: the env said done; 0: cut at the length
 * limit; may be NULL), first_value (the value head at the start state; may be NULL).  The call uses the engine's stream and
 * synchronises once.  It reads the nets' weights and nothing else of the engine: searches, results and device self-play are
 * left exactly as they were, and it may be called between self-play steps.
 *
 * Errors (nothing is written): NULL e / cfg / returns / lengths, a struct_size mismatch, episodes_per_net < 1,
 * max_episode_length < 1, an unknown action_rule: AZG_E_INVALID; a net without weights: AZG_E_STATE; networks of 512 (padded)
 * units and wider: AZG_E_UNSUPPORTED (azg_policy_rollout_ex takes them).  The CPU oracle does not export this: the tests compose
 * the same rollout from its azo_mlp_eval, azo_env_step and draw exports.
 *
 * azg_policy_rollout_ex is the same call for EVERY width the engine accepts: the same start states, action rules, outputs, errors
 * (but the width one) and the same promise to read the nets' weights and nothing else of the engine.  Up to 256 padded units it runs
 * azg_policy_rollout's kernels (same bits).  Wider nets take one of two forms, with equal results bit for bit:
 *   AZG_ROLLOUT_FORM_GROUP  one workgroup per 16 games of one net streams the net's weights every step: any wide shape (LayerNorm,
 *                           one hidden layer, Acrobot's six inputs, every activation, any G, any number of nets), one launch.
 *   AZG_ROLLOUT_FORM_TEAM   the shapes the search runs as teams (padded width 512 or 1024, at least two hidden layers, no LayerNorm,
 *                           at most four inputs): 32 games of one net and HP/64 cooperating workgroups, each computing a 64-unit slice
 *                           of every layer and owning 32/(HP/64) of the games; net k has ceil(G / 32) teams.  All workgroups of a
 *                           launch have to be resident at once: the call runs as many launches, one after the other, as that takes.
 *                           AZG_LS_TEAM=0 forces the group form.  Should a hand-off wait of the team kernel time out, the whole call is
 *                           replayed in the group form (the caller sees correct outputs and form GROUP), team_fallbacks counts it and
 *                           this engine's later rollouts take the group form.  The search's own switches and counters
 *                           (azg_search_info) are not touched.
 * info (may be NULL; a struct_size mismatch: AZG_E_INVALID) reports what ran; it is written on success only. */
#ifndef AZGYM_EVAL_H
#define AZGYM_EVAL_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AZG_ROLLOUT_MODE = 0, AZG_ROLLOUT_SAMPLE = 1 };

typedef struct azg_rollout_config {
    int32_t struct_size;        /* sizeof(azg_rollout_config), checked */
    int32_t episodes_per_net;   /* G */
    int32_t max_episode_length;
    int32_t action_rule;        /* AZG_ROLLOUT_* */
    uint32_t game_id_base;      /* global id of game 0 (keys the start states and the sampling draws) */
    uint32_t episode;           /* which set of start states */
} azg_rollout_config;

int azg_policy_rollout(azg_engine* e, const azg_rollout_config* cfg, double* returns, int32_t* lengths, int32_t* terminated,
                       float* first_value);

enum { AZG_ROLLOUT_FORM_GROUP = 0,   /* one workgroup per 16 games of one net */
       AZG_ROLLOUT_FORM_TEAM  = 1 }; /* 32-game teams of HP/64 workgroups */

typedef struct azg_rollout_info {
    int32_t struct_size;     /* sizeof(azg_rollout_info), checked */
    int32_t form;            /* AZG_ROLLOUT_FORM_* of the launch(es) whose outputs were returned */
    int32_t launches;        /* kernel launches of this call, a fall-back's included */
    int32_t team_fallbacks;  /* team rollouts of this engine that gave up and were replayed as FORM_GROUP, so far */
} azg_rollout_info;

int azg_policy_rollout_ex(azg_engine* e, const azg_rollout_config* cfg, double* returns, int32_t* lengths, int32_t* terminated,
                          float* first_value, azg_rollout_info* info /* may be NULL */);

/* Batched inference for EVERY net of the engine in one launch: azg_mlp_eval for any n_nets (azg_set_population).
 *
 * Net k is evaluated on its own n observations, obs [n_nets][n][obs_dim]; with shared_obs != 0 obs is [n][obs_dim] and every net is
 * evaluated on the same rows (uploaded once).  Outputs, each may be NULL: value [n_nets][n], dist [n_nets][n][n_dist] (azg_mlp_eval's
 * distribution parameters), raw [n_nets][n][1 + n_dist] (the head outputs).  A row's outputs have the bits azg_mlp_eval gives on a
 * one-net engine with net k's weights: they do not depend on n, n_nets, the row's position, the form of the call or the grid.  With
 * n_nets == 1 both calls are azg_mlp_eval (same bits).
 *
 * One kernel launch of (groups, n_nets) workgroups: workgroup (g, k) reads net k's weights once -- into registers where the search keeps
 * that shape resident (`resident`) -- and walks the 16-observation tiles g, g + groups, ... of net k.  groups = min(tiles, cap), the cap
 * chosen so that the workgroups of a large call, over all nets, are all resident at once (the chip filled once); AZG_EVAL_GROUPS=g
 * (read when the engine is created) replaces the cap, for tests.
 *
 * azg_population_mlp_eval takes host arrays and keeps device scratch of its own that only grows.  azg_population_mlp_eval_device takes
 * obs / value / dist / raw in DEVICE memory on the engine's GPU: inputs complete when the call is made (their producer's stream
 * synchronised), no staging and no host copy.  Either enqueues the kernel on the engine's stream and synchronises once: outputs are
 * complete on return.  Both read the nets' weights and nothing else of the engine: they may be called between self-play steps, and after
 * a search without spoiling azg_results, azg_root_children or a later azg_dump_tree.
 *
 * Errors (nothing is written): NULL e / obs, an info with a wrong struct_size, n_nets * n > 2^24, n_nets > 65535: AZG_E_INVALID; a net
 * without weights: AZG_E_STATE.  n == 0: AZG_OK, nothing happens.  info (may be NULL) is written on success only.
 * The CPU oracle does not export these: the tests hold a K-net engine against K single-net engines' azg_mlp_eval.
 *
 * azg_population_root_eval is azg_root_eval for any n_nets: the root's value [n_trees] and distribution parameters [n_trees][n_dist]
 * of the last search, in the tree order of azg_results (net k: trees k*T .. k*T+T-1).  Each may be NULL. */
typedef struct azg_eval_info {   /* written on success only */
    int32_t struct_size;         /* checked */
    int32_t resident;            /* 1: hidden weights register-resident (NREG > 0) */
    int32_t groups;              /* workgroups per net */
    int32_t tiles;               /* 16-observation tiles per net */
} azg_eval_info;

/* host arrays */
int azg_population_mlp_eval(azg_engine* e, const float* obs, size_t n, int32_t shared_obs,
                            float* value, float* dist, float* raw, azg_eval_info* info);
/* the same with obs / value / dist / raw in DEVICE memory on the engine's GPU */
int azg_population_mlp_eval_device(azg_engine* e, const float* obs, size_t n, int32_t shared_obs,
                                   float* value, float* dist, float* raw, azg_eval_info* info);
/* azg_root_eval for any n_nets: [n_trees] / [n_trees][n_dist], tree order as azg_results */
int azg_population_root_eval(azg_engine* e, float* value, float* dist);

#ifdef __cplusplus
}
#endif
#endif
