/* azgym_eval.h -- policy rollouts: whole episodes played by the network alone, no tree (an extension of azgym.h; same ABI
 * version).
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

#ifdef __cplusplus
}
#endif
#endif
