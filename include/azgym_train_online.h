/* azgym_train_online.h -- prioritised replay as published: every minibatch of one native epoch is drawn from priorities refreshed with
 * the errors of the minibatches before it.  An extension of azgym_train_errors.h and azgym_priority.h; same ABI version.
 *
 * The rule, by equivalence.  azg_trainer_epoch_online trains M = n_minibatches minibatches over the engine's own replay ring and is
 * defined as this loop of existing entry points, for m = 0 .. M-1:
 *   1. azg_selfplay_priorities_trained(e, &cfg->prio)
 *   2. azg_selfplay_sample_rows(e, {batch_size, sample_index + m}, order)      (uint32 arithmetic: the index wraps)
 *   3. azg_selfplay_is_weights(e, beta)
 *   4. azg_trainer_epoch_opt_errors (azg_trainer_epoch_nets_errors for the *_nets form) with rows = the ring (group T = n_trees /
 *      n_nets, group stride n_trees, net stride T), weights = azg_selfplay_is_weights_device, errors = azg_selfplay_errors_device,
 *      n_order = batch_size, and opt.step + m and alpha_state.step + m in place of the caller's steps.
 * Where that loop leaves them, bit for bit: the parameters, the optimiser state, log_alpha and its Adam state, the engine's err array,
 * the engine's q array (the last refresh's; it counts as computed, as after azg_selfplay_priorities_trained) and `drawn`, which holds
 * the loop's orders.  loss_sums[k][slot] is the float64 chain from 0.0 over the minibatches' float32 losses in order
 * (azg_trainer_epoch's rule).  One difference: the full weight array is not computed -- only the drawn rows' weights are -- so the call
 * leaves the weights invalidated: azg_selfplay_is_weights_device refuses until the next azg_selfplay_is_weights.  The ring's rows,
 * transitions, games, books and the search index do not move.
 *
 * What runs.  The engine's stream is synchronised on entry; everything is then enqueued on the trainer's stream and the call
 * synchronises once, at its end.  Between the first launch and that synchronisation there is no host synchronisation and no copy but
 * the *_nets settings table (uploaded once in front) and `drawn` (one device-to-host copy after the last minibatch).  Per minibatch, in
 * front of the step's own three launches: q + segment scan + segment minimum in one launch, the segment totals' scan + the net's
 * minimum in one, draw + weight + gather in one -- 3 launches, 5 under AZG_UNSEEN_MAX whose two error-maximum launches stay in front --
 * where the loop takes 10 (8), two synchronisations and two copies.  The loss launch of minibatch m writes err[at]; the refresh of
 * m + 1 reads it in stream order.  Works on every trainer handle (azg_trainer_create, _ex, _wide, _wide_ex).
 *
 * Refusals, every one before the first launch and with nothing written.  NULL trainer: AZG_E_INVALID; otherwise the message is the
 * trainer's (azg_trainer_last_error).  NULL engine or cfg, a wrong struct_size, n_minibatches < 1, batch_size outside 1..max_batch:
 * AZG_E_INVALID.  `prio` and `beta`: the refusals and codes of azg_selfplay_priorities_trained and azg_selfplay_is_weights (no begin,
 * no keep_priorities, no keep_errors: AZG_E_STATE, ...); an empty ring: AZG_E_STATE.  Engine and trainer on different devices, a
 * different n_nets, an observation width that is not the trainer's in_dim, an action count outside 1..16: AZG_E_INVALID.  Then every
 * check of azg_trainer_epoch_opt_errors (azg_trainer_epoch_nets_errors), for every minibatch's Adam step.
 *
 * Not provided: sampling without replacement; a beta schedule inside the call; rows of another rank. */
#ifndef AZGYM_TRAIN_ONLINE_H
#define AZGYM_TRAIN_ONLINE_H
#include "azgym_priority.h"
#include "azgym_train_errors.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct azg_online_epoch {
    int32_t  struct_size;              /* sizeof(azg_online_epoch) */
    int32_t  n_minibatches;            /* M >= 1 */
    int32_t  batch_size;               /* 1 .. the trainer's max_batch; every minibatch has exactly this many rows per net */
    uint32_t sample_index;             /* minibatch m draws under sample_index + m (uint32 arithmetic, wrapping) */
    float    beta;                     /* importance-sampling exponent, finite and >= 0 */
    azg_trained_priority_config prio;  /* the refresh in front of every minibatch */
    int32_t* drawn;                    /* optional HOST array [M][n_nets][batch_size]: the rows drawn, net numbering */
} azg_online_epoch;

/* params, loss_cfg, alpha_state, opt and loss_sums (device, [n_nets][AZG_LOSS_SLOTS] float64) as azg_trainer_epoch_opt_errors takes
 * them. */
int azg_trainer_epoch_online(azg_trainer* t, azg_engine* e, float* params, const azg_online_epoch* cfg, const azg_loss_cfg* loss_cfg,
                             const azg_alpha_state* alpha_state, const azg_optim* opt, double* loss_sums);
/* The same with loss_cfgs[n_nets] and opts[n_nets], as azg_trainer_epoch_nets_errors takes them. */
int azg_trainer_epoch_online_nets(azg_trainer* t, azg_engine* e, float* params, const azg_online_epoch* cfg,
                                  const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state, const azg_optim* opts,
                                  double* loss_sums);

#ifdef __cplusplus
}
#endif
#endif
