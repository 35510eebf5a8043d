/* azgym_train_weighted.h -- the population trainer's losses with a weight per minibatch row.  An extension of azgym_train.h; same ABI
 * version.
 *
 * Prioritised replay (azgym_priority.h) draws training rows in proportion to their priority; the importance-sampling weight
 * w = (q_min / q)^beta of a drawn row (azg_selfplay_is_weights) corrects the expectation the losses are taken under.  Here every
 * entry point that computes losses has a form with one more argument, `weights`, a device pointer to float32 weights:
 *
 *   A weight w_b per minibatch row multiplies every per-row summand of every loss of that row's net before the reduction over the
 *   rows; the reductions stay what they are (`mean` divides by the number of rows, not by the sum of the weights):
 *     policy   policy_coeff * reduce_b(w_b * policy_b)
 *     value    value_coeff * reduce_b(w_b * (V_b - z_b)^2)
 *     entropy  alpha * reduce_b(w_b * H_b)           (the discrete head's per-(row, action) entropy: every action carries the row's w)
 *     alpha_loss of the tuned loss   alpha * mean_b(w_b * (H_b - target)), computed as alpha * (S_wH / n - target * (S_w / n)) with
 *              S_w the sum of the weights in float64
 *   and d_raw[b][.] = (float)(w_b * x), x the float64 value the unweighted kernel rounds: one more float64 multiply in front of the
 *   single rounding.  The weighting is float64 from the float32 weight, inside the row's arithmetic.
 *
 * Weights that all equal 1.0f give the unweighted call's bits in d_raw, losses, log_alpha and its Adam state: every product 1.0 * x
 * is exact, the chains are the same chains and S_w / n is exactly 1.
 *
 * For loss and step the array is [n_nets][n_rows].  For an epoch it is addressed by azg_epoch_rows' rule with a row length of 1: the
 * weight of the row at element `at` of the rows array (in rows, not floats) is weights[at] -- for the replay ring
 * [capacity_steps][n_trees], the array azg_selfplay_is_weights_device returns; for a plain [n_nets][n] rows array, [n_nets][n].  The
 * epoch's gather stages it with the row.  The caller vouches for the addresses and for the values being finite and >= 0; they are taken
 * as they are.
 *
 * Each entry point is its namesake with `weights` added: NULL weights is AZG_E_INVALID; every other check, code and message is the
 * namesake's, every check comes before the first launch and on an error nothing is written.  They work on every trainer handle
 * (azg_trainer_create, _ex, _wide, _wide_ex).  An epoch leaves parameters, optimiser state and alpha state bit for bit where the same
 * minibatches, passed one by one to the weighted step with the gathered weights, leave them; in the per-net forms net k has the bits of
 * a one-net trainer given entry k and net k's weights.  The azg_rmsprop family has no weighted form: *_opt with RMSprop and no clip
 * gives its bits.  The first weighted call allocates the weighted path's own float64 scratch ([n_nets][4][max_batch]); the unweighted
 * path's allocations do not change. */
#ifndef AZGYM_TRAIN_WEIGHTED_H
#define AZGYM_TRAIN_WEIGHTED_H
#include "azgym_train.h"

#ifdef __cplusplus
extern "C" {
#endif

int azg_trainer_loss_weighted(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                              const float* weights, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfg,
                              const azg_alpha_state* alpha_state, float* d_raw, float* losses);
int azg_trainer_loss_nets_weighted(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                                   const float* weights, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfgs,
                                   const azg_alpha_state* alpha_state, float* d_raw, float* losses);

int azg_trainer_step_opt_weighted(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts,
                                  const float* values, const float* weights, int32_t n_rows, int32_t n_actions,
                                  const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_optim* opt, float* grads,
                                  float* raw_out, float* losses);
int azg_trainer_step_nets_weighted(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts,
                                   const float* values, const float* weights, int32_t n_rows, int32_t n_actions,
                                   const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state, const azg_optim* opts, float* grads,
                                   float* raw_out, float* losses);

int azg_trainer_epoch_opt_weighted(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, const int32_t* order,
                                   int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                                   const azg_optim* opt, double* loss_sums, int32_t* n_minibatches);
int azg_trainer_epoch_nets_weighted(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, const int32_t* order,
                                    int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state,
                                    const azg_optim* opts, double* loss_sums, int32_t* n_minibatches);

#ifdef __cplusplus
}
#endif
#endif
