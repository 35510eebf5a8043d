/* azgym_train_errors.h -- the population trainer's value error per trained row, out of the loss launch.  An extension of
 * azgym_train_weighted.h; same ABI version.
 *
 * Prioritised replay's third source of priorities is the learner's own error on the rows it just trained on (azgym_priority.h:
 * azg_selfplay_priorities_trained).  The error of minibatch row b is
 *     e_b = (float)fabs((double)raw[b][0] - (double)z_b)
 * with raw[b][0] the value head's output V of the forward pass that precedes the step and z_b the row's float32 value target: the first
 * two operations the loss of the row performs, so it is the error the row had when it was trained on, and it does not depend on the
 * weights.  A NaN or infinite V gives a NaN or +inf error; nothing is filtered.
 *
 * Each entry point is its *_weighted namesake (azgym_train_weighted.h) with one more argument after `weights`: `errors`, a device
 * pointer to float32 that the loss launch writes; no launch is added.  `weights` may be NULL here, meaning unweighted: d_raw, losses,
 * log_alpha and its Adam state then have the bits of the unweighted call (they are those of weights that all equal 1.0f).  NULL
 * `errors` is AZG_E_INVALID; every other check, code and message is the namesake's, every check comes before the first launch and on
 * an error nothing is written.  They work on every trainer handle (azg_trainer_create, _ex, _wide, _wide_ex).
 *
 * loss forms: errors is dense, [n_nets][n_rows]: errors[k][b] = e_b of net k.
 *
 * epoch forms: errors is addressed like `weights`, by azg_epoch_rows' rule with a row length of 1: the error of the row at element `at`
 * of the rows array (in rows, not floats) goes to errors[at] -- for the replay ring [capacity_steps][n_trees], the array
 * azg_selfplay_errors_device returns; for a plain [n_nets][n] rows array, [n_nets][n].  The epoch's gather stages `at` beside the row
 * and the minibatch's loss launch writes errors[at] = e_b.  A row drawn twice in one minibatch is written twice with the same value; a
 * row in two minibatches keeps the later one's value (the launches are ordered on the trainer's stream); entries of rows that were not
 * drawn are not touched.  Parameters, optimiser state, alpha state and loss_sums are bit for bit those of the *_weighted epoch, or of
 * the plain epoch when weights is NULL.  The caller vouches for the addresses.  The first call allocates the weighted path's scratch
 * and, for an epoch, the staged indices ([n_nets][max_batch] int64); the other paths' allocations do not change.
 *
 * Not provided: errors from azg_trainer_step_*.  These epochs' priorities are fixed while they run; azgym_train_online.h redraws every
 * minibatch from priorities refreshed with the errors of the minibatches before it. */
#ifndef AZGYM_TRAIN_ERRORS_H
#define AZGYM_TRAIN_ERRORS_H
#include "azgym_train_weighted.h"

#ifdef __cplusplus
extern "C" {
#endif

int azg_trainer_loss_errors(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                            const float* weights, float* errors, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfg,
                            const azg_alpha_state* alpha_state, float* d_raw, float* losses);
int azg_trainer_loss_nets_errors(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                                 const float* weights, float* errors, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfgs,
                                 const azg_alpha_state* alpha_state, float* d_raw, float* losses);

int azg_trainer_epoch_opt_errors(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, float* errors,
                                 const int32_t* order, int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfg,
                                 const azg_alpha_state* alpha_state, const azg_optim* opt, double* loss_sums, int32_t* n_minibatches);
int azg_trainer_epoch_nets_errors(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, float* errors,
                                  const int32_t* order, int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfgs,
                                  const azg_alpha_state* alpha_state, const azg_optim* opts, double* loss_sums, int32_t* n_minibatches);

#ifdef __cplusplus
}
#endif
#endif
