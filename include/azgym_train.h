/* azgym_train.h -- population training: one minibatch optimiser step of K nets of one shape in two launches (an extension of
 * azgym.h; same ABI version).
 *
 * A trainer owns scratch only.  The nets' parameters, the RMSprop state and every batch tensor are the caller's device arrays on
 * the trainer's GPU, float32:
 *   params     [n_nets][P]   net k's parameters in azg_set_weights blob order (= state_dict order), P = azg_trainer_param_count.
 *                            This array is the master copy: azg_set_population_weights_device reads it as it stands.
 *   square_avg [n_nets][P]   torch.optim.RMSprop's square_avg of every parameter, same layout
 *   obs        [n_nets][n_rows][in_dim]      net k's own minibatch
 *   raw        [n_nets][n_rows][1 + n_dist]  value head, then the untransformed distribution head (azg_mlp_eval's `raw`)
 *   d_raw      [n_nets][n_rows][1 + n_dist]  d(loss of net k) / d raw
 *   grads      [n_nets][P]   (optional) the parameter gradients, before weight decay
 * Device memory is shared the way azg_set_weights_device shares it: inputs are complete when a call is made (their producer's
 * stream synchronised), outputs are complete when it returns.  That is two synchronisations per minibatch step, whatever n_nets.
 *
 * Supported nets: Linear + activation trunks of 1..3 hidden layers, widths multiples of 16 up to 256, in_dim <= 8, n_dist <= 16,
 * every AZG_ACT_* activation; no LayerNorm.  Anything else: AZG_E_UNSUPPORTED from azg_trainer_create.
 * The arithmetic is float32 on v_mfma_f32_16x16x4_f32 with a fixed summation order and no atomics: the same inputs give the same
 * bits on every run, and net k's results do not depend on n_nets.  Rows are padded to 16 inside; padded rows contribute nothing. */
#ifndef AZGYM_TRAIN_H
#define AZGYM_TRAIN_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct azg_trainer azg_trainer;

/* torch.optim.RMSprop(lr, alpha, eps, weight_decay, momentum=0, centered=False).  momentum, centered and grad_clip must be 0: a
 * per-net global gradient norm needs a pass of its own and is not built (AZG_E_UNSUPPORTED). */
typedef struct azg_rmsprop {
    int32_t struct_size;
    int32_t centered;
    double lr, alpha, eps, weight_decay;
    double momentum;
    double grad_clip;
} azg_rmsprop;

/* Scratch for n_nets nets of shape `desc` and minibatches of 1..max_batch rows per net.  NULL pointers, n_nets < 1 or
 * max_batch < 1: AZG_E_INVALID; a descriptor outside the supported set: AZG_E_UNSUPPORTED (message: azg_trainer_last_error(NULL)). */
int azg_trainer_create(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out);
void azg_trainer_destroy(azg_trainer* t);
const char* azg_trainer_last_error(const azg_trainer* t);
/* P: floats per net */
size_t azg_trainer_param_count(const azg_trainer* t);

/* The forward pass of a minibatch optimiser step (the network half of agents.py:319-392, 539-603: policy.get_train_data's
 * trunk and heads) for every net on its own n_rows rows: one launch.  Writes raw and keeps obs, every layer's activations and
 * activation derivatives in the trainer's scratch for azg_trainer_backward_step.  NULL pointers or n_rows outside
 * 1..max_batch: AZG_E_INVALID, nothing written. */
int azg_trainer_forward(azg_trainer* t, const float* params, const float* obs, int32_t n_rows, float* raw);

/* loss.backward() + optimizer.step() of the same step (agents.py:319-392, 539-603) for every net: one launch.  Back through
 * heads and trunk from d_raw, dW = dZ^T A and db = sum over rows of dZ, then torch's RMSprop update of params and square_avg in
 * place:  g += weight_decay * p;  square_avg = alpha * square_avg + (1 - alpha) * g * g;  p -= lr * g / (sqrt(square_avg) + eps).
 * grads (may be NULL) receives the gradients.  Needs the azg_trainer_forward of the same n_rows before it (else AZG_E_STATE);
 * NULL params / d_raw / opt / square_avg or n_rows outside 1..max_batch: AZG_E_INVALID; momentum, centered or grad_clip set:
 * AZG_E_UNSUPPORTED.  On an error nothing is written. */
int azg_trainer_backward_step(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_rmsprop* opt,
                              float* square_avg, float* grads);

#ifdef __cplusplus
}
#endif
#endif
