/* azgym_train.h -- population training: one minibatch optimiser step of K nets of one shape in two launches, or three with the losses on the device too, and a
 * whole epoch of such steps in one call (an extension of azgym.h; same ABI version).
 *
 * A trainer owns scratch only.  The nets' parameters, the optimiser state and every batch tensor are the caller's device arrays on
 * the trainer's GPU, float32:
 *   params     [n_nets][P]   net k's parameters in azg_set_weights blob order (= state_dict order), P = azg_trainer_param_count.
 *                            This array is the master copy: azg_set_population_weights_device reads it as it stands.
 *   square_avg [n_nets][P]   torch.optim.RMSprop's square_avg of every parameter, same layout
 *   obs        [n_nets][n_rows][in_dim]      net k's own minibatch
 *   raw        [n_nets][n_rows][1 + n_dist]  value head, then the untransformed distribution head (azg_mlp_eval's `raw`)
 *   d_raw      [n_nets][n_rows][1 + n_dist]  d(loss of net k) / d raw
 *   grads      [n_nets][P]   (optional) the parameter gradients, before clipping and weight decay
 *   actions    [n_nets][n_rows][n_actions]   the searched actions of every row (indices for a discrete head), n_actions <= 16
 *   counts     [n_nets][n_rows][n_actions]   their visit counts
 *   values     [n_nets][n_rows]              the value targets
 *   losses     [n_nets][AZG_LOSS_SLOTS]      loss, policy_loss, value_loss, entropy_loss, alpha_loss (0 where a slot does not apply)
 * Device memory is shared the way azg_set_weights_device shares it: inputs are complete when a call is made (their producer's
 * stream synchronised), outputs are complete when it returns.  With the losses in PyTorch (azg_trainer_forward, autograd on raw,
 * azg_trainer_backward_step) that is two synchronisations per minibatch step, whatever n_nets; azg_trainer_step takes the losses on
 * the device as well (azg_trainer_loss's kernel between the two) and synchronises once.  azg_trainer_epoch takes a whole epoch of
 * such steps: it gathers every minibatch from the caller's replay rows where they lie (the self-play ring included) and
 * synchronises once per epoch, whatever the number of minibatches.
 *
 * The optimiser is torch.optim.RMSprop applied in the backward kernel's tile epilogues (azg_rmsprop: the default, no gradient
 * clipping), or, through the *_opt entry points (azg_optim), RMSprop or torch.optim.Adam with an optional per-net clip_grad_norm_:
 * the backward launch then writes the gradients first and runs norm, clip and update as a phase after the last layer.  The *_nets
 * entry points take one azg_optim and one azg_loss_cfg per net, so the nets of one call can differ in every numeric setting.
 *
 * Supported nets: Linear + activation trunks of 1..3 hidden layers, widths multiples of 16 up to 256, in_dim <= 8, n_dist <= 16,
 * every AZG_ACT_* activation; LayerNorm after every trunk activation (nn.LayerNorm's defaults: eps 1e-5, affine) only from a trainer
 * made by azg_trainer_create_ex with options.layernorm set.  Anything else: AZG_E_UNSUPPORTED from azg_trainer_create(_ex).
 * azg_trainer_create_wide takes every shape the search engine takes -- 1..AZG_MAX_HIDDEN_LAYERS (8) hidden layers, widths multiples
 * of 16 up to 1024, no LayerNorm -- and spreads every layer over the chip: one launch per layer in the forward pass, two per layer
 * in the backward pass.  A shape both constructors accept gives the same bits from either trainer.
 * azg_trainer_create_wide_ex with options.layernorm set takes the same shapes with or without LayerNorm after every trunk
 * activation: with it, 2 * n_hidden + 1 launches forward and 3 * n_hidden + 1 backward (a row pass per LayerNorm and direction), and
 * for 1..3 layers of width <= 256 the bits of azg_trainer_create_ex's trainer.
 * The arithmetic is float32 on v_mfma_f32_16x16x4_f32 with a fixed summation order and no atomics: the same inputs give the same
 * bits on every run, and net k's results do not depend on n_nets.  Rows are padded to 16 inside; padded rows contribute nothing.
 * The loss kernel computes every row's terms in float64 from the float32 inputs and every sum over the rows as fixed-order float64
 * chains; d_raw and the loss values are rounded to float32 once. */
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

/* azg_trainer_create with options.  layernorm != 0: a descriptor with layernorm = 1 is accepted as well (one without runs the same
 * kernels azg_trainer_create's trainer runs); every other limit is azg_trainer_create's.  Per trunk layer the parameters are then
 * weight, bias, ln.weight, ln.bias (state_dict order), and P counts them.  Every entry point below works on such a trainer unchanged;
 * the trunk computes Y = LayerNorm(act(Y_prev W^T + b)) with the row statistics in float64 from the float32 activations (a fixed
 * order over a row's columns, independent of n_nets and n_rows), and the gradients of ln.weight / ln.bias are sums over the rows in
 * db's fixed order.  NULL opts or a wrong opts->struct_size: AZG_E_INVALID. */
typedef struct azg_trainer_options {
    int32_t struct_size;
    int32_t layernorm;
} azg_trainer_options;
int azg_trainer_create_ex(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const azg_trainer_options* opts,
                          azg_trainer** out);

/* A trainer for wide nets.  Accepted: Linear + activation trunks of 1..AZG_MAX_HIDDEN_LAYERS hidden layers of widths 16, 32, ... 1024,
 * in_dim <= 8, n_dist <= 16, every AZG_ACT_* activation.  desc->layernorm set (wide LayerNorm trunks are not built) and every other
 * shape outside that set: AZG_E_UNSUPPORTED with a message (azg_trainer_last_error(NULL)); NULL pointers, n_nets < 1 or max_batch < 1:
 * AZG_E_INVALID; a max_batch whose scratch offsets do not fit 32 bits, or a failed allocation: an error code, nothing is leaked
 * and *out is untouched.  The handle is an ordinary azg_trainer: every entry point of this header works on it with the same
 * signatures, checks, error codes, stream behaviour and "on an error nothing is written" rule.  Where azg_trainer_create's trainer
 * makes one launch for the forward pass and one for the backward pass, this one makes a launch per layer and role on the same
 * stream: n_hidden + 1 forward (the layers, the heads) and 2 * n_hidden + 1 backward ((a) dZ of the layer below, (b) dW, db and the
 * optimiser step of the layer; (a) of a layer reads the weights that (b) of the same layer, in the next launch, rewrites); the
 * deferred form (azg_optim with Adam, grad_clip or grad_norms) adds one launch for the norm's 1024 partial chains and one for norm
 * tree, clip and update.  No atomics and no waiting between workgroups.  The summation orders are azg_trainer_create's for every
 * width: an output element is one accumulator chain over its k-blocks of 16 in order, dW sums the batch tiles in order, db is four
 * float64 chains, the norm is 1024 float64 chains and a pairwise tree; so the results do not depend on n_nets or on the run, the
 * fused and the deferred form give the same gradients, and for 1..3 layers of width <= 256 every output (raw, gradients, params,
 * optimiser state, grad_norms, d_raw, losses, an epoch's results) has the bits azg_trainer_create's trainer gives. */
int azg_trainer_create_wide(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out);

/* azg_trainer_create_wide with options.  opts->layernorm != 0: everything azg_trainer_create_wide accepts, with desc->layernorm 0 or
 * 1 (a descriptor without LayerNorm runs exactly the launches of azg_trainer_create_wide's trainer); opts->layernorm == 0: it is
 * azg_trainer_create_wide, its refusal of a LayerNorm descriptor included.  NULL opts or a wrong opts->struct_size: AZG_E_INVALID;
 * every other code and message is azg_trainer_create_wide's, *out is untouched on an error and nothing is leaked.  With LayerNorm
 * the parameters per trunk layer are weight, bias, ln.weight, ln.bias (state_dict order) and P counts them; every entry point works
 * on the handle unchanged.  The arithmetic is azg_trainer_create_ex's, element for element: a row's sums (the mean, the variance of
 * the centred values, backward the means of dx = G * gamma and of dx * X) are sixteen float64 chains -- lane c of the row's sixteen
 * adds columns c, c + 16, ... in order, 64 links at width 1024 -- combined by the same butterfly, divided by the width in float64
 * and rounded once; dgamma and dbeta are db's four float64 chains over the rows.  So for 1..3 layers of width <= 256 every output
 * has the bits azg_trainer_create_ex's trainer gives, and at every width the results depend on neither n_nets nor the run.  Where
 * the one-workgroup kernels have a barrier this trainer has a launch: behind every trunk layer's forward launch a row pass (Y in
 * A's place, X and rstd kept), 2 * n_hidden + 1 launches forward; backward, per layer above the first, (a) stores G = dZ W, a row
 * pass of the LayerNorm below turns act' into dZ of the layer below, and (b) also emits that LayerNorm's dgamma and dbeta into the
 * same optimiser step or gradient store, 3 * n_hidden + 1 launches -- so gamma, like W, is read in a launch before the one that
 * steps it.  The deferred form's two launches are azg_trainer_create_wide's. */
int azg_trainer_create_wide_ex(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const azg_trainer_options* opts,
                               azg_trainer** out);

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

/* ---- Adam, and gradient clipping: the optimiser as a phase of its own after the backward pass ---- */

enum { AZG_OPT_RMSPROP = 0, AZG_OPT_ADAM = 1 };

/* The optimiser of the *_opt entry points, with its state: the caller's device arrays [n_nets][P] float32, updated in place.
 *   AZG_OPT_RMSPROP  torch.optim.RMSprop(lr, alpha, eps, weight_decay), momentum 0, not centered; state0 = square_avg
 *   AZG_OPT_ADAM     torch.optim.Adam(lr, (beta1, beta2), eps, weight_decay), single-tensor form, no amsgrad:
 *                    g += weight_decay * p;  exp_avg += (g - exp_avg) * (1 - beta1);  exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) g g;
 *                    p -= lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps),  t = step + 1;
 *                    state0 = exp_avg_sq, state1 = exp_avg.  `step` = the Adam steps taken before this call (the caller counts).
 * grad_clip != 0: torch.nn.utils.clip_grad_norm_(net k's parameters, grad_clip) between the backward pass and the step, per net:
 * total_norm = the L2 norm of all P gradients (float64 sum in a fixed order, rounded to float32 once), every gradient times
 * min(grad_clip / (total_norm + 1e-6), 1).  grad_norms (may be NULL): [n_nets] float32 device array that receives every net's
 * total_norm, before clipping.
 * With AZG_OPT_RMSPROP, grad_clip == 0 and no grad_norms a call runs the fused kernel of azg_trainer_backward_step and gives its
 * bits.  Otherwise the backward launch takes its deferred form: the same GEMMs in the same order write the gradients to `grads`
 * (or to the trainer's own [n_nets][P] array) and no parameter; then, in the same launch, norm, clip and update.  The gradients are
 * bit for bit the fused form's; RMSprop's arithmetic is the fused form's, Adam's is float64 per element, rounded once. */
typedef struct azg_optim {
    int32_t struct_size;
    int32_t kind;          /* AZG_OPT_* */
    double lr, eps, weight_decay;
    double alpha;          /* AZG_OPT_RMSPROP */
    double beta1, beta2;   /* AZG_OPT_ADAM */
    double grad_clip;      /* 0 = off */
    float* state0;
    float* state1;         /* AZG_OPT_ADAM only (else ignored) */
    float* grad_norms;     /* optional */
    int32_t step;          /* AZG_OPT_ADAM */
} azg_optim;

/* azg_trainer_backward_step with an azg_optim in place of (azg_rmsprop, square_avg).  grads (may be NULL) receives the gradients
 * before clipping and weight decay.  NULL params / d_raw / opt / state0, NULL state1 with Adam, a struct_size mismatch, lr < 0,
 * eps < 0, a beta outside [0, 1) (Adam), grad_clip < 0, step < 0, n_rows outside 1..max_batch:
 * AZG_E_INVALID; an unknown kind: AZG_E_UNSUPPORTED; no azg_trainer_forward of the same n_rows before it: AZG_E_STATE.  On an error
 * nothing is written. */
int azg_trainer_backward_step_opt(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_optim* opt, float* grads);

/* ---- the losses on the device (agent/population_trainer.py: population_terms / population_loss, restated as one kernel) ---- */

enum { AZG_LOSS_ALPHAZERO = 0, AZG_LOSS_A0C = 1, AZG_LOSS_A0C_TUNED = 2 };
enum { AZG_HEAD_DISCRETE = 0, AZG_HEAD_NORMAL = 1, AZG_HEAD_GMM = 2 };
enum { AZG_REDUCE_MEAN = 0, AZG_REDUCE_SUM = 1 };
/* slots of losses[k][] */
enum { AZG_LOSS_TOTAL = 0, AZG_LOSS_POLICY = 1, AZG_LOSS_VALUE = 2, AZG_LOSS_ENTROPY = 3, AZG_LOSS_ALPHA = 4, AZG_LOSS_SLOTS = 5 };

/* What the loss object and the policy carry beyond azg_mlp_desc (which gives n_dist, num_components and the log_std clamp).
 *   AZG_LOSS_ALPHAZERO  policy_coeff * CE(logits, argmax counts, lowest index on ties) + value_coeff * MSE; discrete head only,
 *                       n_actions == n_dist
 *   AZG_LOSS_A0C        policy_coeff * reduce_rows(sum_i (log pi_i - tau log n_i).detach() * log pi_i) + alpha * reduce(entropy)
 *                       + value_coeff * MSE;  n_i = counts_i + 1 for a discrete head
 *   AZG_LOSS_A0C_TUNED  the same with alpha = exp(log_alpha[k]) from before the call, then one Adam step (torch.optim.Adam's
 *                       single-tensor form, no amsgrad) of log_alpha[k] on alpha_loss = mean(alpha * (entropy - target_entropy)), its
 *                       gradient scaled by min(alpha_clip / (|g| + 1e-6), 1) when alpha_clip != 0
 * Heads: DISCRETE (Categorical over n_dist logits; actions are indices 0 .. n_dist - 1; entropy per (row, action) = the row's
 * Categorical entropy), NORMAL (n_dist = 2: mu, log_std) and GMM (n_dist = 3 C: mu | log_std | log_coeff, C <= 5), both of
 * one-dimensional actions squashed to (-action_bound, action_bound) as network/distributions.py's SquashedNormal computes it
 * (action_bound == 0: a plain Normal); entropy per row = -mean_i log pi_i. */
typedef struct azg_loss_cfg {
    int32_t struct_size;
    int32_t kind;        /* AZG_LOSS_* */
    int32_t head;        /* AZG_HEAD_* */
    int32_t reduction;   /* AZG_REDUCE_* */
    double tau, policy_coeff, value_coeff;
    double alpha;            /* AZG_LOSS_A0C */
    double target_entropy;   /* AZG_LOSS_A0C_TUNED, and the Adam settings of log_alpha: */
    double alpha_lr, alpha_beta1, alpha_beta2, alpha_eps, alpha_weight_decay, alpha_clip;
    double action_bound;
} azg_loss_cfg;

/* AZG_LOSS_A0C_TUNED's state, the caller's device arrays [n_nets] float32, updated in place; `step` = the Adam steps taken before
 * this call (the caller counts). */
typedef struct azg_alpha_state {
    int32_t struct_size;
    int32_t step;
    float* log_alpha;
    float* exp_avg;
    float* exp_avg_sq;
} azg_alpha_state;

/* The loss kernel alone, one launch for every net: from raw, the batch and the loss settings to d_raw = d loss_k / d raw[k] (what
 * population_loss(...)["loss"].sum().backward() leaves in raw.grad) and losses; with AZG_LOSS_A0C_TUNED also the Adam step of
 * log_alpha.  alpha_state is needed for AZG_LOSS_A0C_TUNED only (else it may be NULL).  NULL required pointers, n_rows outside
 * 1..max_batch, n_actions outside 1..16 (or != n_dist with AZG_LOSS_ALPHAZERO), a struct_size mismatch: AZG_E_INVALID; an unknown
 * kind / head / reduction, AZG_LOSS_ALPHAZERO with a continuous head, more than 5 components or an n_dist that does not fit the
 * head: AZG_E_UNSUPPORTED.  On an error nothing is written. */
int azg_trainer_loss(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values, int32_t n_rows,
                     int32_t n_actions, const azg_loss_cfg* cfg, const azg_alpha_state* alpha_state, float* d_raw, float* losses);

/* One whole minibatch step of every net: azg_trainer_forward, azg_trainer_loss and azg_trainer_backward_step enqueued back to back
 * with one synchronisation at the end.  raw_out (may be NULL) receives raw; d_raw stays in the trainer (azg_trainer_read_d_raw).
 * Every check of the three calls is made before the first launch: on an error nothing is written. */
int azg_trainer_step(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                     int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                     const azg_rmsprop* opt, float* square_avg, float* grads, float* raw_out, float* losses);

/* azg_trainer_step with an azg_optim: every check of azg_trainer_step and azg_trainer_backward_step_opt before the first launch. */
int azg_trainer_step_opt(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                         int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                         const azg_optim* opt, float* grads, float* raw_out, float* losses);

/* Copies the d_raw [n_nets][n_rows][1 + n_dist] of the last azg_trainer_step to the caller's device array (AZG_E_STATE if there
 * was none of that n_rows). */
int azg_trainer_read_d_raw(azg_trainer* t, int32_t n_rows, float* d_raw);

/* ---- a whole epoch of minibatch steps in one call ---- */

/* Where the replay rows lie.  A row is row_len floats: obs[state_dim] | actions[A] | counts[A] | Q[A] | V_target, A = n_actions
 * (azg_selfplay_rows' layout).  Net k can be asked for rows 0 .. rows_per_net - 1;
 *   row i of net k lives at rows + ((i / group) * group_stride + k * net_stride + i % group) * row_len.
 * A plain [n_nets][n][row_len] array: group = n, net_stride = n (group_stride is never multiplied by anything but 0).
 * The self-play ring [capacity_steps][n_trees][row_len] of azg_selfplay_rows_device, net k playing games k*T .. k*T + T - 1:
 * group = T, group_stride = n_trees, net_stride = T -- net k's row i is step i / T, game i % T.
 * The caller vouches that every such address lies inside its allocation. */
typedef struct azg_epoch_rows {
    int32_t struct_size;
    int32_t row_len;
    int32_t state_dim, n_actions;
    int32_t rows_per_net;
    int32_t group;
    int64_t group_stride;
    int64_t net_stride;
    const float* rows;   /* device */
} azg_epoch_rows;

/* One epoch of azg_trainer_step calls of every net.  order is HOST memory, [n_nets][n_order] row numbers of each net; consecutive
 * slices of batch_size entries are the minibatches, the last one absorbing the remainder (from position i the next minibatch ends
 * at n_order if i + 2 * batch_size > n_order, else at i + batch_size), so a minibatch has 1 .. 2 * batch_size - 1 rows.  Per
 * minibatch m one gather launch (order and the rows to the trainer's staging arrays; the Q columns are not read) and the three
 * launches of azg_trainer_step with alpha_state->step + m, all enqueued without a synchronisation; then one launch adds every
 * minibatch's float32 losses[k][slot] in minibatch order in one float64 chain from 0.0 into loss_sums (device,
 * [n_nets][AZG_LOSS_SLOTS] float64, not rounded), and the call synchronises once.  *n_minibatches receives their number: the Adam steps
 * the caller adds to its count.  params, square_avg and the alpha state end bit for bit where the same minibatches passed one by
 * one to azg_trainer_step leave them.
 * NULL pointers, a struct_size mismatch, batch_size < 1, n_order < 1, n_actions outside 1..16, row_len != state_dim +
 * 3 * n_actions + 1, state_dim != the descriptor's in_dim, rows_per_net < 1, group < 1, negative strides, an order entry outside
 * 0 .. rows_per_net - 1, a largest minibatch beyond max_batch: AZG_E_INVALID; whatever azg_trainer_step refuses is refused with
 * its code.  Every check is made before the first launch: on an error nothing is written. */
int azg_trainer_epoch(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                      int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_rmsprop* opt,
                      float* square_avg, double* loss_sums, int32_t* n_minibatches);

/* azg_trainer_epoch with an azg_optim: minibatch m steps with opt->step + m (and alpha_state->step + m); the caller adds
 * *n_minibatches to both counts.  grad_norms, if given, ends up holding the last minibatch's norms.  params, the optimiser state and
 * the alpha state end bit for bit where the same minibatches passed one by one to azg_trainer_step_opt leave them. */
int azg_trainer_epoch_opt(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                          int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_optim* opt,
                          double* loss_sums, int32_t* n_minibatches);

/* ---- settings per net: a learning-rate (or clip, tau, entropy coefficient ...) sweep in one call ---- */

/* The four *_nets entry points are azg_trainer_backward_step_opt, azg_trainer_loss, azg_trainer_step_opt and azg_trainer_epoch_opt
 * with HOST arrays of n_nets entries, entry k for net k, where those take one struct.  They work on every trainer handle.
 *   may differ per net   azg_optim: lr, eps, weight_decay, alpha, beta1, beta2, grad_clip
 *                        azg_loss_cfg: tau, policy_coeff, value_coeff, alpha, target_entropy, alpha_lr, alpha_beta1, alpha_beta2,
 *                        alpha_eps, alpha_weight_decay, alpha_clip
 *   equal in every entry azg_optim: struct_size, kind, state0, state1, grad_norms, step (the state arrays are [n_nets][P] as before);
 *                        azg_loss_cfg: struct_size, kind, head, reduction, action_bound.  An entry k >= 1 that differs from entry 0
 *                        in one of them: AZG_E_INVALID, the message names the field and k; this is checked before the entries'
 *                        own values.
 * Every entry passes the checks of the *_opt call with their codes (entry 0 first, as that call would make them; the message of a
 * later entry names its net).  All checks are made before the first launch: on an error nothing is written.
 * Net k's outputs -- params, state0 / state1, grads, grad_norms, d_raw, losses, log_alpha and its Adam state, an epoch's loss_sums --
 * are bit for bit what a one-net trainer of the same shape, given entry k through the *_opt entry point, produces from net k's
 * slices; n_nets identical entries give the *_opt call's bits.  The backward pass always takes its deferred form (whose gradients
 * and RMSprop arithmetic are the fused form's, see azg_optim), and the norm, the clip and the bias corrections are per net: a net
 * with grad_clip == 0 is not clipped because another net is, and Adam's 1 - beta^t is computed on the host from entry k's betas.
 * The launch-ready settings of every (minibatch, net) go to a device table of the trainer (grown on demand; a failed allocation is
 * an error before any launch) in one asynchronous copy on the trainer's stream in front of the first launch; every workgroup reads
 * its net's entry from there.  An epoch uploads all its minibatches' entries at once and still synchronises once. */
int azg_trainer_backward_step_nets(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_optim* opts /* [n_nets] */,
                                   float* grads);
int azg_trainer_loss_nets(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values, int32_t n_rows,
                          int32_t n_actions, const azg_loss_cfg* cfgs /* [n_nets] */, const azg_alpha_state* alpha_state, float* d_raw,
                          float* losses);
int azg_trainer_step_nets(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                          int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfgs /* [n_nets] */,
                          const azg_alpha_state* alpha_state, const azg_optim* opts /* [n_nets] */, float* grads, float* raw_out,
                          float* losses);
int azg_trainer_epoch_nets(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                           int32_t batch_size, const azg_loss_cfg* loss_cfgs /* [n_nets] */, const azg_alpha_state* alpha_state,
                           const azg_optim* opts /* [n_nets] */, double* loss_sums, int32_t* n_minibatches);

#ifdef __cplusplus
}
#endif
#endif
