/* azgym_priority.h -- prioritised sampling from the device replay ring.  An extension of azgym_nstep.h's kept transitions; same ABI
 * version.
 *
 * Which stored rows are trained on, and which stored positions are reanalysed, was a uniform pick made on the host.  MuZero's priority
 * of a row is |v - z|: its search value against its (n-step) value target, and both already lie on the device (the kept float64 value
 * of azg_selfplay_keep_transitions and the row's V_target column).  This header adds one fixed-point priority q per stored row
 * (azg_selfplay_priorities) and two proportional draws that run on the device: row numbers per net in the form a training epoch takes
 * as its order (azg_selfplay_sample_rows), and one slot per game in the form azg_selfplay_reanalyse takes as `slots`
 * (azg_selfplay_sample_slots).  Only the drawn indices come back to the host.  The draw is biased towards large priorities; its
 * correction is the importance-sampling weight of every stored row (azg_selfplay_is_weights, below), which stays on the device for the
 * trainer's weighted losses (azgym_train_weighted.h).
 *
 * The rule is exact by construction: any implementation gives the same bits.
 *
 * Priority of the stored row (slot, tree).  float32 arithmetic unless said otherwise.
 *   d:  AZG_PRIO_VALUE_GAP: d = (float)fabs(v - (double)z), v the kept float64 value (azg_selfplay_keep_transitions), z the float32 in
 *       the row's V_target column as it stands.
 *       AZG_PRIO_GIVEN: d = given[slot][tree], the caller's host array ordered like azg_selfplay_rows ([size_steps][n_trees]): a
 *       training loop's own TD errors can drive the draw.
 *   p:  alpha == 0: p = 1.  Otherwise p = azg_expf(alpha * azg_logf(d + eps)) with azg_math.h's functions; the sum and the product are
 *       each rounded to float32 on their own (no fused multiply-add).
 *   q:  uint64 fixed point with 20 fractional bits: q = 1 if !(p >= 2^-20) (NaN lands here), q = 2^40 if p >= 2^20, otherwise
 *       q = (uint64)((double)p * 1048576.0).
 * Every q is at least 1, so every stored row can be drawn, and every sum of q is an exact integer below 2^63: the result does not depend
 * on the order of summation.
 *
 * Row draw: draw d of net k under sample_index.  Net k's rows are numbered as a training epoch over the ring numbers them:
 * i = slot * T + j, slot < size_steps in ring-slot order, j the game within the net (T games per net).  C[i] is the inclusive prefix sum
 * of q in that order, total = C[N - 1].
 *     w = azg_draw(cfg.seed, tree_id_base + k * T, sample_index, d, AZG_STREAM_SAMPLE)
 *     x = (uint64)w.v[0] << 32 | w.v[1]
 *     target = the high 64 bits of x * total
 * and the draw is the least i with C[i] > target.  Draws are with replacement.  Net k's draws depend on nothing but its own rows, its
 * first game's global id, the seed and the index: they are the draws of a one-net engine whose tree_id_base is that id.
 *
 * Slot draw: game t under sample_index.  The same construction over the stored slots of column t in ring-slot order, with
 *     w = azg_draw(cfg.seed, tree_id_base + t, sample_index, 0, AZG_STREAM_SLOT);
 * the result is the least slot whose running sum exceeds target.
 *
 * Importance-sampling weight of the stored row i of net k under beta: prioritised replay's (N P(i))^-beta divided by the largest such
 * weight any stored row of the same net has.  P(i) = q_i / total_k, so N and the total cancel:
 *     w_i = (q_min_k / q_i)^beta,   q_min_k = the least q over net k's stored rows (the set the row draw sums over).
 * q_min_k is an integer minimum (any order).  Then, float32 with every step rounded on its own (no fused multiply-add):
 *     beta == 0 or q_i == q_min_k:  w = 1.0f exactly;
 *     otherwise  r = (float)((double)q_min_k / (double)q_i)  (both at most 2^40: the conversions are exact, the division is rounded once,
 *     then once more to float32) and w = azg_expf(beta * azg_logf(r)).
 * Every w lies in [0, 1] and is whatever azg_expf returns, an underflow for a large beta included.  Normalised by the ring's minimum,
 * not by a minibatch's maximum, a row's weight does not depend on what else was drawn.
 *
 * Priorities fed back from the trainer (azg_selfplay_keep_errors, azg_selfplay_priorities_trained).  The third source of a row's d is
 * the learner's own value error on it: err [capacity_steps][n_trees] float32, slot-aligned with the rows, q and w.  An entry is the
 * error a trainer wrote when it last trained on the row -- e = (float)fabs((double)V - (double)z), azgym_train_errors.h -- or the
 * sentinel -1.0f: never trained on since the row was stored.  The switch-on fills the array with the sentinel and every
 * azg_selfplay_step resets the block of the slot it stores into; a clear, a reanalysis and an n-step call leave it alone.  The row's d:
 *   seen entry (err != -1.0f; NaN is seen):  d = err.
 *   unseen entry, AZG_UNSEEN_MAX:  d = the largest seen error of the row's net (the rows the row draw sums over), taken over the
 *       entries with err >= 0 only -- the sentinel and NaN do not count, +inf does.  Non-negative float32 values order like their bit
 *       patterns read as integers (-0.0f counts as +0.0f), so the maximum is an integer maximum, exact in any order.  A net with no such
 *       entry takes d = 1.0f.
 *   unseen entry, AZG_UNSEEN_VALUE_GAP:  AZG_PRIO_VALUE_GAP's d = (float)fabs(v - (double)z).
 *   unseen entry, AZG_UNSEEN_CONSTANT:  d = unseen_d.
 * p and q follow from d, alpha and eps exactly as above for every finite d.  A d that is NaN or +inf lies outside azg_logf's domain
 * (the function reads its argument's bits and would return a finite number near 89 for either), so with alpha != 0 the trained form
 * decides them before it: a NaN d has p = NaN, hence q = 1; a +inf d has p = +inf, hence q = 2^40.  alpha == 0 gives p = 1, q = 2^20,
 * for every row, these included. */
#ifndef AZGYM_PRIORITY_H
#define AZGYM_PRIORITY_H
#include "azgym_nstep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* where a row's d comes from */
enum { AZG_PRIO_VALUE_GAP = 0, AZG_PRIO_GIVEN = 1 };

/* Keep a priority per stored row beside the replay ring: q [capacity_steps][n_trees] uint64, slot-aligned with the rows, and the scratch
 * of the draws' prefix sums.  on = 1 / 0.  Allowed after azg_*selfplay_begin* at any ring size (priorities are computed by a call, not
 * by the self-play step); the next begin drops it.  AZG_E_STATE before any begin. */
int azg_selfplay_keep_priorities(azg_engine* e, int32_t on);

typedef struct azg_priority_config {
    int32_t struct_size;   /* sizeof(azg_priority_config) */
    int32_t source;        /* AZG_PRIO_* */
    float alpha;           /* >= 0 and finite; 0: every row alike */
    float eps;             /* > 0 and finite */
    const float* given;    /* AZG_PRIO_GIVEN: host array [size_steps][n_trees], every entry >= 0 (not NaN); else not read */
} azg_priority_config;

/* Write q for every stored row by the rule above, and nothing else.  Asynchronous like azg_selfplay_step: one kernel launch (after the
 * upload of `given`, which is copied before the call returns).  Refusals, before anything is launched and with q untouched: no begin or
 * no keep_priorities: AZG_E_STATE; AZG_PRIO_VALUE_GAP without azg_selfplay_keep_transitions: AZG_E_STATE; a wrong struct_size, an
 * unknown source, alpha negative or not finite, eps not positive or not finite: AZG_E_INVALID; AZG_PRIO_GIVEN with a NULL array or with
 * a negative or NaN entry: AZG_E_INVALID.  An empty ring: AZG_OK, nothing is launched. */
int azg_selfplay_priorities(azg_engine* e, const azg_priority_config* cfg);

/* The q of the stored rows, ordered like azg_selfplay_rows ([slot][tree]).  Returns the number of rows copied.  Synchronises the
 * engine's stream.  AZG_E_STATE without keep_priorities. */
int azg_selfplay_priority_values(azg_engine* e, uint64_t* q, size_t max_rows);

typedef struct azg_sample_config {
    int32_t struct_size;     /* sizeof(azg_sample_config) */
    int32_t n_order;         /* draws per net, >= 1 */
    uint32_t sample_index;   /* the draws' counter: the same index gives the same draws */
} azg_sample_config;

/* n_order row draws for every net into the host array order [n_nets][n_order].  The prefix sums and the draws run on the device; one
 * synchronisation and one copy of n_nets * n_order ints.  AZG_E_STATE if no azg_selfplay_priorities has run since the ring's set of
 * stored rows last changed -- a step, a clear or a begin changes it; a reanalysis or an n-step call does not: their priorities are
 * stale but valid -- and for an empty ring; AZG_E_INVALID for n_order < 1, a NULL pointer or a wrong struct_size. */
int azg_selfplay_sample_rows(azg_engine* e, const azg_sample_config* cfg, int32_t* order);

/* One slot draw per game into the host array slots [n_trees]: what azg_selfplay_reanalyse takes as its per-game slots.  The same
 * staleness rule and refusals as azg_selfplay_sample_rows. */
int azg_selfplay_sample_slots(azg_engine* e, uint32_t sample_index, int32_t* slots);

/* Write the importance-sampling weight w (the rule above) of every stored row into a device array [capacity_steps][n_trees] float32,
 * slot-aligned with the rows and with q, and nothing else.  Asynchronous like azg_selfplay_priorities: the per-net minimum in two
 * launches, then one thread per stored row.  The first call allocates the array and the minima (AZG_E_DEVICE if that fails: nothing is
 * launched); it goes where q goes (keep_priorities(0) drops it, the next begin frees it).  Refusals, before any launch and with the
 * array untouched: azg_selfplay_sample_rows' staleness rule and codes (no begin, no keep_priorities, no azg_selfplay_priorities since
 * the ring's set of stored rows last changed, an empty ring: AZG_E_STATE); beta negative or not finite: AZG_E_INVALID. */
int azg_selfplay_is_weights(azg_engine* e, float beta);

/* The device pointer of that array, for a trainer on the same GPU (azg_trainer_epoch_opt_weighted over the ring: the array is addressed
 * like the rows, with a row length of 1).  AZG_E_STATE without keep_priorities, and if no weights were computed since the set of stored
 * rows last changed or since the last azg_selfplay_priorities (a step, a clear, a begin or new priorities invalidate them; a reanalysis
 * or an n-step call does not). */
int azg_selfplay_is_weights_device(azg_engine* e, const float** w);

/* The stored rows' weights as the array holds them, ordered like azg_selfplay_rows.  Returns the number of rows copied.  Synchronises
 * the engine's stream.  AZG_E_STATE without keep_priorities or before the first azg_selfplay_is_weights. */
int azg_selfplay_is_weight_values(azg_engine* e, float* w, size_t max_rows);

/* ---- priorities fed back from the trainer's value errors (the rule: the last paragraph of the head comment) */

/* what an unseen row's d is */
enum { AZG_UNSEEN_MAX = 0, AZG_UNSEEN_VALUE_GAP = 1, AZG_UNSEEN_CONSTANT = 2 };

/* Keep a value error per stored row beside q: err [capacity_steps][n_trees] float32 and the scratch of the per-net maximum.  on = 1 /
 * 0.  Needs azg_selfplay_keep_priorities (AZG_E_STATE otherwise, for on = 1) and is allowed at any ring size, like it; every switch-on
 * fills the whole array with the sentinel -1.0f.  azg_selfplay_keep_priorities(0) switches it off too; the next begin drops it.  While
 * it is on, azg_selfplay_step also sets the n_trees entries of the slot it stores into to the sentinel: one asynchronous 32-bit fill
 * on the engine's stream, after the step's kernel launch, with no synchronisation, allocation or copy.  Off, a step's HIP calls are
 * what they were. */
int azg_selfplay_keep_errors(azg_engine* e, int32_t on);

/* The mutable device pointer of err, for a trainer on the same GPU (azg_trainer_epoch_opt_errors over the ring: the array is addressed
 * like the rows, with a row length of 1).  A switch-off and a new switch-on within one begin leave the array where it is (and refill it);
 * the next begin frees it.  AZG_E_STATE without keep_errors.  The engine orders its own fills and reads on its stream; a trainer that
 * writes from another stream finishes (its calls synchronise) before the next engine call that touches err. */
int azg_selfplay_errors_device(azg_engine* e, float** err);

/* The stored rows' errors as the array holds them, ordered like azg_selfplay_rows.  Returns the number of rows copied.  Synchronises
 * the engine's stream.  AZG_E_STATE without keep_errors. */
int azg_selfplay_error_values(azg_engine* e, float* err, size_t max_rows);

/* Upload errors in the same order: a caller's own errors, a restored checkpoint.  n_rows must equal the stored rows and every entry
 * must be -1.0f, NaN or >= 0: AZG_E_INVALID otherwise, with the array untouched.  AZG_E_STATE without keep_errors.  The array is
 * copied before the call returns. */
int azg_selfplay_set_error_values(azg_engine* e, const float* err, size_t n_rows);

typedef struct azg_trained_priority_config {
    int32_t struct_size;   /* sizeof(azg_trained_priority_config) */
    int32_t unseen;        /* AZG_UNSEEN_* */
    float alpha;           /* >= 0 and finite; 0: every row alike */
    float eps;             /* > 0 and finite */
    float unseen_d;        /* AZG_UNSEEN_CONSTANT: finite and >= 0; else not read */
} azg_trained_priority_config;

/* Write q for every stored row from err by the rule above, and nothing else; q counts as computed exactly as after
 * azg_selfplay_priorities (the draws accept it, weights computed before it are no longer handed out).  Asynchronous: one kernel
 * launch, after the per-net maximum's two under AZG_UNSEEN_MAX.  Refusals, before anything is launched and with q untouched: those of
 * azg_selfplay_priorities with their codes (no begin or no keep_priorities: AZG_E_STATE; a wrong struct_size, alpha negative or not
 * finite, eps not positive or not finite: AZG_E_INVALID), no keep_errors: AZG_E_STATE; an unknown unseen: AZG_E_INVALID;
 * AZG_UNSEEN_VALUE_GAP without azg_selfplay_keep_transitions: AZG_E_STATE; AZG_UNSEEN_CONSTANT with unseen_d negative or not finite:
 * AZG_E_INVALID.  An empty ring: AZG_OK, nothing is launched. */
int azg_selfplay_priorities_trained(azg_engine* e, const azg_trained_priority_config* cfg);

#ifdef __cplusplus
}
#endif
#endif
