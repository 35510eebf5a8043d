/* azgym_priority.h -- prioritised sampling from the device replay ring.  An extension of azgym_nstep.h's kept transitions; same ABI
 * version.
 *
 * Which stored rows are trained on, and which stored positions are reanalysed, was a uniform pick made on the host.  MuZero's priority
 * of a row is |v - z|: its search value against its (n-step) value target, and both already lie on the device (the kept float64 value
 * of azg_selfplay_keep_transitions and the row's V_target column).  This header adds one fixed-point priority q per stored row
 * (azg_selfplay_priorities) and two proportional draws that run on the device: row numbers per net in the form a training epoch takes
 * as its order (azg_selfplay_sample_rows), and one slot per game in the form azg_selfplay_reanalyse takes as `slots`
 * (azg_selfplay_sample_slots).  Only the drawn indices come back to the host.  The draw is biased towards large priorities and nothing
 * here corrects for it: importance-sampling weights are not part of this interface.
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
 * the result is the least slot whose running sum exceeds target. */
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

#ifdef __cplusplus
}
#endif
#endif
