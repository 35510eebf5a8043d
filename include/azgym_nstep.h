/* azgym_nstep.h -- n-step return value targets for the device replay ring.  An extension of azgym.h's device self-play; same ABI
 * version.
 *
 * A replay row's V_target column is the root value of the search that produced the row (azg_config.v_target).  The rewards the game
 * actually paid are not in the row, so the engine keeps them itself on request (azg_selfplay_keep_transitions): four slot-aligned
 * blocks [capacity_steps][n_trees] beside the ring -- the step's reward, its search value as a double, the action taken and how the
 * step ended -- written by the self-play step.  azg_selfplay_nstep_targets then rewrites the V_target column of every stored row as
 *
 *     z_s = r_s + gamma r_{s+1} + ... + gamma^{m-1} r_{s+m-1} + gamma^m v_{s+m}
 *
 * where v is the kept search value: a reanalysis (azgym_reanalyse.h) refreshes v, this call turns it into targets (MuZero's recipe).
 *
 * The rule, for the row at chronological position s of its game column (0: the oldest stored step, last: the newest):
 *   - a step e in s .. s + n_step - 1 that ended its episode by the env's own "done" (AZG_END_TERMINAL) closes the window: the target
 *     is the discounted sum of the rewards s .. e and nothing else -- a terminal state is worth 0;
 *   - otherwise the window bootstraps from the search value of step L = min(s + n_step, last, the first step in s .. s + n_step - 1
 *     that ended by the length limit alone): the target is the discounted rewards s .. L - 1 plus gamma^(L - s) v_L.  The state after a
 *     time-limit step is a reset, its value is unknown, so the window stops at that step's own root; likewise at the newest stored
 *     step, whose successors have not been played yet.
 * The sum is folded from the far end, acc = r_i + gamma * acc in float64 with the product and the sum rounded separately, so the plain
 * numpy recurrence gives the same bits; (float)acc goes into the column.  n_step = 0 writes (float)v_s: the column as the step or the
 * reanalysis left it.  The call is idempotent (it reads the kept doubles, never the column); repeating it after more steps changes
 * only rows whose window grew.  Clearing the ring restarts the kept transitions with it: no window looks behind a clear. */
#ifndef AZGYM_NSTEP_H
#define AZGYM_NSTEP_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How a stored step ended: not at all, by the env's "done" (also where the length limit fell on the same step), by the length limit alone */
enum { AZG_END_NONE = 0, AZG_END_TERMINAL = 1, AZG_END_LENGTH = 2 };

/* Keep every stored step's transition beside the replay ring, slot-aligned with the rows, structure of arrays [capacity_steps][n_trees]:
 *   reward float64 : the reward of the real env step in the units a tree node holds (continuous mode: divided by
 *                    azg_config.reward_scale; discrete mode: as the env pays it)
 *   value  float64 : the step's value target before its rounding to the row's float32 (azg_config.v_target's form); a reanalysis
 *                    of row (slot, t) overwrites it with the fresh search's
 *   action float32 : the action taken
 *   end    int32   : AZG_END_*
 * on = 1 / 0.  Allowed after azg_*selfplay_begin* while the ring is empty (size_steps == 0), else AZG_E_STATE; the next begin drops it. */
int azg_selfplay_keep_transitions(azg_engine* e, int32_t on);

/* The kept transitions of the stored steps, ordered like azg_selfplay_rows ([slot][tree]); any pointer may be NULL.  Returns the number
 * of rows copied.  Synchronises the engine's stream.  AZG_E_STATE without keep_transitions. */
int azg_selfplay_transitions(azg_engine* e, double* reward, double* value, float* action, int32_t* end, size_t max_rows);

/* flags: discount with the search's own gamma -- azg_net_search.gamma of the row's net where a per-net table is set
 * (azg_set_net_search), azg_config.gamma otherwise; `gamma` is then ignored */
enum { AZG_NSTEP_SEARCH_GAMMA = 1 };

typedef struct azg_nstep_config {
    int32_t struct_size;   /* sizeof(azg_nstep_config) */
    int32_t n_step;        /* >= 0; anything beyond the ring's size is the whole stored game */
    double gamma;          /* >= 0 and finite, unless AZG_NSTEP_SEARCH_GAMMA */
    int32_t flags;         /* AZG_NSTEP_* */
} azg_nstep_config;

/* Rewrite the V_target column of every stored row by the rule above; nothing else is written.  Asynchronous like azg_selfplay_step:
 * one kernel launch.  Refusals, before anything is launched and with the ring untouched: no begin or no keep_transitions:
 * AZG_E_STATE; a wrong struct_size, n_step < 0, unknown flag bits, or without AZG_NSTEP_SEARCH_GAMMA a gamma that is negative, NaN or
 * infinite: AZG_E_INVALID.  An empty ring: AZG_OK, nothing is launched. */
int azg_selfplay_nstep_targets(azg_engine* e, const azg_nstep_config* cfg);

#ifdef __cplusplus
}
#endif
#endif
