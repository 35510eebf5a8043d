/* azgym_target.h -- a second weight set in the engine: the games go on with the live weights while stored positions are re-searched,
 * or the nets scored, with a target set (a slowly moving average of the trainer's parameters, azgym_train_ema.h).  An extension of
 * azgym.h and azgym_population.h; same ABI version.  A library may lack these symbols.
 *
 * The engine has two weight sets of the same packed layout, LIVE and TARGET, and one of them is in use: every upload entry point
 * (azg_set_weights, _device, azg_set_net_weights, _device, azg_set_population_weights_device) writes the set in use, and everything
 * that runs a network -- searches, self-play, reanalysis, rollouts, evaluations -- reads it.  An engine starts with LIVE in use and
 * TARGET empty; the TARGET buffer is allocated by the first upload while TARGET is in use.  An engine that never selects TARGET
 * behaves, and allocates, exactly as it did before this header existed.
 *
 * Selecting a set first settles an abandoned team search (as an upload does), then points the kernels' weight arguments at the set
 * and counts as an upload for everything cached about the last search: its results are computed again when asked for, and
 * azg_dump_tree does not re-run it.  No stream synchronisation: launches already made hold their pointers by value.
 *
 * Both sets share one network descriptor and one weight map.  An upload whose descriptor differs from the one in force (shape,
 * activation or head settings) empties the OTHER set, and so does azg_set_population with another number of nets: selecting that set
 * then leaves the engine without weights, and a search fails with its usual no-weights error until the set is uploaded again.
 *
 * Not provided: more than two sets; a choice of set per net within one launch. */
#ifndef AZGYM_TARGET_H
#define AZGYM_TARGET_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { AZG_WEIGHTS_LIVE = 0, AZG_WEIGHTS_TARGET = 1 };

/* Selects the set in use.  AZG_E_INVALID: a NULL engine or another value of `which`. */
int azg_use_weights(azg_engine* e, int32_t which);

/* *in_use: AZG_WEIGHTS_LIVE or AZG_WEIGHTS_TARGET; *target_ready: 1 when every net of the TARGET set has weights.  Either pointer may
 * be NULL. */
int azg_weights_info(const azg_engine* e, int32_t* in_use, int32_t* target_ready);

#ifdef __cplusplus
}
#endif
#endif
