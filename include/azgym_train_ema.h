/* azgym_train_ema.h -- a slowly moving copy of every net's parameters, kept on the device: an exponential moving average updated by one
 * launch behind the optimiser step.  An extension of azgym_train.h; same ABI version.  A library may lack these symbols.
 *
 * The rule, per parameter element, in float32 with every operation rounded by itself (no fused multiply-add):
 *     ema' = ema + om_k * (p - ema),      om_k = (float)(1.0 - decay_k)      (the subtraction in float64 on the host)
 * with p the parameter after the optimiser step and k the element's net.  numpy float32 arithmetic reproduces it bit for bit.  A net
 * whose parameters do not move and whose ema equals them keeps ema == p exactly.  decay 0 gives om = 1: ema + (p - ema), which is p up
 * to one rounding.
 *
 * What runs.  While an average is attached, every optimiser step the trainer takes -- azg_trainer_backward_step*, azg_trainer_step*,
 * every minibatch of every azg_trainer_epoch* form (weighted, errors, online), on every kind of handle (azg_trainer_create, _ex, _wide,
 * _wide_ex) and in every optimiser form (azg_rmsprop, azg_optim, the *_nets tables) -- is counted, from 1 since the attach; behind the
 * backward launch of step s with s % every == 0 one streaming kernel over the n_nets * P floats follows on the trainer's stream.  It
 * adds no synchronisation and no copy.  The count goes on across calls: with every = 3, two epochs of 5 minibatches update after steps
 * 3, 6 and 9.  With nothing attached every entry point launches exactly what it launched before this header existed.
 *
 * `ema` is the caller's device array [n_nets][P] (P = azg_trainer_param_count), initialised by the caller (a copy of the parameters
 * makes warm-up or debiasing unnecessary) and kept alive until the average is detached or the trainer destroyed.  The kernel pairs it
 * with the `params` of the call that steps: ema must not overlap them.  Both 16-byte aligned (any allocation's start): 16-byte loads
 * and stores; otherwise element by element, same numbers.
 *
 * Not provided: warm-up / debiased decays; averages of the optimiser's moments or of the learned temperature. */
#ifndef AZGYM_TRAIN_EMA_H
#define AZGYM_TRAIN_EMA_H
#include "azgym_train.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct azg_ema_cfg {
    int32_t       struct_size;   /* sizeof(azg_ema_cfg) */
    int32_t       n_decay;       /* 1 (every net) or the trainer's n_nets (net k: decay[k]) */
    int32_t       every;         /* >= 1: the average moves after every `every`-th optimiser step */
    int32_t       reserved;      /* 0 */
    float*        ema;           /* DEVICE [n_nets][P], caller-owned */
    const double* decay;         /* HOST [n_decay], each finite and in [0, 1); read during the call only */
} azg_ema_cfg;

/* Attaches the average (replacing one already attached; the step count starts again at 0), or with cfg == NULL detaches it.  Refused
 * with AZG_E_INVALID and the trainer left as it was: a wrong struct_size, a NULL ema or decay, n_decay neither 1 nor n_nets, every < 1,
 * a decay that is not finite or outside [0, 1).  The trainer keeps the pointer, a device table of one float per net (om) and the counts. */
int azg_trainer_set_ema(azg_trainer* t, const azg_ema_cfg* cfg);

/* The counts since the last attach (both 0 when nothing is attached): optimiser steps seen, and launches of the average's kernel.
 * Either pointer may be NULL. */
int azg_trainer_ema_info(const azg_trainer* t, int64_t* steps_seen, int64_t* updates_made);

#ifdef __cplusplus
}
#endif
#endif
