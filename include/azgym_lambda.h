/* azgym_lambda.h -- lambda-return value targets for the device replay ring, one rule per net.  An extension of azgym_nstep.h; same ABI
 * version.
 *
 * azg_selfplay_nstep_targets turns the kept transitions (azg_selfplay_keep_transitions) into ONE target per row: the rewards of a hard
 * window of n_step steps and the search value behind it.  The calls here mix the returns of every shorter window into it, TD(lambda)'s
 * way, and take the rule (n_step, lambda, gamma) per net of a population, so that one engine can compare n = 1 / 5 / all or lambda =
 * 0.5 / 0.9 / 1 across its nets in one launch.
 *
 * The rule, for the row at chronological position s of its game column (0: the oldest stored step, last: the newest), with the rule
 * (n_step, lambda, gamma) of the row's net:
 *   1. n_step == 0: the column gets (float)v_s, exactly as azg_selfplay_nstep_targets writes it.
 *   2. Otherwise the window's far end L and the flag `terminal` are azg_selfplay_nstep_targets' (azgym_nstep.h): the first step in
 *      s .. s + n_step - 1 that ended its episode closes the window -- a terminal end (AZG_END_TERMINAL) with no bootstrap, a length-limit
 *      end (AZG_END_LENGTH) at that step's own root --; if there is none, L = min(s + n_step, last).
 *   3. The target is folded from the far end in float64, every product and every sum rounded by itself, om = 1.0 - lambda computed
 *      once in float64:
 *
 *          acc = terminal ? 0.0 : v_L;   i = terminal ? L : L - 1
 *          if (i >= s) { acc = r_i + gamma * acc;  --i }             the first fold: the plain bootstrap (or the terminal reward)
 *          while (i >= s) { acc = r_i + gamma * ((om * v_{i+1}) + (lambda * acc));  --i }
 *          column = (float)acc
 *
 *      r and v are the kept reward and the kept float64 search value.  v_{i+1} is always a stored step inside the window, so nothing is
 *      read past L; a reanalysis (azgym_reanalyse.h) refreshes it, as it does for the n-step targets.
 *
 * This is the n-truncated lambda-return  (1 - lambda) sum_{m < M} lambda^(m-1) G^(m)  +  lambda^(M-1) G^(M),  G^(m) the m-step return of
 * azgym_nstep.h and M the window's length in steps.
 *
 * Edge identities, wherever no accumulator is a signed zero (lambda * acc and om * v keep a zero's sign, which x + 0.0 may drop):
 *   - lambda = 1 gives azg_selfplay_nstep_targets' bits at the same n_step (om = 0: acc = r_i + gamma * (0 + acc));
 *   - lambda = 0 gives the bits of n_step = 1 (om = 1: every fold restarts from r_i + gamma * v_{i+1});
 *   - n_step = 1 gives the same bits for every lambda (the window holds the first fold alone).
 *
 * The calls are idempotent (they read the kept doubles, never the column) and write the V_target column of the stored rows and nothing
 * else.  The priorities of azgym_priority.h read that column, so they follow these targets as they follow the n-step ones. */
#ifndef AZGYM_LAMBDA_H
#define AZGYM_LAMBDA_H
#include "azgym_nstep.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct azg_return_rule {
    int32_t struct_size;   /* sizeof(azg_return_rule) */
    int32_t n_step;        /* >= 0; anything beyond the ring's size is the whole stored game */
    double lambda;         /* in [0, 1] */
    double gamma;          /* >= 0 and finite, unless AZG_NSTEP_SEARCH_GAMMA */
    int32_t flags;         /* AZG_NSTEP_SEARCH_GAMMA or 0 */
} azg_return_rule;

/* Rewrite the V_target column of every stored row by the rule above, the same rule for every net.  Asynchronous like
 * azg_selfplay_nstep_targets: one small copy (the rule table, from memory the engine owns) and one kernel launch on the engine's stream.
 * With AZG_NSTEP_SEARCH_GAMMA net k discounts with azg_net_search.gamma where a per-net table is set (azg_set_net_search), with
 * azg_config.gamma otherwise; `gamma` is then ignored.
 * Refusals, before anything is copied or launched and with the ring untouched: no begin or no keep_transitions: AZG_E_STATE; a NULL
 * rule, a wrong struct_size, n_step < 0, unknown flag bits, a lambda that is NaN or outside [0, 1], or without AZG_NSTEP_SEARCH_GAMMA a
 * gamma that is negative, NaN or infinite: AZG_E_INVALID.  An empty ring: AZG_OK, nothing is copied or launched. */
int azg_selfplay_lambda_targets(azg_engine* e, const azg_return_rule* rule);

/* The same with a rule per net: rules[k], k < n_nets (azg_set_population; 1 without), is the rule of net k's games.  Net k's rows get
 * bit for bit what azg_selfplay_lambda_targets with rules[k] writes there; n_nets equal entries are that call.  Every entry is checked
 * as above (the message names the net), and struct_size and flags must be the same in all of them: an entry k >= 1 that differs from
 * entry 0 in either is AZG_E_INVALID, the message naming the field and k. */
int azg_selfplay_lambda_targets_nets(azg_engine* e, const azg_return_rule* rules);

#ifdef __cplusplus
}
#endif
#endif
