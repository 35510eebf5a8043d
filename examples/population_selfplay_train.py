#!/usr/bin/env python3
"""Population self-play + training: K seeds' nets trained at once in one engine, the population form of selfplay_train.py.
Net k's games (--games-per-seed of them, global game ids k*T ...) are played on the device together with every other net's
(azg_population_selfplay_begin: one search launch and one self-play launch per step for the whole population); each iteration
downloads the new replay rows, trains every net on its own rows with its own optimiser, one net after another, and re-uploads
the changed nets (one gather launch for all of them when the nets live on the GPU).  --trainer device takes every net's
minibatch step at once instead (agent.population_trainer.PopulationTrainer: two HIP launches per step for all nets, the losses
in PyTorch between them); --trainer device-fused computes the losses on the device too (three launches, one host round trip);
--trainer device-epoch takes the whole epoch of those steps in one native call that reads the rows straight from the self-play ring
(PopulationTrainer.train_epoch_ring: no copy of the rows, one synchronisation per iteration instead of one per minibatch).
--optimizer adam and --grad-clip X give every net the reference's Adam settings and gradient clipping, on every trainer.
--c-ucts / --gammas / --search-epsilons (and, continuous games, --c-pws / --kappas) sweep the SEARCH's settings over the seeds as --lrs
sweeps the learning rate: one value per seed, every net still searched in the one launch (PopulationSelfPlay net_settings; hidden widths up
to 256, and with --wide every width: net_settings_wide=True).
--n-rollouts-per-seed sweeps the SIMULATION BUDGET the same way: one value in 1 .. --n-rollouts per seed, net k runs its own number of
simulations per search while --n-rollouts stays the engine's capacity (PopulationSelfPlay net_rollouts); alone or with the sweeps above.
--layernorm builds every net with LayerNorm after each trunk activation; the device trainers are then built with layernorm=True.
--wide builds the device trainers with wide=True, which trains nets of up to 8 hidden layers and widths up to 1024 (--hidden 1024
1024 1024 1024).  The search engine holds several such nets too: nets it searches as teams of 32 trees (padded width >= 512, two or
more hidden layers, no LayerNorm, at most four observations) need --games-per-seed to be a multiple of 32 when there is more than one
seed -- --seeds 3 11 --hidden 512 512 --wide --games-per-seed 32 -- and every other shape takes any number.  --wide --layernorm
together build the trainers with wide_layernorm=True: wide nets with LayerNorm.  --eval-episodes works at every width: wide nets are
rolled out on the device too, all seeds in one call (--seeds 3 11 --hidden 512 512 --wide --games-per-seed 32 --eval-episodes 32).

--replay-steps R keeps the newest R self-play steps in the device ring across iterations (the reference's overwrite-the-oldest
buffer, PopulationSelfPlay fifo=True) and every iteration trains on rows picked from all of them, instead of on the iteration's own
steps; it needs the nets on the GPU.  --reanalyse-slots N then searches N random stored steps again with the current weights before
each iteration's training and overwrites their targets (PopulationSelfPlay.reanalyse: MuZero's Reanalyse, on the device).  It applies
where rows stay in the ring -- --replay-steps, or --trainer device-epoch -- and is refused elsewhere.

--n-step N trains the value heads on n-step returns instead of the search's root value: the discounted rewards of the next N steps
plus the discounted search value after them, computed on the device from the transitions kept beside the ring (PopulationSelfPlay
n_step=N; an episode's terminal step closes the window, a time limit and the newest stored step bootstrap from their own search value).
--td-lambda L beside it mixes the returns of the windows 1 .. N into a lambda-return (PopulationSelfPlay td_lambda=L; 1: the n-step
return).  --n-steps N0 N1 ... and --td-lambdas L0 L1 ... give every seed its own window and lambda: one engine, one launch, rule k for
seed k's rows (--n-steps in place of --n-step; --td-lambdas beside either).

--prioritized-alpha A [--prioritized-eps E], with --replay-steps and --n-step, replaces the uniform pick of training rows by a draw
in proportion to (|search value - value target| + E)^A, made on the device from priorities kept beside the ring (PopulationSelfPlay
prioritized=..., sample_order); with --reanalyse-slots N the reanalysed positions are drawn the same way, one per game and search.
--prioritized-beta B corrects the draw's bias: after the draw the engine computes every stored row's importance-sampling weight
(the net's least priority / the row's priority)^B on the device (is_weights), and the population trainer multiplies it into the row's
losses -- --trainer device-epoch reads the weights where they lie (train_epoch_ring(weights="priority")), --trainer device and
device-fused pass the gathered weights to update.  It needs one of those three trainers.
--prioritized-feedback {max,value_gap} closes the loop: with --trainer device-epoch every iteration runs priorities -> sample_order ->
is_weights -> train_epoch_ring(errors=True), the epoch's loss launches write each trained row's |V - z| into the engine's ring and the
next draw's priorities come from those errors; rows not trained on since they were stored take the net's largest trained error (max)
or |search value - value target| (value_gap).  --prioritized-online beside it is prioritised replay as published: the iteration's
ceil(train-rows / batch-size) minibatches run in one native call (train_online_ring), each drawn from priorities refreshed with the
errors of the minibatches before it.
The draw is with replacement and biased; the loss is not reweighted (no importance-sampling weights).

--pbt-every N turns the sweep into population-based training (alphazero_gym_amd.pbt): after every N-th iteration the seeds are ranked
by --pbt-score (selfplay: the mean return of the episodes finished since the last such step; eval / eval-search: that iteration's
--eval-episodes / --eval-search-episodes returns), the worst --pbt-fraction of them take the weights, optimiser state, learned
temperature and settings of seeds drawn from the best fraction, and every --pbt-explore NAME[:f1,f2[:min:max]] hyper-parameter they
inherited is multiplied by one of its factors (default 0.8,1.25) and clipped.  It needs a device trainer and at least two seeds.
--pbt-explore lr builds the trainer with per_net=True; c_uct / gamma / epsilon / c_pw / kappa and n_rollouts give the engine its per-seed
table from iteration 0, filled with the shared values; n_step / td_lambda / target_gamma turn --n-step / --td-lambda into per-seed lists.

    python examples/population_selfplay_train.py --game CartPole-v0 --seeds 0 1 2 3 4 5 6 7 --games-per-seed 64 --iters 30

--ema-decay D keeps a slowly moving copy of every net on the device (PopulationTrainer ema=D: after every --ema-every-th optimiser
step, one more launch behind it, ema += (1 - D) (weights - ema)); it needs a device trainer.  --reanalyse-target and --eval-target
hand that copy to the engine as its second, target weight set after each training phase (PopulationSelfPlay.upload_target_flat) and
run --reanalyse-slots' searches (MuZero's target network), respectively --eval-episodes' and --eval-search-episodes' evaluations,
with it (nets="target"), while the games go on with the weights as last trained.

--refresh-values-every N (with --n-step / --n-steps and --replay-steps or --trainer device-epoch) refreshes, after every N-th
iteration's self-play, the value every stored step's n-step target bootstraps from: one forward pass of the value head per stored row,
one launch for all seeds (PopulationSelfPlay.refresh_values), instead of the value its search left there; --refresh-target takes the
averaged weights for it (MuZero Reanalyse's value targets; needs --ema-decay).

Seed k sets net k's initial weights (torch.manual_seed), and its own np.random.RandomState picks the training rows and the
minibatch shuffles.  Prints one JSON line per iteration: per-seed mean return of the episodes finished in it and mean loss, and
the time spent in self-play, training and weight sync.  --eval-episodes N adds eval_return: each seed's raw policy (no search) over
the same N start states, the number by which the seeds can be ranked.  --eval-search-episodes E adds eval_search_return beside it:
every game of every seed plays E whole episodes under MCTS -- the seed's own settings and budget, the greedy final-action rule -- on the
device in one call and on state of its own (PopulationSelfPlay.evaluate_search): each seed's return as the agent acts, over those same
start states; with --n-rollouts-per-seed it is a strength-against-budget curve."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from alphazero_gym_amd import run  # noqa: E402
from selfplay_train import build_agent  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="CartPole-v0")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--games-per-seed", type=int, default=64)
    ap.add_argument("--n-rollouts", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps-per-iter", type=int, default=20)
    ap.add_argument("--train-rows", type=int, default=512, help="replay rows sampled per seed and iteration")
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 128])
    ap.add_argument("--max-episode-length", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--lrs", type=float, nargs="+", default=None,
                    help="a learning-rate sweep: one value per --seeds entry, in place of --lr.  The device trainers are then built "
                         "with per_net=True (which implies optimizers='agents'): every net steps with its own lr in the same launches")
    sweep = "one value per --seeds entry: net k searches with its own value, all nets still in one search launch per step "
    ap.add_argument("--c-ucts", type=float, nargs="+", default=None, help="a sweep of the search's c_uct, " + sweep)
    ap.add_argument("--gammas", type=float, nargs="+", default=None, help="a sweep of the search's discount gamma, " + sweep)
    ap.add_argument("--search-epsilons", type=float, nargs="+", default=None, help="a sweep of the search's epsilon-greedy epsilon, " + sweep)
    ap.add_argument("--c-pws", type=float, nargs="+", default=None,
                    help="continuous games: a sweep of progressive widening's c_pw, " + sweep + "(the rows are as wide as the widest net's)")
    ap.add_argument("--kappas", type=float, nargs="+", default=None, help="continuous games: a sweep of progressive widening's kappa, " + sweep)
    ap.add_argument("--n-rollouts-per-seed", type=int, nargs="+", default=None,
                    help="a sweep of the search's simulation budget, one value in 1 .. --n-rollouts per --seeds entry: net k runs its own "
                         "number of simulations, all nets still in one search launch per step; --n-rollouts stays the engine's capacity")
    ap.add_argument("--optimizer", choices=["rmsprop", "adam"], default="rmsprop",
                    help="every net's optimiser; adam: the reference's Adam settings (run.ADAM).  With adam or --grad-clip the device "
                         "trainers are built with optimizers='agents'")
    ap.add_argument("--grad-clip", type=float, default=0.0, help="clip_grad_norm_ bound of every net's optimiser step (0: off)")
    ap.add_argument("--layernorm", action="store_true",
                    help="LayerNorm after every trunk activation (the reference's policy.layernorm); the device trainers get layernorm=True "
                         "(with --wide: wide_layernorm=True)")
    ap.add_argument("--wide", action="store_true",
                    help="build the device trainers with wide=True: 1-8 hidden layers of widths 16 ... 1024 (with --layernorm: "
                         "wide_layernorm=True, the wide trainer that takes LayerNorm trunks).  With several "
                         "seeds, nets the engine searches as 32-tree teams (width >= 512, two or more hidden layers, no LayerNorm, at most "
                         "four observations) need --games-per-seed to be a multiple of 32")
    ap.add_argument("--engine-seed", type=int, default=34, help="the engine's RNG seed (shared; games differ by their global ids)")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--trainer", choices=["torch", "device", "device-fused", "device-epoch"], default="torch",
                    help="torch: agent.update net by net; device: every net's optimiser step in two HIP launches (PopulationTrainer) with "
                         "the losses in PyTorch between them; device-fused: the losses in a kernel of the same step (losses='device'); "
                         "device-epoch: device-fused's arithmetic, the whole epoch in one call on the rows in the self-play ring")
    ap.add_argument("--eval-episodes", type=int, default=0,
                    help="after every iteration play this many whole episodes per seed with the raw policy, no search, on the device in "
                         "one call (PopulationSelfPlay.evaluate; any width, --wide nets included) and add the per-seed mean return as "
                         "eval_return; every seed starts from the same states, so the numbers can be ranked (0: no evaluation)")
    ap.add_argument("--eval-rule", choices=["mode", "sample"], default="mode", help="the evaluation's action rule")
    ap.add_argument("--eval-search-episodes", type=int, default=0,
                    help="after every iteration let every game of every seed play this many whole episodes under MCTS (the seed's own "
                         "search settings and budget, the greedy final-action rule) on the device in one call "
                         "(PopulationSelfPlay.evaluate_search) and add the per-seed mean return as eval_search_return, over "
                         "--eval-episodes' start states; the self-play's games are left as they are (0: no evaluation)")
    ap.add_argument("--replay-steps", type=int, default=0,
                    help="keep the newest R self-play steps in the device ring across iterations (FIFO) and train on rows picked from all "
                         "of them (0: every iteration trains on its own steps and clears the ring); R >= --steps-per-iter, nets on the GPU")
    ap.add_argument("--reanalyse-slots", type=int, default=0,
                    help="before each iteration's training, search this many random stored steps again with the current weights and "
                         "overwrite their targets (0: off); with --replay-steps or --trainer device-epoch")
    ap.add_argument("--refresh-values-every", type=int, default=0,
                    help="after every N-th iteration's self-play, refresh the bootstrap value of every stored step from the value head "
                         "(one forward pass per row, one launch: PopulationSelfPlay.refresh_values) and compute the value targets again "
                         "(0: off); needs --n-step / --n-steps, with --replay-steps or --trainer device-epoch")
    ap.add_argument("--n-step", type=int, default=None,
                    help="value targets are n-step returns over the stored steps (discounted with each net's search gamma) instead of "
                         "the search's root value; 0 keeps the root value (default: off, nothing is kept)")
    ap.add_argument("--n-steps", type=int, nargs="+", default=None,
                    help="a sweep of --n-step, one window per --seeds entry (in place of --n-step): seed k's value targets follow its "
                         "own window, all seeds still in one launch")
    ap.add_argument("--td-lambda", type=float, default=None,
                    help="with --n-step / --n-steps: value targets are lambda-returns, the returns of the windows 1 .. N mixed with "
                         "weights (1 - L) L^(m-1) and the longest taking the rest; 1 is the n-step return, 0 the 1-step return (default: off)")
    ap.add_argument("--td-lambdas", type=float, nargs="+", default=None,
                    help="a sweep of --td-lambda, one value per --seeds entry (in place of --td-lambda)")
    ap.add_argument("--prioritized-alpha", type=float, default=None,
                    help="draw the training rows (and with --reanalyse-slots the reanalysed positions) in proportion to "
                         "(|search value - value target| + eps)^alpha on the device instead of uniformly; needs --replay-steps and "
                         "--n-step (default: off, nothing is kept)")
    ap.add_argument("--prioritized-eps", type=float, default=1e-3, help="the eps of --prioritized-alpha")
    ap.add_argument("--prioritized-beta", type=float, default=None,
                    help="correct the prioritised draw's bias: multiply every drawn row's losses by its importance-sampling weight "
                         "(least priority of the net / the row's priority)^beta, computed on the device; needs --prioritized-alpha and a --trainer other than torch "
                         "(default: off, no weight is computed)")
    ap.add_argument("--prioritized-feedback", choices=["max", "value_gap"], default=None,
                    help="close the loop of prioritised replay: the priorities come from the learners' own value errors |V - z| on the "
                         "rows they trained on, written by the training epoch's loss launches into the engine's ring; a row not trained "
                         "on since it was stored takes the largest trained error of its net (max) or |search value - value target| "
                         "(value_gap); needs --prioritized-alpha and --trainer device-epoch (default: off, nothing is kept)")
    ap.add_argument("--prioritized-online", action="store_true",
                    help="prioritised replay as published: one native call per iteration (train_online_ring) trains "
                         "ceil(train-rows / batch-size) minibatches, each drawn from priorities refreshed with the errors of the "
                         "minibatches before it; needs --prioritized-feedback (default: off, one draw per iteration)")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of every net's weights on the device, updated behind the optimiser steps "
                         "(PopulationTrainer ema=D, D in [0, 1)); needs a --trainer other than torch (default: off)")
    ap.add_argument("--ema-every", type=int, default=1, help="with --ema-decay: the average moves after every N-th optimiser step")
    ap.add_argument("--reanalyse-target", action="store_true",
                    help="--reanalyse-slots' searches run with the averaged weights, the engine's target set, instead of the weights as "
                         "last trained; needs --ema-decay and --reanalyse-slots")
    ap.add_argument("--refresh-target", action="store_true",
                    help="--refresh-values-every's values come from the averaged weights, the engine's target set (MuZero Reanalyse's "
                         "value targets); needs --ema-decay and --refresh-values-every")
    ap.add_argument("--eval-target", action="store_true",
                    help="--eval-episodes / --eval-search-episodes score the averaged weights, the engine's target set; needs "
                         "--ema-decay and one of the two")
    ap.add_argument("--pbt-every", type=int, default=0,
                    help="population-based training: after every N-th iteration the worst seeds copy the best ones and perturb what "
                         "--pbt-explore names (0: off, the run is a plain sweep); needs a --trainer other than torch and two seeds or more")
    ap.add_argument("--pbt-fraction", type=float, default=0.25,
                    help="the share of the seeds replaced at a PBT step, floor(seeds * F) of them, drawn from as many of the best; in (0, 0.5]")
    ap.add_argument("--pbt-explore", nargs="+", default=None, metavar="NAME[:f1,f2[:min:max]]",
                    help="hyper-parameters a replaced seed perturbs after inheriting them: one of " + ", ".join(PBT_DEFAULTS) + "; "
                         "the value is multiplied by one of the factors (default 0.8,1.25) and clipped to min .. max (default: per name)")
    ap.add_argument("--pbt-score", choices=["selfplay", "eval", "eval-search"], default="selfplay",
                    help="what ranks the seeds: selfplay, the mean return of the episodes finished since the last PBT step (a seed with "
                         "none takes the lowest score); eval, --eval-episodes' eval_return; eval-search, --eval-search-episodes' "
                         "eval_search_return")
    a = ap.parse_args(argv)
    why = check_replay(a) or check_pbt(a) or check_ema(a)
    if why:
        ap.error(why)
    if a.eval_search_episodes < 0:
        ap.error("--eval-search-episodes must be >= 0")
    if a.lrs is not None and len(a.lrs) != len(a.seeds):
        ap.error(f"--lrs needs one value per --seeds entry ({len(a.seeds)}), got {len(a.lrs)}")
    for flag, vals in search_sweeps(a).items():
        if vals is not None and len(vals) != len(a.seeds):
            ap.error(f"--{flag} needs one value per --seeds entry ({len(a.seeds)}), got {len(vals)}")
    if a.n_rollouts_per_seed is not None:
        if len(a.n_rollouts_per_seed) != len(a.seeds):
            ap.error(f"--n-rollouts-per-seed needs one value per --seeds entry ({len(a.seeds)}), got {len(a.n_rollouts_per_seed)}")
        if not all(1 <= n <= a.n_rollouts for n in a.n_rollouts_per_seed):
            ap.error(f"--n-rollouts-per-seed: every budget lies in 1 .. --n-rollouts ({a.n_rollouts}), the engine's capacity")
    why = check_population_shape(a)
    if why:
        ap.error(why)
    return a


def search_sweeps(a):
    """The search-setting sweeps by flag name."""
    return {"c-ucts": a.c_ucts, "gammas": a.gammas, "search-epsilons": a.search_epsilons, "c-pws": a.c_pws, "kappas": a.kappas}


def net_settings(a):
    """PopulationSelfPlay's ``net_settings`` for the sweeps given (None: no sweep, every net searches with the shared settings)."""
    keys = {"c-ucts": "c_uct", "gammas": "gamma", "search-epsilons": "epsilon", "c-pws": "c_pw", "kappas": "kappa"}
    given = {keys[flag]: vals for flag, vals in search_sweeps(a).items() if vals is not None}
    if not given:
        return None
    return [{key: vals[k] for key, vals in given.items()} for k in range(len(a.seeds))]


def search_kwargs(a):
    """PopulationSelfPlay's keywords for the sweeps given: ``net_settings``, ``net_rollouts`` (--n-rollouts-per-seed), and with --wide
    the opt-in that lets nets of width >= 512 search with them (``net_settings_wide=True``).  No sweep: the shared settings, no keyword."""
    kw = {}
    explored = pbt_names(a)
    settings = net_settings(a)
    if settings is None and any(n in PBT_SEARCH_NAMES for n in explored):   # the table a PBT step writes to, filled with the shared values
        settings = [{} for _ in a.seeds]
    if settings is not None:
        kw["net_settings"] = settings
    if getattr(a, "n_rollouts_per_seed", None) is not None:
        kw["net_rollouts"] = list(a.n_rollouts_per_seed)
    elif "n_rollouts" in explored:
        kw["net_rollouts"] = [a.n_rollouts] * len(a.seeds)
    if kw and a.wide:
        kw["net_settings_wide"] = True
    return kw


# --pbt-explore's names: (min, max) where no min:max is given; None: taken from the run (pbt_explore)
PBT_DEFAULTS = {"lr": (1e-6, 1.0), "weight_decay": (0.0, 1.0), "grad_clip": (0.0, 100.0), "tau": (0.0, 10.0), "policy_coeff": (0.0, 100.0),
                "value_coeff": (0.0, 100.0), "alpha": (0.0, 10.0), "c_uct": (0.0, 100.0), "gamma": (0.0, 1.0), "epsilon": (0.0, 1.0),
                "c_pw": None, "kappa": None, "n_rollouts": None, "n_step": None, "td_lambda": (0.0, 1.0), "target_gamma": (0.0, 1.0)}
PBT_FACTORS = (0.8, 1.25)
PBT_TRAINER_NAMES = ("lr", "weight_decay", "grad_clip", "tau", "policy_coeff", "value_coeff", "alpha")
PBT_LOSS_NAMES = ("tau", "policy_coeff", "value_coeff", "alpha")
PBT_SEARCH_NAMES = ("c_uct", "gamma", "epsilon", "c_pw", "kappa")


def pbt_explore(a):
    """PopulationBasedTraining's ``explore`` for --pbt-explore, in the order given ({}: nothing is perturbed).  Raises ValueError
    saying why an entry cannot be read.  Where no min:max is given: PBT_DEFAULTS, and for the settings the engine's size bounds --
    n_rollouts 1 .. --n-rollouts, c_pw and kappa up to the widest the engine is created for, n_step 0 .. the ring's steps."""
    out = {}
    for item in getattr(a, "pbt_explore", None) or []:
        parts = item.split(":")
        name = parts[0]
        if name not in PBT_DEFAULTS:
            raise ValueError(f"--pbt-explore: {name!r} is not a hyper-parameter it can perturb ({', '.join(PBT_DEFAULTS)})")
        if name in out:
            raise ValueError(f"--pbt-explore names {name!r} twice: once per hyper-parameter")
        if len(parts) not in (1, 2, 4):
            raise ValueError(f"--pbt-explore {item!r}: the forms are NAME, NAME:f1,f2,... and NAME:f1,f2,...:min:max")
        try:
            factors = [float(f) for f in parts[1].split(",")] if len(parts) > 1 else list(PBT_FACTORS)
        except ValueError:
            factors = []
        if not factors or not all(np.isfinite(f) and f > 0 for f in factors):
            raise ValueError(f"--pbt-explore {item!r}: the factors are positive numbers separated by commas")
        if len(parts) == 4:
            try:
                lo, hi = float(parts[2]), float(parts[3])
            except ValueError:
                lo, hi = 1.0, 0.0
            if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo <= hi):
                raise ValueError(f"--pbt-explore {item!r}: min and max are numbers with 0 <= min <= max")
        elif PBT_DEFAULTS[name] is not None:
            lo, hi = PBT_DEFAULTS[name]
        elif name == "n_rollouts":
            lo, hi = 1, a.n_rollouts
        elif name == "n_step":
            lo, hi = 0, getattr(a, "replay_steps", 0) or a.steps_per_iter
        else:   # c_pw, kappa: not beyond the widening the engine is created for (the shared default, or the widest of a sweep)
            given = getattr(a, "c_pws" if name == "c_pw" else "kappas", None)
            lo, hi = 0.05, max(given) if given else (1.0 if name == "c_pw" else 0.5)
        out[name] = {"factors": factors, "min": lo, "max": hi}
        if name in ("n_rollouts", "n_step"):
            out[name]["integer"] = True
    return out


def check_pbt(a):
    """Why the --pbt-* flags cannot be honoured as given (None: they can)."""
    every = getattr(a, "pbt_every", 0)
    if every < 0:
        return "--pbt-every must be >= 0"
    if not every:
        if getattr(a, "pbt_explore", None) is not None:
            return "--pbt-explore perturbs what a PBT step copied: it needs --pbt-every N"
        return None
    if a.trainer == "torch":
        return ("--pbt-every clones nets inside the population trainer: use --trainer device, device-fused or device-epoch (the "
                "per-agent update loop of --trainer torch has no trainer to copy rows in)")
    if len(a.seeds) < 2:
        return f"--pbt-every ranks the seeds against each other: it needs two --seeds entries or more, got {len(a.seeds)}"
    if not 0.0 < a.pbt_fraction <= 0.5:
        return "--pbt-fraction must lie in (0, 0.5]: the replaced seeds and their sources are different seeds"
    try:
        explore = pbt_explore(a)
    except ValueError as e:
        return str(e)
    lossy = [n for n in explore if n in PBT_LOSS_NAMES]
    if lossy and a.trainer == "device":
        return (f"--pbt-explore {lossy[0]}: per-seed loss settings need the losses on the device: use --trainer device-fused or "
                "device-epoch")
    rule = target_rule(a)
    if ("n_step" in explore or "target_gamma" in explore) and rule["n_step"] is None:
        return "--pbt-explore n_step / target_gamma perturbs the value-target rule: it needs --n-step N or --n-steps"
    if "td_lambda" in explore and rule["td_lambda"] is None:
        return "--pbt-explore td_lambda perturbs the lambda-return's lambda: it needs --td-lambda L or --td-lambdas"
    if a.pbt_score == "eval" and a.eval_episodes <= 0:
        return "--pbt-score eval ranks the seeds by eval_return: it needs --eval-episodes N"
    if a.pbt_score == "eval-search" and a.eval_search_episodes <= 0:
        return "--pbt-score eval-search ranks the seeds by eval_search_return: it needs --eval-search-episodes E"
    return None


def check_ema(a):
    """Why the --ema-* / --*-target flags cannot be honoured as given (None: they can)."""
    decay, every = getattr(a, "ema_decay", None), getattr(a, "ema_every", 1)
    if decay is None:
        for flag, on in (("--ema-every", every != 1), ("--reanalyse-target", getattr(a, "reanalyse_target", False)),
                         ("--refresh-target", getattr(a, "refresh_target", False)), ("--eval-target", getattr(a, "eval_target", False))):
            if on:
                return f"{flag} is about the averaged weights: it needs --ema-decay D"
        return None
    if not (np.isfinite(decay) and 0.0 <= decay < 1.0) or every < 1:
        return "--ema-decay must lie in [0, 1) and --ema-every be >= 1"
    if a.trainer == "torch":
        return ("--ema-decay: the average is kept by the population trainer behind its optimiser steps: use --trainer device, "
                "device-fused or device-epoch")
    if getattr(a, "reanalyse_target", False) and not a.reanalyse_slots:
        return "--reanalyse-target chooses the weights of --reanalyse-slots' searches: it needs --reanalyse-slots N"
    if getattr(a, "refresh_target", False) and not getattr(a, "refresh_values_every", 0):
        return "--refresh-target chooses the weights of --refresh-values-every's values: it needs --refresh-values-every N"
    if getattr(a, "eval_target", False) and a.eval_episodes <= 0 and getattr(a, "eval_search_episodes", 0) <= 0:
        return "--eval-target chooses the weights of the evaluations: it needs --eval-episodes N or --eval-search-episodes E"
    return None


def pbt_names(a):
    """The names --pbt-explore perturbs, in order ([] without --pbt-every)."""
    return list(pbt_explore(a)) if getattr(a, "pbt_every", 0) else []


def check_replay(a):
    """Why --replay-steps / --reanalyse-slots cannot be honoured as given (None: they can)."""
    if a.replay_steps < 0 or a.reanalyse_slots < 0:
        return "--replay-steps and --reanalyse-slots must be >= 0"
    if getattr(a, "n_step", None) is not None and a.n_step < 0:
        return "--n-step must be >= 0"
    n_steps, lambdas = getattr(a, "n_steps", None), getattr(a, "td_lambdas", None)
    if n_steps is not None:
        if getattr(a, "n_step", None) is not None:
            return "--n-steps gives every seed its own window: use it in place of --n-step"
        if len(n_steps) != len(a.seeds) or min(n_steps) < 0:
            return f"--n-steps needs one value >= 0 per --seeds entry ({len(a.seeds)}), got {n_steps}"
    if lambdas is not None:
        if getattr(a, "td_lambda", None) is not None:
            return "--td-lambdas gives every seed its own lambda: use it in place of --td-lambda"
        if len(lambdas) != len(a.seeds):
            return f"--td-lambdas needs one value per --seeds entry ({len(a.seeds)}), got {len(lambdas)}"
    given = lambdas if lambdas is not None else [] if getattr(a, "td_lambda", None) is None else [a.td_lambda]
    if given and target_rule(a)["n_step"] is None:
        return "--td-lambda / --td-lambdas need --n-step N or --n-steps: the window the returns are mixed in"
    if not all(0.0 <= lam <= 1.0 for lam in given):
        return "--td-lambda / --td-lambdas must be in [0, 1]"
    if a.replay_steps and a.replay_steps < a.steps_per_iter:
        return f"--replay-steps ({a.replay_steps}) must hold at least one iteration's steps (--steps-per-iter {a.steps_per_iter})"
    if a.replay_steps and not a.device.startswith("cuda"):
        return "--replay-steps trains from the device ring where it lies: it needs --device cuda"
    if getattr(a, "prioritized_alpha", None) is not None:
        if not a.replay_steps:
            return "--prioritized-alpha draws from the rows kept in the FIFO ring: use it with --replay-steps R"
        if target_rule(a)["n_step"] is None:
            return "--prioritized-alpha needs --n-step N: the priority is |search value - n-step target|, and both are kept only then"
        if not (a.prioritized_alpha >= 0.0 and a.prioritized_eps > 0.0):
            return "--prioritized-alpha must be >= 0 and --prioritized-eps > 0"
    if getattr(a, "prioritized_beta", None) is not None:
        if getattr(a, "prioritized_alpha", None) is None:
            return "--prioritized-beta weighs rows drawn by priority: it needs --prioritized-alpha A"
        if not (a.prioritized_beta >= 0.0 and np.isfinite(a.prioritized_beta)):
            return "--prioritized-beta must be finite and >= 0"
        if a.trainer == "torch":
            return ("--prioritized-beta: the weighted losses are the population trainer's: use --trainer device, device-fused or "
                    "device-epoch (the per-agent update loop of --trainer torch takes no weights)")
    if getattr(a, "prioritized_feedback", None) is not None:
        if getattr(a, "prioritized_alpha", None) is None:
            return "--prioritized-feedback feeds the priorities of the prioritised draw: it needs --prioritized-alpha A"
        if a.trainer != "device-epoch":
            return ("--prioritized-feedback: the errors come out of the native epoch over the ring: use --trainer device-epoch (the "
                    "per-agent update loop of --trainer torch and the update calls of device and device-fused write none)")
    if getattr(a, "prioritized_online", False) and getattr(a, "prioritized_feedback", None) is None:
        return "--prioritized-online redraws from the learners' own errors: it needs --prioritized-feedback (and --trainer device-epoch)"
    if getattr(a, "refresh_values_every", 0) < 0:
        return "--refresh-values-every must be >= 0"
    if getattr(a, "refresh_values_every", 0):
        if target_rule(a)["n_step"] is None:
            return "--refresh-values-every refreshes the values the n-step targets bootstrap from: it needs --n-step N or --n-steps"
        if not (a.replay_steps or a.trainer == "device-epoch"):
            return ("--refresh-values-every rewrites values that stay beside the device ring: use it with --replay-steps R (the FIFO "
                    "ring) or with --trainer device-epoch")
    if a.reanalyse_slots and not (a.replay_steps or a.trainer == "device-epoch"):
        return ("--reanalyse-slots rewrites rows that stay in the device ring: use it with --replay-steps R (the FIFO ring) or with "
                "--trainer device-epoch; the other modes copy the rows out and clear the ring every iteration")
    return None


def target_rule(a):
    """PopulationSelfPlay's ``n_step`` and ``td_lambda`` for --n-step / --n-steps and --td-lambda / --td-lambdas (None: off)."""
    n_steps, lambdas = getattr(a, "n_steps", None), getattr(a, "td_lambdas", None)
    return {"n_step": list(n_steps) if n_steps is not None else getattr(a, "n_step", None),
            "td_lambda": list(lambdas) if lambdas is not None else getattr(a, "td_lambda", None)}


def pbt_target_rule(a):
    """``target_rule`` with what --pbt-explore perturbs of it as per-seed lists (a PBT step writes list entries): a scalar --n-step /
    --td-lambda repeated for every seed, and ``target_gamma`` as one None (the seed's search gamma) per seed.  No such name: the same."""
    rule, K = target_rule(a), len(a.seeds)
    for name in pbt_names(a):
        if name in ("n_step", "td_lambda") and not isinstance(rule[name], list):
            rule[name] = [rule[name]] * K
        elif name == "target_gamma":
            rule["target_gamma"] = [None] * K
    return rule


def check_population_shape(a):
    """Why the search engine would refuse this population (None: it takes it): several nets that it searches as teams of 32 trees
    need a multiple of 32 games each (_capi.lockstep_shaped).  Asked before anything is built."""
    from alphazero_gym_amd import _capi
    from alphazero_gym_amd.envs import make_game
    in_dim = make_game(a.game).observation_space.shape[0]
    if len(a.seeds) > 1 and a.games_per_seed % 32 != 0 and _capi.lockstep_shaped(in_dim, a.hidden, a.layernorm):
        return (f"--hidden {' '.join(map(str, a.hidden))} on {a.game} is searched as teams of 32 trees, one net per team: with "
                f"{len(a.seeds)} seeds --games-per-seed must be a multiple of 32 (got {a.games_per_seed}); or run one seed")
    return None


def prioritized(a):
    """PopulationSelfPlay's ``prioritized`` for --prioritized-alpha / --prioritized-eps / --prioritized-beta / --prioritized-feedback
    (None: off)."""
    if getattr(a, "prioritized_alpha", None) is None:
        return None
    out = {"alpha": a.prioritized_alpha, "eps": getattr(a, "prioritized_eps", 1e-3)}
    if getattr(a, "prioritized_beta", None) is not None:
        out["beta"] = a.prioritized_beta
    if getattr(a, "prioritized_feedback", None) is not None:
        out["feedback"] = a.prioritized_feedback
    return out


def build_population(a):
    """One agent per seed (its initial weights drawn after torch.manual_seed(seed)) and the self-play engine of them all."""
    agents = []
    for i, s in enumerate(a.seeds):
        torch.manual_seed(s)
        lr = a.lrs[i] if a.lrs is not None else a.lr
        agent, state_dim = build_agent(a.game, a.hidden, a.n_rollouts, a.device, lr, a.optimizer, a.grad_clip, a.layernorm)
        agents.append(agent)
    m = agents[0].mcts
    sp = run.PopulationSelfPlay([ag.nn for ag in agents], game=a.game, games_per_net=a.games_per_seed, n_rollouts=a.n_rollouts,
                                c_uct=m.c_uct, gamma=m.gamma, epsilon=m.epsilon, c_pw=getattr(m, "c_pw", 1.0),
                                kappa=getattr(m, "kappa", 0.5), max_episode_length=a.max_episode_length,
                                capacity_steps=getattr(a, "replay_steps", 0) or a.steps_per_iter, fifo=bool(getattr(a, "replay_steps", 0)),
                                reanalyse=getattr(a, "reanalyse_slots", 0) > 0, prioritized=prioritized(a), **pbt_target_rule(a),
                                seed=a.engine_seed, device_id=torch.cuda.current_device() if a.device.startswith("cuda") else 0, **search_kwargs(a))
    return agents, state_dim, sp


def train(a, log=print, on_rows=None, on_end=None):
    """Runs the loop; returns the per-iteration records.  ``on_rows(it, rows)``, if given, sees every iteration's per-seed rows;
    ``on_end(agents)`` the agents after the last iteration."""
    agents, state_dim, sp = build_population(a)
    K = sp.engine.kmax
    rngs = [np.random.RandomState(s) for s in a.seeds]
    on_gpu = a.device.startswith("cuda")
    fs0, fc0 = np.zeros(len(a.seeds)), np.zeros(len(a.seeds), np.int64)
    trainer = None
    pbt_every = getattr(a, "pbt_every", 0)
    per_net = a.lrs is not None or any(n in PBT_TRAINER_NAMES for n in pbt_names(a))   # (a PBT step writes per-seed trainer settings)
    if a.trainer != "torch":
        from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
        trainer = PopulationTrainer(agents, max_batch=max(512, 2 * a.batch_size), losses="torch" if a.trainer == "device" else "device",
                                    optimizers="agents" if (a.optimizer != "rmsprop" or a.grad_clip or per_net) else "rmsprop",
                                    per_net=per_net,
                                    layernorm=a.layernorm and not a.wide, wide=a.wide and not a.layernorm,
                                    wide_layernorm=a.wide and a.layernorm,
                                    **({"ema": {"decay": a.ema_decay, "every": getattr(a, "ema_every", 1)}}
                                       if getattr(a, "ema_decay", None) is not None else {}))
    replay_steps, reanalyse_slots = getattr(a, "replay_steps", 0), getattr(a, "reanalyse_slots", 0)
    by_priority = sp.prioritized is not None
    weighted = by_priority and "beta" in sp.prioritized
    feedback = by_priority and "feedback" in sp.prioritized

    # the averaged weights as the engine's target set: what --reanalyse-target's searches and --eval-target's evaluations run with
    reanalyse_nets = {"nets": "target"} if getattr(a, "reanalyse_target", False) else {}
    eval_nets = {"nets": "target"} if getattr(a, "eval_target", False) else {}
    refresh_every = getattr(a, "refresh_values_every", 0)
    refresh_nets = {"nets": "target"} if getattr(a, "refresh_target", False) else {}

    def upload_target():
        if reanalyse_nets or eval_nets or refresh_nets:
            sp.upload_target_flat(trainer.desc, trainer.ema)

    upload_target()   # (the average starts as a copy of the weights)

    def reanalyse():
        if by_priority:   # one search per "slot": every game re-searches the position drawn for it
            for _ in range(reanalyse_slots):
                sp.reanalyse(by="priority", **reanalyse_nets)
        else:
            sp.reanalyse(n=reanalyse_slots, **reanalyse_nets)

    def refresh(it):   # every stored step's bootstrap value from the value head, then the value targets again
        if refresh_every and (it + 1) % refresh_every == 0:
            sp.refresh_values(**refresh_nets)

    def pick_rows(k, rng, n):
        """Net k's training rows of this iteration: the device's prioritised draw, else the seed's own uniform pick."""
        if prio_order is not None:
            return prio_order[k].astype(np.int64)
        return rng.choice(n, size=min(a.train_rows, n), replace=False)

    pbt = None
    if pbt_every:
        from alphazero_gym_amd.pbt import PopulationBasedTraining
        pbt = PopulationBasedTraining(sp, trainer, pbt_explore(a), fraction=a.pbt_fraction, seed=a.engine_seed)
        pbt_fs, pbt_fc = fs0.copy(), fc0.copy()   # finished_returns() at the last PBT step
    ring_view = None
    t0 = time.time()
    history = []
    for it in range(a.iters):
        t1 = time.time()
        if a.trainer == "device-epoch":   # the rows stay in the ring
            rows = None
            n_ring = sp.play_device(a.steps_per_iter)[0] * sp.games_per_net
            refresh(it)
            if reanalyse_slots:   # stored steps searched again with the weights as last trained: fresh targets, same observations
                reanalyse()
            sp.engine.sync()
        elif replay_steps:   # the FIFO ring: the newest replay_steps steps, every net's rows read where they lie
            if ring_view is None:
                from alphazero_gym_amd.agent.buffers import DeviceReplay
                ring_view = DeviceReplay(sp.engine, 1)
            size = sp.play_device(a.steps_per_iter)[0]
            refresh(it)
            if reanalyse_slots:
                reanalyse()
            rows = sp._split(ring_view.rows(), size)
            n_ring = size * sp.games_per_net
        else:
            rows = sp.collect_device(a.steps_per_iter) if on_gpu else sp.collect(a.steps_per_iter)
        t2 = time.time()
        if on_rows is not None:
            if rows is None:
                from alphazero_gym_amd.agent.buffers import DeviceReplay
                on_rows(it, sp._split(DeviceReplay(sp.engine, 1).rows(), n_ring // sp.games_per_net))
            else:
                on_rows(it, rows)
        losses = []
        # (net k's rows are numbered slot * T + game in the ring and in _split's copies alike)
        online = feedback and rows is None and getattr(a, "prioritized_online", False)
        prio_order = sp.sample_order(min(a.train_rows, n_ring)) if by_priority and not online else None
        if weighted and not online:   # the weights of the priorities the draw was just made from
            sp.is_weights()
        if online:   # every minibatch redrawn from the refreshed priorities, inside one native call
            n_mb = -(-min(a.train_rows, n_ring) // a.batch_size)
            infos = trainer.train_online_ring(sp, n_mb, batch_size=a.batch_size)
            losses = [info["loss"] / n_mb for info in infos]
        elif rows is None:   # the other trainers' picks and shuffles from the same streams, composed into one order per net
            order = []
            for k, rng in enumerate(rngs):
                pick = pick_rows(k, rng, n_ring)
                order.append(pick[np.random.RandomState(int(rng.randint(2 ** 31 - 1))).permutation(len(pick))])
            # (--prioritized-feedback: the epoch's loss launches write the rows' errors back, the next iteration's draw reads them)
            infos = trainer.train_epoch_ring(sp, np.stack(order), batch_size=a.batch_size, weights="priority" if weighted else None,
                                             **({"errors": True} if feedback else {}))
            if not replay_steps:
                sp.engine.selfplay_clear()
            losses = [info["loss"] / max(1, len(order[0]) // a.batch_size) for info in infos]
        elif trainer is None:
            for k, (agent, rng, r) in enumerate(zip(agents, rngs, rows)):
                pick = pick_rows(k, rng, r.shape[0])
                info = run.train_on_rows(agent, r[torch.from_numpy(pick).to(r.device)], state_dim, K, batch_size=a.batch_size,
                                         shuffle_seed=int(rng.randint(2 ** 31 - 1)))
                losses.append(info["loss"] / max(1, len(pick) // a.batch_size))
        else:   # the same rows and shuffles, every net's minibatch step at once
            picked, seeds, picked_w = [], [], []
            if weighted:   # [size, n_games] -> net k's rows in _split's numbering, slot * T + game
                T = sp.games_per_net
                w_ring = torch.from_numpy(sp.engine.selfplay_is_weight_values()).to(rows[0].device).reshape(-1, sp.n_games)
            for k, (rng, r) in enumerate(zip(rngs, rows)):
                pick = pick_rows(k, rng, r.shape[0])
                at = torch.from_numpy(pick).to(r.device)
                picked.append(r[at])
                if weighted:
                    picked_w.append(w_ring[:, k * T:(k + 1) * T].reshape(-1)[at])
                seeds.append(int(rng.randint(2 ** 31 - 1)))
            infos = trainer.train_on_rows(picked, state_dim, K, batch_size=a.batch_size, shuffle_seeds=seeds,
                                          weights=torch.stack(picked_w) if weighted else None)
            losses = [info["loss"] / max(1, picked[0].shape[0] // a.batch_size) for info in infos]
        t3 = time.time()
        if trainer is None:
            sp.sync_weights()
        else:
            sp.upload_flat(trainer.desc, trainer.flat)
            upload_target()
        t4 = time.time()
        fs, fc = sp.finished_returns()
        mean_ret = (fs - fs0) / np.maximum(fc - fc0, 1)
        history.append({"iter": it, "mean_return": [round(float(x), 2) for x in mean_ret],
                        "episodes_finished": [int(x) for x in fc - fc0], "loss": [round(float(x), 4) for x in losses],
                        "selfplay_s": round(t2 - t1, 4), "train_s": round(t3 - t2, 4), "sync_s": round(t4 - t3, 4),
                        "weight_sync": sp.last_weight_sync,
                        "env_steps": (it + 1) * a.steps_per_iter * sp.n_games, "elapsed_s": round(time.time() - t0, 2)})
        if a.eval_episodes > 0:   # the nets as just trained and uploaded, each by itself, over the same start states
            ev = sp.evaluate(a.eval_episodes, rule=a.eval_rule, **eval_nets)
            history[-1]["eval_return"] = [round(float(x), 2) for x in ev["mean_return"]]
            ev_raw = ev
        if getattr(a, "eval_search_episodes", 0) > 0:   # the same nets acting with their search, over those same start states
            ev = sp.evaluate_search(a.eval_search_episodes, **eval_nets)
            history[-1]["eval_search_return"] = [round(float(x), 2) for x in ev["mean_return"]]
            ev_search = ev
        if pbt is not None and (it + 1) % pbt_every == 0:   # exploit / explore on the nets as just trained, then uploaded again
            if a.pbt_score == "selfplay":
                done = fc - pbt_fc
                scores = (fs - pbt_fs) / np.maximum(done, 1)
                if (done > 0).any():   # (a seed that finished no episode since the last step ranks with the worst)
                    scores[done == 0] = scores[done > 0].min()
                pbt_fs, pbt_fc = fs, fc
            else:
                scores = (ev_raw if a.pbt_score == "eval" else ev_search)["mean_return"]
            rec = pbt.step(scores)
            history[-1]["pbt"] = {"src": rec["src"], "scores": [round(float(x), 4) for x in scores],
                                  "explored": {str(k): v for k, v in rec["explored"].items()}}
            upload_target()   # (a replaced seed's average is its source's)
        if log:
            log(json.dumps(history[-1]), flush=True)
        fs0, fc0 = fs, fc
    if trainer is not None:
        trainer.close()
    if on_end is not None:
        on_end(agents)
    sp.close()
    return history


def main():
    train(parse_args())


if __name__ == "__main__":
    main()
