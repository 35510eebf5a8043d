#!/usr/bin/env python3
"""Batched self-play + training, end to end on one GPU: the scaled-out form of run_continuous.py:111-142 /
run_discrete.py:94-122.  B games live on the device (azg_selfplay_*: search, final action, env step, resets, replay rows);
every iteration downloads the new replay rows, runs the reference's loss / optimiser step in PyTorch on a random subset,
and re-syncs the weights into the engine.

    python examples/selfplay_train.py --game CartPole-v0 --games 512 --n-rollouts 32 --iters 30
    python examples/selfplay_train.py --game Pendulum-v1 --games 512 --n-rollouts 50 --iters 40

Prints the mean return of the episodes finished in each iteration (one JSON line per iteration).

--replay-steps R keeps the newest R self-play steps in the device ring across iterations (the reference's overwrite-the-oldest buffer)
and trains on rows picked from all of them; --reanalyse-slots N then searches N random stored steps again with the current weights
before each iteration's training and overwrites their targets (DeviceSelfPlay.reanalyse).  One process, policy on the GPU.

--n-step N trains the value head on n-step returns instead of the search's root value: the discounted rewards of the next N steps plus
the discounted search value after them, computed on the device from the transitions kept beside the ring (DeviceSelfPlay n_step=N;
an episode's terminal step closes the window, a time limit and the newest stored step bootstrap from their own search value).
--td-lambda L beside it mixes the returns of the windows 1 .. N into a lambda-return (DeviceSelfPlay td_lambda=L; 1: the n-step return).
--refresh-values-every M (with --n-step and --replay-steps) refreshes, after every M-th iteration's self-play, the value every stored
step's target bootstraps from: one forward pass of the value head per stored row, one launch (DeviceSelfPlay.refresh_values), instead of
the value its search left there.

--prioritized-alpha A [--prioritized-eps E], with --replay-steps and --n-step, replaces the uniform pick of training rows by a draw in
proportion to (|search value - value target| + E)^A, made on the device from priorities kept beside the ring (DeviceSelfPlay
prioritized=..., sample_order); with --reanalyse-slots N the reanalysed positions are drawn the same way, one per game and search.  The
draw is with replacement and biased; --prioritized-beta B corrects for it: every drawn row's losses are multiplied by its
importance-sampling weight (least priority / the row's priority)^B, computed on the device (DeviceSelfPlay.is_weights), and the
optimiser steps go through a one-net PopulationTrainer(losses="device"), whose update takes the gathered weights.
--prioritized-feedback {max,value_gap} closes the loop: every iteration runs priorities -> sample_order -> is_weights -> one native
epoch over the ring (train_epoch_ring(errors=True)) whose loss launches write each trained row's |V - z| into the engine's ring, and the
next draw's priorities come from those errors; rows not trained on since they were stored take the largest trained error (max) or
|search value - value target| (value_gap).  --prioritized-online beside it is prioritised replay as published: the iteration's
ceil(train-rows / batch-size) minibatches run in one native call (PopulationTrainer.train_online_ring), each drawn from priorities
refreshed with the errors of the minibatches before it.

--eval-search-episodes E adds eval_search_return: after every iteration every game plays E whole episodes under MCTS with the greedy
final-action rule, on the device in one call and on state of its own (DeviceSelfPlay.evaluate_search): the return of the agent as it
acts, over the same start states at every iteration.

Multi-GPU (one process per GPU, RCCL):  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
    examples/selfplay_train.py ...    Every rank plays --games games of its own (global game ids rank*games ...), the replay
rows are all-gathered, rank 0 runs the optimiser step and broadcasts the weights (alphazero_gym_amd/distributed.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alphazero_gym_amd import distributed as D, run  # noqa: E402
from alphazero_gym_amd.agent.agents import ContinuousAgent, DiscreteAgent  # noqa: E402


def build_agent(game, hidden, n_rollouts, device, lr, optimizer="rmsprop", grad_clip=0.0, layernorm=False):
    """optimizer: "rmsprop" (run.RMSPROP) or "adam" (run.ADAM, the reference's Adam settings); grad_clip: the agent's clip_grad_norm_
    bound (0: off); layernorm: nn.LayerNorm after every trunk activation (policy.layernorm)."""
    opt = dict(run.ADAM if optimizer == "adam" else run.RMSPROP, lr=lr)
    loss = dict(run.LOSS_TUNED, device=device)
    if game.lower().startswith("pendulum"):
        cfg = run.CONTINUOUS_DEFAULTS
        policy = dict(cfg["policy"], hidden_dimensions=hidden, representation_dim=3, action_dim=1, action_bound=2.0,
                      layernorm=layernorm)
        mcts = dict(cfg["mcts"], n_rollouts=n_rollouts, device=device)
        return ContinuousAgent(policy_cfg=policy, mcts_cfg=mcts, loss_cfg=loss, optimizer_cfg=opt, device=device,
                               **dict(cfg["agent"], grad_clip=grad_clip)), 3
    cfg = run.DISCRETE_DEFAULTS
    g = game.lower()   # MountainCar-v0: two observations, three actions; Acrobot-v1: six observations, three actions
    obs_dim, n_act = (2, 3) if g.startswith("mountaincar") else ((6, 3) if g.startswith("acrobot") else (4, 2))
    policy = dict(cfg["policy"], hidden_dimensions=hidden, representation_dim=obs_dim, action_dim=1, num_actions=n_act,
                  layernorm=layernorm)
    mcts = dict(cfg["mcts"], n_rollouts=n_rollouts, device=device, num_actions=n_act)
    return DiscreteAgent(policy_cfg=policy, mcts_cfg=mcts, loss_cfg=loss, optimizer_cfg=opt, device=device,
                         **dict(cfg["agent"], grad_clip=grad_clip)), obs_dim


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="CartPole-v0")
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--n-rollouts", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps-per-iter", type=int, default=20)
    ap.add_argument("--train-rows", type=int, default=2048, help="replay rows sampled per iteration")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 128])
    ap.add_argument("--max-episode-length", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--optimizer", choices=["rmsprop", "adam"], default="rmsprop", help="adam: the reference's Adam settings (run.ADAM)")
    ap.add_argument("--grad-clip", type=float, default=0.0, help="clip_grad_norm_ bound of every optimiser step (0: off)")
    ap.add_argument("--layernorm", action="store_true", help="LayerNorm after every trunk activation (the reference's policy.layernorm)")
    ap.add_argument("--seed", type=int, default=34)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--replay-steps", type=int, default=0,
                    help="keep the newest R self-play steps in the device ring across iterations (FIFO) and train on rows picked from all "
                         "of them (0: every iteration trains on its own steps); R >= --steps-per-iter, one process, --device cuda")
    ap.add_argument("--reanalyse-slots", type=int, default=0,
                    help="before each iteration's training, search this many random stored steps again with the current weights and "
                         "overwrite their targets (0: off); needs --replay-steps")
    ap.add_argument("--eval-search-episodes", type=int, default=0,
                    help="after every iteration let every game play this many whole episodes under MCTS with the greedy final-action "
                         "rule, on the device in one call (DeviceSelfPlay.evaluate_search), and add their mean return as "
                         "eval_search_return; the self-play's games are left as they are (0: no evaluation)")
    ap.add_argument("--n-step", type=int, default=None,
                    help="value targets are n-step returns over the stored steps (discounted with the search's gamma) instead of the "
                         "search's root value; 0 keeps the root value (default: off, nothing is kept)")
    ap.add_argument("--td-lambda", type=float, default=None,
                    help="with --n-step N: value targets are lambda-returns, the returns of the windows 1 .. N mixed with weights "
                         "(1 - L) L^(m-1) and the longest taking the rest; 1 is the n-step return, 0 the 1-step return (default: off)")
    ap.add_argument("--refresh-values-every", type=int, default=0,
                    help="after every M-th iteration's self-play, refresh the bootstrap value of every stored step from the value head "
                         "(one forward pass per row, one launch: DeviceSelfPlay.refresh_values) and compute the value targets again "
                         "(0: off); needs --n-step and --replay-steps")
    ap.add_argument("--prioritized-alpha", type=float, default=None,
                    help="draw the training rows (and with --reanalyse-slots the reanalysed positions) in proportion to "
                         "(|search value - value target| + eps)^alpha on the device instead of uniformly; needs --replay-steps and "
                         "--n-step (default: off, nothing is kept)")
    ap.add_argument("--prioritized-eps", type=float, default=1e-3, help="the eps of --prioritized-alpha")
    ap.add_argument("--prioritized-beta", type=float, default=None,
                    help="correct the prioritised draw's bias: multiply every drawn row's losses by its importance-sampling weight "
                         "(least priority of the net / the row's priority)^beta, computed on the device; needs --prioritized-alpha "
                         "(default: off, no weight is computed)")
    ap.add_argument("--prioritized-feedback", choices=["max", "value_gap"], default=None,
                    help="close the loop of prioritised replay: the priorities come from the learner's own value errors |V - z| on the "
                         "rows it trained on, written by the training epoch's loss launches into the engine's ring; a row not trained "
                         "on since it was stored takes the largest trained error (max) or |search value - value target| (value_gap); "
                         "needs --prioritized-alpha (default: off, nothing is kept)")
    ap.add_argument("--prioritized-online", action="store_true",
                    help="prioritised replay as published: one native call per iteration (train_online_ring) trains "
                         "ceil(train-rows / batch-size) minibatches, each drawn from priorities refreshed with the errors of the "
                         "minibatches before it; needs --prioritized-feedback (default: off, one draw per iteration)")
    a = ap.parse_args(argv)
    if a.eval_search_episodes < 0:
        ap.error("--eval-search-episodes must be >= 0")
    if a.replay_steps < 0 or a.reanalyse_slots < 0:
        ap.error("--replay-steps and --reanalyse-slots must be >= 0")
    if a.n_step is not None and a.n_step < 0:
        ap.error("--n-step must be >= 0")
    if a.td_lambda is not None:
        if a.n_step is None:
            ap.error("--td-lambda needs --n-step N: the window the returns are mixed in")
        if not 0.0 <= a.td_lambda <= 1.0:
            ap.error("--td-lambda must be in [0, 1]")
    if a.replay_steps and a.replay_steps < a.steps_per_iter:
        ap.error(f"--replay-steps ({a.replay_steps}) must hold at least one iteration's steps (--steps-per-iter {a.steps_per_iter})")
    if a.replay_steps and (not a.device.startswith("cuda") or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--replay-steps trains from the device ring where it lies: one process with --device cuda")
    if a.reanalyse_slots and not a.replay_steps:
        ap.error("--reanalyse-slots rewrites rows that stay in the device ring: use it with --replay-steps R (the FIFO ring); without it "
                 "every iteration copies its rows out and clears the ring")
    if a.refresh_values_every < 0:
        ap.error("--refresh-values-every must be >= 0")
    if a.refresh_values_every and (a.n_step is None or not a.replay_steps):
        ap.error("--refresh-values-every refreshes the values the n-step targets bootstrap from, beside the device ring: it needs "
                 "--n-step N and --replay-steps R")
    if a.prioritized_alpha is not None:
        if not a.replay_steps:
            ap.error("--prioritized-alpha draws from the rows kept in the FIFO ring: use it with --replay-steps R")
        if a.n_step is None:
            ap.error("--prioritized-alpha needs --n-step N: the priority is |search value - n-step target|, and both are kept only then")
        if not (a.prioritized_alpha >= 0.0 and a.prioritized_eps > 0.0):
            ap.error("--prioritized-alpha must be >= 0 and --prioritized-eps > 0")
    if a.prioritized_beta is not None:
        if a.prioritized_alpha is None:
            ap.error("--prioritized-beta weighs rows drawn by priority: it needs --prioritized-alpha A")
        if not (a.prioritized_beta >= 0.0 and np.isfinite(a.prioritized_beta)):
            ap.error("--prioritized-beta must be finite and >= 0")
    if a.prioritized_feedback is not None and a.prioritized_alpha is None:
        ap.error("--prioritized-feedback feeds the priorities of the prioritised draw: it needs --prioritized-alpha A")
    if a.prioritized_online and a.prioritized_feedback is None:
        ap.error("--prioritized-online redraws from the learner's own errors: it needs --prioritized-feedback")
    return a


def weighted_epoch(trainer, rows, weights, state_dim, K, batch_size, shuffle_seed):
    """run.train_on_rows's epoch through a one-net PopulationTrainer: the same shuffle and minibatches, every minibatch passed to
    ``update`` with its rows' importance-sampling weights."""
    from alphazero_gym_amd.agent.population_trainer import minibatch_bounds
    order = np.random.RandomState(shuffle_seed).permutation(rows.shape[0])
    sums = {}
    for i, j in minibatch_bounds(rows.shape[0], batch_size):
        idx = torch.from_numpy(order[i:j]).to(rows.device)
        b = rows[idx].unsqueeze(0)
        batch = (b[..., :state_dim], b[..., state_dim:state_dim + K], b[..., state_dim + K:state_dim + 2 * K],
                 b[..., state_dim + 2 * K:state_dim + 3 * K], b[..., -1])
        for key, val in trainer.update(batch, weights=weights[idx].unsqueeze(0))[0].items():
            sums[key] = sums.get(key, 0.0) + val
    return sums


def train(a, log=print):
    """Runs the loop; returns the per-iteration records."""
    import torch.distributed as dist
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    torch.manual_seed(a.seed)   # same initial weights on every rank
    agent, state_dim = build_agent(a.game, a.hidden, a.n_rollouts, a.device, a.lr, a.optimizer, a.grad_clip, a.layernorm)
    continuous = state_dim == 3
    m = agent.mcts
    replay_steps, reanalyse_slots = getattr(a, "replay_steps", 0), getattr(a, "reanalyse_slots", 0)
    prioritized = None
    if getattr(a, "prioritized_alpha", None) is not None:
        prioritized = {"alpha": a.prioritized_alpha, "eps": getattr(a, "prioritized_eps", 1e-3)}
        if getattr(a, "prioritized_beta", None) is not None:
            prioritized["beta"] = a.prioritized_beta
        if getattr(a, "prioritized_feedback", None) is not None:
            prioritized["feedback"] = a.prioritized_feedback
    weighted = prioritized is not None and "beta" in prioritized
    feedback = prioritized is not None and "feedback" in prioritized
    sp = run.DeviceSelfPlay(agent.nn, game=a.game, n_games=a.games, n_rollouts=a.n_rollouts, c_uct=m.c_uct, gamma=m.gamma,
                            epsilon=m.epsilon, c_pw=getattr(m, "c_pw", 1.0), kappa=getattr(m, "kappa", 0.5),
                            max_episode_length=a.max_episode_length, capacity_steps=replay_steps or a.steps_per_iter, fifo=bool(replay_steps),
                            reanalyse=reanalyse_slots > 0, n_step=getattr(a, "n_step", None), prioritized=prioritized,
                            td_lambda=getattr(a, "td_lambda", None), seed=a.seed, rank=rank,
                            device_id=torch.cuda.current_device() if a.device.startswith("cuda") else 0)
    K = sp.engine.kmax if continuous else 2
    rng = np.random.RandomState(a.seed)
    trainer = None
    if weighted or feedback:   # the weighted losses and the errors are the population trainer's: one net, the agent's own optimiser and clip
        from alphazero_gym_amd.agent.population_trainer import PopulationTrainer
        wide = len(a.hidden) > 3 or max(a.hidden) > 256
        trainer = PopulationTrainer([agent], max_batch=max(512, 2 * a.batch_size), losses="device", optimizers="agents",
                                    layernorm=a.layernorm and not wide, wide=wide and not a.layernorm, wide_layernorm=wide and a.layernorm)
    fs0, fc0 = 0.0, 0
    t0 = time.time()
    history = []
    # with the policy on the GPU the replay rows never leave HBM: the ring is wrapped as a torch tensor (zero copy), the
    # all-gather runs device to device over xGMI, and the minibatches are gathered on the GPU
    on_gpu = a.device.startswith("cuda")
    replay = sp.replay(a.batch_size) if on_gpu else None
    for it in range(a.iters):
        if replay_steps:   # the FIFO ring: the newest replay_steps steps stay where they lie, all of them are this iteration's rows
            sp.play(a.steps_per_iter)
            refresh_every = getattr(a, "refresh_values_every", 0)
            if refresh_every and (it + 1) % refresh_every == 0:   # every stored step's bootstrap value from the value head
                sp.refresh_values()
            if reanalyse_slots and prioritized:   # one search per "slot": every game re-searches the position drawn for it
                for _ in range(reanalyse_slots):
                    sp.reanalyse(by="priority")
            elif reanalyse_slots:   # stored steps searched again with the weights as last trained: fresh targets, same observations
                sp.reanalyse(n=reanalyse_slots)
            rows = replay.rows()
        else:
            rows = sp.collect_device(a.steps_per_iter, replay) if on_gpu else sp.collect(a.steps_per_iter)
        if world > 1:
            # every rank plays a.games games for steps_per_iter steps: equal blocks, known without a length exchange (whatever a.games
            # and the world size are: the job as a whole plays a.games * world games)
            rows = D.gather_replay_rows(rows, counts=[rows.shape[0]] * world)
        info = {"loss": 0.0}
        online = feedback and getattr(a, "prioritized_online", False)
        if online:   # every minibatch redrawn from the refreshed priorities, inside one native call
            pick = np.empty(-(-min(a.train_rows, rows.shape[0]) // a.batch_size) * a.batch_size, np.int64)
        elif prioritized:   # (the ring's rows in slot order are the engine's own numbering slot * games + game)
            pick = sp.sample_order(min(a.train_rows, rows.shape[0]))[0].astype(np.int64)
        else:
            pick = rng.choice(rows.shape[0], size=min(a.train_rows, rows.shape[0]), replace=False)
        if online:
            info = trainer.train_online_ring(sp, len(pick) // a.batch_size, batch_size=a.batch_size)[0]
            sp.upload_flat(trainer.desc, trainer.flat)
        elif feedback:   # priorities -> sample_order -> is_weights -> one native epoch over the ring that writes the rows' errors back
            if weighted:
                sp.is_weights()
            order = pick[np.random.RandomState(it).permutation(len(pick))][None, :]
            info = trainer.train_epoch_ring(sp, order, batch_size=a.batch_size, weights="priority" if weighted else None, errors=True)[0]
            sp.upload_flat(trainer.desc, trainer.flat)
        elif weighted:   # the weights of the priorities the draw was made from, in the ring's row numbering
            sp.is_weights()
            w = torch.from_numpy(sp.engine.selfplay_is_weight_values()).to(rows.device)
            at = torch.from_numpy(pick).to(rows.device)
            info = weighted_epoch(trainer, rows[at], w[at], state_dim, K, a.batch_size, it)
            sp.upload_flat(trainer.desc, trainer.flat)
        elif rank == 0:
            info = run.train_on_rows(agent, rows[torch.from_numpy(pick).to(rows.device)], state_dim, K, batch_size=a.batch_size, shuffle_seed=it)
        if world > 1:
            D.broadcast_weights(agent.nn, src=0)
        fsum, fcnt, _ = sp.engine.selfplay_stats()
        stats = torch.tensor([float(fsum.sum()), float(fcnt.sum())], dtype=torch.float64)
        if world > 1:
            stats = stats.to(a.device if a.device.startswith("cuda") else "cpu")
            dist.all_reduce(stats)
        fs, fc = float(stats[0]), int(stats[1])
        mean_ret = (fs - fs0) / max(fc - fc0, 1)
        n_batches = max(1, len(pick) // a.batch_size)
        history.append({"iter": it, "episodes_finished": fc - fc0, "mean_return": round(mean_ret, 2),
                        "loss": round(info["loss"] / n_batches, 4), "env_steps": (it + 1) * a.steps_per_iter * a.games * world,
                        "elapsed_s": round(time.time() - t0, 1)})
        if getattr(a, "eval_search_episodes", 0) > 0:   # the net as just trained, acting with its search (this rank's games)
            ev = sp.evaluate_search(a.eval_search_episodes)
            history[-1]["eval_search_return"] = round(float(ev["mean_return"][0]), 2)
        if log and rank == 0:
            log(json.dumps(history[-1]), flush=True)
        fs0, fc0 = fs, fc
    if trainer is not None:
        trainer.close()
    return history


def main():
    a = parse_args()
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        if a.device.startswith("cuda"):
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
        else:
            dist.init_process_group("gloo")
    train(a)


if __name__ == "__main__":
    main()
