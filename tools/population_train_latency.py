#!/usr/bin/env python3
"""One minibatch optimiser step of K nets, three ways in the same process: the loop of K agent.update calls,
PopulationTrainer.update (two HIP launches + the losses in PyTorch), with its split into forward launch, PyTorch loss part and
backward launch, and PopulationTrainer(losses="device").update (three launches, the losses on the device).  GPU box only:
    python tools/population_train_latency.py [--ks 1,8,64,256] [--batch 128] [--reps 20] [--warmup 5] [--out profiles/population_train_latency.txt]
Configurations: CartPole 2x128 ReLU and Pendulum 3x128 ELU (run.DISCRETE_DEFAULTS / CONTINUOUS_DEFAULTS, A0CLossTuned, RMSprop).
Every figure is the median wall ms of --reps repetitions after --warmup, host clock around work that ends in a synchronise.  The
file's header carries the errors printed by tests/test_population_trainer.py (--grad-errors FILE, the output of pytest -s: gradients
against autograd, raw against azg_mlp_eval, first-step losses against float64; --loss-errors FILE, the same of
tests/test_population_device_loss.py: the largest error per head and loss) and the compiler's resource report of the kernels.

--epoch measures a whole epoch instead (--rows rows per net in minibatches of --batch): PopulationTrainer.train_epoch (one native
call on a [K, n, row] array), train_epoch_ring (the same call on the self-play ring itself) and train_on_rows with
losses="device" (one native call, one synchronisation and one host copy per minibatch, the minibatches gathered by torch), all three
in one process on the same rows -- a PopulationSelfPlay's ring of K nets x 16 games -- CartPole 2x128 ReLU and Pendulum 3x128 ELU
with a mixture of 2:
    python tools/population_train_latency.py --epoch [--ks 1,8,64,256] [--rows 512] [--batch 128] [--out profiles/population_train_latency_epoch.txt]

--optimizer adam and / or --grad-clip X measure PopulationTrainer(optimizers="agents", losses="device").update (the backward launch in
its deferred form: gradients first, then norm, clip and update) against the loop of agent.update calls of the same agents and against
the fused RMSprop step (default agents, losses="device") in the same process, CartPole 2x128 ReLU and Pendulum 3x128 ELU with a
mixture of 2:
    python tools/population_train_latency.py --optimizer adam --grad-clip 1.0    (writes profiles/population_train_latency_adam.txt)

--layernorm measures the step of agents whose trunks have nn.LayerNorm after every activation (policy.layernorm = True):
PopulationTrainer(layernorm=True).update with the losses in PyTorch and on the device against the loop of agent.update calls of the
same LayerNorm agents, and beside them the device-loss step of the same nets without LayerNorm, all in one process:
    python tools/population_train_latency.py --layernorm    (writes profiles/population_train_latency_layernorm.txt)

--wide measures PopulationTrainer(wide=True) on nets the first trainer refuses -- Pendulum 4x1024 ELU with a mixture of 2 (config E's
net) and CartPole 2x512 ReLU, K in 1,4,16 -- with the losses in PyTorch and on the device against the loop of agent.update calls of
the same agents, all in one process; with --epoch also train_epoch against train_on_rows on synthetic rows.  The header carries the
gradient errors of tests/test_population_trainer_wide.py (--grad-errors FILE), the launches per step and the compiler's resource
report of the wide kernels:
    python tools/population_train_latency.py --wide [--epoch]    (writes profiles/population_train_latency_wide.txt)

--wide --layernorm measures PopulationTrainer(wide_layernorm=True) on the same nets with LayerNorm trunks (1, 4, 16 of the 4x1024 nets,
1 ... 256 of the 2x512 ones) against the loop of agent.update calls on those agents, and beside it the same nets without LayerNorm
on PopulationTrainer(wide=True) from the same run:
    python tools/population_train_latency.py --wide --layernorm [--epoch]    (writes profiles/population_train_latency_wide_layernorm.txt)

--per-net measures a learning-rate sweep, K nets with K different lr, four ways in one process: (a) PopulationTrainer(per_net=True,
optimizers="agents", losses="device").update, every net reading its own settings from the trainer's device table; (b) the same
trainer without per_net on agents of one lr (the shared-settings deferred step); (c) K one-net PopulationTrainers stepped in turn;
(d) the loop of agent.update calls.  CartPole 2x128 at K = 1, 8, 64, 256 and Pendulum 4x1024 (wide=True) at K = 1, 4, 16.  (a) and
(b) are measured --rounds times in turn; the spread of a figure is the largest minus the smallest of its medians, and the file says
whether (a) stays within (b)'s spread.  --bench FILE appends bench.py result lines recorded elsewhere:
    python tools/population_train_latency.py --per-net    (writes profiles/population_train_latency_pernet.txt)"""
import argparse
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from alphazero_gym_amd import _capi, run  # noqa: E402
from alphazero_gym_amd.agent import population_trainer as PT  # noqa: E402
from alphazero_gym_amd.envs import make_game  # noqa: E402

CONFIGS = {"cartpole_2x128": ("discrete", 4, 2), "pendulum_3x128": ("continuous", 3, 8)}   # kind, state_dim, actions per row


def _batches(kind, K, B, S, A, seed=0):
    g = torch.Generator().manual_seed(seed)
    states = torch.randn((K, B, S), generator=g)
    actions = torch.arange(A, dtype=torch.float32).repeat(K, B, 1) if kind == "discrete" else torch.rand((K, B, A), generator=g) * 3.6 - 1.8
    counts = torch.randint(1, 9, (K, B, A), generator=g).float()
    v = torch.randn((K, B), generator=g)
    return tuple(t.cuda() for t in (states, actions, counts, counts.clone(), v))


def _median_ms(fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def measure(name, K, B, reps, warmup):
    kind, S, A = CONFIGS[name]
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, dict(device="cuda"))
    env = make_game(cfg["game"])
    torch.manual_seed(0)
    agents = [run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)]
    stacked = _batches(kind, K, B, S, A)
    per_net = [tuple(t[k] for t in stacked) for k in range(K)]

    def loop():
        for a, b in zip(agents, per_net):
            a.update(b)

    t_loop = _median_ms(loop, reps, warmup)
    tr = PT.PopulationTrainer(agents, max_batch=max(512, 2 * B))
    t_pop = _median_ms(lambda: tr.update(stacked), reps, warmup)
    # the split: the same three parts, each timed on its own
    states, actions, counts, _, v = stacked
    values = v.reshape(K, B, 1)
    raw = torch.empty((K, B, tr.trainer.n_raw), device="cuda")
    t_fwd = _median_ms(lambda: tr.trainer.forward(tr.flat.data_ptr(), states.data_ptr(), B, raw.data_ptr()), reps, warmup)
    box = {}

    def loss_part():
        r = raw.detach().requires_grad_(True)
        losses = PT.population_loss(tr.policy, tr.loss, r, actions, counts, values, tr.log_alpha, tr.alpha_optimizer)
        losses["loss"].sum().backward()
        box["d_raw"] = r.grad.contiguous()
        PT.per_net(losses)

    t_loss = _median_ms(loss_part, reps, warmup)

    def bwd():
        tr.trainer.forward(tr.flat.data_ptr(), states.data_ptr(), B, raw.data_ptr())
        tr.trainer.backward_step(tr.flat.data_ptr(), box["d_raw"].data_ptr(), B, tr.opt, tr.square_avg.data_ptr(), None)

    t_bwd = _median_ms(bwd, reps, warmup) - t_fwd
    tr.close()
    # the losses on the device: new agents of the same seed (the first trainer's close() left its agents usable, but trained)
    torch.manual_seed(0)
    fused = PT.PopulationTrainer([run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)], max_batch=max(512, 2 * B), losses="device")
    t_fused = _median_ms(lambda: fused.update(stacked), reps, warmup)
    fused.close()
    return t_loop, t_pop, t_fwd, t_loss, t_bwd, t_fused


def measure_optim(name, K, B, reps, warmup, optimizer, grad_clip):
    """(loop of agent.update, optimizers="agents" step, fused RMSprop step) median ms, losses on the device in both trainers."""
    kind, S, A = CONFIGS[name]
    over = dict(device="cuda", policy=dict(num_components=2)) if kind == "continuous" else dict(device="cuda")
    base = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, over)
    cfg = dict(base, agent=dict(base["agent"], grad_clip=grad_clip))
    if optimizer == "adam":
        cfg["optimizer"] = dict(run.ADAM)
    env = make_game(cfg["game"])
    stacked = _batches(kind, K, B, S, A)
    per_net = [tuple(t[k] for t in stacked) for k in range(K)]

    def agents_of(c):
        torch.manual_seed(0)
        return [run.make_agent(kind, c, env, tree_id_base=k) for k in range(K)]

    agents = agents_of(cfg)

    def loop():
        for a, b in zip(agents, per_net):
            a.update(b)

    t_loop = _median_ms(loop, reps, warmup)
    tr = PT.PopulationTrainer(agents_of(cfg), max_batch=max(512, 2 * B), losses="device", optimizers="agents")
    t_opt = _median_ms(lambda: tr.update(stacked), reps, warmup)
    tr.close()
    fused = PT.PopulationTrainer(agents_of(base), max_batch=max(512, 2 * B), losses="device")
    t_fused = _median_ms(lambda: fused.update(stacked), reps, warmup)
    fused.close()
    return t_loop, t_opt, t_fused


def measure_layernorm(name, K, B, reps, warmup):
    """(loop of agent.update, layernorm=True step with torch losses, with device losses, the plain nets' device-loss step) median ms."""
    kind, S, A = CONFIGS[name]
    base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
    cfg = run._merge(base, dict(device="cuda", policy=dict(layernorm=True)))
    plain_cfg = run._merge(base, dict(device="cuda"))
    env = make_game(cfg["game"])
    stacked = _batches(kind, K, B, S, A)
    per_net = [tuple(t[k] for t in stacked) for k in range(K)]

    def agents_of(c):
        torch.manual_seed(0)
        return [run.make_agent(kind, c, env, tree_id_base=k) for k in range(K)]

    agents = agents_of(cfg)

    def loop():
        for a, b in zip(agents, per_net):
            a.update(b)

    t_loop = _median_ms(loop, reps, warmup)
    out = [t_loop]
    for c, kw in ((cfg, dict(layernorm=True)), (cfg, dict(layernorm=True, losses="device")), (plain_cfg, dict(losses="device"))):
        tr = PT.PopulationTrainer(agents_of(c), max_batch=max(512, 2 * B), **kw)
        out.append(_median_ms(lambda: tr.update(stacked), reps, warmup))
        tr.close()
    return out


# --wide: kind, state_dim, actions per row, hidden widths, policy overrides
WIDE_CONFIGS = {"pendulum_4x1024_gmm2": ("continuous", 3, 8, [1024] * 4, dict(num_components=2)),
                "cartpole_2x512": ("discrete", 4, 2, [512, 512], {})}


def measure_wide(name, K, B, reps, warmup, epoch_rows=0, layernorm=False):
    """(loop of agent.update, wide step with torch losses, with device losses[, train_epoch, train_on_rows]) median ms.
    layernorm: the agents have LayerNorm trunks and the trainer is PopulationTrainer(wide_layernorm=True); the last entry is then the
    device-loss step of the same nets without LayerNorm on PopulationTrainer(wide=True)."""
    kind, S, A, hidden, over = WIDE_CONFIGS[name]
    base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
    plain_cfg = run._merge(base, dict(device="cuda", policy=dict(over, hidden_dimensions=hidden)))
    cfg = run._merge(plain_cfg, dict(policy=dict(layernorm=True))) if layernorm else plain_cfg
    env = make_game(cfg["game"])
    stacked = _batches(kind, K, B, S, A)
    per_net = [tuple(t[k] for t in stacked) for k in range(K)]

    def agents_of(c=cfg):
        torch.manual_seed(0)
        return [run.make_agent(kind, c, env, tree_id_base=k) for k in range(K)]

    agents = agents_of()

    def loop():
        for a, b in zip(agents, per_net):
            a.update(b)

    out = [_median_ms(loop, reps, warmup)]
    del agents
    which = dict(wide_layernorm=True) if layernorm else dict(wide=True)
    for losses in ("torch", "device"):
        tr = PT.PopulationTrainer(agents_of(), max_batch=max(512, 2 * B), losses=losses, **which)
        out.append(_median_ms(lambda: tr.update(stacked), reps, warmup))
        if losses == "device" and epoch_rows:
            big = _batches(kind, K, epoch_rows, S, A, seed=1)
            rows = torch.cat([big[0], big[1], big[2], big[3], big[4].unsqueeze(-1)], dim=-1).contiguous()
            seeds = list(range(K))
            out.append(_median_ms(lambda: tr.train_epoch(rows, S, A, batch_size=B, shuffle_seeds=seeds), reps, warmup))
            out.append(_median_ms(lambda: tr.train_on_rows(rows, S, A, batch_size=B, shuffle_seeds=seeds), reps, warmup))
        tr.close()
    if layernorm:
        tr = PT.PopulationTrainer(agents_of(plain_cfg), max_batch=max(512, 2 * B), wide=True, losses="device")
        out.append(_median_ms(lambda: tr.update(stacked), reps, warmup))
        tr.close()
    return out


PERNET_CONFIGS = {"cartpole_2x128": ("discrete", 4, 2, [128, 128], {}, False, "1,8,64,256"),
                  "pendulum_4x1024": ("continuous", 3, 8, [1024] * 4, dict(num_components=2), True, "1,4,16")}


def measure_pernet(name, K, B, reps, warmup, rounds):
    """((a) medians per round, (b) medians per round, (c), (d)) in ms: the per-net step with K different lr, the shared-settings
    deferred step, K one-net trainers in turn, the loop of agent.update."""
    kind, S, A, hidden, over, wide, _ = PERNET_CONFIGS[name]
    base = run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS
    cfg = run._merge(base, dict(device="cuda", policy=dict(over, hidden_dimensions=hidden)))
    env = make_game(cfg["game"])
    stacked = _batches(kind, K, B, S, A)
    per_net = [tuple(t[k] for t in stacked) for k in range(K)]
    kw = dict(max_batch=max(512, 2 * B), losses="device", optimizers="agents", wide=wide)

    def agents_of(sweep):
        torch.manual_seed(0)
        agents = [run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)]
        if sweep:
            for k, ag in enumerate(agents):
                ag.optimizer.param_groups[0]["lr"] *= 1.0 + k / K
        return agents

    nets = PT.PopulationTrainer(agents_of(True), per_net=True, **kw)
    shared = PT.PopulationTrainer(agents_of(False), **kw)
    t_a, t_b = [], []
    for _ in range(rounds):
        t_a.append(_median_ms(lambda: nets.update(stacked), reps, warmup))
        t_b.append(_median_ms(lambda: shared.update(stacked), reps, warmup))
    nets.close()
    shared.close()
    ones = [PT.PopulationTrainer([ag], **kw) for ag in agents_of(True)]
    singles = [tuple(t[k:k + 1] for t in stacked) for k in range(K)]

    def in_turn():
        for tr, b in zip(ones, singles):
            tr.update(b)

    t_c = _median_ms(in_turn, reps, warmup)
    for tr in ones:
        tr.close()
    agents = agents_of(True)

    def loop():
        for ag, b in zip(agents, per_net):
            ag.update(b)

    t_d = _median_ms(loop, reps, warmup)
    return t_a, t_b, t_c, t_d


def main_pernet(a):
    lines = ["# tools/population_train_latency.py --per-net: one minibatch optimiser step of K nets with K different learning rates, batch %d, "
             "one MI355X; median wall ms of %d repetitions after %d warm-up, every figure of a row in one process; (a) and (b) measured %d "
             "times in turn, spread = largest - smallest of a figure's medians" % (a.batch, a.reps, a.warmup, a.rounds),
             "# (a) PopulationTrainer(per_net=True, optimizers='agents', losses='device').update: azg_trainer_step_nets, settings from the device table",
             "# (b) PopulationTrainer(optimizers='agents', losses='device').update on agents of one lr: azg_trainer_step_opt's deferred form",
             "# (c) K one-net PopulationTrainers stepped in turn  (d) the loop of K agent.update calls"]
    outside = []
    for name in a.configs.split(","):
        ks = a.ks if a.ks else PERNET_CONFIGS[name][6]
        for K in [int(k) for k in ks.split(",")]:
            t_a, t_b, t_c, t_d = measure_pernet(name, K, a.batch, a.reps, a.warmup, a.rounds)
            med_a, med_b = float(np.median(t_a)), float(np.median(t_b))
            spread = max(t_b) - min(t_b)
            within = med_a - med_b <= spread
            if not within:
                outside.append(f"{name} K={K}: (a) {med_a:.3f} ms against (b) {med_b:.3f} ms + spread {spread:.3f} ms")
            lines.append(f"  {name} K={K:4d} (a) per-net {med_a:8.3f} ms [{min(t_a):.3f} .. {max(t_a):.3f}]  (b) shared {med_b:8.3f} ms "
                         f"[{min(t_b):.3f} .. {max(t_b):.3f}]  (a) - (b) {med_a - med_b:+7.3f} ms  spread of (b) {spread:6.3f} ms  "
                         f"{'within' if within else 'OUTSIDE'}  (c) one-net trainers {t_c:9.3f} ms  {t_c / med_a:7.2f}x  "
                         f"(d) agent.update loop {t_d:9.3f} ms  {t_d / med_a:7.2f}x")
            print(lines[-1], flush=True)
    lines.append("# target: (a) stays within the measured spread of (b).  "
                 + ("It does at every point." if not outside else "It does NOT at: " + "; ".join(outside)))
    if a.bench and os.path.exists(a.bench):
        lines.append("# bench.py --gpus 1 of the parent commit's library and of this build's, in turn in one run (the search code is the same):")
        lines += ["#   " + ln.rstrip() for ln in open(a.bench) if ln.strip()]
    return lines


def main_wide_layernorm(a):
    lines = ["# tools/population_train_latency.py --wide --layernorm%s: one minibatch optimiser step of K wide nets with LayerNorm trunks "
             "(PopulationTrainer(wide_layernorm=True), RMSprop fused into the backward launches), batch %d, one MI355X; median wall ms of %d "
             "repetitions after %d warm-up, every row in one process" % (" --epoch" if a.epoch else "", a.batch, a.reps, a.warmup),
             "# launches per step of a net with L hidden layers: forward 2 L + 1, loss kernel 1, backward 3 L + 1 (fused RMSprop): 5 L + 3; "
             "Adam / grad_clip / grad_norms: + 2 (norm chains, update), + 1 without a norm"]
    misses = []
    for name in a.configs.split(","):
        lines.append(f"# {name} with LayerNorm: loop of K agent.update | PopulationTrainer(wide_layernorm=True).update | ratio | "
                     "PopulationTrainer(wide_layernorm=True, losses='device').update | ratio to the loop"
                     + (f" | train_epoch of {a.rows} rows per net | train_on_rows" if a.epoch else "")
                     + " | the same nets without LayerNorm, PopulationTrainer(wide=True, losses='device').update | LayerNorm / plain")
        ks = a.ks if a.ks else ("1,4,16" if name.startswith("pendulum") else "1,4,16,64,256")
        for K in [int(k) for k in ks.split(",")]:
            t = measure_wide(name, K, a.batch, a.reps, a.warmup, a.rows if a.epoch else 0, layernorm=True)
            line = (f"  {name} K={K:4d} loop {t[0]:9.3f} ms  wide_layernorm {t[1]:8.3f} ms  {t[0] / t[1]:7.2f}x  device losses {t[2]:8.3f} ms  "
                    f"{t[0] / t[2]:7.2f}x")
            if a.epoch:
                line += f"  epoch {t[3]:9.3f} ms  train_on_rows {t[4]:9.3f} ms"
            line += f"  plain nets {t[-1]:8.3f} ms  {t[2] / t[-1]:6.3f}x"
            if t[2] > t[0]:
                misses.append(f"{name} K={K}: device-loss step {t[2]:.3f} ms against the loop's {t[0]:.3f} ms")
            lines.append(line)
            print(line, flush=True)
    lines.append("# held to: the device-loss step's median must not exceed the loop's at any point measured.  "
                 + ("Every point holds." if not misses else "MISSED at: " + "; ".join(misses)))
    return lines


def main_wide(a):
    lines = ["# tools/population_train_latency.py --wide%s: one minibatch optimiser step of K wide nets (PopulationTrainer(wide=True), RMSprop "
             "fused into the backward launches), batch %d, one MI355X; median wall ms of %d repetitions after %d warm-up, every row in one process"
             % (" --epoch" if a.epoch else "", a.batch, a.reps, a.warmup)]
    if a.grad_errors and os.path.exists(a.grad_errors):
        lines.append("# gradient errors against float64 autograd, max|g - g64| / max|g64| per parameter tensor (tests/test_population_trainer_wide.py; "
                     "the bound is the factor times the float32 autograd error):")
        log = [ln.strip().lstrip(".") for ln in open(a.grad_errors)]
        lines += ["#   " + ln for ln in log if ln.startswith("grad ")]
        lines.append("# raw against azg_mlp_eval's raw (bound 1e-5):")
        lines += ["#   " + ln for ln in log if ln.startswith("forward vs ")]
        lines.append("# first-step loss dictionary against float64 (test_end_to_end):")
        lines += ["#   " + ln for ln in log if ln.startswith("wide continuous ")]
    lines.append("# launches per step of a net with L hidden layers: forward L + 1, loss kernel 1, backward 2 L + 1 (fused RMSprop): 3 L + 3; "
                 "Adam / grad_clip / grad_norms: + 2 (norm chains, update), + 1 without a norm")
    for name in a.configs.split(","):
        L = len(WIDE_CONFIGS[name][3])
        lines.append(f"#   {name}: {3 * L + 3} launches per step ({3 * L + 5} in the deferred form); an epoch adds one gather launch per "
                     "minibatch and one loss-sum launch")
    ru = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "resource_usage.py"), "dispatch_train_wide", "train"],
                        capture_output=True, text=True)
    lines.append("# tools/resource_usage.py dispatch_train_wide:")
    lines += ["#   " + ln for ln in ru.stdout.splitlines()]
    misses = []
    for name in a.configs.split(","):
        lines.append(f"# {name}: loop of K agent.update | PopulationTrainer(wide=True).update | ratio | "
                     "PopulationTrainer(wide=True, losses='device').update | ratio to the loop"
                     + (f" | train_epoch of {a.rows} rows per net | train_on_rows | train_on_rows / train_epoch" if a.epoch else ""))
        for K in [int(k) for k in a.ks.split(",")]:
            t = measure_wide(name, K, a.batch, a.reps, a.warmup, a.rows if a.epoch else 0)
            line = (f"  {name} K={K:4d} loop {t[0]:9.3f} ms  wide {t[1]:8.3f} ms  {t[0] / t[1]:7.2f}x  device losses {t[2]:8.3f} ms  "
                    f"{t[0] / t[2]:7.2f}x")
            if a.epoch:
                line += f"  epoch {t[3]:9.3f} ms  train_on_rows {t[4]:9.3f} ms  {t[4] / t[3]:6.2f}x"
            if t[2] > t[0]:
                misses.append(f"{name} K={K}: device-loss step {t[2]:.3f} ms against the loop's {t[0]:.3f} ms")
            lines.append(line)
            print(line, flush=True)
    lines.append("# held to: the device-loss step's median must not exceed the loop's at any point measured.  "
                 + ("Every point holds." if not misses else "MISSED at: " + "; ".join(misses)))
    return lines


def main_layernorm(a):
    lines = ["# tools/population_train_latency.py --layernorm: one minibatch optimiser step of K nets with LayerNorm trunks, batch %d, one "
             "MI355X; median wall ms of %d repetitions after %d warm-up, all four in one process" % (a.batch, a.reps, a.warmup)]
    for name in a.configs.split(","):
        lines.append(f"# {name}: loop of K agent.update (LayerNorm agents) | PopulationTrainer(layernorm=True).update | ratio | "
                     "PopulationTrainer(layernorm=True, losses='device').update | ratio to the loop | the same nets without LayerNorm, "
                     "losses='device' | LayerNorm / plain")
        for K in [int(k) for k in a.ks.split(",")]:
            t_loop, t_pop, t_dev, t_plain = measure_layernorm(name, K, a.batch, a.reps, a.warmup)
            lines.append(f"  {name} K={K:4d} loop {t_loop:9.3f} ms  layernorm=True {t_pop:8.3f} ms  {t_loop / t_pop:7.2f}x  "
                         f"device losses {t_dev:8.3f} ms  {t_loop / t_dev:7.2f}x  plain nets {t_plain:8.3f} ms  {t_dev / t_plain:6.3f}x")
            print(lines[-1], flush=True)
    return lines


def main_optim(a):
    lines = ["# tools/population_train_latency.py --optimizer %s --grad-clip %g: one minibatch optimiser step of K nets, batch %d, one MI355X; "
             "median wall ms of %d repetitions after %d warm-up, all three in one process" % (a.optimizer, a.grad_clip, a.batch, a.reps, a.warmup)]
    for name in a.configs.split(","):
        lines.append(f"# {name}: loop of K agent.update ({a.optimizer}, grad_clip {a.grad_clip:g}) | PopulationTrainer(optimizers='agents', "
                     "losses='device').update | ratio | fused RMSprop step (losses='device') | deferred / fused")
        for K in [int(k) for k in a.ks.split(",")]:
            t_loop, t_opt, t_fused = measure_optim(name, K, a.batch, a.reps, a.warmup, a.optimizer, a.grad_clip)
            lines.append(f"  {name} K={K:4d} loop {t_loop:9.3f} ms  optimizers='agents' {t_opt:8.3f} ms  {t_loop / t_opt:7.2f}x  "
                         f"fused RMSprop {t_fused:8.3f} ms  {t_opt / t_fused:6.3f}x")
            print(lines[-1], flush=True)
    return lines


def measure_epoch(name, K, n_rows, B, reps, warmup, T=16):
    """(train_epoch, train_epoch_ring, train_on_rows) median ms for one epoch of n_rows rows per net in minibatches of B."""
    from alphazero_gym_amd.agent.buffers import DeviceReplay
    kind, S, _ = CONFIGS[name]
    over = dict(device="cuda", policy=dict(num_components=2)) if kind == "continuous" else dict(device="cuda")
    cfg = run._merge(run.CONTINUOUS_DEFAULTS if kind == "continuous" else run.DISCRETE_DEFAULTS, over)
    env = make_game(cfg["game"])
    torch.manual_seed(0)
    agents = [run.make_agent(kind, cfg, env, tree_id_base=k) for k in range(K)]
    m = cfg["mcts"]
    steps = (n_rows + T - 1) // T
    sp = run.PopulationSelfPlay([a.nn for a in agents], game=cfg["game"], games_per_net=T, n_rollouts=8, c_uct=m["c_uct"], gamma=m["gamma"],
                                epsilon=m["epsilon"], c_pw=m.get("c_pw", 1.0), kappa=m.get("kappa", 0.5), capacity_steps=steps)
    sp.play_device(steps)
    copies = torch.stack(sp._split(DeviceReplay(sp.engine, 1).rows(), steps))[:, :n_rows].contiguous()
    A = sp.engine.kmax
    tr = PT.PopulationTrainer(agents, max_batch=max(512, 2 * B), losses="device")
    seeds = list(range(K))

    def ring():
        order = np.stack([np.random.RandomState(s).permutation(n_rows) for s in seeds])
        tr.train_epoch_ring(sp, order, batch_size=B)

    t_epoch = _median_ms(lambda: tr.train_epoch(copies, S, A, batch_size=B, shuffle_seeds=seeds), reps, warmup)
    t_ring = _median_ms(ring, reps, warmup)
    t_rows = _median_ms(lambda: tr.train_on_rows(copies, S, A, batch_size=B, shuffle_seeds=seeds), reps, warmup)
    # the split of train_epoch: the K host permutations (all three paths build them) and the native call on a prepared order
    t_perm = _median_ms(lambda: np.stack([np.random.RandomState(s).permutation(n_rows) for s in seeds]), reps, warmup)
    order = np.stack([np.random.RandomState(s).permutation(n_rows) for s in seeds]).astype(np.int32)
    where = _capi.epoch_rows(copies.data_ptr(), S, A, n_rows)
    t_call = _median_ms(lambda: tr._epoch("train_epoch", where, order, B), reps, warmup)
    tr.close()
    sp.close()
    return t_epoch, t_ring, t_rows, t_perm, t_call, A


def main_epoch(a):
    n_mb = len(PT.minibatch_bounds(a.rows, a.batch))
    lines = ["# tools/population_train_latency.py --epoch: one epoch of K nets, %d rows per net in minibatches of %d (%d minibatches), one "
             "MI355X; median wall ms of %d repetitions after %d warm-up, all three in one process on the same self-play rows"
             % (a.rows, a.batch, n_mb, a.reps, a.warmup)]
    ru = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "resource_usage.py"), "dispatch_train", "train"],
                        capture_output=True, text=True)
    lines.append("# tools/resource_usage.py dispatch_train:")
    lines += ["#   " + ln for ln in ru.stdout.splitlines()]
    for name in a.configs.split(","):
        lines.append(f"# {name}: train_epoch | train_epoch_ring | train_on_rows(losses='device') | train_on_rows / train_epoch | "
                     "train_on_rows / train_epoch_ring | of train_epoch: the K host permutations alone | the native call with its host copy "
                     "alone")
        for K in [int(k) for k in a.ks.split(",")]:
            t_epoch, t_ring, t_rows, t_perm, t_call, A = measure_epoch(name, K, a.rows, a.batch, a.reps, a.warmup)
            lines.append(f"  {name} K={K:4d} A={A:2d} epoch {t_epoch:8.3f} ms  epoch on the ring {t_ring:8.3f} ms  train_on_rows {t_rows:8.3f} ms  "
                         f"{t_rows / t_epoch:6.2f}x  {t_rows / t_ring:6.2f}x  permutations {t_perm:8.3f} ms  native call {t_call:7.3f} ms")
            print(lines[-1], flush=True)
    return lines


def _worst_loss_errors(path):
    """The 'loss <head> <loss> <reduction> B=.. net . <key>: float32 torch error X, kernel error Y' lines of pytest -s, reduced to the
    largest pair per (head, loss, d_raw or loss values)."""
    worst = {}
    for ln in open(path):
        ln = ln.strip().lstrip(".")
        if not ln.startswith("loss ") or "kernel error" not in ln:
            continue
        w = ln.split()
        key = (w[1], w[2], "d_raw (relative)" if w[7].startswith("d_raw") else "loss values (absolute)")
        e_y, e_k = float(w[-4].rstrip(",")), float(w[-1])
        old = worst.get(key, (0.0, 0.0))
        worst[key] = (max(old[0], e_y), max(old[1], e_k))
    return ["#   %s %s %s: float32 torch error <= %.3g, kernel error <= %.3g" % (k + v) for k, v in sorted(worst.items())]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--grad-errors", default=None, help="output of pytest -s tests/test_population_trainer.py: its 'grad' lines go into the header")
    ap.add_argument("--loss-errors", default=None, help="output of pytest -s tests/test_population_device_loss.py: the largest errors go into the header")
    ap.add_argument("--epoch", action="store_true", help="measure a whole epoch: train_epoch, train_epoch_ring and train_on_rows")
    ap.add_argument("--rows", type=int, default=512, help="--epoch: rows per net")
    ap.add_argument("--optimizer", choices=["rmsprop", "adam"], default="rmsprop", help="adam (the reference's settings): measure optimizers='agents'")
    ap.add_argument("--grad-clip", type=float, default=0.0, help="a bound > 0: measure optimizers='agents' with gradient clipping")
    ap.add_argument("--layernorm", action="store_true", help="measure PopulationTrainer(layernorm=True) on LayerNorm agents")
    ap.add_argument("--wide", action="store_true", help="measure PopulationTrainer(wide=True) on 4x1024 and 2x512 nets (with --epoch: an epoch too)")
    ap.add_argument("--per-net", action="store_true", help="measure PopulationTrainer(per_net=True) on a learning-rate sweep (see the docstring)")
    ap.add_argument("--rounds", type=int, default=3, help="--per-net: how often (a) and (b) are measured in turn")
    ap.add_argument("--bench", default=None, help="--per-net: a file of bench.py result lines to append")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.per_net:
        a.ks = "" if a.ks == ap.get_default("ks") else a.ks
        if a.configs == ap.get_default("configs"):
            a.configs = ",".join(PERNET_CONFIGS)
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "population_train_latency_pernet.txt")
        with open(out, "w") as f:
            f.write("\n".join(main_pernet(a)) + "\n")
        return
    if a.wide and a.layernorm:
        a.ks = "" if a.ks == ap.get_default("ks") else a.ks   # (the default: 1, 4, 16 of the 4x1024 nets, 1 ... 256 of the 2x512 ones)
        if a.configs == ap.get_default("configs"):
            a.configs = ",".join(WIDE_CONFIGS)
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "population_train_latency_wide_layernorm.txt")
        with open(out, "w") as f:
            f.write("\n".join(main_wide_layernorm(a)) + "\n")
        return
    if a.wide:
        if a.ks == ap.get_default("ks"):
            a.ks = "1,4,16"
        if a.configs == ap.get_default("configs"):
            a.configs = ",".join(WIDE_CONFIGS)
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "population_train_latency_wide.txt")
        with open(out, "w") as f:
            f.write("\n".join(main_wide(a)) + "\n")
        return
    if a.layernorm:
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "population_train_latency_layernorm.txt")
        with open(out, "w") as f:
            f.write("\n".join(main_layernorm(a)) + "\n")
        return
    if a.optimizer != "rmsprop" or a.grad_clip:
        out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "population_train_latency_adam.txt")
        with open(out, "w") as f:
            f.write("\n".join(main_optim(a)) + "\n")
        return
    if a.epoch:
        text = "\n".join(main_epoch(a)) + "\n"
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        return
    lines = ["# tools/population_train_latency.py: one minibatch optimiser step of K nets, batch %d, one MI355X; median wall ms of %d "
             "repetitions after %d warm-up" % (a.batch, a.reps, a.warmup)]
    if a.grad_errors and os.path.exists(a.grad_errors):
        lines.append("# gradient errors against float64 autograd, max|g - g64| / max|g64| per parameter tensor (tests/test_population_trainer.py):")
        log = [ln.strip().lstrip(".") for ln in open(a.grad_errors)]
        lines += ["#   " + ln for ln in log if ln.startswith("grad ")]
        lines.append("# raw against azg_mlp_eval's raw (bound 1e-5):")
        lines += ["#   " + ln for ln in log if ln.startswith("forward vs ")]
        lines.append("# first-step loss dictionaries against float64 (test_end_to_end_update):")
        lines += ["#   " + ln for ln in log if ln.startswith(("discrete ", "continuous "))]
    if a.loss_errors and os.path.exists(a.loss_errors):
        lines.append("# the loss kernel against float64 population_loss, largest of all nets, reductions and batch sizes (tests/test_population_device_loss.py):")
        lines += _worst_loss_errors(a.loss_errors)
    ru = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "resource_usage.py"), "dispatch_train", "train"],
                        capture_output=True, text=True)
    lines.append("# tools/resource_usage.py dispatch_train:")
    lines += ["#   " + ln for ln in ru.stdout.splitlines()]
    for name in a.configs.split(","):
        lines.append(f"# {name}: loop of K agent.update | PopulationTrainer.update | ratio | forward launch | PyTorch loss part | backward launch | "
                     "PopulationTrainer(losses='device').update | ratio to losses='torch'")
        for K in [int(k) for k in a.ks.split(",")]:
            t_loop, t_pop, t_fwd, t_loss, t_bwd, t_fused = measure(name, K, a.batch, a.reps, a.warmup)
            lines.append(f"  {name} K={K:4d} loop {t_loop:9.3f} ms  population {t_pop:8.3f} ms  {t_loop / t_pop:7.2f}x  "
                         f"forward {t_fwd:7.3f}  loss {t_loss:7.3f}  backward {t_bwd:7.3f}  device losses {t_fused:8.3f} ms  {t_pop / t_fused:6.2f}x")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
