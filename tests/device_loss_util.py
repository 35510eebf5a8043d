"""What the tests of the population trainer's device losses share (test_population_device_loss.py, its _edges file,
test_trainer_edges_host.py and trainer_edges.py): the heads and losses under test, seeded loss inputs, population_loss on the CPU as
truth and yardstick, and azg_trainer_loss through a native trainer.  Importing it needs neither a GPU nor the native library."""
import numpy as np
import torch

from alphazero_gym_amd import _capi
from alphazero_gym_amd.agent.losses import A0CLoss, A0CLossTuned, AlphaZeroLoss
from alphazero_gym_amd.agent.population_trainer import population_loss
from alphazero_gym_amd.network.policies import make_policy
from trainer_util import DEV, native

BOUND = 2.0
# head: (kind, logits or components, actions per row)
HEADS = {"discrete2": ("discrete", 2, 2), "discrete3": ("discrete", 3, 3), "normal": ("normal", 1, 8), "gmm2": ("gmm", 2, 5),
         "gmm5": ("gmm", 5, 16)}
LOG_ALPHA0 = [float(np.log(a)) for a in (0.5, 1.0, 2.0, 0.25, 1.5)]


def make_head(head):
    kind, n, _ = HEADS[head]
    torch.manual_seed(0)
    if kind == "discrete":
        return make_policy(3, 1, "discrete", [16], "relu", num_actions=n)
    return make_policy(3, 1, "normal", [16], "elu", num_components=n, action_bound=BOUND)


def make_loss(name, reduction, clip=0.0):
    if name == "alphazero":
        return AlphaZeroLoss(policy_coeff=1.0, value_coeff=0.5, reduction=reduction)
    if name == "a0c":
        return A0CLoss(tau=0.1, policy_coeff=0.1, alpha=0.05, value_coeff=1.0, reduction=reduction)
    return A0CLossTuned(action_dim=1, alpha_init=1.0, lr=1e-3, tau=0.1, policy_coeff=0.1, value_coeff=1.0, reduction=reduction,
                        grad_clip=clip, device="cpu")


def make_inputs(head, K, B, seed):
    """(raw [K, B, 1 + n_dist], actions [K, B, A], counts [K, B, A], values [K, B]) on the CPU, float32."""
    kind, n, A = HEADS[head]
    g = torch.Generator().manual_seed(seed)
    n_dist = {"discrete": n, "normal": 2, "gmm": 3 * n}[kind]
    raw = torch.randn((K, B, 1 + n_dist), generator=g)
    if kind == "normal":
        raw[..., 2] *= 4.0            # log_std on both sides of the clamp [-5, 2]
    elif kind == "gmm":
        raw[..., 1 + n:1 + 2 * n] *= 4.0
    if kind == "discrete":
        actions = torch.arange(A, dtype=torch.float32).repeat(K, B, 1)
        counts = torch.randint(0, 9, (K, B, A), generator=g).float()
    else:
        actions = 0.98 * BOUND * torch.tanh(torch.randn((K, B, A), generator=g))
        extra = torch.randint(0, A, (K, B, 25 - A), generator=g)      # positive integers that sum to 25
        counts = torch.ones((K, B, A)).scatter_add_(2, extra, torch.ones(extra.shape))
    values = torch.randn((K, B), generator=g)
    return raw, actions, counts, values


def torch_loss(policy, loss, inputs, dtype, log_alpha=None, alpha_optimizer=None):
    """population_loss on the CPU in ``dtype``: ({key: [K]}, raw.grad)."""
    raw, actions, counts, values = (x.detach().to(dtype) for x in inputs)
    raw = raw.clone().requires_grad_(True)
    out = population_loss(policy, loss, raw, actions, counts, values.unsqueeze(-1), log_alpha, alpha_optimizer)
    out["loss"].sum().backward()
    return {k: v.detach() for k, v in out.items()}, raw.grad


def kernel_loss(tr, cfg, inputs, state=None):
    """azg_trainer_loss: (losses [K, 5], d_raw) on the CPU."""
    raw, actions, counts, values = (x.to(DEV).contiguous() for x in inputs)
    d_raw = torch.full_like(raw, float("nan"))
    losses = torch.full((raw.shape[0], 5), float("nan"), device=DEV)
    torch.cuda.synchronize()
    tr.loss(raw.data_ptr(), actions.data_ptr(), counts.data_ptr(), values.data_ptr(), raw.shape[1], actions.shape[2], cfg, state,
            d_raw.data_ptr(), losses.data_ptr())
    return losses.cpu(), d_raw.cpu()


def make_trainer(head, K, max_batch=128):
    policy = make_head(head)
    desc = _capi.policy_tensors(policy)[0]
    return policy, native().HipTrainer(desc, K, max_batch)


def alpha_tensors(K, dtype=torch.float32, device=DEV):
    return (torch.tensor(LOG_ALPHA0[:K], dtype=dtype, device=device), torch.zeros(K, dtype=dtype, device=device),
            torch.zeros(K, dtype=dtype, device=device))


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))
