"""Values at the edges of the population trainer's inputs: the counterpart of edge_values.py for the device trainer.  What self-play
at the edges of the value range writes into the replay rows -- actions on +-bound, log sigma on and beyond both clamps, one-sided
mixture shares, peaked logits -- as hand-built loss rows; and hand-built networks that put every hidden pre-activation of sixteen
units on a kink of the activation's derivative, or a whole LayerNorm row on one value.

Shared by the CPU tests (test_trainer_edges_host.py) and the GPU tests (test_population_device_loss_edges.py,
test_population_trainer_edges.py); numpy and CPU torch only."""
import functools

import numpy as np
import torch

from alphazero_gym_amd.network.policies import make_policy
from device_loss_util import make_head

BOUND = 2.0
LMIN, LMAX = -5.0, 2.0                   # make_policy's log_param_min / log_param_max
MU_HI, MU_LO = 40.0, -40.0               # edge_values.continuous_case's mu_hi / mu_lo: tanh saturates, every action is +-bound
SUB = float(np.finfo(np.float32).smallest_subnormal)
INF = float("inf")


def nxt(x, towards):
    """The float32 neighbour of x in the direction of ``towards``."""
    return float(np.nextafter(np.float32(x), np.float32(towards)))


# ------------------------------------------------------------------------------------------------ a. continuous loss rows
# head: (components, actions per row)
CONT_HEADS = {"normal": (1, 8), "gmm2": (2, 5), "gmm5": (5, 16)}

# log sigma: on the end, one float32 step inside, one step outside, far outside.  torch.clamp passes the gradient on the first two.
LS_LOW = (LMIN, nxt(LMIN, 0.0), nxt(LMIN, -INF), -20.0)
LS_HIGH = (LMAX, nxt(LMAX, 0.0), nxt(LMAX, INF), 20.0)
LS_GATE = (True, True, False, False)

B_IN, NB_IN = nxt(BOUND, 0.0), nxt(-BOUND, 0.0)
ACTION_POOL = (BOUND, -BOUND, B_IN, NB_IN, 0.0, -0.0, 0.5, -1.25, 1.9, -1.999, 1e-3, -0.75)
# mu: the exact pre-image of the action 0.0 (dx == 0), both saturated means, and the float32 nearest to the pre-image of the action 0.5
MU_PRE = float(np.float32(np.arctanh(0.5 / (BOUND + 1e-6))))
MUS = (0.0, MU_HI, MU_LO, MU_PRE)
LC_INTERIOR = (0.3, -0.4, 0.1, -1.0, 0.6)
LC_FAR, LC_GONE = -80.0, -800.0          # exp(-80) = 1.8e-35: a share that rounds to 1 beside it; exp(-800) == 0 in float64
COUNTS = (1.0, 25.0, 1.0, 4.0, 9.0)      # log(1) == 0 beside 25
VALUES = (0.0, 1e6, -1e6, 0.5, -3.0, 1e3, -0.0, 7.25)
V_HAT = (0.25, -2.0, 1e3, 0.0)


def _cont_net(head):
    """One net's rows: a list of (raw, actions, counts, value, gate[C], lc pattern).  Within a row every component has the row's mu
    and a log sigma of the row's class (all near -5 or all near 2): with sigma = e^-5 components that differ in either would have
    responsibilities of exactly 0 for every action, and a zero gradient that no clamp made.  The component that the -800 log
    coefficient removes is one that the clamp gates."""
    C, A = CONT_HEADS[head]
    rows = []
    for cls in (LS_LOW, LS_HIGH):
        for rot in range(4):
            for m, mu in enumerate(MUS):
                n = len(rows)
                ls = [cls[(rot + k) % 4] for k in range(C)]
                gate = [LS_GATE[(rot + k) % 4] for k in range(C)]
                raw = [V_HAT[n % 4]] + [mu] * C + ls
                pattern = None
                if C > 1:
                    pattern = ("equal", "far", "gone", "interior")[(rot + m) % 4]
                    gated = [k for k in range(C) if not gate[k]]
                    if pattern == "gone" and not gated:
                        pattern = "far"
                    lc = [0.25] * C
                    if pattern == "far" and m % 2 == 0:     # one component 80 below the others ...
                        lc[m % C] += LC_FAR
                    elif pattern == "far":                  # ... or all the others 80 below one: its share rounds to 1
                        lc = [0.25 + LC_FAR] * C
                        lc[m % C] = 0.25
                    elif pattern == "gone":
                        lc[gated[0]] += LC_GONE
                    elif pattern == "interior":
                        lc = list(LC_INTERIOR[:C])
                    raw += lc
                actions = [ACTION_POOL[(3 * n + i) % len(ACTION_POOL)] for i in range(A)]
                counts = [COUNTS[(i + n) % len(COUNTS)] for i in range(A)]
                rows.append((raw, actions, counts, VALUES[n % len(VALUES)], gate, pattern))
    return rows


@functools.lru_cache(maxsize=None)
def continuous_table(head):
    """{"raw" [2, B, 1 + n_dist], "actions" [2, B, A], "counts" [2, B, A], "values" [2, B]: float32 CPU tensors; "gate" [2, B, C]: whether
    torch.clamp passes the log sigma's gradient; "pattern": the rows' log-coefficient patterns per net}.  Net 1 is net 0 mirrored
    (mu and actions negated) with the rows in reverse order and values a quarter the size."""
    C, A = CONT_HEADS[head]
    net0 = _cont_net(head)
    net1 = []
    for raw, actions, counts, value, gate, pattern in reversed(net0):
        raw = [raw[0]] + [-x for x in raw[1:1 + C]] + raw[1 + C:]
        net1.append((raw, [-a for a in actions], counts, 0.25 * value, gate, pattern))
    nets = (net0, net1)
    f = lambda i: torch.tensor([[r[i] for r in net] for net in nets], dtype=torch.float32)
    return {"raw": f(0), "actions": f(1), "counts": f(2), "values": f(3),
            "gate": torch.tensor([[r[4] for r in net] for net in nets]), "pattern": [[r[5] for r in net] for net in nets]}


def log_std_columns(head):
    C, _ = CONT_HEADS[head]
    return slice(1 + C, 1 + 2 * C)


# ------------------------------------------------------------------------------------------------ b. discrete loss rows
DISCRETE_HEADS = {"discrete2": 2, "discrete3": 3, "discrete16": 16}
LOGIT_PATTERNS = ("equal", "far", "gone", "interior")       # one logit 80 / 800 above the rest: exp(-800) == 0 in float64
COUNT_PATTERNS = ("zero", "tied", "big", "plain")


def _disc_net(n, shift):
    rows = []
    for li, lp in enumerate(LOGIT_PATTERNS):
        for ci, cp in enumerate(COUNT_PATTERNS):
            r = len(rows)
            logits = [0.5] * n if lp == "equal" else [0.1 * ((7 * j + r) % 5) - 0.2 for j in range(n)]
            if lp in ("far", "gone"):
                logits[(r + shift) % n] += 80.0 if lp == "far" else 800.0
            if cp == "zero":
                counts = [0.0] * n
            elif cp == "tied":              # the largest count twice, the first of them not at index 0 where there is room
                counts = [2.0] * n
                counts[n - 1] = 5.0
                counts[1 if n > 2 else 0] = 5.0
            elif cp == "big":
                counts = [3.0] * n
                counts[(r + shift) % n] = float(2 ** 24)
            else:
                counts = [float((2 * j + r) % 9) for j in range(n)]
            rows.append(([V_HAT[r % 4]] + logits, [float(j) for j in range(n)], counts, VALUES[r % len(VALUES)], lp, cp))
    return rows


@functools.lru_cache(maxsize=None)
def discrete_table(head):
    """{"raw" [2, 16, 1 + n], "actions" [2, 16, n] (every index 0 .. n - 1), "counts" [2, 16, n], "values" [2, 16], "logit_pattern",
    "count_pattern": per net and row}.  Net 1 peaks another logit and another count, rows reversed."""
    n = DISCRETE_HEADS[head]
    nets = (_disc_net(n, 0), list(reversed(_disc_net(n, 1))))
    f = lambda i: torch.tensor([[r[i] for r in net] for net in nets], dtype=torch.float32)
    return {"raw": f(0), "actions": f(1), "counts": f(2), "values": f(3), "logit_pattern": [[r[4] for r in net] for net in nets],
            "count_pattern": [[r[5] for r in net] for net in nets]}


def head_policy(head):
    """device_loss_util.py's make_head, and its 16-logit sibling."""
    if head == "discrete16":
        torch.manual_seed(0)
        return make_policy(3, 1, "discrete", [16], "relu", num_actions=16)
    return make_head(head)


def table(head):
    """The four input tensors of a head's table, in make_inputs' order."""
    t = continuous_table(head) if head in CONT_HEADS else discrete_table(head)
    return t["raw"], t["actions"], t["counts"], t["values"]


# ------------------------------------------------------------------------------------------------ c. kink nets
ACTIVATIONS = ("relu", "elu", "leakyrelu", "relu6", "silu", "hardswish")
KINK_UNITS = 16
_SATURATION = (20.0, -20.0, 88.0, -88.0, 104.0, -104.0)     # SiLU's expf(-z) overflows past 88.7, ELU's expm1 is -1 below -17
_INTERIOR = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)


def kink_table(act):
    """Sixteen float32 biases: +-0 and the kinks of the activation's derivative with their float32 neighbours on both sides, the
    saturation points, and interior values to make sixteen."""
    t = [0.0, -0.0, SUB, -SUB]
    if act == "relu6":
        t += [6.0, nxt(6.0, 0.0), nxt(6.0, INF)]
    if act == "hardswish":
        t += [3.0, nxt(3.0, 0.0), nxt(3.0, INF), -3.0, nxt(-3.0, 0.0), nxt(-3.0, -INF)]
    t += _SATURATION
    t += _INTERIOR[:KINK_UNITS - len(t)]
    assert len(t) == KINK_UNITS
    return np.array(t, np.float32)


def dact64(act, z):
    """act'(z) in float64 with torch's conventions at the kinks (what float64 autograd multiplies by; the CPU test holds it to
    autograd): 0 at ReLU's and 1 at ELU's 0, 0 at both ends of ReLU6, and for Hardswish 0 at -3 and 1 at 3."""
    z = np.asarray(z, np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
    return {"relu": np.where(z > 0, 1.0, 0.0), "elu": np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0))),
            "leakyrelu": np.where(z > 0, 1.0, 0.01), "relu6": np.where((z > 0) & (z < 6), 1.0, 0.0),
            "silu": s * (1.0 + z * (1.0 - s)), "hardswish": np.where(z <= -3, 0.0, np.where(z < 3, z / 3.0 + 0.5, 1.0))}[act]


def representable_derivative(act):
    """[16] bool: the kink units whose float64 derivative is 0 or at least 2^-24.  The device forms ELU's derivative as a + 1 from the
    float32 a = expm1(z), and SiLU's from a float32 sigmoid: a derivative below half an ulp of 1 may round to 0 there (an absolute
    error below 2^-24 of the derivative's scale, which the tensor's tolerance holds), so only on these units is the device's zero
    pattern the float64 one."""
    d = np.abs(dact64(act, kink_table(act)))
    return (d == 0) | (d >= 2.0 ** -24)


@functools.lru_cache(maxsize=None)
def kink_net(act):
    """make_policy(4, 1, "discrete", [32, 32], act, num_actions=2): units 0-15 of both hidden layers have a zero weight row and
    kink_table(act) as bias, so their Z is the bias for every observation; units 16-31 and the heads are seeded random."""
    torch.manual_seed(900 + ACTIVATIONS.index(act))
    pol = make_policy(4, 1, "discrete", [32, 32], act, num_actions=2)
    table = torch.from_numpy(kink_table(act))
    with torch.no_grad():
        for lin in (pol.trunk[0], pol.trunk[2]):
            lin.weight[:KINK_UNITS] = 0.0
            lin.bias[:KINK_UNITS] = table
    return pol


@functools.lru_cache(maxsize=None)
def kink_data():
    """(obs [18, 4], d_raw [18, 3]): 17 seeded observations and one all-zero row."""
    g = torch.Generator().manual_seed(77)
    obs = torch.cat([torch.randn((17, 4), generator=g), torch.zeros((1, 4))])
    d_raw = torch.randn((18, 3), generator=g) / 18
    return obs, d_raw


# ------------------------------------------------------------------------------------------------ d. a LayerNorm net
LN_ZERO_ROW = 5


@functools.lru_cache(maxsize=None)
def layernorm_net():
    """[48, 80] ReLU with LayerNorm, gamma = 1 + 0.5 randn, beta = 0.5 randn, and first-layer biases <= 0 (one of them 0): the
    all-zero observation leaves every unit of the first layer at exactly 0, a LayerNorm row of equal values."""
    torch.manual_seed(950)
    pol = make_policy(4, 1, "discrete", [48, 80], "relu", num_actions=2, layernorm=True)
    g = torch.Generator().manual_seed(951)
    with torch.no_grad():
        for mod in pol.trunk:
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.5 * torch.randn(mod.bias.shape, generator=g))
        pol.trunk[0].bias.copy_(-pol.trunk[0].bias.abs())
        pol.trunk[0].bias[0] = 0.0
    return pol


@functools.lru_cache(maxsize=None)
def layernorm_data():
    """(obs [17, 4], d_raw [17, 3]): seeded, row LN_ZERO_ROW of the observations all zero."""
    g = torch.Generator().manual_seed(78)
    obs = torch.randn((17, 4), generator=g)
    obs[LN_ZERO_ROW] = 0.0
    d_raw = torch.randn((17, 3), generator=g) / 17
    return obs, d_raw
