"""GPU: azg_trainer_loss at the edges of its inputs (trainer_edges.py's hand-built rows: actions on +-bound and their float32
neighbours, log sigma on and one step beyond both clamps, saturated means, vanished mixture components and logits, counts of 0 and
2^24) and at the row counts where train_loss_kernel's row loop and tr_colsum64's tails change course.

At the edge rows float32 PyTorch is no yardstick (it is 1e-2 of the largest d_raw element off: atanh of a float32 quotient next to
its pole), so there the kernel, whose row arithmetic is float64 rounded once, is held to the float64 reference itself."""
import numpy as np
import pytest
import torch

import trainer_edges as E
import trainer_util as TU
from alphazero_gym_amd import _capi
from device_loss_util import LOG_ALPHA0, alpha_tensors, kernel_loss, make_inputs, make_loss, make_trainer, torch_loss, ulp32

pytestmark = pytest.mark.gpu

NOISE = 2.0 ** -30      # float64 PyTorch's own error at the squash's pole, with a 4 x margin over test_trainer_edges_host.py's pin

EDGE_CASES = [(h, l) for h in E.DISCRETE_HEADS for l in ("alphazero", "a0c", "a0c_tuned")] + [
    (h, l) for h in E.CONT_HEADS for l in ("a0c", "a0c_tuned")]


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("head,loss_name", EDGE_CASES, ids=lambda v: str(v))
def test_edge_rows_against_float64(head, loss_name, reduction):
    """K = 2, the table as the batch.  Per element |d_raw - truth| <= ulp32(|truth|) + 2^-30 max|truth of that net|, per loss key
    |got - truth| <= ulp32(|truth|) + 2^-30 |truth|; float32 PyTorch's error is printed beside the kernel's and enters no bound.
    Exactly: d_raw's zeros on the log sigma columns are the float64 gradient's (the clamp's gate, ends included), and AlphaZero's
    target among tied or all-zero counts is the lowest index."""
    K = 2
    policy = E.head_policy(head)
    desc = _capi.policy_tensors(policy)[0]
    inputs = E.table(head)
    B = inputs[0].shape[1]
    loss = make_loss(loss_name, reduction)
    tuned = loss_name == "a0c_tuned"
    la64 = torch.tensor(LOG_ALPHA0[:K], dtype=torch.float64, requires_grad=True) if tuned else None
    la32 = torch.tensor(LOG_ALPHA0[:K], dtype=torch.float32, requires_grad=True) if tuned else None
    truth, g64 = torch_loss(policy, loss, inputs, torch.float64, la64)
    yard, g32 = torch_loss(policy, loss, inputs, torch.float32, la32)
    state = None
    if tuned:
        la, m, v = alpha_tensors(K)
        state = _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr())
    tr = TU.native().HipTrainer(desc, K, 64)
    got, d_raw = kernel_loss(tr, _capi.loss_cfg(policy, loss), inputs, state)
    tr.close()
    assert torch.isfinite(d_raw).all() and torch.isfinite(got).all()
    fails = []
    for k in range(K):
        scale = float(g64[k].abs().max())
        bound = TU.ulp(g64[k]) + NOISE * scale
        e_k = (d_raw[k].double() - g64[k]).abs()
        e_y = (g32[k].double() - g64[k]).abs()
        print(f"edge loss {head} {loss_name} {reduction} B={B} net {k} d_raw: kernel error {float((e_k / bound).max()):.3g} of its bound "
              f"({float(e_k.max()) / scale:.3g} of the largest), float32 torch {float((e_y / bound).max()):.3g} of it "
              f"({float(e_y.max()) / scale:.3g} of the largest)")
        if not bool((e_k <= bound).all()):
            at = int((e_k / bound).argmax())
            fails.append(("d_raw", k, divmod(at, d_raw.shape[2]), float((e_k / bound).max())))
        for slot, key in enumerate(_capi.LOSS_KEYS):
            if key not in truth:
                assert float(got[k, slot]) == 0.0, (key, k)
                continue
            t = float(truth[key][k])
            b = ulp32(t) + NOISE * abs(t)
            e_y, e_k = abs(float(yard[key][k]) - t), abs(float(got[k, slot]) - t)
            print(f"edge loss {head} {loss_name} {reduction} B={B} net {k} {key}: kernel error {e_k / b:.3g} of its bound, float32 torch {e_y / b:.3g}")
            if not e_k <= b:
                fails.append((key, k, e_k / b))
    assert set(truth) == set(_capi.LOSS_KEYS_OF[_capi.loss_cfg(policy, loss).kind])
    assert not fails, fails
    if head in E.CONT_HEADS:
        cols = E.log_std_columns(head)
        gate = E.continuous_table(head)["gate"]
        assert torch.equal(g64[..., cols] == 0, ~gate)                       # (the CPU test's: every gate edge is in the table)
        assert torch.equal(d_raw[..., cols] == 0, g64[..., cols] == 0)
    elif loss_name == "alphazero":
        t = E.discrete_table(head)
        counts, checked = t["counts"], 0
        for k in range(K):
            for b in range(B):
                tied = t["count_pattern"][k][b] in ("zero", "tied")
                if not tied or t["logit_pattern"][k][b] in ("far", "gone"):
                    continue                     # (a softmax probability of 0 or 1 leaves no sign to read)
                lowest = int(np.argmax(counts[k, b].numpy()))                # numpy: the first of equals
                assert int((counts[k, b] == counts[k, b].max()).sum()) > 1
                sign = d_raw[k, b, 1:] < 0                                   # p_j - [j == target] is negative at the target only
                assert int(sign.sum()) == 1 and int(sign.nonzero()[0]) == lowest, (k, b)
                checked += 1
        assert checked >= 8


ROWS = [2, 3, 5, 255, 256, 257, 511, 512]


@pytest.mark.parametrize("head", ["gmm2", "discrete3"])
def test_row_counts(head):
    """max_batch 512, n_rows on both sides of the row loop's second trip (256 lanes) and at every tail of the four-chain column sum:
    losses and d_raw meet test_d_raw_and_losses_against_autograd's rule (4 x float32 PyTorch + 1 ulp against float64) in both
    reductions.  With reduction "sum" a row's d_raw does not depend on the number of rows (with "mean" it carries 1 / n_rows), so
    there the 257-row call's first 256 rows equal the 256-row call's bit for bit, and the 512-row call's first 511 the 511-row
    call's.  After the 512-row call the tuned loss's log_alpha, exp_avg and exp_avg_sq meet test_alpha_step's bound against float64
    Adam."""
    K = 2
    policy, tr = make_trainer(head, K, max_batch=512)
    full = make_inputs(head, K, 512, 4100)
    fails, kept = [], {}
    for reduction in ("mean", "sum"):
        loss = make_loss("a0c_tuned", reduction)
        cfg = _capi.loss_cfg(policy, loss)
        for n in ROWS:
            inputs = tuple(x[:, :n].contiguous() for x in full)
            refs = {}
            for dtype in (torch.float64, torch.float32):
                p = torch.tensor(LOG_ALPHA0[:K], dtype=dtype, requires_grad=True)
                opt = torch.optim.Adam([p], lr=1e-3)
                losses, grad = torch_loss(policy, loss, inputs, dtype, p, opt)
                refs[dtype] = (losses, grad, (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]))
            (truth, g64, a64), (yard, g32, a32) = refs[torch.float64], refs[torch.float32]
            la, m, v = alpha_tensors(K)
            got, d_raw = kernel_loss(tr, cfg, inputs, _capi.alpha_state(0, la.data_ptr(), m.data_ptr(), v.data_ptr()))
            assert torch.isfinite(d_raw).all() and torch.isfinite(got).all(), (reduction, n)
            kept[reduction, n] = d_raw
            for k in range(K):
                scale = float(g64[k].abs().max())
                e_y = float((g32[k].double() - g64[k]).abs().max()) / scale
                e_k = float((d_raw[k].double() - g64[k]).abs().max()) / scale
                print(f"rows {head} {reduction} n_rows={n} net {k} d_raw: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
                if not e_k <= 4 * e_y + ulp32(scale) / scale:
                    fails.append(("d_raw", reduction, n, k, e_y, e_k))
                for slot, key in enumerate(_capi.LOSS_KEYS):
                    t = float(truth[key][k])
                    e_y, e_k = abs(float(yard[key][k]) - t), abs(float(got[k, slot]) - t)
                    print(f"rows {head} {reduction} n_rows={n} net {k} {key}: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
                    if not e_k <= 4 * e_y + ulp32(t):
                        fails.append((key, reduction, n, k, e_y, e_k))
                if n == 512:
                    for name, dev, t64, t32 in zip(("log_alpha", "exp_avg", "exp_avg_sq"), (la, m, v), a64, a32):
                        t = float(t64[k])
                        e_y, e_k = abs(float(t32[k]) - t), abs(float(dev[k].cpu()) - t)
                        print(f"rows {head} {reduction} n_rows=512 net {k} {name}: float32 torch error {e_y:.3g}, kernel error {e_k:.3g}")
                        if not e_k <= 4 * e_y + ulp32(t):
                            fails.append((name, reduction, k, e_y, e_k))
            if n == 512:
                assert not torch.equal(la.cpu(), torch.tensor(LOG_ALPHA0[:K]))
    tr.close()
    assert not fails, fails
    for small, large in ((256, 257), (511, 512), (2, 3), (3, 5)):
        assert torch.equal(kept["sum", large][:, :small], kept["sum", small]), f"d_raw of rows 0..{small - 1} differs between {small} and {large} rows"
