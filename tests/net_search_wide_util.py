"""Shared by the tests of per-net search settings at padded widths >= 512 (azg_set_net_search_ex with AZG_NET_SEARCH_WIDE): the rows
of the matrix, the three nets' settings, and the number of trees each row's nets get."""
import net_search_util as N
import parity_util as P
import test_population_wide as W

K = 3
NARROW_PW = N.NARROW_PW   # net 1's widening in continuous mode: (0.6, 0.45), never more children than a row's own pair entitles a node to


def matrix_rows():
    """Every parity_util.CONFIGS row with a hidden width >= 512 (by index), and test_population_wide's LayerNorm row (the row itself)."""
    return [ci for ci, cfg in enumerate(P.CONFIGS) if max(cfg[2]) >= 512] + [W.PENDULUM_2x512_LN]


def cfg_of(row):
    return P.CONFIGS[row] if isinstance(row, int) else row


def row_id(row):
    return f"cfg{row}" if isinstance(row, int) else "pendulum_2x512_ln"


def net_settings(row):
    """Net 0: the row's own settings.  Net 1: c_uct x 4, gamma 0.9, epsilon 0.25, and in continuous mode the narrow widening pair.
    Net 2: c_uct x 0.25 and gamma 0.97.  (Every wide row has gamma 1 and epsilon 0: one launch mixes the closed-form backup with the
    general chain, and cached selections with epsilon-greedy descents.)"""
    s0 = N.shared_settings(cfg_of(row))
    assert s0["gamma"] == 1.0 and s0["epsilon"] == 0.0, s0
    s1 = dict(s0, c_uct=s0["c_uct"] * 4.0, gamma=0.9, epsilon=0.25)
    if "c_pw" in s0:
        s1.update(c_pw=NARROW_PW[0], kappa=NARROW_PW[1])
    s2 = dict(s0, c_uct=s0["c_uct"] * 0.25, gamma=0.97)
    return [s0, s1, s2]


def lockstep_shaped(row):
    return bool(W._lockstep_shaped(cfg_of(row)))


def trees_per_net(row):
    """Lock-step shaped rows: 32, one team per net -- three teams read three different records.  One-launch rows: 19, a full and a ragged
    16-tree workgroup per net."""
    return 32 if lockstep_shaped(row) else 19


def cases():
    """(row, variant) as test_population_wide._matrix chooses them: the rows that are not lock-step shaped run on the search kernel
    whatever is forced, so `launches` and `persistent` would re-run their default."""
    out = []
    for row in matrix_rows():
        for v in W.VARIANTS:
            if P.moot(cfg_of(row), v) or (not lockstep_shaped(row) and v in ("launches", "persistent")):
                continue
            out.append((row, v))
    return out


def result_width(row, n_sims):
    """The population engine's Kmax (continuous mode: the row's own widening, the widest of the three; discrete: None)."""
    s0 = N.shared_settings(cfg_of(row))
    return N.kmax_of(s0, n_sims) if "c_pw" in s0 else None


def oracle(row, T, settings=None, nets=K):
    """What the population must compute: `nets` oracle engines, net k created with settings[k], its weights and tree_id_base + k*T."""
    kw, desc, blobs, roots, carry = W._inputs(cfg_of(row), T, nets)
    st = net_settings(row)[:nets] if settings is None else settings
    return N.oracle_nets(kw, desc, blobs, roots, carry, W.SIDX, st, width=result_width(row, kw["n_sims"]))

