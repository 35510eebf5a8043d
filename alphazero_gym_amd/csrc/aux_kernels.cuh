// aux_kernels.cuh -- result gathering and the device-resident self-play step (compiled in one translation unit: engine_selfplay.hip).
// The self-play step has two kernels that differ in where the root's children come from and how the final action is picked over them:
// selfplay_kernel16 (at most 16 root children, 16 lanes per game, from MCTS.return_results) and selfplay_kernel (more, continuous
// mode only, one thread per game, from the published trees).  What follows the pick is selfplay_finish for both, and the game itself
// is env.cuh's game_obs / game_step, shared with the policy rollouts (rollout.cuh).
// A row's actions | counts | Q columns and its value target have one definition per form (row_targets16, row_targets), shared by the
// self-play kernels and by the reanalysis kernels, which rewrite those columns of a stored row from a fresh search of its kept state.
// The pick has one definition per form too (final_pick16, final_pick), shared by the self-play kernels and by the search rollouts at the
// end of this file (azgym_search_rollout.h): whole evaluation episodes under MCTS, the same step without a replay row.
#pragma once
#include "records.h"
#include "replay_ring.h"
#include "env.cuh"
#include "tree.cuh"
#include "results.cuh"
#include "../../include/azgym_nstep.h"

// ------------------------------------------------------------------------------------------------ result gathering

// MCTS.return_results for all trees from their published (global) form: 16 trees per workgroup.
#define RS_TREES 16
__global__ __launch_bounds__(16 * RS_TREES) void results_kernel(KParams P) {
    const int sub = threadIdx.x & 15;
    const int tree = blockIdx.x * RS_TREES + (threadIdx.x >> 4);
    if (tree >= P.B) return;
    const size_t tb = (size_t)tree * P.R;
    TreeStore<TS_GLOBAL> ts;
    ts.hot = P.hot + tb;
    ts.child = P.child + tb * P.Kp;
    ts.prior = P.prior + tb;
    if (P.mode == AZG_MODE_CONTINUOUS) results_for_tree<true, TS_GLOBAL>(P, ts, P.cold + tb, P.action + tb, tb, tree, sub);
    else results_for_tree<false, TS_GLOBAL>(P, ts, P.cold + tb, P.action + tb, tb, tree, sub);
}

// ------------------------------------------------------------------------------------------------ the self-play step

// One self-play step after a search: replay row, the agent's final action rule, the real env step, episode bookkeeping and the
// next search's root (the CPU oracle restates the same arithmetic for the parity tests).  Kmax, the value target and the env are
// KParams' res_Kmax, res_v_target and env_id.
// The agents' final-action rule and the step its AZG_STREAM_ACT draw is keyed with
struct ActRule {
    int deterministic;
    int final_selection;      // AZG_FS_*
    double agent_eps;         // ContinuousAgent.epsilon
    const double* ctab;       // (c / m)^temperature at [m (m + 1) / 2 + c], 0 <= c <= m <= n_sims, built by the host (NULL: temperature 1)
    unsigned step_idx;
};
struct SelfPlay {
    int max_len;
    int S_obs;                // width of the env's observation: the row's first columns
    ActRule rule;
    int* t; int* episode; int* fcnt;
    double* ret; double* fsum;
    float* rows;          // this step's block [B][row_len]
    double* states;       // this step's block of the state ring [B][S] (azg_selfplay_keep_states), NULL: states are not kept
    // this step's blocks [B] of the kept transitions (azg_selfplay_keep_transitions, azgym_nstep.h), all NULL: not kept
    double* tr_reward; double* tr_value; float* tr_action; int* tr_end;
    double* roots; int* carry;
};

// What follows the pick, for one game by its one writer: the row's observation and value-target columns, the real env step with the
// picked action, the episode's books and the next search's root.  carry: the visit count of the picked child's node where the next
// search may start from it (discrete mode), else 0; an episode's end drops it.  Where transitions are kept, the step's entry: the reward
// in a tree node's units (Cold::r: continuous mode divides by reward_scale, as tree_phases.cuh does), the value target before its
// rounding, the action and how the step ended.
__device__ __forceinline__ void selfplay_finish(const KParams& P, const SelfPlay& sp, int tree, float* row, float action, double v_target,
                                                int carry) {
    const int S = P.S;
    double root[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < S; ++k) root[k] = sp.roots[(size_t)tree * S + k];
    if (sp.states)   // the state this step's search started from, beside its row
        for (int k = 0; k < S; ++k) sp.states[(size_t)tree * S + k] = root[k];
    // (the MountainCars' observation is (position, velocity), S_obs = 2; Acrobot: six)
    float obs[8];
    double sn;
    game_obs(P.env_id, root, obs, &sn);
    for (int k = 0; k < 8; ++k) if (k < sp.S_obs) row[k] = obs[k];
    row[sp.S_obs + 3 * P.res_Kmax] = (float)v_target;
    double ns[4] = {0.0, 0.0, 0.0, 0.0}, r;
    int done;
    game_step(P.env_id, root, sn, action, ns, &r, &done);
    double ret = sp.ret[tree] + r;
    int t = sp.t[tree] + 1;
    if (sp.tr_reward) {
        sp.tr_reward[tree] = P.mode == AZG_MODE_CONTINUOUS ? r / P.reward_scale : r;
        sp.tr_value[tree] = v_target;
        sp.tr_action[tree] = action;
        sp.tr_end[tree] = done ? AZG_END_TERMINAL : (t >= sp.max_len ? AZG_END_LENGTH : AZG_END_NONE);
    }
    if (done || t >= sp.max_len) {
        sp.fsum[tree] = sp.fsum[tree] + ret;
        sp.fcnt[tree] += 1;
        ret = 0.0;
        t = 0;
        const int ep = sp.episode[tree] + 1;
        sp.episode[tree] = ep;
        azg_reset_state(P.seed, (unsigned)(P.tree_base + tree), (unsigned)ep, azg_reset_kind(P.env_id), ns);
        carry = 0;
    }
    sp.carry[tree] = carry;
    sp.ret[tree] = ret;
    sp.t[tree] = t;
    for (int k = 0; k < S; ++k) sp.roots[(size_t)tree * S + k] = ns[k];
}

// Lane `sub` of a game's 16 on the root's children as MCTS.return_results left them (written by the search kernel's epilogue from its
// LDS-resident trees, or by results_kernel after the lock-step / team kernels): no tree record is read here, so a search need not
// publish its trees.  root_totals16 returns the root's totals; want_target (a constant at every call): with the value target, whose
// on-policy form is added up in the reference's order, reading the lanes' values by shuffles (executed by the whole row: loop bounds
// are row-uniform).  row_targets16 also writes the row's actions | counts | Q columns side by side.
struct RootLane { int edge_n, node_n; double Q; float act; bool has; };
struct RootTotals { int nc, tot, cmax, amax; double qmax, v_target; };
__device__ __forceinline__ RootTotals root_totals16(const KParams& P, int tree, int sub, RootLane& h, bool want_target) {
    const bool cont = P.mode == AZG_MODE_CONTINUOUS;
    const int K = P.res_Kmax;
    RootTotals r;
    const int nc = P.res_nch[tree];
    // lane a: root child a
    const bool has = sub < nc;
    {
        const size_t o = (size_t)tree * K + (sub < K ? sub : 0);
        const int cn = P.res_child_n[o];                   // the child node's visit count, -1: the edge has no child node yet
        h.edge_n = has ? P.res_counts[o] : 0;
        h.Q = has ? P.res_Q[o] : 0.0;
        h.node_n = (has && cn >= 0) ? cn : 0;
    }
    h.has = has;
    h.act = has ? (cont ? P.res_actions[(size_t)tree * K + sub] : (float)sub) : 0.0f;
    int tot = has ? h.edge_n : 0;
    double qmax = has ? h.Q : -__builtin_huge_val();
    int ckey = has ? ((h.edge_n << 4) | (15 - sub)) : -1;          // largest count, lowest index on ties (counts < 2^27)
    for (int m = 1; m < 16; m <<= 1) {
        tot += __shfl_xor(tot, m, 16);
        const double o = __shfl_xor(qmax, m, 16);
        qmax = o > qmax ? o : qmax;
        const int ok = __shfl_xor(ckey, m, 16);
        ckey = ok > ckey ? ok : ckey;
    }
    if (nc == 0) qmax = 0.0;
    double onp = 0.0;
    if (want_target && P.res_v_target == AZG_VT_ON_POLICY) {
        if (!cont) {
            for (int a = 0; a < nc; ++a) onp += ((double)__shfl(h.edge_n, a, 16) / (double)tot) * __shfl(h.Q, a, 16);
        } else {
            for (int a = 0; a < nc; ++a) {
                const double qa = __shfl(h.Q, a, 16);
                for (int b2 = 0; b2 < nc; ++b2) onp += ((double)__shfl(h.edge_n, b2, 16) / (double)tot) * qa;
            }
        }
    }
    r.nc = nc; r.tot = tot; r.qmax = qmax; r.cmax = ckey >> 4; r.amax = 15 - (ckey & 15);
    r.v_target = P.res_v_target == AZG_VT_ON_POLICY ? onp : qmax;
    return r;
}
__device__ __forceinline__ RootTotals row_targets16(const KParams& P, int tree, int sub, float* targets, RootLane& h) {
    const RootTotals r = root_totals16(P, tree, sub, h, true);
    const int K = P.res_Kmax;
    if (sub < K) {
        targets[sub] = h.act;
        targets[K + sub] = h.has ? (float)h.edge_n : 0.0f;
        targets[2 * K + sub] = h.has ? (float)h.Q : 0.0f;
    }
    return r;
}

// The final action of a game with at most 16 root children, for the game's 16 lanes (all of them return the pick; the shuffles are
// executed by the whole row: loop bounds are row-uniform).  Everything whose float64 order matters (normaliser sums, the inverse-CDF
// walk of numpy's random.choice) is added up in the reference's order, reading the lanes' values by shuffles.
__device__ __forceinline__ int final_pick16(const KParams& P, const ActRule& ar, unsigned gtree, const RootTotals& rt, const RootLane& h) {
    const bool cont = P.mode == AZG_MODE_CONTINUOUS;
    const int nc = rt.nc, cmax = rt.cmax;
    const bool has = h.has;
    // discrete: the lane's unnormalised pi entry (stable_normalizer's x / max(x), to the temperature)
    double x = 0.0;
    if (!cont && has) {
        if (ar.final_selection == AZG_FS_MAX_VALUE) x = h.Q / rt.qmax;
        else x = ar.ctab ? ar.ctab[(size_t)cmax * (cmax + 1) / 2 + h.edge_n] : (double)h.edge_n / (double)cmax;
    }
    int pick = 0;
    if (cont) {
        // ContinuousAgent.act (agents.py:524-535): actions[Qs.argmax()] / actions[counts.argmax()], first index on ties
        pick = rt.amax;
        if (ar.final_selection == AZG_FS_MAX_VALUE) {
            double qb = 0.0;
            for (int a = 0; a < nc; ++a) { const double q = __shfl(h.Q, a, 16); if (a == 0 || q > qb) { qb = q; pick = a; } }
        }
        if (ar.agent_eps != 0.0) {
            // epsilon_greedy (agents.py:471-490): random.random() < epsilon -> np.random.choice(actions)
            azg_u32x4 b = azg_draw(P.seed, gtree, ar.step_idx, 0u, AZG_STREAM_ACT);
            if ((double)azg_u01(b.v[0]) < ar.agent_eps) pick = (int)(b.v[1] % (unsigned)nc);
        }
    } else {
        // DiscreteAgent.act (agents.py:294-301): pi = stable_normalizer(Qs | counts, temperature) (helpers.py:26-27), then
        // pi.argmax() or np.random.choice(len(pi), p=pi) (cdf = cumsum(pi); cdf /= cdf[-1]; first index with u < cdf)
        double sum = 0.0;
        for (int a = 0; a < nc; ++a) sum = sum + __shfl(x, a, 16);
        const double pi = has ? __builtin_fabs(x / sum) : 0.0;
        double best = 0.0, cum = 0.0;
        for (int a = 0; a < nc; ++a) {
            const double pa = __shfl(pi, a, 16);
            if (a == 0 || pa > best) { best = pa; pick = a; }
            cum = cum + pa;
        }
        if (!ar.deterministic) {
            azg_u32x4 b = azg_draw(P.seed, gtree, ar.step_idx, 0u, AZG_STREAM_ACT);
            const double u = ((double)b.v[0] + 0.5) * (1.0 / 4294967296.0);
            const double last = cum;
            double c = 0.0;
            pick = nc - 1;
            bool found = false;
            for (int a = 0; a < nc; ++a) {
                const double pa = __shfl(pi, a, 16);
                if (!found) {
                    c = c + pa;
                    if (u < c / last) { pick = a; found = true; }
                }
            }
        }
    }
    return pick;
}

// The common case (at most 16 root children: every LDS-tree configuration): 16 lanes per game, lane a = root child a.  The replay
// row is written by the lanes side by side (row_targets16); totals are row reductions that do not depend on the order (integer sum,
// maximum, first index of the largest count); everything whose float64 order matters (on-policy target, normaliser sums, the
// inverse-CDF walk of numpy's random.choice) is added up in the reference's order, reading the lanes' values by shuffles
// (final_pick16); the game's first lane finishes the step (selfplay_finish).  Same arithmetic as selfplay_kernel below (roots with
// more children) and as the oracle.
#define SP_TREES 16
__global__ __launch_bounds__(16 * SP_TREES) void selfplay_kernel16(KParams P, SelfPlay sp) {
    const int sub = threadIdx.x & 15;
    const int tree = blockIdx.x * SP_TREES + (threadIdx.x >> 4);
    if (tree >= P.B) return;
    const bool cont = P.mode == AZG_MODE_CONTINUOUS;
    const unsigned gtree = (unsigned)(P.tree_base + tree);
    const int K = P.res_Kmax, S_obs = sp.S_obs;
    float* row = sp.rows + (size_t)tree * (S_obs + 3 * K + 1);
    RootLane h;
    const RootTotals rt = row_targets16(P, tree, sub, row + S_obs, h);
    const int pick = final_pick16(P, sp.rule, gtree, rt, h);
    const float pact = __shfl(h.act, pick, 16);
    const int pnode_n = __shfl(h.node_n, pick, 16);   // (0 where the picked edge has no child node yet)
    if (sub != 0) return;
    selfplay_finish(P, sp, tree, row, pact, rt.v_target, cont ? 0 : pnode_n);
}

// A root's child edges in the published (global) trees, for one thread: child a's record id (beyond the last child: record 0, the
// root itself, so that no read leaves the tree), its record and its action
struct RootEdges {
    const KParams& P;
    size_t tb;
    int nc;
    __device__ __forceinline__ RootEdges(const KParams& P_, int tree) : P(P_), tb((size_t)tree * P_.R), nc(P_.hot[(size_t)tree * P_.R].n_child) {}
    __device__ __forceinline__ int id(int a) const { return a < nc ? (int)P.child[tb * P.Kp + a] : 0; }
    __device__ __forceinline__ RecL rec(int a) const { return P.hot[tb + id(a)]; }
    __device__ __forceinline__ float act(int a) const { return P.action[tb + id(a)]; }
};
// The root's totals from those edges (continuous mode): the first index of the largest count and, with want_target (a constant at
// every call), the value target.  row_targets also writes the row's actions | counts | Q columns.
__device__ __forceinline__ double root_totals(const KParams& P, const RootEdges& re, int* amax_out, bool want_target) {
    const int nc = re.nc;
    double qmax = 0.0, onp = 0.0;
    long tot = 0;
    int cmax = 0, amax = 0;
    for (int a = 0; a < nc; ++a) {
        const RecL h = re.rec(a);
        tot += h.edge_n;
        if (a == 0 || h.Q > qmax) qmax = h.Q;
        if (a == 0 || h.edge_n > cmax) { cmax = h.edge_n; amax = a; }
    }
    if (want_target && P.res_v_target == AZG_VT_ON_POLICY)
        for (int a = 0; a < nc; ++a)
            for (int b = 0; b < nc; ++b) onp += ((double)re.rec(b).edge_n / (double)tot) * re.rec(a).Q;
    *amax_out = amax;
    return P.res_v_target == AZG_VT_ON_POLICY ? onp : qmax;
}
__device__ __forceinline__ double row_targets(const KParams& P, const RootEdges& re, float* targets, int* amax_out) {
    const int K = P.res_Kmax, nc = re.nc;
    for (int a = 0; a < K; ++a) {
        const bool has = a < nc;
        const RecL h = re.rec(a);
        targets[a] = has ? re.act(a) : 0.0f;
        targets[K + a] = has ? (float)h.edge_n : 0.0f;
        targets[2 * K + a] = has ? (float)h.Q : 0.0f;
    }
    return root_totals(P, re, amax_out, true);
}
// The final action of a game from those edges (continuous mode), by one thread; amax: root_totals' first index of the largest count.
__device__ __forceinline__ int final_pick(const KParams& P, const ActRule& ar, unsigned gtree, const RootEdges& re, int amax) {
    const int nc = re.nc;
    // ContinuousAgent.act (agents.py:524-535): actions[Qs.argmax()] / actions[counts.argmax()], first index on ties
    int pick = amax;
    if (ar.final_selection == AZG_FS_MAX_VALUE) {
        double qb = 0.0;
        for (int a = 0; a < nc; ++a) { const double q = re.rec(a).Q; if (a == 0 || q > qb) { qb = q; pick = a; } }
    }
    if (ar.agent_eps != 0.0) {
        // epsilon_greedy (agents.py:471-490): random.random() < epsilon -> np.random.choice(actions)
        azg_u32x4 b = azg_draw(P.seed, gtree, ar.step_idx, 0u, AZG_STREAM_ACT);
        if ((double)azg_u01(b.v[0]) < ar.agent_eps) pick = (int)(b.v[1] % (unsigned)nc);
    }
    return pick;
}

// Roots with more than 16 children: one thread per game, reading the root's child edges from the published (global) trees, so this
// path needs no launch_results.  Continuous mode only: more than 16 children per node take progressive widening -- a discrete Kmax is
// the env's 2 or 3 actions (azg_engine_create) -- and azg_selfplay_step refuses anything else before it launches.  A continuous search
// never reuses a subtree: carry is 0.
#define SPW_THREADS 64
__global__ __launch_bounds__(SPW_THREADS) void selfplay_kernel(KParams P, SelfPlay sp) {
    const int tree = blockIdx.x * blockDim.x + threadIdx.x;
    if (tree >= P.B) return;
    const unsigned gtree = (unsigned)(P.tree_base + tree);
    const int K = P.res_Kmax, S_obs = sp.S_obs;
    float* row = sp.rows + (size_t)tree * (S_obs + 3 * K + 1);
    const RootEdges re(P, tree);
    int amax = 0;
    const double v_target = row_targets(P, re, row + S_obs, &amax);
    const int pick = final_pick(P, sp.rule, gtree, re, amax);
    selfplay_finish(P, sp, tree, row, re.act(pick), v_target, 0);
}

// ------------------------------------------------------------------------------------------------ reanalysis of stored rows

// Search stored positions again (azg_selfplay_reanalyse): tree t takes the kept state of its own game column in ring slot slots[t]
// (NULL: `slot` for every tree) as a fresh root.  slots, when given, is the device copy the host has range-checked.
struct Reanalyse {
    const int* slots;
    int slot;
    int S_obs;
    const double* states;   // the state ring [capacity_steps][B][S]
    float* rows;            // the replay ring [capacity_steps][B][row_len]
    double* roots; int* carry;   // the search's staging roots [B][S] and carried counts [B] (zero)
    double* tr_value;       // the kept float64 value targets [capacity_steps][B] (azg_selfplay_keep_transitions), NULL: not kept
};
__device__ __forceinline__ int reanalyse_slot(const Reanalyse& ra, int tree) { return ra.slots ? ra.slots[tree] : ra.slot; }
__device__ __forceinline__ float* reanalyse_row(const KParams& P, const Reanalyse& ra, int tree) {
    return ra.rows + ((size_t)reanalyse_slot(ra, tree) * P.B + tree) * (size_t)(ra.S_obs + 3 * P.res_Kmax + 1);
}

#define RA_THREADS 256
__global__ __launch_bounds__(RA_THREADS) void reanalyse_gather_kernel(KParams P, Reanalyse ra) {
    const int tree = blockIdx.x * blockDim.x + threadIdx.x;
    if (tree >= P.B) return;
    const double* src = ra.states + ((size_t)reanalyse_slot(ra, tree) * P.B + tree) * P.S;
    for (int k = 0; k < P.S; ++k) ra.roots[(size_t)tree * P.S + k] = src[k];
    ra.carry[tree] = 0;
}

// The two self-play kernels without the pick, the env step and the books: the target columns of row (slot, tree) from the search that
// just ran.  The observation columns stay; every row has one writer.
__global__ __launch_bounds__(16 * SP_TREES) void reanalyse_kernel16(KParams P, Reanalyse ra) {
    const int sub = threadIdx.x & 15;
    const int tree = blockIdx.x * SP_TREES + (threadIdx.x >> 4);
    if (tree >= P.B) return;
    float* row = reanalyse_row(P, ra, tree);
    RootLane h;
    const RootTotals rt = row_targets16(P, tree, sub, row + ra.S_obs, h);
    if (sub != 0) return;
    row[ra.S_obs + 3 * P.res_Kmax] = (float)rt.v_target;
    if (ra.tr_value) ra.tr_value[(size_t)reanalyse_slot(ra, tree) * P.B + tree] = rt.v_target;
}
__global__ __launch_bounds__(SPW_THREADS) void reanalyse_kernel(KParams P, Reanalyse ra) {
    const int tree = blockIdx.x * blockDim.x + threadIdx.x;
    if (tree >= P.B) return;
    float* row = reanalyse_row(P, ra, tree);
    const RootEdges re(P, tree);
    int amax = 0;
    const double v_target = row_targets(P, re, row + ra.S_obs, &amax);
    row[ra.S_obs + 3 * P.res_Kmax] = (float)v_target;
    if (ra.tr_value) ra.tr_value[(size_t)reanalyse_slot(ra, tree) * P.B + tree] = v_target;
}

// ------------------------------------------------------------------------------------------------ n-step return targets

// The V_target column of every stored row from the kept transitions (azg_selfplay_nstep_targets, include/azgym_nstep.h states the
// rule).  One thread per stored row: thread pos * B + tree takes the row at chronological position pos of game column `tree`, so
// consecutive lanes are consecutive trees of one slot and every load of the [slot][tree] arrays is coalesced.  Position p lies in
// ring slot (oldest + p) mod size.  A streaming pass: a forward scan of at most n_step end kinds, a backward fold over as many
// rewards, one store.
struct NStep {
    int B, T;                 // games; games per net
    int size, oldest;         // stored steps; the ring slot of the oldest one
    int n_step;               // (the host clamps it to size: a longer window cannot reach further)
    int row_len, vcol;        // a row's length and its V_target column
    double gamma;             // where nets is NULL
    const NetSearchRec* nets; // AZG_NSTEP_SEARCH_GAMMA with a per-net table: net tree / T discounts with its own gamma
    const double* reward; const double* value; const int* end;   // [capacity_steps][B]
    float* rows;              // the replay ring [capacity_steps][B][row_len]
};
#define NS_THREADS 256
__global__ __launch_bounds__(NS_THREADS) void nstep_targets_kernel(NStep ns) {
    const long long idx = (long long)blockIdx.x * NS_THREADS + threadIdx.x;
    if (idx >= (long long)ns.size * ns.B) return;
    const int s = (int)(idx / ns.B), tree = (int)(idx - (long long)s * ns.B);
    const double gamma = ns.nets ? ns.nets[tree / ns.T].gamma : ns.gamma;
    const int last = ns.size - 1;
    // element (position p, tree) of a [slot][tree] array (p <= last: the sum stays below 2 * size)
    auto at = [&](int p) { int slot = ns.oldest + p; if (slot >= ns.size) slot -= ns.size; return (size_t)slot * ns.B + tree; };
    // the window's far end: the first step in s .. s + n_step - 1 that ended its episode, else L = min(s + n_step, last)
    int L = s + ns.n_step < last ? s + ns.n_step : last;
    const int hi = s + ns.n_step - 1 < last ? s + ns.n_step - 1 : last;
    bool terminal = false;
    for (int i = s; i <= hi; ++i) {
        const int end = ns.end[at(i)];
        if (end != AZG_END_NONE) { L = i; terminal = end == AZG_END_TERMINAL; break; }
    }
    // terminal: rewards s .. L and nothing beyond; else rewards s .. L - 1 and L's search value
    double acc = 0.0;
    int i = L;
    if (!terminal) { acc = ns.value[at(L)]; i = L - 1; }
    for (; i >= s; --i) acc = ns.reward[at(i)] + gamma * acc;
    ns.rows[at(s) * (size_t)ns.row_len + ns.vcol] = (float)acc;
}

// ------------------------------------------------------------------------------------------------ lambda-return targets

// The same column by a rule per net (azg_selfplay_lambda_targets / _nets, include/azgym_lambda.h states the rule): net tree / T mixes
// the returns of the windows 1 .. n_step with its own lambda and discounts with its own gamma.  The host resolves every net's rule
// into one record of the table below (n_step clamped to the ring's size, gamma the search's where the flag asks for it, om = 1 - lambda).
// One thread per stored row in nstep_targets_kernel's order, its scan for the window's far end, and its fold with one more load per
// step: the kept value of the step after the one whose reward is added.
struct LambdaTargets {
    int B, T;                 // games; games per net
    int size, oldest;         // stored steps; the ring slot of the oldest one
    int row_len, vcol;        // a row's length and its V_target column
    const ReturnRuleRec* rules;   // [n_nets] (replay_ring.h)
    const double* reward; const double* value; const int* end;   // [capacity_steps][B]
    float* rows;              // the replay ring [capacity_steps][B][row_len]
};
__global__ __launch_bounds__(NS_THREADS) void lambda_targets_kernel(LambdaTargets lt) {
    const long long idx = (long long)blockIdx.x * NS_THREADS + threadIdx.x;
    if (idx >= (long long)lt.size * lt.B) return;
    const int s = (int)(idx / lt.B), tree = (int)(idx - (long long)s * lt.B);
    const ReturnRuleRec rule = lt.rules[tree / lt.T];
    const int last = lt.size - 1;
    // element (position p, tree) of a [slot][tree] array (p <= last: the sum stays below 2 * size)
    auto at = [&](int p) { int slot = lt.oldest + p; if (slot >= lt.size) slot -= lt.size; return (size_t)slot * lt.B + tree; };
    // the window's far end: the first step in s .. s + n_step - 1 that ended its episode, else L = min(s + n_step, last)
    int L = s + rule.n_step < last ? s + rule.n_step : last;
    const int hi = s + rule.n_step - 1 < last ? s + rule.n_step - 1 : last;
    bool terminal = false;
    for (int i = s; i <= hi; ++i) {
        const int end = lt.end[at(i)];
        if (end != AZG_END_NONE) { L = i; terminal = end == AZG_END_TERMINAL; break; }
    }
    double acc = 0.0;
    int i = L;
    if (!terminal) { acc = lt.value[at(L)]; i = L - 1; }
    // the first fold: the plain bootstrap from L's search value, or the terminal step's reward alone
    if (i >= s) { acc = lt.reward[at(i)] + rule.gamma * acc; --i; }
    // every nearer step mixes the search value of the step after it into what comes back from beyond
    for (; i >= s; --i) {
        const double mix = rule.om * lt.value[at(i + 1)] + rule.lambda * acc;
        acc = lt.reward[at(i)] + rule.gamma * mix;
    }
    lt.rows[at(s) * (size_t)lt.row_len + lt.vcol] = (float)acc;
}

// ------------------------------------------------------------------------------------------------ search rollouts

// Whole evaluation episodes under MCTS (azg_search_rollout, include/azgym_search_rollout.h): every game plays E episodes, each step
// an ordinary search from the call's own roots followed by one of the step kernels below -- the self-play step without a replay row.
// Tree t = k*T + j starts its i-th episode from the reset state of global game game_id_base + j, episode episode + i; the draws stay
// keyed by tree_base + t.
struct SearchRollout {
    int max_len, E, T;            // episode length limit, episodes per game, games per net
    unsigned game_id_base, episode;
    ActRule rule;
    int* t; int* ep;              // [B] steps into the running episode, episodes finished (E: the game is parked)
    double* ret;                  // [B] the running episode's return
    double* returns; int* lengths; int* terminated;   // [B][E]
    double* roots; int* carry;    // the searches' roots [B][S] and carried counts [B]
    int* unfinished;              // games that have not finished their E-th episode
};

#define SR_THREADS 256
__global__ __launch_bounds__(SR_THREADS) void search_rollout_init_kernel(KParams P, SearchRollout sr) {
    const int tree = blockIdx.x * blockDim.x + threadIdx.x;
    if (tree == 0) *sr.unfinished = P.B;
    if (tree >= P.B) return;
    double ns[4] = {0.0, 0.0, 0.0, 0.0};
    azg_reset_state(P.seed, sr.game_id_base + (unsigned)(tree % sr.T), sr.episode, azg_reset_kind(P.env_id), ns);
    for (int k = 0; k < P.S; ++k) sr.roots[(size_t)tree * P.S + k] = ns[k];
    sr.carry[tree] = 0;
    sr.t[tree] = 0;
    sr.ep[tree] = 0;
    sr.ret[tree] = 0.0;
    for (int i = 0; i < sr.E; ++i) {
        sr.returns[(size_t)tree * sr.E + i] = 0.0;
        sr.lengths[(size_t)tree * sr.E + i] = 0;
        sr.terminated[(size_t)tree * sr.E + i] = 0;
    }
}

// What follows the pick, for one game by its one writer: the real env step with the picked action, the episode's books, its outputs at
// its end and the next search's root.  carry: as selfplay_finish.  A parked game (E episodes finished) is left as it is.
__device__ __forceinline__ void search_rollout_finish(const KParams& P, const SearchRollout& sr, int tree, float action, int carry) {
    int ep = sr.ep[tree];
    if (ep >= sr.E) return;
    const int S = P.S;
    double root[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < S; ++k) root[k] = sr.roots[(size_t)tree * S + k];
    float obs[8];
    double sn;
    game_obs(P.env_id, root, obs, &sn);
    double ns[4] = {0.0, 0.0, 0.0, 0.0}, r;
    int done;
    game_step(P.env_id, root, sn, action, ns, &r, &done);
    double ret = sr.ret[tree] + r;
    int t = sr.t[tree] + 1;
    if (done || t >= sr.max_len) {
        const size_t o = (size_t)tree * sr.E + ep;
        sr.returns[o] = ret;
        sr.lengths[o] = t;
        sr.terminated[o] = done ? 1 : 0;
        ret = 0.0;
        t = 0;
        ep += 1;
        sr.ep[tree] = ep;
        // (after the E-th episode: the root the game is parked on)
        azg_reset_state(P.seed, sr.game_id_base + (unsigned)(tree % sr.T), sr.episode + (unsigned)ep, azg_reset_kind(P.env_id), ns);
        carry = 0;
        if (ep == sr.E) atomicSub(sr.unfinished, 1);
    }
    sr.carry[tree] = carry;
    sr.ret[tree] = ret;
    sr.t[tree] = t;
    for (int k = 0; k < S; ++k) sr.roots[(size_t)tree * S + k] = ns[k];
}

// The two self-play kernels without the row: totals, pick (final_pick16 / final_pick) and search_rollout_finish.
__global__ __launch_bounds__(16 * SP_TREES) void search_rollout_kernel16(KParams P, SearchRollout sr) {
    const int sub = threadIdx.x & 15;
    const int tree = blockIdx.x * SP_TREES + (threadIdx.x >> 4);
    if (tree >= P.B) return;
    RootLane h;
    const RootTotals rt = root_totals16(P, tree, sub, h, false);
    const int pick = final_pick16(P, sr.rule, (unsigned)(P.tree_base + tree), rt, h);
    const float pact = __shfl(h.act, pick, 16);
    const int pnode_n = __shfl(h.node_n, pick, 16);   // (0 where the picked edge has no child node yet)
    if (sub != 0) return;
    search_rollout_finish(P, sr, tree, pact, P.mode == AZG_MODE_CONTINUOUS ? 0 : pnode_n);
}
__global__ __launch_bounds__(SPW_THREADS) void search_rollout_kernel(KParams P, SearchRollout sr) {
    const int tree = blockIdx.x * blockDim.x + threadIdx.x;
    if (tree >= P.B) return;
    const RootEdges re(P, tree);
    int amax = 0;
    (void)root_totals(P, re, &amax, false);
    const int pick = final_pick(P, sr.rule, (unsigned)(P.tree_base + tree), re, amax);
    search_rollout_finish(P, sr, tree, re.act(pick), 0);
}
