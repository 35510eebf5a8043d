// team.cuh -- wide networks (hidden width >= 512), the whole search as ONE persistent launch of cooperating workgroups.
//
// The lock-step path (lockstep.cuh) pays five kernel boundaries per simulation step and runs its small, latency-bound tree
// kernel (64 workgroups) while the other 192 CUs wait.  Here the batch is cut into TEAMS: 32 trees (two 16-tree groups) and the
// NU = HP/64 workgroups that compute the 64-unit slices of every layer for exactly those trees.  A team never needs data of
// another team, so nothing in the launch is grid-wide.  Every workgroup of a team also OWNS 32/NU of the team's trees (2 at
// HP = 1024) for the whole search -- resident in its LDS when they fit, like the persistent search kernel's -- and walks them
// with the first lanes of its first wave.  Per simulation step a team goes
//     tree phases + first layer (every workgroup, its own trees)  ->  hidden layer 1 .. n (every workgroup, one tile each)
// and hands activations and head partials from workgroup to workgroup through global memory, one monotonic counter per
// hand-off (arrive = one atomic add per workgroup, wait = one lane polling).
//
// Visibility (MI355X: a CU's vector L1 is never refreshed by other CUs' stores, the XCD L2s are not coherent with each other):
// every handed-off byte is stored AND loaded with sc1 buffer instructions (TileMem<true>: write-through past the L2, loads
// around the L1); an arriving workgroup drains its stores (s_waitcnt vmcnt(0) in every wave), meets at its barrier, then one
// lane adds to the counter; a waiting workgroup polls with an sc1 load from one lane and releases the others through its
// barrier.  Placement (blockIdx % 8 = XCD under round-robin dispatch) is used for speed only: by default a team's slices are
// spread over the XCDs so that each XCD's L2 holds its slices' weights.  (In the other mapping, a team on one XCD, the team
// checks at run time that it really sits on one -- its workgroups' XCC_IDs -- and then keeps its hand-off stores plain: they
// write through the L1 into that XCD's L2, where the team's sc1 loads find them.)
// Deadlock: every workgroup of the grid has to be resident; the host checks the occupancy before choosing this path, and every
// wait is bounded -- on a time-out the launch raises an abort flag, all workgroups leave, and the host falls back.
// The arithmetic is the lock-step path's (ls_tile, tree_phase_a/b): bit-identical results.
//
// Measured at config E (1024 trees, 4x1024, MI355X): 13.3 ms per search against 14.9 ms for the per-layer launches (16.6 ms in
// round 1).  Per step (tools/team_profile.py, 153k cycles = 64 us): the three tiles 104k (two workgroups per CU side by side:
// 94 % of the matrix pipe's rate while they run), hand-off waits 21k (4 per step, across XCDs), tree phases + first layer
// 21k.  The two workgroups of a CU (blocks b and b + 256: tools/team_census.py) belong to different teams; shifting one team
// by half a step (re-measured in round 5 with the weights-direct tile: 12.80 / 12.82 ms with a 30k / 60k-cycle head start against 12.81)
// or gating it on its partner's progress did not pay (two tiles side by side take 35k cycles, one alone 24k:
// running them together is the efficient state), nor did making the first layer inside the first hidden layer's staging
// (+18k cycles per step) or as a team phase of MFMA tiles behind an observation hand-off (same time as the vector-ALU form
// here, one hand-off more).
#pragma once
#include "lockstep.cuh"

#define TEAM_CNT_STRIDE 32      // counters 128 bytes apart
#define TEAM_MAX_CNT 8          // counter 0: first layer of the step written; l: hidden layer l written
#define TEAM_CNT_XA (TEAM_MAX_CNT - 1)   // max XCC_ID of the team's workgroups
#define TEAM_CNT_XB (TEAM_MAX_CNT - 2)   // max (7 - XCC_ID)
#ifndef TEAM_SPREAD
#define TEAM_SPREAD 1           // 1: a team's unit slices spread over the XCDs (weights L2-resident); 0: a team on one XCD
#endif
#ifndef TEAM_SAME_XCD
#define TEAM_SAME_XCD 1         // plain hand-off stores (kept in the XCD's L2) once the team is seen to sit on one XCD
#endif
#ifndef TEAM_DEFER
#define TEAM_DEFER 1            // the new node's bookkeeping behind the workgroup's arrival at the hand-off (0: A/B builds)
#endif
#ifndef TEAM_LDS_COLD
#define TEAM_LDS_COLD 1         // the default form (32-tree teams, two workgroups per CU, trees of <= 255 records): the cold records, returns and actions in LDS
#endif                          // too (the weights-direct tile left the room), written out once at the end of the search
// bytes per tree of that: Cold[R] + edge_W[R] + action[R]
__host__ __device__ inline size_t team_cold_bytes(int R) { return ((size_t)R * (64 + 8 + 4) + 15) / 16 * 16; }
#ifndef TEAM_TILE_DBG
#define TEAM_TILE_DBG 0          // timing experiments only (lockstep.cuh: ls_tile's DBG): wrong results
#endif
#ifndef TEAM_WD
#define TEAM_WD 1                // 1: ls_tile_wd (weights straight into registers, only the activations staged); 0: ls_tile
#endif
#if TEAM_WD
#define LS_TILE_STAGE_F4(KC, TG) (2 * (TG) * (KC) * 64)          // float4 entries of the tile routine's two stages (activations only)
#else
#define LS_TILE_STAGE_F4(KC, TG) (2 * (4 + (TG)) * (KC) * 64)   // float4 entries of the tile routine's two stages (TG tree groups, UT = 4)
#endif

struct TeamCtl {
    unsigned* cnt;         // [teams][TEAM_MAX_CNT][TEAM_CNT_STRIDE]
    unsigned* abort;       // != 0: a wait timed out, everybody leaves
    unsigned spin_limit;   // polls (about 0.15 us each) a wait may take: 1 << 23 is more than a second
};

// dynamic LDS of a team workgroup: the tile stages, sqrt_tab, pw_need, then (LDS trees) the workgroup's trees
__host__ __device__ inline size_t team_tree_bytes(int R, bool cont, int tlds) {
    if (tlds == TS_GLOBAL) return 0;
    size_t per = (size_t)R * 16 + (cont ? (size_t)POOL_UNITS(R) * (tlds == TS_LDS9 ? 8 : 4) : (size_t)R * 4);
    return (per + 15) / 16 * 16;
}
// (the stages double as the head partials' landing area between tiles: NCH * 64 float4, at most 16 * 64)
__host__ __device__ inline size_t team_table_off(int kc, int tg = 2) { size_t f4 = LS_TILE_STAGE_F4(kc, tg); return (f4 < 1024 ? 1024 : f4) * 16; }
__host__ __device__ inline size_t team_tree_off(int tab_n, int n_sims, int kc, int tg = 2) {
    return (team_table_off(kc, tg) + (size_t)tab_n * 8 + (size_t)(n_sims + 2) * 4 + 15) / 16 * 16;
}

// all of this workgroup's hand-off stores are on their way: drain, meet, one lane arrives
__device__ __forceinline__ void team_arrive(unsigned* c) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wait until the counter reaches `target`; false (uniform over the workgroup): aborted
__device__ __forceinline__ bool team_wait(const unsigned* c, unsigned target, const TeamCtl& T, volatile int* s_ok) {
    unsigned* abort = T.abort;
    if (threadIdx.x == 0) {
        int ok = 1;
        unsigned spins = 0;
        if (T.spin_limit == 0u) {   // (tests: every wait counts as timed out)
            __hip_atomic_store(abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = 0;
        } else {
            // (Round 5 measured two polls in flight, half a round trip apart, so that a poll issued just before the counter moves is
            // followed by one that sees it sooner: 13.20 against 13.15 ms per search at 1024 trees, 23.32 against 23.29 at 2048 -- a wait
            // ends when the slowest of the team's workgroups arrives, not when the poll notices; not kept.)
            while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                __builtin_amdgcn_s_sleep(2);
                if ((++spins & 15u) == 0u) {
                    if (spins > T.spin_limit) __hip_atomic_store(abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (__hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { ok = 0; break; }
                }
            }
        }
        *s_ok = ok;
    }
    __syncthreads();
    const bool ok = *s_ok != 0;
    __syncthreads();   // everybody has read the verdict before the next wait overwrites it
    return ok;
}

#ifdef AZG_STAMPS
#define TSTAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define TADD(slot, a, b) tacc[slot] += (b) - (a)
#else
#define TSTAMP(v)
#define TADD(slot, a, b)
#endif

// KC: k-blocks per staged chunk of the tile routine; MINB: workgroups that have to fit a CU side by side (2: the default form,
// 1024 trees at HP = 1024; 3 and 4 (shorter chunks: smaller stages, fewer registers): larger batches -- while one workgroup of a
// CU waits at a hand-off or walks its trees, the others keep the matrix pipe busy).
// SPEC: compile-time knowledge about run-time parameters for the tree phases (tree_phases.cuh: Spec<>; 0 = the general code).
// TT: trees of a team, 32 or 64 (TGN = 2 or 4 tree groups: the tile is TT trees x 64 units; 64 halves the weight bytes staged per
// MFMA and the barriers per MFMA, and needs twice the batch for the same number of workgroups).
// POP: the population form (lockstep.cuh: ls_net_wofs) -- the team's net's weights; 32-tree teams only, so that a team serves one net.
template <int ENV, int HP, bool GMM, int TLDS, int KC = LS_KC, int MINB = 2, int SPEC = 0, int TT = 32, bool POP = false>
__global__ __launch_bounds__(256, MINB) void ls_team_kernel(KParams P, LockStep L, TeamCtl T, int TQ, int g_base) {
#define TEAM_TREE_PARAMS(g0) P   // (the tree phases read the launch's shared settings)
#include "team_kernel_body.inc"
#undef TEAM_TREE_PARAMS
}

// Per-net MCTS settings (lockstep.cuh: ls_net_params): the base population form -- 32-tree teams, two per CU, the general tree phases --
// whose workgroups read their team's net's record once at kernel entry, outside the simulation loop, and walk their trees with it.
// Budgets: the simulation loop and its two `k < n_sims` tests read PT.n_sims, the net's own; team_tree_off and the s_pw fill keep
// P.n_sims, the engine's (layout).  Who waits for whom: team_wait / team_arrive work on the TEAM's counters (cnt: one block per 32
// trees) with targets NU * (k + 1), and a workgroup's barriers are its own.  All NU workgroups of a team derive their net from the
// team's first tree group, read the same record and so run the same k = 0 .. n_sims: each arrives exactly once per hand-off the others
// wait for, and the team leaves together after its own last step.  No wait spans two teams, so a team that has left owes nothing.
template <int ENV, int HP, bool GMM, int TLDS, int KC = LS_KC, int MINB = 2>
__global__ __launch_bounds__(256, MINB) void ls_team_kernel_nets(KParams P, LockStep L, TeamCtl T, int TQ, int g_base, NetSearchTable nets) {
    constexpr int SPEC = 0, TT = 32;
    constexpr bool POP = true;
#define TEAM_TREE_PARAMS(g0) ls_net_params(P, nets, g0)
#include "team_kernel_body.inc"
#undef TEAM_TREE_PARAMS
}
