// search_kernel.cuh -- the persistent search kernel: one launch = all n_sims traces of B trees.  A workgroup of NW waves
// owns NG groups of 16 trees (one 16-column MFMA tile each):
//   NW = 4, NG = 1: one wave per SIMD, 4 trees per wave (any network);
//   NW = 8, NG = 1: two waves per SIMD for the network phase, four of the eight walk the trees (4 each): the shape of BASELINE config C;
//   NW = 8, NG = 2: two waves per SIMD, 32 trees = two groups that share every network phase (one barrier per step) and walk together, all
//                   eight waves walking: the second wave of a SIMD fills the other's LDS / memory waits, nothing more -- MFMA and vector
//                   time of a SIMD add up -- (pays off when the batch has more 16-tree groups than the device has CUs).
// NT < 16 ("half-filled tiles"): a group holds only NT = 8 (or 4) trees, the other columns of its MFMA tile carry zeros: more,
// smaller workgroups.  Measured on MI355X (config B's network, ms per search at 2048 / 4096 / 8192 trees): NT = 16: 0.469 / 0.482 /
// 0.626; NT = 8: 0.451 / 0.594 / 1.115; NT = 4: 0.549 / 1.049 / 2.040.  A step of a workgroup takes about as long with 8 trees
// as with 16 (it is a chain of dependent instructions, not a throughput problem), and two workgroups that share a CU slow each
// other down by about 30 %: splitting 4096 trees into 512 half-filled workgroups (two per CU) LOSES 23 % against 256 full ones.
// NT = 8 is used where it does pay: batches of at most 8 trees per CU (one workgroup per CU either way, fewer trees per wave: -4 %).
#pragma once
#include "records.h"
#include "env.cuh"
#include "mlp.cuh"
#include "tree.cuh"
#include "tree_phases.cuh"
#include "results.cuh"
#ifndef AZG_DEFER
#define AZG_DEFER 1   // eight-wave / 16-tree continuous kernels: the new node's bookkeeping behind the barrier, first layer by the non-walking waves (0: A/B builds)
#endif
#ifndef AZG_EARLY_PATH
#define AZG_EARLY_PATH 1      // with AZG_HELPER_POLICY: the backup's path rewards / returns are requested in front of the network phase (0: A/B builds)
#endif
#ifndef AZG_HELPER_POLICY
#define AZG_HELPER_POLICY 1   // the same kernels: a leaf's mu / sigma by a non-walking wave during the tree phases, the walking waves take V only (0: A/B builds)
#endif

// Dynamic LDS layout of a workgroup, shared by the kernel and the host's launch planning
struct LdsLayout {
    size_t act_off;    // activation buffers: nbuf x NG groups x HP*64 bytes
    size_t tree_off;   // (TLDS) per-tree regions
    size_t per_tree;   // bytes per tree: R records of 16 B + child-list pool (continuous) or R priors (discrete) (+ env states)
    size_t state_off;  // offset of a tree's env-state slots inside its region (0: none)
    size_t total;
};
// lds_state (discrete LDS trees): n_sims + 1 slots of 4 doubles per tree for the env states of the expanded nodes
__host__ __device__ inline LdsLayout lds_layout(int tab_n, int n_sims, int HP, int NG, int nbuf, int R, bool cont, int tlds, int lds_state = 0, int NT = 16) {
    LdsLayout L;
    L.act_off = ((size_t)tab_n * 8 + (size_t)(n_sims + 2) * 2 + 15) / 16 * 16;
    L.tree_off = L.act_off + (size_t)nbuf * NG * HP * 64;
    L.per_tree = (size_t)R * 16 + (cont ? (size_t)POOL_UNITS(R) * (tlds == TS_LDS9 ? 8 : 4) : (size_t)R * 4);   // 4 ids per pool unit
    L.per_tree = (L.per_tree + 15) / 16 * 16;
    L.state_off = 0;
    if (lds_state && !cont && tlds != TS_GLOBAL) { L.state_off = L.per_tree; L.per_tree += (size_t)(n_sims + 1) * 32; }
    L.total = L.tree_off + (tlds != TS_GLOBAL ? L.per_tree * NT * NG : 0);
    return L;
}
// activation buffers a kernel variant needs: one when a single register-resident hidden layer reads what layer 0 wrote
__host__ __device__ constexpr int act_buffers(int NREG) { return NREG == 1 ? 1 : 2; }

// SPEC: compile-time knowledge about run-time parameters (tree_phases.cuh: Spec<>; 0 = the general code)
template <int ENV, int HP, int NREG, int TLDS, bool GMM, int NW, int NG, int NT = 16, int SPEC = 0>
__global__ __launch_bounds__(64 * NW, NT < 16 ? 2 : 1) void search_kernel(KParams P) {
    const KParams& PN = P;   // (the body reads the network's tensors through PN: see search_kernel_nets)
#include "search_kernel_body.inc"
}

// Per-net MCTS settings (azg_set_net_search): the same kernel for a population whose nets search with settings of their own.  A
// workgroup belongs to one net (wnet, as in the body); it reads that net's record -- wave-uniform loads: the index comes from the
// workgroup id -- into a copy of the parameter block, points the copy's widening table at the net's own, and runs the body above on
// the copy: the tree phases read c_uct, gamma, epsilon, pw0 and (through s_pw) pw_need from `P` as they always did.  The network
// phase and the weight loads keep reading the kernel argument itself (PN): it indexes the per-layer pointer arrays at run time,
// which would pin a copy of the whole block in scratch memory (728 bytes per lane in every weight-streaming kernel) instead of
// leaving the copy's fields in scalar registers.  SPEC = 0 only: the compile-time specialisations assume one parameter set for the launch.
// The copy's n_sims is the net's own simulation budget: the body bounds its loops and clamps its widening look-ups with P.n_sims and
// takes everything that is layout (lds_layout, the length of s_pw, the state slots, the table stride) from PN.n_sims, the engine's.
// Who waits for whom: every wait of the body is workgroup-wide -- __syncthreads, the first-layer counter s_l0 and the policy mailbox
// s_mb (both in the workgroup's LDS, step numbers the workgroup's own), s_done (counts this workgroup's trees).  A workgroup belongs
// to ONE net, so all of its threads hold the same bound, run the same number of steps and leave together; no workgroup waits for
// another, so nets of different budgets in one grid never meet.
template <int ENV, int HP, int NREG, int TLDS, bool GMM, int NW, int NG, int NT = 16, int SPEC = 0>
__global__ __launch_bounds__(64 * NW, NT < 16 ? 2 : 1) void search_kernel_nets(KParams P0, NetSearchTable nets) {
    static_assert(SPEC == 0, "per-net settings run the general kernels");
    const KParams& PN = P0;
    KParams P = P0;
    {
        const int k = (int)blockIdx.x / P0.net_wgs;   // (< the table's n_nets: the grid has n_nets * net_wgs workgroups)
        const NetSearchRec& r = nets.rec[k];
        P.c_uct = r.c_uct; P.gamma = r.gamma; P.epsilon = r.epsilon;
        P.c_uct_f = r.c_uct_f; P.gamma_f = r.gamma_f; P.pw0 = r.pw0; P.n_sims = r.n_sims;
        P.pw_need = nets.pw_need + (size_t)k * (P0.n_sims + 2);
    }
#include "search_kernel_body.inc"
}
