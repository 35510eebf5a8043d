// dispatch.cuh -- host-side choice and launch of the persistent search kernel variants (included by the dispatch_*.hip
// translation units, each of which instantiates azg_persistent_search for one family of them).
#pragma once
#include <hip/hip_ext.h>

#include "engine_host.h"
#include "env.cuh"
#include "mlp.cuh"
#include "tree.cuh"
#include "search_kernel.cuh"

// One kernel variant: checks that its LDS plan fits the 160 KB of a CU (static + dynamic), then launches.
// Returns hipErrorInvalidConfiguration (nothing launched) when it does not fit.
// NETS: search_kernel_nets, which takes the engine's table of per-net MCTS settings (azg_set_net_search) as a second argument.
template <bool NETS, int ENV, int HP, int NREG, int TLDS, bool GMM, int NW, int NG, int NT = 16, int SPEC = 0>
static hipError_t launch_g(azg_engine* e) {
    static_assert(!NETS || SPEC == 0, "per-net settings run the general kernels");
    const auto kern_of = [] {
        if constexpr (NETS) return search_kernel_nets<ENV, HP, NREG, TLDS, GMM, NW, NG, NT, SPEC>;
        else return search_kernel<ENV, HP, NREG, TLDS, GMM, NW, NG, NT, SPEC>;
    };
    auto kern = kern_of();
    static KernelAttrs attrs;
    int static_lds = 0;
    hipError_t rc = attrs.static_bytes((const void*)kern, &static_lds);
    if (rc != hipSuccess) return rc;
    // discrete LDS trees: the expanded nodes' env states go to LDS too when the CU has room for them -- and when that does not
    // cost a second resident workgroup: a batch with more workgroups than CUs runs two of them side by side on a CU if their LDS
    // allows it, which is worth far more (CartPole, 8192 trees, 2x128: 0.62 ms per search against 0.94 ms)
    constexpr bool CONT = EnvFamily<ENV>::CONT;
    const LdsLayout with_state = lds_layout(e->tab_n, e->cfg.n_sims, HP, NG, act_buffers(NREG), e->R, CONT, TLDS, 1, NT);
    const LdsLayout without = lds_layout(e->tab_n, e->cfg.n_sims, HP, NG, act_buffers(NREG), e->R, CONT, TLDS, 0, NT);
    const long n_wg = azg_padded_trees(e, NT * NG) / (NT * NG);
    const size_t room = 160 * 1024 - (size_t)static_lds;   // (the CU's LDS left for the dynamic part)
    const bool costs_a_neighbour = n_wg > e->n_cus && 2 * (without.total + static_lds) <= 160 * 1024 && 2 * (with_state.total + static_lds) > 160 * 1024;
    e->P.lds_state = (!CONT && TLDS != TS_GLOBAL && with_state.total <= room && !costs_a_neighbour && !e->opt.no_lds_state) ? 1 : 0;
    const size_t lds = e->P.lds_state ? with_state.total : without.total;
    if (lds > room) return hipErrorInvalidConfiguration;
    rc = attrs.set_dyn_lds(e, (const void*)kern, lds);
    if (rc != hipSuccess) return rc;
    dim3 grid((unsigned)n_wg), block(64 * NW);
    e->P.net_wgs = (int)(n_wg / e->n_nets);   // (every net's segment padded to whole workgroups: search_kernel.cuh)
    LaunchRecord& r = e->last;
    r.form = AZG_FORM_PERSISTENT; r.tree_lds = TLDS; r.spec = SPEC; r.nets = NETS;
    r.waves = NW; r.groups = NG; r.tile_trees = NT;
    // the launch carries its own start / stop events (azg_last_search_ms): stamps of the dispatch packet itself -- event records
    // around it are two more packets in the queue, 7 us per search on a stream of back-to-back searches (measured, config C)
    if constexpr (NETS) hipExtLaunchKernelGGL(kern, grid, block, (unsigned)lds, e->stream, e->ev0, e->ev1, 0, e->P, e->net_search);
    else hipExtLaunchKernelGGL(kern, grid, block, (unsigned)lds, e->stream, e->ev0, e->ev1, 0, e->P);
    r.timed = 1;
    return hipGetLastError();
}

// Kernels specialised at compile time for the common parameter set (tree_phases.cuh: Spec<1> -- no epsilon-greedy selection,
// lowest-index ties, and in the discrete family CartPole's two actions) exist for the shapes the BASELINE configurations and their
// neighbours run on: one register-resident hidden->hidden layer, full tiles, trees in LDS with 8-bit ids.  Everything else, and
// every engine whose parameters differ, runs the general kernels (AZG_NO_SPEC=1 forces them: tests).
// An engine that carries per-net settings (NETS) always runs the general kernels, whatever its shared settings are.
template <bool NETS, int ENV, int HP, int NREG, int TLDS, int NW, int NG, int NT = 16>
static hipError_t launch_t(azg_engine* e) {
    if constexpr (EnvFamily<ENV>::CONT && NW == 4 && NT == 16 && TLDS != TS_LDS9) {   // (mixture heads: LDS trees of up to 255 records, else global)
        if (e->P.ncomp >= 2) return launch_g<NETS, ENV, HP, NREG, TLDS, true, NW, NG>(e);
    }
    if constexpr (!NETS && NREG == 1 && TLDS == TS_LDS8 && NT == 16 && ENV != AZG_ENV_ACROBOT) {
        // (+ Pendulum-v1 in the Pendulum family; + no carried root count beyond the sqrt table in the discrete family)
        const bool common = e->cfg.epsilon == 0.0 && e->cfg.tie_break == AZG_TIE_FIRST &&
                            (ENV != AZG_ENV_PENDULUM_V1 || e->cfg.env_id == AZG_ENV_PENDULUM_V1) &&
                            (ENV != AZG_ENV_CARTPOLE || (e->cfg.env_id == AZG_ENV_CARTPOLE && e->cfg.num_actions == 2 &&
                                                         (long)e->carry_max + e->cfg.n_sims + 2 <= (long)e->tab_n));
        if (common && !e->opt.no_spec) return launch_g<false, ENV, HP, NREG, TLDS, false, NW, NG, NT, 1>(e);
    }
    return launch_g<NETS, ENV, HP, NREG, TLDS, false, NW, NG, NT>(e);
}

// Variant choice.  Trees live in LDS when they fit (8-bit record ids, 16-bit counts, <= 16 children per node, the CU's 160 KB).
// The general shape is the 4-wave / 16-tree workgroup.  2x256 squashed-Normal networks (continuous mode) run with eight waves: while
// every 16-tree group can have a CU of its own, as 16-tree workgroups whose eight waves share the network phase and whose first four
// walk the trees (4 % faster than four waves; with all eight walking it only tied); once a batch has more groups than the device has
// CUs, as 32-tree workgroups: two groups per network phase, the second wave of a SIMD in the other's LDS / memory waits (1.27x at 8192 trees).
// AZG_WAVES=4|8, AZG_GROUPS=1|2 force a shape (tests).
template <bool NETS, int ENV, int HP, int NREG>
static hipError_t launch(azg_engine* e) {
    // Trees of 256 .. 511 records stay in LDS (9-bit ids) for the squashed-Normal / discrete heads of networks up to 256 wide; the
    // mixture head's and the wide networks' kernels exist for 8-bit ids and for global trees only (round 6: 32 instantiations fewer)
    const TreeStorage st = azg_tree_storage(e, HP < 512 && e->P.ncomp < 2);
    const int ts = st.ts;
    e->last.lds_exit = st.lds_exit;
    // (Continuous mode only.  The discrete family's 8-wave shapes were measured slower than its 4-wave ones -- CartPole, 8192 trees,
    // 2x256: 1.03 ms against 0.99 ms per search, and they were the only kernels of the family that spilled registers -- and are gone.)
    if constexpr (HP == 256 && NREG == 1 && EnvFamily<ENV>::CONT) {
        bool two = azg_padded_trees(e, 16) / 16 > e->n_cus;
        if (e->opt.groups == 2) two = true;
        if (e->opt.groups == 1) two = false;
        // eight waves either way (round 4): 32-tree workgroups when the batch has more groups than CUs, else 16-tree workgroups whose
        // eight waves share the network phase while four of them walk the trees (search_kernel.cuh).  AZG_WAVES=4 forces the old shape.
        bool want8 = true;
        if (e->opt.waves == 4) want8 = false;
        if (want8 && ts == TS_LDS8 && e->P.ncomp < 2) {
            hipError_t rc = hipErrorInvalidConfiguration;
            if (two) rc = launch_t<NETS, ENV, HP, NREG, TS_LDS8, 8, 2>(e);
            if (rc == hipErrorInvalidConfiguration) rc = launch_t<NETS, ENV, HP, NREG, TS_LDS8, 8, 1>(e);
            if (rc != hipErrorInvalidConfiguration) return rc;
        }
    }
    // Half-filled tiles (small register-resident networks, LDS trees): batches of at most 8 trees per CU run as 8-tree workgroups
    // (search_kernel.cuh has the measurements: with more trees than that, full tiles win).  AZG_TILE_TREES=16|8 forces a shape (tests).
    if constexpr (HP <= 128 && NREG == 1) {
        if (ts == TS_LDS8 && e->P.ncomp < 2) {
            int nt = azg_padded_trees(e, 8) <= 8L * e->n_cus ? 8 : 16;
            if (e->opt.tile_trees) nt = e->opt.tile_trees;
            if (nt == 8) {
                hipError_t rc = launch_t<NETS, ENV, HP, NREG, TS_LDS8, 4, 1, 8>(e);
                if (rc != hipErrorInvalidConfiguration) return rc;
            }
        }
    }
    if (ts == TS_LDS8) {
        hipError_t rc = launch_t<NETS, ENV, HP, NREG, TS_LDS8, 4, 1>(e);
        if (rc != hipErrorInvalidConfiguration) return rc;
    }
    if constexpr (HP < 512) {
        if (ts == TS_LDS9) {
            hipError_t rc = launch_t<NETS, ENV, HP, NREG, TS_LDS9, 4, 1>(e);
            if (rc != hipErrorInvalidConfiguration) return rc;
        }
    }
    if (ts != TS_GLOBAL) e->last.lds_exit = AZG_LDS_EXIT_SIZE;   // (the LDS variants do not fit the CU's 160 KB)
    return launch_t<NETS, ENV, HP, NREG, TS_GLOBAL, 4, 1>(e);
}

// hidden widths (padded) 512 and 1024: every layer's weights streamed from L2, trees in LDS with 8-bit ids or in global memory
template <bool NETS, int ENV>
static hipError_t wide_launch(azg_engine* e) {
    if (e->HP == 512) return launch<NETS, ENV, 512, 0>(e);
    if (e->HP == 1024) return launch<NETS, ENV, 1024, 0>(e);
    return hipErrorInvalidValue;
}

// hidden widths (padded) 64 and 128, or (WIDE) 256 and up (one or two hidden->hidden layers are kept in registers; deeper trunks
// stream their weights from L2: any depth)
template <bool NETS, int ENV, bool WIDE>
static hipError_t persistent_search(azg_engine* e) {
    const int HP = e->HP, NR = e->nreg;
    if constexpr (!WIDE) {
        if (HP == 64) return NR == 1 ? launch<NETS, ENV, 64, 1>(e) : NR == 2 ? launch<NETS, ENV, 64, 2>(e) : launch<NETS, ENV, 64, 0>(e);
        if (HP == 128) return NR == 1 ? launch<NETS, ENV, 128, 1>(e) : NR == 2 ? launch<NETS, ENV, 128, 2>(e) : launch<NETS, ENV, 128, 0>(e);
    } else {
        if (HP == 256) return NR == 1 ? launch<NETS, ENV, 256, 1>(e) : launch<NETS, ENV, 256, 0>(e);
        // (per-net settings at these widths: azg_persistent_search_nets_wide below, translation units of its own)
        if constexpr (!NETS) return wide_launch<NETS, ENV>(e);
    }
    return hipErrorInvalidValue;
}
template <int ENV, bool WIDE>
hipError_t azg_persistent_search(azg_engine* e) { return persistent_search<false, ENV, WIDE>(e); }
// the same choice of shape with search_kernel_nets (instantiated by the dispatch_nets_*.hip translation units)
template <int ENV, bool WIDE>
hipError_t azg_persistent_search_nets(azg_engine* e) { return persistent_search<true, ENV, WIDE>(e); }
// ... and search_kernel_nets at widths 512 and 1024 (azg_set_net_search_ex with AZG_NET_SEARCH_WIDE): the shapes that are not lock-step
// shaped, and anything under AZG_FORCE_PERSISTENT=1 (instantiated by the dispatch_nets_wide_*.hip translation units)
template <int ENV>
hipError_t azg_persistent_search_nets_wide(azg_engine* e) { return wide_launch<true, ENV>(e); }
