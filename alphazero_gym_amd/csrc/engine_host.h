// engine_host.h -- the engine object behind the C ABI, the helpers its translation units share, the host-side rules every kernel form
// shares, and the entry points of the kernel translation units.  The C ABI: azg_engine.hip (creation, roots, search, results, dump,
// info), engine_weights.hip (weight re-layout, populations), engine_selfplay.hip (device self-play on the engine's one ReplayRing,
// replay_ring.h; search rollouts; the results kernel's launch), engine_selftest.hip (probes), dispatch_rollout.hip (policy rollouts, with
// their kernel), dispatch_population_eval.hip (a population's batched inference, with its kernel).  The search kernels are compiled in
// several translation units (dispatch_*.hip: one family of template instantiations each) so that the library builds in parallel.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "hip_host.h"
#include "records.h"
#include "replay_ring.h"
#include "../../include/azgym_population.h"
#include "../../include/azgym_target.h"

// diagnostic switches (environment variables, read once when the engine is created): force the other code paths in tests
struct EngineOptions {
    int force_persistent = 0;      // AZG_FORCE_PERSISTENT=1: wide networks on the one-launch kernel instead of the lock-step path
    int force_stream_weights = 0;  // AZG_FORCE_STREAM_WEIGHTS=1: hidden->hidden weights streamed from L2 instead of register-resident
    int force_global_tree = 0;     // AZG_FORCE_GLOBAL_TREE=1: trees in global memory instead of LDS
    int waves = 0;                 // AZG_WAVES=4|8 (0: automatic)
    int groups = 0;                // AZG_GROUPS=1|2 (0: automatic)
    int trace_cap = 0;             // AZG_TRACE_CAP=n: traces a discrete tree may run per simulation step (0: automatic)
    int no_spec = 0;               // AZG_NO_SPEC=1: the general kernels where a compile-time specialised one exists (dispatch.cuh)
    int tile_trees = 0;            // AZG_TILE_TREES=16|8: trees per 16-column MFMA tile of the small-network kernels (0: automatic)
    int ls_team = 1;               // AZG_LS_TEAM=0: the per-layer launches instead of the persistent team kernel (team.cuh)
    int team_wide = 1;             // AZG_TEAM_WIDE=0: only the first form of the team kernel, 32-tree teams at two workgroups per CU (batches beyond that
                                   // then take the per-layer launches)
    int team_tt = 0;               // AZG_TEAM_TT=32 / 64: only teams of that many trees (default 0: 32, and 64 for batches beyond two 32-tree workgroups per CU)
    long team_spin_limit = 1L << 23;   // AZG_TEAM_SPIN_LIMIT=n: polls a team hand-off may wait before the launch gives up (tests: 0)
    int no_lds_state = 0;          // AZG_NO_LDS_STATE set: discrete LDS trees keep the expanded nodes' env states in the cold records only
    int publish_always = 0;        // AZG_PUBLISH_TREES=1: every search writes its LDS trees out in the global format (diagnostic tools)
    int rollout_teams = 0;         // AZG_ROLLOUT_TEAMS=n: at most n teams per launch of the team rollout (tests: several launches; 0: all that fit)
    int eval_groups = 0;           // AZG_EVAL_GROUPS=g: workgroups per net of azg_population_mlp_eval, instead of its own cap (tests; 0: automatic)
    static EngineOptions from_env();   // (azg_engine.hip)
};
#define AZG_MAX_DEVICES 64    // per-device caches of kernel attributes (host side)

// What the last search ran as: azg_search_resident resets it, the launch fills it in, kernel_name / azg_search_info read it
struct LaunchRecord {
    int form = AZG_FORM_NONE;                 // AZG_FORM_*: search_kernel, lock-step launches, team kernel
    int tree_lds = TS_GLOBAL, spec = 0;       // the kernel's tree storage (TS_*, records.h) and SPEC argument
    int lds_exit = AZG_LDS_NOT_APPLICABLE;    // AZG_LDS_*: why search_kernel's trees were not LDS-resident (azg_tree_storage)
    int waves = 0, groups = 0, tile_trees = 0;   // search_kernel: waves / tree groups per workgroup, trees per group (16, or 8 / 4)
    int team_kc = 0, team_minb = 0, team_tt = 0, team_parts = 0;   // team kernel: chunk length, workgroups per CU, trees per team, launches
    int team_pop = 0;                         // ... and its population instantiation (team.cuh: POP)
    int nets = 0;                             // the launch took the per-net settings table (azg_set_net_search): search_kernel_nets,
                                              // ls_team_kernel_nets, ls_tree_kernel_nets
    int timed = 0;                            // the launch recorded ev0 / ev1 itself (hipExtLaunchKernelGGL)
};

// Where every element of the engine's weight buffer comes from, for one network shape (engine_weights.hip: build_weight_map)
struct WeightMap {
    bool valid = false;
    azg_mlp_desc desc;
    int HP = 0;
    std::vector<unsigned> src;   // per output float: 1 + index into the caller's blob, 0 = padding zero
    size_t oW0, oW0b, ob0, oW0u, ob0u, oWl[MAX_STREAM_LAYERS], obl[MAX_STREAM_LAYERS], oWh, obh, olg[MAX_STREAM_LAYERS], olb[MAX_STREAM_LAYERS];
};

// The weight set that is not in use (include/azgym_target.h): the engine's d_wblob, w_floats, net_have and mlp_ready of that set
struct IdleWeights {
    DeviceAllocs mem;
    float* blob = nullptr;
    size_t floats = 0;
    std::vector<char> have;
    int ready = 0;
    void drop() { mem.clear(); blob = nullptr; floats = 0; have.clear(); ready = 0; }   // (its owner's device current, no reader in flight)
};

// return_results' five arrays in ONE device block (float64 parts first) with a pinned host mirror: byte offsets for B trees of at most K
// root children.  Every array ends where the next one begins.
struct ResultsLayout {
    size_t Q = 0, vt = 0, actions = 0, counts = 0, nch = 0, bytes = 0;
    ResultsLayout() = default;
    ResultsLayout(size_t B, size_t K) : vt(B * K * 8), actions(vt + B * 8), counts(actions + B * K * 4), nch(counts + B * K * 4), bytes(nch + B * 4) {}
};

// The engine's stream and the events around a search.  A base of azg_engine: destroyed after every member, that is after the memory.
struct EngineQueue {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~EngineQueue() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// (deleted by azg_engine_destroy with its device current and its stream idle)
struct azg_engine : EngineQueue {
    azg_config cfg{};
    EngineOptions opt;
    int carry_max = 0;       // largest carried root visit count of the uploaded roots
    int S_env = 0, S_obs = 0, Kmax = 0, Kp = 0, R = 0, nd = 0, tab_n = 0;
    int mlp_ready = 0, HP = 0, n_hidden = 0, nreg = 0;
    int n_cus = 256;         // compute units of the device
    LaunchRecord last;       // what the last search ran as
    KParams P{};
    DeviceAllocs mem;                // everything allocated once at creation
    DeviceAllocs wblob_mem; float* d_wblob = nullptr;   // every re-laid-out weight tensor of the current network in one buffer (reused while the shape stays)
    size_t w_floats = 0;
    std::vector<float> w_stage;      // host staging of that buffer
    WeightMap wmap;                  // the re-layout as an index map, rebuilt when the network shape changes
    DeviceAllocs wmap_mem; unsigned* d_wmap = nullptr;   // its device copy (azg_set_weights_device)
    DeviceAllocs dist_mem;           // continuous mode: per-node mixture cache + root distribution staging, sized by the head
    int dist_nd = -1, dist_ncomp = -1;
    // results staging
    float* d_actions = nullptr; int* d_counts = nullptr; double* d_Q = nullptr; double* d_vt = nullptr; int* d_nch = nullptr;
    int* d_child_n = nullptr; double* d_child_state = nullptr; float* d_rootV = nullptr; float* d_rootdist = nullptr;
    ResultsLayout res;                                // d_Q | d_vt | d_actions | d_counts | d_nch in one block
    char* d_res_block = nullptr; PinnedBlock h_res;   // ... and its pinned host mirror
    double* d_roots = nullptr; int* d_carry = nullptr;
    uint32_t search_idx = 0;
    ReplayRing ring;                 // device self-play: the replay ring, its books, game settings and kept columns (replay_ring.h)
    DeviceBuffer sp_order_buf;       // azg_selfplay_sample_rows: the drawn row numbers [n_nets][n_order] (grow-only)
    DeviceBuffer sr_buf, sr_ctab;    // azg_search_rollout: its roots, carried counts, books and outputs in one block; its (c / m)^temperature table (grow-only)
    unsigned* d_team_cnt = nullptr; size_t team_cnt_bytes = 0;   // team kernel: hand-off counters + abort word
    int team_pending = 0;    // a team kernel has been launched since its abort word was last read
    int team_fallbacks = 0;  // searches it gave up on (redone by the per-layer launches)
    uint32_t team_search_idx = 0;
    int lds_warned = 0;      // the one stderr line about it has been printed
    LockStep ls{};           // lock-step path for wide networks (lockstep.cuh)
    DeviceAllocs ls_mem;
    int ls_hp = 0;
    DeviceAllocs eval_mem; float* d_eval = nullptr; size_t eval_floats = 0;   // scratch of azg_mlp_eval (grow-only)
    DeviceAllocs peval_mem; float* d_peval = nullptr; size_t peval_floats = 0;   // scratch of azg_population_mlp_eval (grow-only)
    DeviceAllocs rollout_mem; char* d_rollout = nullptr; size_t rollout_bytes = 0;   // outputs of azg_policy_rollout (grow-only)
    std::vector<char> rollout_stage;                                                  // ... and their host copy
    // team rollouts (rollout_team.cuh) own their hand-off memory, grow-only: activations and head partials (ro_ls.act / parts, sized in
    // team x width units), live-game counts and counters + abort word (sized in teams).  Nothing of the search's (ls, d_team_cnt) is used.
    DeviceAllocs ro_team_mem; LockStep ro_ls{}; float* d_ro_live = nullptr; unsigned* d_ro_cnt = nullptr;
    size_t ro_team_units = 0; int ro_team_cap = 0;
    int ro_team_off = 0;        // a team rollout of this engine gave up: its rollouts take the group form from then on (opt.ls_team is the search's)
    int ro_team_fallbacks = 0;  // team rollouts that gave up and were replayed in the group form
    int searched = 0, results_valid = 0;
    int publish_once = 0;    // set by azg_dump_tree around its re-run of the last search
    int published = 0;       // the last search's trees are in global memory (global-tree / lock-step / team forms always are)
    int redo_ok = 0;         // roots, carried counts and weights are still the ones the last search ran on: azg_dump_tree may re-run it
    int n_nets = 1;          // azg_set_population: the trees split into n_nets nets of n_trees / n_nets trees (1: one network)
    std::vector<char> net_have = std::vector<char>(1, 0);   // net k has weights (azg_set_net_weights); d_wblob holds n_nets blocks of w_floats
    // include/azgym_target.h: which of the two weight sets d_wblob / w_floats / net_have / mlp_ready describe (AZG_WEIGHTS_*), and the
    // other one, parked; both follow wmap.  Nothing is allocated for the parked set until an upload writes it while it is in use
    int w_in_use = 0;
    IdleWeights w_idle;
    // azg_set_net_search: per-net MCTS settings.  net_search.rec != nullptr: the engine carries a table and searches with the kernels that
    // take it.  net_search_wide: the table came with AZG_NET_SEARCH_WIDE (azg_set_net_search_ex) and may be searched at widths >= 512
    DeviceAllocs net_search_mem; NetSearchTable net_search{};
    int net_search_wide = 0;
    int net_sims_max = 0;    // the table's largest per-net simulation budget (azg_net_search::n_sims): the per-layer launches' step count
    std::vector<double> net_search_gamma;   // the table's gammas [n_nets] on the host (the lambda-return rules resolve theirs from it); empty: no table
    DeviceAllocs stamp_mem; size_t stamp_n = 0;   // rows of the diagnostic stamp buffer (P.stamps)
    uint32_t last_search_idx = 0;   // the search index the last search ran under (azg_dump_tree re-runs it with this one)
    float ms_kept = 0.0f; int ms_kept_valid = 0;   // kernel time of the last search, kept across azg_dump_tree's re-run of it
    std::string err;
};

// ---- shared by the engine's translation units (engine-bound; DeviceScope and the memory owners: hip_host.h)

// records msg as e's last error (e NULL: as the creation error) and returns code (azg_engine.hip)
int fail(azg_engine* e, int code, const std::string& msg);

#define HIPCHK(e, call)                                                                                  \
    do {                                                                                                 \
        hipError_t _rc = (call);                                                                         \
        if (_rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(_rc)); \
    } while (0)
#define ON_DEVICE(e)                                     \
    DeviceScope _scope((e)->cfg.device_id);              \
    if (!_scope.ok) return fail(e, AZG_E_DEVICE, "hipSetDevice failed")
#define D2H(dst, src, bytes) do { if (dst) HIPCHK(e, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); } while (0)

template <typename T>
static int dalloc(azg_engine* e, DeviceAllocs& mem, T** p, size_t n) {
    if ((*p = mem.alloc<T>(n))) return AZG_OK;
    return fail(e, AZG_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(mem.last));
}

// An abandoned team search (team_pending) is redone before anything reads its trees or changes its inputs: synchronises the stream
// and re-runs the search where the team kernel gave up; nothing, and no synchronisation, when no team kernel is pending (azg_engine.hip)
int settle_team(azg_engine* e);
// What azg_search_resident refuses before it launches anything: weights not set, a settings table on wide nets without the wide flag
// (azg_engine.hip)
int search_refusal(azg_engine* e);
// return_results of the last search on e->stream where the search kernel did not write them itself (engine_selfplay.hip)
int launch_results(azg_engine* e);

// Rows (16 counters each) of the diagnostic stamp buffer: one per wave of the search kernel -- four waves per 4 trees at the least
// filled tile shape, eight waves per 16-tree workgroup (also when the batch has fewer than 16 trees) -- or eight counters per
// team-kernel workgroup (16 workgroups per 32 trees, at least one team).
static inline size_t stamp_rows(size_t B) {
    size_t r = ((B + 3) / 4) * 4;
    const size_t r8 = ((B + 15) / 16) * 8, team = ((B + 31) / 32) * 16 * 3 / 2;   // (team kernel: 8 + 16 counters per workgroup)
    if (r8 > r) r = r8;
    if (team > r) r = team;
    return r < 16 ? 16 : r;
}

// Trees the persistent kernel's grid covers with tpw trees per workgroup: every net's segment padded to whole workgroups (one net: the
// batch rounded up to tpw).  The launch planning (dispatch.cuh) sizes the grid and picks its shapes from this count.
static inline long azg_padded_trees(const azg_engine* e, int tpw) {
    const long T = e->cfg.n_trees / e->n_nets;
    return (long)e->n_nets * ((T + tpw - 1) / tpw * tpw);
}

// Progressive widening (NodeContinuous.check_pw, states.py:271-273: python float pow + math.ceil, evaluated on the host with libm): the
// children a node with n visits is entitled to, n = 0 .. n_sims + 1, into pw; returns the largest entitlement a search reaches (Kmax).
// (Entry n does not depend on n_sims: a table built for a smaller budget is a prefix of one built for a larger.)
static inline int azg_pw_table(double c_pw, double kappa, int n_sims, std::vector<int>& pw) {
    pw.assign((size_t)n_sims + 2, 0);
    int kmax = 1;
    for (int n = 0; n < n_sims + 2; ++n) {
        double v = std::ceil(c_pw * std::pow((double)(n + 1), kappa));
        if (v > 1e6) v = 1e6;
        pw[n] = (int)v;
        if (n < n_sims && pw[n] > kmax) kmax = pw[n];
    }
    return kmax;
}
// azg_engine_create's rule for the widening parameters (continuous mode)
static inline bool azg_pw_params_ok(double c_pw, double kappa) { return c_pw > 0.0 && c_pw < 1e6 && kappa >= 0.0 && kappa <= 8.0; }

// Lock-step shaped: a network an unforced engine searches on the team / per-layer path (padded width HP >= 512, at least two hidden
// layers, no LayerNorm, at most four inputs -- those kernels' first layer takes one k-step).  Every other wide network runs on the
// one-launch search kernel.  A population of lock-step shaped nets needs a multiple of 32 trees per net (engine_weights.hip): every
// 32-tree team, and every tile pair of the per-layer kernels, then belongs to exactly one net (lockstep.cuh: ls_net_wofs).
static inline bool azg_lockstep_shaped(int HP, int n_hidden, bool layernorm, int in_dim) {
    return HP >= 512 && n_hidden >= 2 && !layernorm && in_dim <= 4;
}

// The kernels' environment family, their ENV template argument (env.cuh: EnvFamily): 0 CartPole / MountainCar, 5 Acrobot,
// 4 MountainCarContinuous, 2 both Pendulum versions
static inline int azg_kernel_env(const azg_config& c) {
    if (c.mode == AZG_MODE_DISCRETE) return c.env_id == AZG_ENV_ACROBOT ? AZG_ENV_ACROBOT : AZG_ENV_CARTPOLE;
    return c.env_id == AZG_ENV_MOUNTAINCAR_CONT ? AZG_ENV_MOUNTAINCAR_CONT : AZG_ENV_PENDULUM_V1;
}

// Where a search's trees live, and why not in LDS.  LDS trees: <= 16 children per node; 8-bit ids / 16-bit counts up to 255 records,
// 9-bit ids / 11-bit counts up to 511 (the root's count is the largest: carried + n_sims).  lds9: the form has 9-bit-id kernels.
// (Whether the workgroup's LDS plan fits the CU's 160 KB, AZG_LDS_EXIT_SIZE, is found out by the launch.)
struct TreeStorage { int ts, lds_exit; };
static inline TreeStorage azg_tree_storage(const azg_engine* e, bool lds9) {
    const long nmax = (long)e->carry_max + e->cfg.n_sims + 2;
    if (e->opt.force_global_tree) return {TS_GLOBAL, AZG_LDS_EXIT_FORCED};
    if (e->Kp != 16) return {TS_GLOBAL, AZG_LDS_EXIT_CHILDREN};
    if (e->R <= 255) return nmax < 65536 ? TreeStorage{TS_LDS8, AZG_LDS_RESIDENT} : TreeStorage{TS_GLOBAL, AZG_LDS_EXIT_COUNTS};
    if (e->R > 511 || !lds9) return {TS_GLOBAL, AZG_LDS_EXIT_RECORDS};
    return nmax < 2048 ? TreeStorage{TS_LDS9, AZG_LDS_RESIDENT} : TreeStorage{TS_GLOBAL, AZG_LDS_EXIT_COUNTS};
}

// Host-side attributes of one kernel, a static next to its launch.  Per device (the dynamic-LDS attribute belongs to the device's copy
// of the kernel) and atomic: engines on several devices or host threads may share a kernel.
struct KernelAttrs {
    std::atomic<int> static_lds{-1};
    std::atomic<size_t> dyn_lds[AZG_MAX_DEVICES] = {};   // dynamic LDS last set on the device (0: never)
    std::atomic<int> per_cu[AZG_MAX_DEVICES] = {};       // workgroups per CU at that dynamic LDS (0: not asked)

    hipError_t static_bytes(const void* kern, int* bytes) {
        if ((*bytes = static_lds.load(std::memory_order_relaxed)) >= 0) return hipSuccess;
        hipFuncAttributes fa;
        hipError_t rc = hipFuncGetAttributes(&fa, kern);
        if (rc == hipSuccess) static_lds.store(*bytes = (int)fa.sharedSizeBytes, std::memory_order_relaxed);
        return rc;
    }
    // lets launches on the engine's device take `bytes` of dynamic LDS (hipFuncSetAttribute only when that differs from the last value set)
    hipError_t set_dyn_lds(const azg_engine* e, const void* kern, size_t bytes) {
        std::atomic<size_t>& last = dyn_lds[e->cfg.device_id % AZG_MAX_DEVICES];
        if (last.load(std::memory_order_relaxed) == bytes) return hipSuccess;
        hipError_t rc = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (rc == hipSuccess) last.store(bytes, std::memory_order_relaxed);
        return rc;
    }
    // set_dyn_lds, then the workgroups of `threads` threads that fit a CU with `bytes` of dynamic LDS each
    hipError_t occupancy(const azg_engine* e, const void* kern, int threads, size_t bytes, int* blocks) {
        std::atomic<int>& cached = per_cu[e->cfg.device_id % AZG_MAX_DEVICES];
        *blocks = cached.load(std::memory_order_relaxed);
        if (*blocks > 0 && dyn_lds[e->cfg.device_id % AZG_MAX_DEVICES].load(std::memory_order_relaxed) == bytes) return hipSuccess;
        hipError_t rc = set_dyn_lds(e, kern, bytes);
        if (rc == hipSuccess) rc = hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, kern, threads, bytes);
        if (rc == hipSuccess) cached.store(*blocks, std::memory_order_relaxed);
        return rc;
    }
};

// One search of all trees on e->stream with the kernels of family ENV (azg_kernel_env), by path; defined in the headers named, instantiated
// in the dispatch_*.hip translation units.  hipErrorInvalidValue: no kernel for this width; hipErrorNotReady (team kernel): its workgroups
// cannot all be resident, use the per-layer launches.
template <int ENV, bool WIDE> hipError_t azg_persistent_search(azg_engine* e);   // search_kernel, widths up to 128 / 256 and up (dispatch.cuh)
template <int ENV, bool WIDE> hipError_t azg_persistent_search_nets(azg_engine* e);   // the same as search_kernel_nets (per-net settings, widths up to 256)
template <int ENV> hipError_t azg_lockstep_search(azg_engine* e);   // wide networks: the team kernel, else per-layer launches (ls_dispatch.cuh)
template <int ENV> hipError_t azg_team_search(azg_engine* e);       // (team_dispatch.cuh)
// the three wide paths with the per-net settings table (azg_set_net_search_ex, AZG_NET_SEARCH_WIDE): search_kernel_nets at widths 512 and
// 1024, ls_team_kernel_nets, ls_tree_kernel_nets
template <int ENV> hipError_t azg_persistent_search_nets_wide(azg_engine* e);
template <int ENV> hipError_t azg_lockstep_search_nets(azg_engine* e);
template <int ENV> hipError_t azg_team_search_nets(azg_engine* e);
// the team kernel's forms for more than two 32-tree workgroups per CU (config E's network; team_dispatch.cuh); dry: residency check only
hipError_t azg_team_wide_forms(azg_engine* e, int g_base, int G, bool dry, bool common, bool t32, bool t64);
// policy rollout in the team form (dispatch_rollout_team.hip): every team of the call as one or more launches on e->stream, counted into
// *launches; the counters and the abort word (*abort_word: its device address) are zeroed first.  hipErrorNotReady: not a shape or a
// device the team form can hold resident, nothing was launched -- use the group form.
hipError_t azg_rollout_team(azg_engine* e, const struct Rollout& ro, int* launches, unsigned** abort_word);
// batched network inference of n observations (device pointers) on e->stream (mlp_eval.cuh)
hipError_t azg_dispatch_mlp_eval(azg_engine* e, const float* obs, int n, float* value, float* dist, float* raw);
