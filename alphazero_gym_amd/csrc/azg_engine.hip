// azg_engine.hip -- MI355X (gfx950) batched MCTS engine behind the C ABI of include/azgym.h.
//
// One persistent kernel launch runs a whole MCTS search (all n_sims simulations) for B independent trees.
//   * workgroup = 256 threads = 4 waves = one group of 16 trees (= one 16-row MFMA tile of leaf evaluations);
//     a workgroup never talks to another one, so there is no grid-wide synchronisation anywhere.
//   * tree phase: a 16-lane sub-wave owns one tree.  Lanes scan the <=16 children of a node in parallel
//     (PUCT / progressive-widening UCT, float64), arg-max by a 4-step butterfly, step the closed-form
//     environment, expand, and back the return up the path.
//   * network phase: the policy/value MLP for the 16 new leaves on v_mfma_f32_16x16x4_f32.  Activations are
//     kept transposed ([unit][tree]) so that an MFMA's D registers are the next layer's B operand as they
//     stand; hidden->hidden weights can live in the 512-entry VGPR/AGPR file for the whole search (NREG>0).
// Reference semantics: alphazero/search/mcts.py (search 418-462 / 656-702, selectionUCT 464-493 / 704-741,
// backprop 241-267, return_results 269-307), alphazero/search/states.py, alphazero/network/policies.py.
// The arithmetic (operation order, float32/float64 placement) is specified by oracle/azg_oracle.c, which is pinned
// to the reference by tests/golden; this file must agree with it bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine_host.h"
#include "../../include/azg_math.h"

static std::string g_create_err;

int fail(azg_engine* e, int code, const std::string& msg) {
    if (e) e->err = msg; else g_create_err = msg;
    return code;
}

// ---- lock-step path (wide networks): a few grid-wide launches per simulation step
static int ls_prepare(azg_engine* e) {
    if (e->ls_hp == e->HP) return AZG_OK;
    e->ls_mem.clear();
    // tree groups padded to a multiple of 4: the tiled layer kernel works on 4 groups per workgroup
    const size_t B = e->cfg.n_trees, G = ((B + TREES_PER_WG - 1) / TREES_PER_WG + 3) / 4 * 4, HP = e->HP;
    float* obsT; float *a0, *a1, *parts; LsTree* tr; LsLane* ln;
    e->team_cnt_bytes = (((B + 31) / 32) * 8 * 32 + 32) * sizeof(unsigned);   // per team 8 counters 128 B apart, + the abort word
    if (dalloc(e, e->ls_mem, &e->d_team_cnt, e->team_cnt_bytes / 4) ||
        dalloc(e, e->ls_mem, &obsT, G * 64) || dalloc(e, e->ls_mem, &a0, G * HP * 16) || dalloc(e, e->ls_mem, &a1, G * HP * 16) ||
        dalloc(e, e->ls_mem, &parts, G * (HP / 64) * 64 * 4) || dalloc(e, e->ls_mem, &tr, B) ||
        dalloc(e, e->ls_mem, &ln, B * 16))
        return AZG_E_DEVICE;
    e->ls.obsT = obsT; e->ls.act[0] = (f32x4*)a0; e->ls.act[1] = (f32x4*)a1; e->ls.parts = (f32x4*)parts;
    e->ls.tree = tr; e->ls.lane = ln;
    // the padding groups are computed like the others (their columns never mix with real ones): give them defined inputs
    if (hipMemset(obsT, 0, G * 64 * sizeof(float)) != hipSuccess || hipMemset(a0, 0, G * HP * 16 * sizeof(float)) != hipSuccess || hipMemset(a1, 0, G * HP * 16 * sizeof(float)) != hipSuccess) return AZG_E_DEVICE;
    e->ls_hp = e->HP;
    return AZG_OK;
}

static bool use_lockstep(const azg_engine* e) {
    if (e->opt.force_persistent) return false;
    return azg_lockstep_shaped(e->HP, e->n_hidden, e->P.layernorm != 0, e->S_obs);
}

// One search of all trees on e->stream: the kernels of the engine's family (azg_kernel_env) on its path, by network width.
template <int ENV>
static hipError_t search_path(azg_engine* e, bool lockstep) {
    if (lockstep) {
        if constexpr (ENV == AZG_ENV_ACROBOT) return hipErrorInvalidValue;   // (six network inputs: never lock-step, use_lockstep)
        else return e->net_search.rec ? azg_lockstep_search_nets<ENV>(e) : azg_lockstep_search<ENV>(e);
    }
    if (e->net_search.rec)
        return e->HP <= 128 ? azg_persistent_search_nets<ENV, false>(e) : e->HP <= 256 ? azg_persistent_search_nets<ENV, true>(e) : azg_persistent_search_nets_wide<ENV>(e);
    return e->HP <= 128 ? azg_persistent_search<ENV, false>(e) : azg_persistent_search<ENV, true>(e);
}
static hipError_t search_launch(azg_engine* e, bool lockstep) {
    switch (azg_kernel_env(e->cfg)) {
        case AZG_ENV_CARTPOLE: return search_path<AZG_ENV_CARTPOLE>(e, lockstep);
        case AZG_ENV_MOUNTAINCAR_CONT: return search_path<AZG_ENV_MOUNTAINCAR_CONT>(e, lockstep);
        case AZG_ENV_ACROBOT: return search_path<AZG_ENV_ACROBOT>(e, lockstep);
        default: return search_path<AZG_ENV_PENDULUM_V1>(e, lockstep);
    }
}

// The persistent team kernel leaves instead of hanging when one of its waits times out (its workgroups were not all resident,
// e.g. another process holds part of the GPU): it raises a word that is read here, after the stream has been synchronised.
// The search is then run again, with the same search index, as per-layer launches -- which the engine uses from then on.
static int team_check(azg_engine* e) {
    unsigned flag = 0;
    e->team_pending = 0;
    if (hipMemcpy(&flag, e->d_team_cnt + (e->team_cnt_bytes / 4 - 1), 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(e, AZG_E_DEVICE, "reading the team kernel's status failed");
    if (flag) e->opt.ls_team = 0;
    if (flag == 0) return AZG_OK;
    e->team_fallbacks += 1;
    e->search_idx = e->team_search_idx;
    int rc = azg_search_resident(e);
    if (rc) return rc;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(e, AZG_E_DEVICE, "hipStreamSynchronize failed");
    return AZG_OK;
}
int settle_team(azg_engine* e) {
    if (!e->team_pending) return AZG_OK;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return team_check(e);
}

// What azg_search_resident refuses before it launches anything (azg_selfplay_reanalyse asks first, before its own launches)
int search_refusal(azg_engine* e) {
    if (!e->mlp_ready)
        return fail(e, AZG_E_STATE, e->n_nets > 1 ? "azg_set_net_weights has not been called for every net of the population"
                                                 : "azg_set_weights has not been called");
    // a table set through azg_set_net_search is searched at widths up to 256 only; the team kernel, the per-layer launches and the wide
    // networks' one-launch kernels take one that came with AZG_NET_SEARCH_WIDE
    if (e->net_search.rec && e->HP >= 512 && !e->net_search_wide)
        return fail(e, AZG_E_UNSUPPORTED, "per-net search settings (azg_set_net_search) need a padded hidden width of at most 256: nets of width >= 512 "
                                          "search with the engine's shared settings (azg_set_net_search(e, NULL, 0) returns to them), or with a table "
                                          "set through azg_set_net_search_ex with AZG_NET_SEARCH_WIDE");
    return AZG_OK;
}

// Per environment (AZG_ENV_*): float64 words of a state, network inputs, discrete actions (0: a continuous-action env)
struct EnvFacts { int state_words, obs_width, discrete, n_actions; };
static constexpr EnvFacts kEnv[AZG_ENV_ACROBOT + 1] = {
    {4, 4, 1, 2},   // CartPole
    {2, 3, 0, 0},   // Pendulum-v0
    {2, 3, 0, 0},   // Pendulum-v1
    {2, 2, 1, 3},   // MountainCar
    {2, 2, 0, 0},   // MountainCarContinuous
    {4, 6, 1, 3},   // Acrobot
};

// a search cannot start from a terminal state (the Pendulums have none)
static bool root_is_terminal(int env_id, const double* s) {
    switch (env_id) {
        case AZG_ENV_CARTPOLE: {
            const double theta_thr = 12.0 * 2.0 * 3.141592653589793 / 360.0, x_thr = 2.4;
            return (s[0] < -x_thr) || (s[0] > x_thr) || (s[2] < -theta_thr) || (s[2] > theta_thr);
        }
        case AZG_ENV_ACROBOT: return azg_acrobot_terminal(s);
        // (mcts.py:382-383, 599-600; the flag is at 0.5 in MountainCar-v0, at 0.45 in MountainCarContinuous-v0)
        case AZG_ENV_MOUNTAINCAR: return s[0] >= 0.5 && s[1] >= 0.0;
        case AZG_ENV_MOUNTAINCAR_CONT: return s[0] >= 0.45 && s[1] >= 0.0;
        default: return false;
    }
}

// every AZG_* switch of EngineOptions (AZG_QUIET is read where the one warning is printed)
EngineOptions EngineOptions::from_env() {
    const auto digit = [](const char* name, int dflt) {   // a single leading digit
        const char* v = getenv(name);
        return (v && v[0] >= '0' && v[0] <= '9') ? v[0] - '0' : dflt;
    };
    const auto num = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; };
    EngineOptions o;
    o.force_persistent = digit("AZG_FORCE_PERSISTENT", 0) == 1;
    o.force_stream_weights = digit("AZG_FORCE_STREAM_WEIGHTS", 0) == 1;
    o.force_global_tree = digit("AZG_FORCE_GLOBAL_TREE", 0) == 1;
    o.no_spec = digit("AZG_NO_SPEC", 0) == 1;
    o.waves = digit("AZG_WAVES", o.waves);
    o.groups = digit("AZG_GROUPS", o.groups);
    { const int t = num("AZG_TRACE_CAP"); o.trace_cap = t > 0 ? t : 0; }
    { const int t = num("AZG_TILE_TREES"); o.tile_trees = (t == 16 || t == 8) ? t : 0; }
    o.ls_team = digit("AZG_LS_TEAM", o.ls_team);
    o.team_wide = digit("AZG_TEAM_WIDE", o.team_wide);
    o.team_tt = num("AZG_TEAM_TT");
    if (const char* v = getenv("AZG_TEAM_SPIN_LIMIT")) o.team_spin_limit = atol(v);
    o.no_lds_state = getenv("AZG_NO_LDS_STATE") != nullptr;
    o.publish_always = digit("AZG_PUBLISH_TREES", 0) == 1;
    { const int t = num("AZG_ROLLOUT_TEAMS"); o.rollout_teams = t > 0 ? t : 0; }
    { const int t = num("AZG_EVAL_GROUPS"); o.eval_groups = t > 0 ? t : 0; }
    return o;
}

extern "C" {

int azg_abi_version(void) { return AZG_ABI_VERSION; }

const char* azg_last_error(const azg_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

void azg_engine_destroy(azg_engine* e) {
    if (!e) return;
    DeviceScope scope(e->cfg.device_id);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    delete e;   // (its memory, then its events and stream)
}

// Two HIP runtimes in one process (PyTorch-ROCm wheels bundle their own libamdhip64 under the system library's SONAME; whichever is
// loaded first serves every library that comes later -- unless the other one was pulled in by path, as `import torch` does):
// the second one to initialise then finds no GPU or hangs.  Seen from here as two different libamdhip64 files in the process's
// memory map; reported instead of risking either.  Returns the number of distinct files and their paths.
static int mapped_hip_runtimes(std::string& paths) {
    // scanned once per process: the answer can only change by loading yet another runtime behind this library's back, and a process
    // that creates engines in a loop should not re-parse its memory map every time
    static int cached_n = -1;
    static std::string cached_paths;
    if (cached_n >= 0) { paths = cached_paths; return cached_n; }
    std::vector<std::string> seen;
    FILE* f = fopen("/proc/self/maps", "r");
    if (!f) return 0;
    char line[1024];
    while (fgets(line, sizeof line, f)) {
        if (!strstr(line, "libamdhip64")) continue;
        const char* p = strchr(line, '/');
        if (!p) continue;
        std::string path(p);
        while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) path.pop_back();
        bool dup = false;
        for (const auto& q : seen) dup = dup || q == path;
        if (!dup) seen.push_back(path);
    }
    fclose(f);
    paths.clear();
    for (const auto& q : seen) paths += (paths.empty() ? "" : ", ") + q;
    cached_paths = paths;
    cached_n = (int)seen.size();
    return cached_n;
}

// Everything of a new engine that can fail once the object exists (e->cfg is valid): sizes, stream and events, device memory, KParams.
static int engine_build(azg_engine* e) {
    const azg_config* cfg = &e->cfg;
    e->opt = EngineOptions::from_env();
    e->S_env = kEnv[cfg->env_id].state_words;
    e->S_obs = kEnv[cfg->env_id].obs_width;
    const int ns = cfg->n_sims;
    std::vector<int> pw(ns + 2, 0);
    if (cfg->mode == AZG_MODE_CONTINUOUS) {
        e->Kmax = azg_pw_table(cfg->c_pw, cfg->kappa, ns, pw);
        e->R = ns + 2;
        e->nd = 2;
    } else {
        e->Kmax = cfg->num_actions;
        e->R = 1 + cfg->num_actions * (ns + 1);
        e->nd = cfg->num_actions;
    }
    if (e->R > 32767) return fail(e, AZG_E_UNSUPPORTED, "tree too large: records per tree must be < 32768");
    if (cfg->tie_break == AZG_TIE_RANDOM && e->Kmax > 16) return fail(e, AZG_E_UNSUPPORTED, "tie_break random supports at most 16 children per node");
    e->Kp = (e->Kmax + 15) / 16 * 16;
    // sqrt(n+1) table: node visit counts reach n_sims (+ the carried root count in discrete mode; beyond 3 n_sims the kernel
    // computes the root's square root in place)
    e->tab_n = cfg->mode == AZG_MODE_CONTINUOUS ? ns + 2 : 4 * ns + 4;
    ON_DEVICE(e);
    (void)hipDeviceGetAttribute(&e->n_cus, hipDeviceAttributeMultiprocessorCount, cfg->device_id);
    HIPCHK(e, hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIPCHK(e, hipEventCreate(&e->ev0));
    HIPCHK(e, hipEventCreate(&e->ev1));
    KParams& P = e->P;
    const size_t B = (size_t)cfg->n_trees, R = (size_t)e->R, K = (size_t)e->Kmax;
    RecL* hot; Cold* cold; double* edge_W; float* action; float* prior; unsigned short* child; int* n_rec;
    int* d_pw; double* d_sq; unsigned long long* stamps;
    e->res = ResultsLayout(B, K);
    e->stamp_n = stamp_rows(B);   // (diagnostic builds: one row of 16 counters per wave)
    DeviceAllocs& mem = e->mem;
    if (dalloc(e, mem, &hot, B * R) || dalloc(e, mem, &cold, B * R) || dalloc(e, mem, &edge_W, B * R) || dalloc(e, mem, &action, B * R) ||
        dalloc(e, mem, &prior, B * R) || dalloc(e, mem, &child, B * R * e->Kp) || dalloc(e, mem, &n_rec, B) ||
        dalloc(e, mem, &d_pw, (size_t)ns + 2) || dalloc(e, mem, &d_sq, (size_t)e->tab_n) || dalloc(e, mem, &e->d_roots, B * e->S_env) ||
        dalloc(e, mem, &e->d_carry, B) || dalloc(e, mem, &e->d_res_block, e->res.bytes) || dalloc(e, mem, &e->d_child_n, B * K) ||
        dalloc(e, mem, &e->d_child_state, B * K * e->S_env) || dalloc(e, mem, &e->d_rootV, B) || dalloc(e, mem, &e->d_rootdist, B * e->nd) ||
        dalloc(e, e->stamp_mem, &stamps, e->stamp_n * 16))
        return AZG_E_DEVICE;
    // (azg_results is one device-to-host copy of the block into its pinned mirror, not five)
    HIPCHK(e, hipHostMalloc(&e->h_res.p, e->res.bytes, hipHostMallocDefault));
    char* const blk = e->d_res_block;
    e->d_Q = (double*)(blk + e->res.Q); e->d_vt = (double*)(blk + e->res.vt); e->d_actions = (float*)(blk + e->res.actions);
    e->d_counts = (int*)(blk + e->res.counts); e->d_nch = (int*)(blk + e->res.nch);
    std::vector<double> sq(e->tab_n);
    for (int n = 0; n < e->tab_n; ++n) sq[n] = std::sqrt((double)(n + 1));
    HIPCHK(e, hipMemcpy(d_pw, pw.data(), sizeof(int) * (ns + 2), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(d_sq, sq.data(), sizeof(double) * e->tab_n, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemset(hot, 0, B * R * sizeof(RecL)));
    HIPCHK(e, hipMemset(e->d_carry, 0, B * sizeof(int)));
    P.B = cfg->n_trees; P.n_sims = ns; P.R = e->R; P.Kp = e->Kp; P.A = cfg->num_actions; P.nd = e->nd;
    P.trace_cap = e->opt.trace_cap > 0 ? e->opt.trace_cap : 5;   // (config B on MI355X: 0.484 ms with 1, 0.388 with 3, 0.371 with 5 or 6, 0.43 with 8)
    P.tie_random = cfg->tie_break == AZG_TIE_RANDOM; P.env_id = cfg->env_id; P.v1 = cfg->env_id == AZG_ENV_PENDULUM_V1; P.tree_base = cfg->tree_id_base; P.mode = cfg->mode;
    P.c_uct = cfg->c_uct; P.gamma = cfg->gamma; P.epsilon = cfg->epsilon; P.reward_scale = cfg->reward_scale;
    P.c_uct_f = (float)cfg->c_uct; P.gamma_f = (float)cfg->gamma; P.bound_f = (float)cfg->action_bound;
    P.seed = cfg->seed; P.S = e->S_env; P.tab_n = e->tab_n; P.pw0 = cfg->mode == AZG_MODE_CONTINUOUS ? pw[0] : 0;
    P.roots = e->d_roots; P.carry = e->d_carry;
    P.hot = hot; P.cold = cold; P.edge_W = edge_W; P.action = action; P.prior = prior; P.child = child;
    P.n_rec = n_rec; P.pw_need = d_pw; P.sqrt_tab = d_sq; P.stamps = stamps;
    P.res_actions = e->d_actions; P.res_counts = e->d_counts; P.res_Q = e->d_Q; P.res_vt = e->d_vt; P.res_nch = e->d_nch;
    P.res_child_n = e->d_child_n; P.res_child_state = e->d_child_state; P.res_root_V = e->d_rootV; P.res_root_dist = e->d_rootdist;
    P.res_Kmax = e->Kmax; P.res_v_target = cfg->v_target;
    P.net_T = cfg->n_trees; P.net_wgs = 1; P.net_wstride = 0;
    return AZG_OK;
}

int azg_engine_create(const azg_config* cfg, azg_engine** out) {
    if (!cfg || !out) return fail(nullptr, AZG_E_INVALID, "null argument");
    {
        std::string rts;
        const char* allow = getenv("AZG_ALLOW_MULTI_HIP");
        if (mapped_hip_runtimes(rts) > 1 && !(allow && allow[0] == '1'))
            return fail(nullptr, AZG_E_DEVICE, ("two HIP runtimes are mapped in this process (" + rts + "): load PyTorch (import torch) BEFORE "
                                               "libazgym_hip.so so that both use PyTorch's copy; if they are meant to coexist (differing "
                                               "SONAMEs, a deliberate second copy), set AZG_ALLOW_MULTI_HIP=1").c_str());
    }
    if (cfg->struct_size != (int32_t)sizeof(azg_config)) return fail(nullptr, AZG_E_INVALID, "azg_config size mismatch");
    if (cfg->n_trees < 1 || cfg->n_sims < 1) return fail(nullptr, AZG_E_INVALID, "n_trees and n_sims must be >= 1");
    if (cfg->env_id < 0 || cfg->env_id > AZG_ENV_ACROBOT) return fail(nullptr, AZG_E_INVALID, "unknown env_id");
    const bool discrete_env = kEnv[cfg->env_id].discrete;
    if (cfg->mode == AZG_MODE_DISCRETE && !discrete_env)
        return fail(nullptr, AZG_E_UNSUPPORTED, "discrete mode requires a discrete-action env (CartPole, MountainCar, Acrobot)");
    if (cfg->mode == AZG_MODE_CONTINUOUS && discrete_env)
        return fail(nullptr, AZG_E_UNSUPPORTED, "continuous mode requires a continuous-action env (Pendulum, MountainCarContinuous)");
    if (cfg->mode == AZG_MODE_DISCRETE && cfg->num_actions != kEnv[cfg->env_id].n_actions)
        return fail(nullptr, AZG_E_INVALID, "num_actions does not match the env (CartPole 2, MountainCar 3, Acrobot 3)");
    if (cfg->tie_break != AZG_TIE_FIRST && cfg->tie_break != AZG_TIE_RANDOM) return fail(nullptr, AZG_E_INVALID, "unknown tie_break");
    // progressive widening (states.py:271-275): ceil(c_pw (n + 1)^kappa) children; with c_pw <= 0 no node is ever entitled to a child and the
    // reference's first selection takes the arg-max of an empty list (helpers.py:30-52 raises)
    if (cfg->mode == AZG_MODE_CONTINUOUS && !azg_pw_params_ok(cfg->c_pw, cfg->kappa))
        return fail(nullptr, AZG_E_INVALID, "c_pw must be > 0 and kappa >= 0 (progressive widening: ceil(c_pw (n + 1)^kappa) children)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, AZG_E_DEVICE, "no HIP device available");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, AZG_E_DEVICE, "device_id out of range");
    azg_engine* e = new azg_engine();
    e->cfg = *cfg;
    const int rc = engine_build(e);
    if (rc != AZG_OK) {   // the partly built engine goes, its message stays as the creation error
        const std::string msg = e->err;
        azg_engine_destroy(e);
        return fail(nullptr, rc, msg);
    }
    *out = e;
    return AZG_OK;
}

int azg_set_search_index(azg_engine* e, uint32_t idx) { if (!e) return AZG_E_INVALID; e->search_idx = idx; return AZG_OK; }

int azg_upload_roots(azg_engine* e, const double* roots, const int32_t* carry) {
    if (!e || !roots) return AZG_E_INVALID;
    const int B = e->cfg.n_trees, S = e->S_env;
    for (int i = 0; i < B; ++i)
        if (root_is_terminal(e->cfg.env_id, roots + (size_t)i * S)) return fail(e, AZG_E_TERMINAL_ROOT, "Can't do tree search from a terminal node");
    int cmax = 0;
    if (carry)
        for (int i = 0; i < B; ++i) {
            if (carry[i] < 0 || carry[i] > (1 << 30)) return fail(e, AZG_E_INVALID, "root_n_carry out of range");
            // MCTSContinuous never reuses a tree (no forward(): mcts.py:589-600 builds a fresh root for every search); its kernels' sqrt
            // table ends at n_sims + 1
            if (carry[i] != 0 && e->cfg.mode == AZG_MODE_CONTINUOUS)
                return fail(e, AZG_E_INVALID, "root_n_carry: continuous searches start from a fresh root (no carried count)");
            if (carry[i] > cmax) cmax = carry[i];
        }
    ON_DEVICE(e);
    { int trc = settle_team(e); if (trc) return trc; }   // an abandoned team search is redone on the roots it was started with
    e->carry_max = cmax;
    e->redo_ok = 0;
    HIPCHK(e, hipMemcpyAsync(e->d_roots, roots, sizeof(double) * (size_t)B * S, hipMemcpyHostToDevice, e->stream));
    if (carry) HIPCHK(e, hipMemcpyAsync(e->d_carry, carry, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, e->stream));
    else HIPCHK(e, hipMemsetAsync(e->d_carry, 0, sizeof(int) * (size_t)B, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AZG_OK;
}

int azg_search_resident(azg_engine* e) {
    if (!e) return AZG_E_INVALID;
    { int rrc = search_refusal(e); if (rrc) return rrc; }
    ON_DEVICE(e);
    e->P.search_idx = e->search_idx;
    e->last_search_idx = e->search_idx;
    e->ms_kept_valid = 0;
    e->P.publish = (e->opt.publish_always || e->publish_once) ? 1 : 0;
    e->team_search_idx = e->search_idx;
    e->last = LaunchRecord();
    const bool lockstep = use_lockstep(e);
    if (lockstep) { int prc = ls_prepare(e); if (prc) return prc; }
    if (lockstep) HIPCHK(e, hipEventRecord(e->ev0, e->stream));   // (several launches; the one-launch search kernel stamps ev0 / ev1 itself)
    const hipError_t rc = search_launch(e, lockstep);
    if (rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string("search kernel launch: ") + hipGetErrorString(rc));
    if (!e->last.timed) HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    e->search_idx += 1;
    e->searched = 1;
    const bool persistent = e->last.form == AZG_FORM_PERSISTENT;
    e->results_valid = persistent ? 1 : 0;   // the one-launch search kernel writes return_results in its epilogue
    e->published = (!persistent || e->last.tree_lds == TS_GLOBAL || e->P.publish) ? 1 : 0;
    e->redo_ok = 1;
    if (persistent && e->last.tree_lds == TS_GLOBAL && e->last.lds_exit != AZG_LDS_EXIT_FORCED && !e->lds_warned) {
        e->lds_warned = 1;
        static const char* why[] = {"", "more than 511 records per tree (n_sims + 2)", "more than 16 children per node (c_pw / kappa)",
                                    "the workgroup's LDS plan exceeds the CU's 160 KB", "", "",
                                    "the root's visit count (carried + n_sims) overflows the LDS records' counters"};
        const int x = e->last.lds_exit;
        const char* reason = x == AZG_LDS_EXIT_RECORDS && e->R <= 511 ? "more than 255 records per tree (n_sims + 2) for this network's kernels"
                                                                      : (x >= 0 && x < (int)(sizeof(why) / sizeof(why[0])) ? why[x] : "");
        if (!getenv("AZG_QUIET"))
            fprintf(stderr, "azgym: the trees of this search do not fit LDS residency (%s): they are kept in global memory -- same results, "
                            "slower tree walk (azg_search_info; once per engine)\n", reason);
    }
    return AZG_OK;
}

int azg_sync(azg_engine* e) {
    if (!e) return AZG_E_INVALID;
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return settle_team(e);
}

int azg_search(azg_engine* e, const double* roots, const int32_t* carry) {
    int rc = azg_upload_roots(e, roots, carry);
    if (rc) return rc;
    rc = azg_search_resident(e);
    if (rc) return rc;
    return azg_sync(e);
}

int azg_last_search_ms(azg_engine* e, float* ms) {
    if (!e || !ms) return AZG_E_INVALID;
    if (!e->searched) return fail(e, AZG_E_STATE, "no search has run");
    ON_DEVICE(e);
    HIPCHK(e, hipEventSynchronize(e->ev1));
    { int trc = settle_team(e); if (trc) return trc; }   // (the time of the launches that redid an abandoned team search, not of the abandoned launch)
    if (e->ms_kept_valid) { *ms = e->ms_kept; return AZG_OK; }   // (azg_dump_tree re-ran the search since: the time of the search itself)
    HIPCHK(e, hipEventElapsedTime(ms, e->ev0, e->ev1));
    return AZG_OK;
}

static int gather_results(azg_engine* e) {
    ON_DEVICE(e);
    int rc = launch_results(e);
    if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return AZG_OK;
}

int azg_results(azg_engine* e, float* actions, int32_t* counts, double* Q, double* v_target, int32_t* n_children) {
    if (!e) return AZG_E_INVALID;
    ON_DEVICE(e);
    int rc = launch_results(e);
    if (rc) return rc;
    // one copy of the whole block into pinned memory behind the search (and results) on the engine's stream, then host copies
    const ResultsLayout& L = e->res;
    HIPCHK(e, hipMemcpyAsync(e->h_res.p, e->d_res_block, L.bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const char* h = (const char*)e->h_res.p;
    if (Q) memcpy(Q, h + L.Q, L.vt - L.Q);
    if (v_target) memcpy(v_target, h + L.vt, L.actions - L.vt);
    if (actions) memcpy(actions, h + L.actions, L.counts - L.actions);
    if (counts) memcpy(counts, h + L.counts, L.nch - L.counts);
    if (n_children) memcpy(n_children, h + L.nch, L.bytes - L.nch);
    return AZG_OK;
}

int azg_results_resident(azg_engine* e, const float** actions, const int32_t** counts, const double** Q, const double** v_target,
                         const int32_t** n_children) {
    if (!e) return AZG_E_INVALID;
    ON_DEVICE(e);
    int rc = launch_results(e);
    if (rc) return rc;
    if (actions) *actions = e->d_actions;
    if (counts) *counts = e->d_counts;
    if (Q) *Q = e->d_Q;
    if (v_target) *v_target = e->d_vt;
    if (n_children) *n_children = e->d_nch;
    return AZG_OK;
}

int azg_root_children(azg_engine* e, int32_t* child_n, double* child_state) {
    if (!e) return AZG_E_INVALID;
    int rc = gather_results(e);
    if (rc) return rc;
    size_t B = e->cfg.n_trees, K = e->Kmax;
    D2H(child_n, e->d_child_n, B * K * 4);
    D2H(child_state, e->d_child_state, B * K * e->S_env * 8);
    return AZG_OK;
}

int azg_root_eval(azg_engine* e, float* value, float* dist) {
    if (!e) return AZG_E_INVALID;
    if (e->n_nets > 1) return fail(e, AZG_E_UNSUPPORTED, "azg_root_eval: not available for populations (azg_set_population > 1): azg_population_root_eval takes them");
    int rc = gather_results(e);
    if (rc) return rc;
    size_t B = e->cfg.n_trees;
    D2H(value, e->d_rootV, B * 4);
    D2H(dist, e->d_rootdist, B * e->nd * 4);
    return AZG_OK;
}

int azg_mlp_eval(azg_engine* e, const float* obs, size_t n, float* value, float* dist, float* raw) {
    if (!e || !obs) return AZG_E_INVALID;
    if (e->n_nets > 1) return fail(e, AZG_E_UNSUPPORTED, "azg_mlp_eval: not available for populations (azg_set_population > 1): azg_population_mlp_eval evaluates every net");
    if (!e->mlp_ready) return fail(e, AZG_E_STATE, "azg_set_weights has not been called");
    if (n == 0) return AZG_OK;
    if (n > (size_t)1 << 24) return fail(e, AZG_E_INVALID, "too many observations in one call");
    ON_DEVICE(e);
    const size_t So = e->S_obs, nd = e->nd;
    const size_t need = n * (So + 1 + nd + 1 + nd);
    if (need > e->eval_floats) {
        e->eval_mem.clear();
        e->eval_floats = 0;
        if (dalloc(e, e->eval_mem, &e->d_eval, need)) return AZG_E_DEVICE;
        e->eval_floats = need;
    }
    float* d_obs = e->d_eval;
    float* d_v = d_obs + n * So;
    float* d_d = d_v + n;
    float* d_r = d_d + n * nd;
    HIPCHK(e, hipMemcpyAsync(d_obs, obs, n * So * 4, hipMemcpyHostToDevice, e->stream));
    hipError_t rc = azg_dispatch_mlp_eval(e, d_obs, (int)n, d_v, d_d, d_r);
    if (rc != hipSuccess) return fail(e, AZG_E_DEVICE, std::string("mlp_eval kernel launch: ") + hipGetErrorString(rc));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    D2H(value, d_v, n * 4);
    D2H(dist, d_d, n * nd * 4);
    D2H(raw, d_r, n * (nd + 1) * 4);
    return AZG_OK;
}

int azg_dump_tree(azg_engine* e, int32_t* n_records, int32_t* parent, int32_t* edge_n, double* edge_W, double* edge_Q,
                  float* edge_action, int32_t* node_n, double* node_r, float* node_V, uint8_t* node_flags) {
    if (!e) return AZG_E_INVALID;
    if (!e->searched) return fail(e, AZG_E_STATE, "no search has run");
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    { int trc = settle_team(e); if (trc) return trc; }
    if (!e->published) {
        // The search kernel keeps its trees in LDS and, on the product path, writes out only return_results.  A dump re-runs the
        // last search -- same roots, weights and search index: the same trees, bit for bit -- with the trees published this once.
        if (!e->redo_ok)
            return fail(e, AZG_E_STATE, "the last search's trees were not written out and its inputs have changed since (self-play step, new "
                                        "roots or weights): dump right after the search, or set AZG_PUBLISH_TREES=1");
        // (with the index THAT search ran under -- azg_set_search_index may have moved the counter since -- and without disturbing
        // the counter or the timing of the search being inspected: azg_last_search_ms keeps reporting that search, not the re-run)
        float ms_before = 0.0f;
        HIPCHK(e, hipEventElapsedTime(&ms_before, e->ev0, e->ev1));
        const uint32_t idx_now = e->search_idx;
        e->publish_once = 1;
        e->search_idx = e->last_search_idx;
        int rc = azg_search_resident(e);
        e->publish_once = 0;
        e->search_idx = idx_now;
        if (rc) return rc;
        HIPCHK(e, hipStreamSynchronize(e->stream));
        { int trc = settle_team(e); if (trc) return trc; }
        e->ms_kept = ms_before; e->ms_kept_valid = 1;
    }
    size_t B = e->cfg.n_trees, R = e->R;
    std::vector<RecL> hot(B * R);
    std::vector<Cold> cold(B * R);
    std::vector<int> nrec(B);
    std::vector<double> ew(B * R);
    std::vector<float> ac(B * R);
    HIPCHK(e, hipMemcpy(hot.data(), e->P.hot, B * R * sizeof(RecL), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(cold.data(), e->P.cold, B * R * sizeof(Cold), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(nrec.data(), e->P.n_rec, B * 4, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(ew.data(), e->P.edge_W, B * R * 8, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(ac.data(), e->P.action, B * R * 4, hipMemcpyDeviceToHost));
    const bool cont = e->cfg.mode == AZG_MODE_CONTINUOUS;
    const int A = e->cfg.num_actions;
    for (size_t i = 0; i < B; ++i) {
        if (n_records) n_records[i] = nrec[i];
        for (size_t j = 0; j < R; ++j) {
            size_t o = i * R + j;
            bool in = (int)j < nrec[i];
            const RecL& h = hot[o];
            bool ex = in && (h.flags & FLAG_EXPANDED);
            if (parent) parent[o] = in ? (j == 0 ? -1 : h.parent) : 0;
            if (edge_n) edge_n[o] = in ? h.edge_n : 0;
            if (edge_W) edge_W[o] = in ? ew[o] : 0.0;
            if (edge_Q) edge_Q[o] = in ? h.Q : 0.0;
            if (edge_action) edge_action[o] = in ? (cont ? ac[o] : (j == 0 ? 0.0f : (float)((j - 1) % A))) : 0.0f;
            if (node_n) node_n[o] = in ? h.node_n : 0;
            if (node_r) node_r[o] = ex ? cold[o].r : 0.0;
            if (node_V) node_V[o] = ex ? cold[o].V : 0.0f;
            if (node_flags) node_flags[o] = in ? h.flags : 0;
        }
    }
    return AZG_OK;
}

// the kernel(s) of the last search as rocprofv3 names them (template arguments: ENV, HP, NREG, tree storage, mixture head, waves, tree
// groups, trees per group, compile-time specialisation; team kernel: ..., staging chunk length, workgroups per CU -- see search_kernel.cuh / team.cuh)
static int kernel_name(const azg_engine* e, char* buf, size_t n) {
    const int env = azg_kernel_env(e->cfg);
    const char* gmm = (env != AZG_ENV_CARTPOLE && e->P.ncomp >= 2) ? "true" : "false";
    const LaunchRecord& r = e->last;
    switch (r.form) {
        case AZG_FORM_PERSISTENT: return snprintf(buf, n, r.nets ? "search_kernel_nets<%d, %d, %d, %d, %s, %d, %d, %d, %d>" : "search_kernel<%d, %d, %d, %d, %s, %d, %d, %d, %d>", env, e->HP, e->nreg, r.tree_lds, gmm, r.waves, r.groups, r.tile_trees, r.spec);
        case AZG_FORM_PER_LAYER: return snprintf(buf, n, "%s<%d, ...> + ls_layer0_kernel + ls_hidden_tiled_kernel<%d, ...> per simulation step",
                                                 r.nets ? "ls_tree_kernel_nets" : "ls_tree_kernel", env, e->HP);
        case AZG_FORM_TEAM:
            if (r.nets) return snprintf(buf, n, "ls_team_kernel_nets<%d, %d, %s, %d, %d, %d>", env, e->HP, gmm, r.tree_lds, r.team_kc, r.team_minb);
            return snprintf(buf, n, "ls_team_kernel<%d, %d, %s, %d, %d, %d, %d, %d%s>", env, e->HP, gmm, r.tree_lds, r.team_kc, r.team_minb, r.spec, r.team_tt,
                                            r.team_pop ? ", true" : "");   // (a population's instantiation: POP)
        default: return snprintf(buf, n, "(no search yet)");
    }
}

// include/azgym.h: what the last search ran as (kernel form, tree residency and why, team fall-backs)
int azg_search_info(azg_engine* e, azg_search_report* info) {
    if (!e || !info) return AZG_E_INVALID;
    if (info->struct_size != (int32_t)sizeof(azg_search_report)) return fail(e, AZG_E_INVALID, "azg_search_info: struct_size mismatch");
    if (e->searched && e->team_pending) {   // (an abandoned team search is redone before its form is reported)
        ON_DEVICE(e);
        int trc = settle_team(e);
        if (trc) return trc;
    }
    memset(info, 0, sizeof(*info));
    info->struct_size = (int32_t)sizeof(azg_search_report);
    const LaunchRecord& r = e->last;
    info->kernel_form = e->searched ? r.form : AZG_FORM_NONE;
    info->max_records = e->R; info->max_children = e->Kmax;
    info->team_fallbacks = e->team_fallbacks;
    if (!e->searched) { kernel_name(e, info->kernel_name, sizeof(info->kernel_name)); info->lds_exit = AZG_LDS_RESIDENT; return AZG_OK; }
    info->tree_storage = r.form == AZG_FORM_PERSISTENT ? r.tree_lds : AZG_TREES_GLOBAL;   // (the team kernel only stages its trees in LDS)
    info->lds_exit = r.lds_exit;
    info->spec = r.spec;
    info->waves = r.waves; info->groups = r.groups; info->tile_trees = r.tile_trees;
    if (r.form == AZG_FORM_TEAM) { info->team_trees = r.team_tt; info->team_per_cu = r.team_minb; info->team_parts = r.team_parts; }
    float ms = 0.0f;
    int rc = azg_last_search_ms(e, &ms);
    if (rc) return rc;
    info->last_ms = ms;
    kernel_name(e, info->kernel_name, sizeof(info->kernel_name));
    return AZG_OK;
}

int azg_max_children(const azg_engine* e) { return e ? e->Kmax : AZG_E_INVALID; }
int azg_max_records(const azg_engine* e) { return e ? e->R : AZG_E_INVALID; }
int azg_env_state_dim(const azg_engine* e) { return e ? e->S_env : AZG_E_INVALID; }
int azg_obs_dim(const azg_engine* e) { return e ? e->S_obs : AZG_E_INVALID; }

int azg_synthetic_roots(azg_engine* e, double* roots) {
    if (!e || !roots) return AZG_E_INVALID;
    for (int i = 0; i < e->cfg.n_trees; ++i)
        azg_reset_state(e->cfg.seed, (uint32_t)(e->cfg.tree_id_base + i), 0u, azg_reset_kind(e->cfg.env_id), roots + (size_t)i * e->S_env);
    return AZG_OK;
}

}  // extern "C"
