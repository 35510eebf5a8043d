// policy rollouts, team form (rollout_team.cuh): the kernel's instantiations, its residency rule, buffers and launches.  A translation
// unit of its own, so that the search's team kernels and the group rollout keep their code and resources.
#include "engine_host.h"
#include "rollout_team.cuh"

// the rollout's own hand-off memory for `teams` teams per launch at width HP (grow-only)
static hipError_t rollout_team_buffers(azg_engine* e, int teams, int HP) {
    const size_t units = (size_t)teams * HP;
    if (units <= e->ro_team_units && teams <= e->ro_team_cap) return hipSuccess;
    const size_t U = units > e->ro_team_units ? units : e->ro_team_units;
    const int C = teams > e->ro_team_cap ? teams : e->ro_team_cap;
    e->ro_team_mem.clear();
    e->ro_team_units = 0; e->ro_team_cap = 0;
    // per team: two 16-game groups of HP / 16 tiles x 64 lanes float4 per activation buffer, HP / 64 chunks x 64 lanes float4 of head
    // partials; 2 x 16 live-count words; TEAM_MAX_CNT counters 128 bytes apart; behind the last team's counters the abort word
    float *a0, *a1, *parts;
    if (dalloc(e, e->ro_team_mem, &a0, U * 32) || dalloc(e, e->ro_team_mem, &a1, U * 32) || dalloc(e, e->ro_team_mem, &parts, U * 8) ||
        dalloc(e, e->ro_team_mem, &e->d_ro_live, (size_t)C * 32) ||
        dalloc(e, e->ro_team_mem, &e->d_ro_cnt, (size_t)C * TEAM_MAX_CNT * TEAM_CNT_STRIDE + TEAM_CNT_STRIDE))
        return hipErrorOutOfMemory;
    e->ro_ls = LockStep{};
    e->ro_ls.act[0] = (f32x4*)a0; e->ro_ls.act[1] = (f32x4*)a1; e->ro_ls.parts = (f32x4*)parts;
    e->ro_team_units = U; e->ro_team_cap = C;
    return hipSuccess;
}

// Residency as team_launch_form's (team_dispatch.cuh): two workgroups per CU by __launch_bounds__, the occupancy query's answer capped at
// 6, and a launch holds at most usable * n_cus / NU teams.  More teams than that run as successive launches: teams are independent and
// nothing carries over between them.
template <int HP>
static hipError_t rollout_team_launch(azg_engine* e, const Rollout& ro, int* launches, unsigned** abort_word) {
    constexpr int NU = HP / 64;
    if (e->n_hidden - 1 >= TEAM_CNT_XB) return hipErrorNotReady;   // (one counter per hidden layer, as in the search)
    auto kern = rollout_team_kernel<HP>;
    const size_t lds = rollout_team_lds();
    static KernelAttrs attrs;
    int per_cu = 0;
    hipError_t rc = attrs.occupancy(e, (const void*)kern, 256, lds, &per_cu);
    if (rc != hipSuccess) return rc;
    const int usable = per_cu < 6 ? per_cu : 6;
    long cap = (long)usable * e->n_cus / NU;
    if (cap < 1) return hipErrorNotReady;
    if (e->opt.rollout_teams > 0 && cap > e->opt.rollout_teams) cap = e->opt.rollout_teams;
    const int tpn = (ro.G + 31) / 32;
    const long total = (long)tpn * e->n_nets;
    const int per = (int)(total < cap ? total : cap);
    rc = rollout_team_buffers(e, per, HP);
    if (rc != hipSuccess) return rc;
    const size_t cnt_words = (size_t)e->ro_team_cap * TEAM_MAX_CNT * TEAM_CNT_STRIDE;
    TeamCtl T;
    T.cnt = e->d_ro_cnt;
    T.abort = e->d_ro_cnt + cnt_words;
    T.spin_limit = (unsigned)e->opt.team_spin_limit;
    *abort_word = T.abort;
    for (long base = 0; base < total; base += per) {
        const int TQ = (int)(total - base < per ? total - base : per);
        // the first launch of the call: the counters and the abort word; the later ones: their teams' counters
        rc = hipMemsetAsync(e->d_ro_cnt, 0, (base == 0 ? cnt_words + TEAM_CNT_STRIDE : (size_t)TQ * TEAM_MAX_CNT * TEAM_CNT_STRIDE) * sizeof(unsigned), e->stream);
        if (rc != hipSuccess) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)(TQ * NU)), dim3(256), lds, e->stream, e->P, ro, e->ro_ls, T, e->d_ro_live, TQ, (int)base, tpn);
        rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
        *launches += 1;
    }
    return hipSuccess;
}

hipError_t azg_rollout_team(azg_engine* e, const Rollout& ro, int* launches, unsigned** abort_word) {
    if (e->HP == 512) return rollout_team_launch<512>(e, ro, launches, abort_word);
    if (e->HP == 1024) return rollout_team_launch<1024>(e, ro, launches, abort_word);
    return hipErrorNotReady;
}
