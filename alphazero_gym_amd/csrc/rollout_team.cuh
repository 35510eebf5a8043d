// rollout_team.cuh -- policy rollouts of wide networks (azg_policy_rollout_ex, include/azgym_eval.h) as ONE persistent launch of
// cooperating workgroups: the team form.  rollout_kernel (rollout.cuh) streams a whole net's hidden weights per 16 games per step;
// here the games are cut into TEAMS as team.cuh cuts a search's trees: 32 games of one net (two 16-game groups) and the NU = HP/64
// workgroups that compute the 64-unit slices of every layer for exactly those games.  Every workgroup reads 1/NU of the hidden
// weights, a team is spread over NU CUs, and with TEAM_SPREAD's block mapping each XCD's L2 keeps its slices' weights.
// A workgroup also OWNS 32/NU of the team's games (4 at HP = 512, 2 at HP = 1024): one lane per game in wave 0 keeps the game's
// float64 state, return, step count and flags in registers for the whole rollout, as rollout_kernel's lanes do.  Per step a team goes
//     observations + first layer (every workgroup, its own games)  ->  hidden layer 1 .. n-1 (every workgroup, one tile each)
//     ->  head partials of its own games into LDS  ->  action, env step, return (the owner lanes)
// with team.cuh's hand-offs and nothing else: team_arrive / team_wait on one monotonic counter per hand-off, every handed-off byte
// stored and loaded with sc1 (TileMem<true>, write-through always: no same-XCD variant here), one lane polling with a bounded spin
// and the abort word.  On a time-out every workgroup leaves, nothing is written, and the host replays the call in the group form.
// The arithmetic is the lock-step path's (team_first_layer, ls_tile_wd, chunked head sums over 64-unit chunks) followed by
// rollout_action: the results are the group form's and the CPU rollout's, bit for bit.
#pragma once
#include "team_dispatch.cuh"   // (team.cuh, and TEAM_KC32: the chunk length of the search's 32-tree teams)
#include "rollout.cuh"

// The network's first layer of a workgroup's OWN TPW games, all HP units of it, on the vector ALU straight from the observations in
// LDS (s_obs: [4 features][TPW]), written into the team's first activation buffer in the hidden layers' B-operand layout.
// A COPY of ls_team_kernel's first_layer lambda (team.cuh), statement for statement: the same fma chain from the bias over k = 0..3 as
// the MFMA form, bit for bit.  Not shared: with the lambda lifted into a function of both kernels three of the search's team kernels
// changed their spilled-SGPR counts (63 -> 65, 71 -> 75, 102 -> 98; profiles/population_wide_resource_usage.txt), and the search
// kernels' code is not this header's to change.  Keep the two in step.
template <int HP, int TPW>
__device__ __forceinline__ void team_first_layer(const KParams& P, const TileMem<true>& act0, bool wt_now, const float* s_obs, int us, int g0,
                                                 size_t wofs) {
    const int tid = threadIdx.x;
    constexpr int TPT = 256 / TPW;                       // threads per game
    constexpr int UPT = HP / TPT;                        // units per thread
    const int j = tid / TPT, u0 = (tid % TPT) * UPT;
    static_assert(UPT % 4 == 0, "whole float4s of units per thread");
    const int c = us * TPW + j;                          // the game within the team: group g0 + c / 16, column c % 16
    const float x0 = s_obs[0 * TPW + j], x1 = s_obs[1 * TPW + j], x2 = s_obs[2 * TPW + j], x3 = s_obs[3 * TPW + j];
    TileMem<true> out = act0;
    out.wt = wt_now;
#pragma unroll
    for (int h = 0; h < UPT / 4; ++h) {
        const int u = u0 + 4 * h;
        f32x4 acc = net_ptr(P.b0u, wofs)[u / 4];
        const f32x4* W0u = net_ptr(P.W0u, wofs);
        const f32x4 wa = W0u[u], wb = W0u[u + 1], wc = W0u[u + 2], wd = W0u[u + 3];
        acc.x = __builtin_fmaf(wa.x, x0, acc.x); acc.x = __builtin_fmaf(wa.y, x1, acc.x); acc.x = __builtin_fmaf(wa.z, x2, acc.x); acc.x = __builtin_fmaf(wa.w, x3, acc.x);
        acc.y = __builtin_fmaf(wb.x, x0, acc.y); acc.y = __builtin_fmaf(wb.y, x1, acc.y); acc.y = __builtin_fmaf(wb.z, x2, acc.y); acc.y = __builtin_fmaf(wb.w, x3, acc.y);
        acc.z = __builtin_fmaf(wc.x, x0, acc.z); acc.z = __builtin_fmaf(wc.y, x1, acc.z); acc.z = __builtin_fmaf(wc.z, x2, acc.z); acc.z = __builtin_fmaf(wc.w, x3, acc.z);
        acc.w = __builtin_fmaf(wd.x, x0, acc.w); acc.w = __builtin_fmaf(wd.y, x1, acc.w); acc.w = __builtin_fmaf(wd.z, x2, acc.w); acc.w = __builtin_fmaf(wd.w, x3, acc.w);
        // unit u = 16 t + 4 g + r of game column cc -> float4 ((group * HP/16 + t) * 64 + g * 16 + cc), component r
        out.store4(((size_t)(g0 + c / 16) * (HP / 16) + u / 16) * 64 + ((u % 16) / 4) * 16 + c % 16, act4<true>(P.act, acc));
    }
}

// Launch `TQ` teams from global team `team_base`; a net has `tpn` = ceil(G / 32) teams, team T belongs to net T / tpn and carries that
// net's games 32 * (T % tpn) .. + 31 (columns beyond G hold no game and are finished from the start).  L: the rollout's own activation
// and head-partial buffers, indexed by the team's place in THIS launch (launches of one call follow each other on the stream).
// live: [TQ][2][16] words, the owners' live-game counts (see the loop).
template <int HP>
__global__ __launch_bounds__(256, 2) void rollout_team_kernel(KParams P, Rollout ro, LockStep L, TeamCtl T, float* live, int TQ, int team_base,
                                                              int tpn) {
    constexpr int NU = HP / 64, NCH = HP / 64, TPW = 32 / NU, KC = TEAM_KC32;
    static_assert(NU % 8 == 0 && TPW >= 1, "a team's slices are dealt out over the eight XCDs");
    extern __shared__ f32x4 s_ab[];     // the tile routine's two stages; between tiles the head partials of this workgroup's games
    __shared__ float s_obs[32];         // [4 features][TPW] observations of this workgroup's games
    __shared__ float s_bhead[16];
    __shared__ int s_ok;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // (Acrobot's six network inputs make its nets the group form's: its RK4 step, the one user of scratch memory behind game_step,
    // is not compiled into this kernel)
    __builtin_assume(P.env_id != AZG_ENV_ACROBOT);
    // team and slice of this workgroup: ls_team_kernel's TEAM_SPREAD mapping (blockIdx % 8 = XCD under round-robin dispatch, NU / 8
    // slices of every team on each XCD)
    const int x = blockIdx.x % 8, jb = blockIdx.x / 8, sp = NU / 8;
    const int tq = jb / sp, us = x * sp + jb % sp;
    if (tq >= TQ) return;               // (never: the grid is TQ * NU blocks)
    const int g0 = 2 * tq;              // the team's two 16-game groups in the buffers of this launch
    unsigned* cnt = T.cnt + (size_t)tq * TEAM_MAX_CNT * TEAM_CNT_STRIDE;
    const int team = team_base + tq, net = team / tpn;
    const size_t wofs = (size_t)net * P.net_wstride;          // taken once: the team's net for the whole rollout
    const int n_layers = P.n_hidden - 1;                      // hidden->hidden layers 1 .. n_layers
    if (tid < 16) s_bhead[tid] = P.bhead[wofs + tid];
    if (tid < 32) s_obs[tid] = 0.0f;
    // ---- this workgroup's games: lane j < TPW of wave 0 owns column us * TPW + j of the team
    const bool owner = tid < TPW;
    const int col = us * TPW + (owner ? tid : 0);
    const int game = (team % tpn) * 32 + col;
    const bool mine = owner && game < ro.G;
    const unsigned gid = ro.game_id_base + (unsigned)game;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ret = 0.0;
    int len = 0, term = 0;
    float v0 = 0.0f;
    bool fin = !mine;
    if (mine) {
        // (the reset law as a constant per call: azg_reset_state's loops then unroll and the state stays in registers, no scratch memory)
        switch (azg_reset_kind(P.env_id)) {
            case AZG_RESET_CARTPOLE: azg_reset_state(P.seed, gid, ro.episode, AZG_RESET_CARTPOLE, s); break;
            case AZG_RESET_MOUNTAINCAR: azg_reset_state(P.seed, gid, ro.episode, AZG_RESET_MOUNTAINCAR, s); break;
            default: azg_reset_state(P.seed, gid, ro.episode, AZG_RESET_PENDULUM, s); break;
        }
    }
    const TileMem<true> act0(L.act[0], true), parts_mem(L.parts), live_mem(live);
    __syncthreads();
    // Step t.  Every game of the team is at step t while it is live, so the loop index is the games' step count and max_len bounds
    // the loop for every workgroup without communication.
    for (int t = 0; t < ro.max_len; ++t) {
        double sn = 0.0;   // Pendulum: sin(theta) of the state observed, for its step
        if (owner) {
            float obs[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (mine) game_obs(P.env_id, s, obs, &sn);   // (a finished game: its frozen state's observation, as in the group form)
#pragma unroll
            for (int k = 0; k < 4; ++k) s_obs[k * TPW + tid] = obs[k];
        }
        // The early exit has to be taken by all NU workgroups at the same step: every owner publishes how many of its games are live
        // with the step's first-layer hand-off, and everybody adds the team's NU words up behind the wait on counter 0.  The words
        // are indexed by the step's parity, so a fast owner writing step t + 1's count never touches the word a slow reader still
        // has to read for step t.  (Even one word per workgroup would do: an owner writes step t + 1's count only behind the last
        // hidden layer's hand-off of step t, which every workgroup reaches after it has read step t's counts.)
        if (wave == 0) {
            const int n_live = __popcll(__ballot(!fin));
            if (lane == 0) live_mem.store1(((size_t)tq * 2 + (t & 1)) * 16 + us, (float)n_live);
        }
        __syncthreads();
        team_first_layer<HP, TPW>(P, act0, true, s_obs, us, g0, wofs);
        team_arrive(cnt);
        if (!team_wait(cnt, (unsigned)(NU * (t + 1)), T, &s_ok)) return;
        {
            // (every wave reads the same NU words, which nobody overwrites before the step after next: a uniform verdict without a barrier)
            const float v = lane < NU ? live_mem.load1(((size_t)tq * 2 + (t & 1)) * 16 + lane) : 0.0f;
            if (!__any(v != 0.0f)) break;
        }
        // ---- the hidden layers: this workgroup's 64-unit slice of each, for the team's 32 games
        for (int l = 1; l <= n_layers; ++l) {
            const int in_buf = (l - 1) & 1;
            if (l == n_layers) ls_tile_wd<HP, true, 2, true, KC>(P, L, l, in_buf, us, g0, s_ab, true, wofs);
            else ls_tile_wd<HP, false, 2, true, KC>(P, L, l, in_buf, us, g0, s_ab, true, wofs);
            team_arrive(cnt + l * TEAM_CNT_STRIDE);
            if (!team_wait(cnt + l * TEAM_CNT_STRIDE, (unsigned)(NU * (t + 1)), T, &s_ok)) return;
        }
        // ---- the head partials of this workgroup's games (chunk w, output row group q, game slot j -> s_ab[w * 64 + q * 16 + j]:
        // head_output's layout with the slot as the column), then action and step by the owner lanes
        for (int i = tid; i < NCH * 4 * TPW; i += 256) {
            const int w = i / (4 * TPW), q = (i / TPW) % 4, j = i % TPW, c = us * TPW + j;
            s_ab[w * 64 + q * 16 + j] = parts_mem.load4(((size_t)(g0 + c / 16) * NCH + w) * 64 + q * 16 + c % 16);
        }
        __syncthreads();
        if (!fin) {
            if (t == 0) v0 = head_output<NCH, 64>(s_ab, s_bhead, tid, 0);
            const float a = rollout_action<NCH>(P, ro, s_ab, s_bhead, tid, gid, (unsigned)t);
            double ns[4] = {0.0, 0.0, 0.0, 0.0}, r;
            int done;
            game_step(P.env_id, s, sn, a, ns, &r, &done);
            ret = ret + r;
            len = t + 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = ns[k];
            if (done || len >= ro.max_len) { fin = true; term = done ? 1 : 0; }
        }
        // (s_obs and the stages are next written behind barriers that every wave passes after these reads: the one in front of the
        // first layer, team_arrive's)
    }
    if (mine) {   // one writer per output element
        const size_t o = (size_t)net * ro.G + game;
        ro.returns[o] = ret;
        ro.lengths[o] = len;
        ro.terminated[o] = term;
        ro.first_value[o] = v0;
    }
}

// dynamic LDS of a team-rollout workgroup: the tile stages (between tiles: the head partials' landing area, team_table_off)
static inline size_t rollout_team_lds() { return team_table_off(TEAM_KC32, 2); }
