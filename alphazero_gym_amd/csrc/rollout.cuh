// rollout.cuh -- policy rollouts (azg_policy_rollout / azg_policy_rollout_ex, include/azgym_eval.h): whole episodes played by the network alone, one launch.
// Grid (ceil(G / 16), n_nets): one workgroup carries 16 games of one net from reset through every step.  Per step the games'
// observations go to LDS, mlp_forward runs (the search's network phase: same MFMA chains and chunked head sums, so the head outputs
// are azg_mlp_eval's), and one lane per game turns them into an action, steps the env in float64 and adds the reward; observing and
// stepping are env.cuh's game_obs / game_step, the game interface this kernel shares with the self-play step.  A finished game
// is frozen (its lane skips the step; its column still rides through the network and every barrier); the loop ends when wave 0 finds
// no live game, which it tells the workgroup through LDS, so the exit is uniform.  No atomics: every output has one writer.
// NREG > 0: the hidden->hidden weights stay in registers for the whole rollout (the nets the search keeps resident: resident_layers,
// engine_weights.hip); NREG == 0: they are streamed from L2 every step (any depth, LayerNorm, the rare activations).  The first layer
// and (NREG > 0) the head are register-resident either way -- up to HP = 256.  HP = 512 / 1024 (azg_policy_rollout_ex: NREG == 0 only)
// stream the first layer too, as mlp_eval_kernel does: the GROUP form of the wide rollouts, which takes every wide shape and is what
// the team form (rollout_team.cuh) falls back to.
#pragma once
#include "records.h"
#include "env.cuh"
#include "mlp.cuh"
#include "../../include/azgym_eval.h"

struct Rollout {
    int G, max_len, rule;
    unsigned game_id_base, episode;
    double* returns;      // [n_nets][G]
    int* lengths;         // [n_nets][G]
    int* terminated;      // [n_nets][G]
    float* first_value;   // [n_nets][G]
};

// the action of game column tl from the head outputs of step t (gid: the game's global id)
template <int NCH>
__device__ __forceinline__ float rollout_action(const KParams& P, const Rollout& ro, const f32x4* parts, const float* s_bhead, int tl,
                                                unsigned gid, unsigned t) {
    const bool sample = ro.rule == AZG_ROLLOUT_SAMPLE;
    if (P.mode == AZG_MODE_DISCRETE) {
        const int A = P.nd;
        float mx = head_output<NCH, 64>(parts, s_bhead, tl, 1);
        int best = 0;
        for (int a = 1; a < A; ++a) { const float v = head_output<NCH, 64>(parts, s_bhead, tl, 1 + a); if (v > mx) { mx = v; best = a; } }
        if (!sample) return (float)best;
        // softmax as azg_mlp_eval's dist (DiscretePolicy.predict_pi), then the inverse-CDF walk in float64
        float sum = 0.0f;
        for (int a = 0; a < A; ++a) sum = sum + azg_expf(head_output<NCH, 64>(parts, s_bhead, tl, 1 + a) - mx);
        const azg_u32x4 b = azg_draw(P.seed, gid, t, 0u, AZG_STREAM_ACT);
        const double u = ((double)b.v[0] + 0.5) * (1.0 / 4294967296.0);
        double c = 0.0;
        int pick = A - 1;
        bool found = false;
        for (int a = 0; a < A; ++a) {
            const float p = azg_expf(head_output<NCH, 64>(parts, s_bhead, tl, 1 + a) - mx) / sum;
            c = c + (double)p;
            if (!found && u < c) { pick = a; found = true; }
        }
        return (float)pick;
    }
    float mu, sg;
    if (P.ncomp >= 2) {
        float gd[3 * GMM_MAXC];
        gmm_params<NCH, 64>(parts, s_bhead, tl, P.ncomp, P.ls_min, P.ls_max, gd);
        if (sample) {
            gmm_pick(gd, P.ncomp, P.seed, gid, t, 0u, &mu, &sg);
        } else {
            float lc = head_output<NCH, 64>(parts, s_bhead, tl, 1 + 2 * P.ncomp);
            mu = gd[0]; sg = gd[GMM_MAXC];
#pragma unroll
            for (int c = 1; c < GMM_MAXC; ++c)
                if (c < P.ncomp) {
                    const float v = head_output<NCH, 64>(parts, s_bhead, tl, 1 + 2 * P.ncomp + c);
                    if (v > lc) { lc = v; mu = gd[c]; sg = gd[GMM_MAXC + c]; }
                }
        }
    } else {
        mu = head_output<NCH, 64>(parts, s_bhead, tl, 1);
        float ls = head_output<NCH, 64>(parts, s_bhead, tl, 2);
        ls = ls < P.ls_min ? P.ls_min : (ls > P.ls_max ? P.ls_max : ls);
        sg = azg_expf(ls);
    }
    const float eps = sample ? azg_normal(P.seed, gid, t, 0u) : 0.0f;
    return P.bound_f * azg_tanhf(mu + sg * eps);
}

template <int HP, int NREG>
__global__ __launch_bounds__(256, 1) void rollout_kernel(KParams P, Rollout ro) {
    constexpr int NCH = head_chunks<HP>();
    __shared__ f32x4 s_parts[NCH * 64];
    __shared__ float s_obsT[128];   // [8 input rows][16 games]
    __shared__ float s_bhead[16];
    __shared__ float s_ln[2 * 64];
    __shared__ int s_live;
    extern __shared__ f32x4 s_act[];   // two activation buffers of HP/16 tiles x 64 lanes
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int net = blockIdx.y;
    const size_t wofs = (size_t)net * P.net_wstride;
    if (tid < 16) s_bhead[tid] = P.bhead[wofs + tid];
    // this net's weights, read once: the first layer, and with NREG > 0 the hidden->hidden layers and the head
    typedef WRegs<HP, NREG, 4> WR;
    WR wr;
    constexpr int NTW = HP / 64;
    if constexpr (HP <= 256) {   // (wider: mlp_forward streams the first layer too, as in mlp_eval_kernel)
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            wr.w0[i] = P.W0[wofs + (wave * NTW + i) * 64 + lane];
            if (P.in8) wr.w0b[i] = P.W0b[wofs + (wave * NTW + i) * 64 + lane];
            wr.b0[i] = net_ptr(P.b0, wofs)[(wave * NTW + i) * 64 + lane];
        }
    }
    if constexpr (NREG > 0) {
        constexpr int S4 = HP / 16;
#pragma unroll
        for (int l = 0; l < NREG; ++l) {
#pragma unroll
            for (int i = 0; i < NTW; ++i) {
                wr.b[l][i] = net_ptr(P.bl[l], wofs)[(wave * NTW + i) * 64 + lane];
#pragma unroll
                for (int s4 = 0; s4 < S4; ++s4) wr.w[l][i][s4] = net_ptr(P.Wl[l], wofs)[((wave * NTW + i) * S4 + s4) * 64 + lane];
            }
        }
#pragma unroll
        for (int i = 0; i < NTW; ++i) wr.wh[i] = net_ptr(P.Whead, wofs)[(wave * NTW + i) * 64 + lane];
    }
    // the game of lanes 0..15 of wave 0 (rows of the last group beyond G: no game, finished from the start)
    const int game = blockIdx.x * 16 + tid;
    const bool mine = tid < 16 && game < ro.G;
    const unsigned gid = ro.game_id_base + (unsigned)game;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, ret = 0.0;
    int t = 0, term = 0;
    float v0 = 0.0f;
    bool fin = !mine;
    if (mine) azg_reset_state(P.seed, gid, ro.episode, azg_reset_kind(P.env_id), s);
#ifdef AZG_STAMPS
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    for (;;) {
        double sn = 0.0;   // Pendulum: sin(theta) of the state observed, for its step
        if (tid < 16) {
            float obs[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            if (mine) game_obs(P.env_id, s, obs, &sn);
#pragma unroll
            for (int k = 0; k < 8; ++k) s_obsT[k * 16 + tid] = obs[k];
        }
        if (wave == 0) {
            const int live = __any(!fin);
            if (lane == 0) s_live = live;
        }
        __syncthreads();
        // (s_live and s_obsT are next written behind mlp_forward's closing barrier, which every wave passes after reading them)
        if (!s_live) break;
        mlp_forward<HP, NREG, 4, 1, 64, WR, 16, true>(P, wr, s_obsT, s_act, s_act + HP / 16 * 64, s_parts, s_ln, wave, lane STAMP_ARG, nullptr, 0, wofs);
        if (!fin) {
            if (t == 0) v0 = head_output<NCH, 64>(s_parts, s_bhead, tid, 0);
            const float a = rollout_action<NCH>(P, ro, s_parts, s_bhead, tid, gid, (unsigned)t);
            double ns[4] = {0.0, 0.0, 0.0, 0.0}, r;
            int done;
            game_step(P.env_id, s, sn, a, ns, &r, &done);
            ret = ret + r;
            t += 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = ns[k];
            if (done || t >= ro.max_len) { fin = true; term = done ? 1 : 0; }
        }
    }
    if (mine) {
        const size_t o = (size_t)net * ro.G + game;
        ro.returns[o] = ret;
        ro.lengths[o] = t;
        ro.terminated[o] = term;
        ro.first_value[o] = v0;
    }
}

template <int HP, int NREG>
static hipError_t rollout_launch(azg_engine* e, const Rollout& ro) {
    auto kern = rollout_kernel<HP, NREG>;
    const size_t lds = (size_t)2 * HP * 64;
    static KernelAttrs attrs;
    hipError_t rc = attrs.set_dyn_lds(e, (const void*)kern, lds);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)((ro.G + 15) / 16), (unsigned)e->n_nets), dim3(256), lds, e->stream, e->P, ro);
    return hipGetLastError();
}
