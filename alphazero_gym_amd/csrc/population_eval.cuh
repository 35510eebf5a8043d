// population_eval.cuh -- batched inference for every net of a population in one launch (azg_population_mlp_eval / _device,
// include/azgym_eval.h): the search's network phase without a game attached, net by blockIdx.y as in rollout_kernel.
// Grid (groups, n_nets): workgroup (g, k) evaluates net k on the 16-observation tiles g, g + groups, ... of that net's rows.  Net k's
// weights are read ONCE per workgroup, exactly as rollout_kernel takes them: the first layer, and with NREG > 0 the hidden->hidden layers
// and the head, into registers (the nets the search keeps resident: e->nreg); NREG == 0 streams the hidden layers from L2 per tile (any
// depth, LayerNorm, the rare activations), and HP = 512 / 1024 the first layer too -- mlp_eval_kernel's form and LDS plan, with the
// tile loop around it.  Per tile only the observations change: they go to LDS, mlp_forward runs (same MFMA chains and chunked head sums
// as azg_mlp_eval; rollout.cuh already relies on NREG > 0 and NREG == 0 agreeing bit for bit) and lanes 0..15 of wave 0 write one row
// each with mlp_eval_kernel's epilogue (eval_write_row).  A row's bits therefore do not depend on n, n_nets, groups or its position.
// No atomics, no waiting between workgroups: every output has one writer.
#pragma once
#include "records.h"
#include "mlp.cuh"
#include "mlp_eval.cuh"
#include "../../include/azgym_eval.h"

struct PopEval {
    const float* obs;     // [n_nets][n][S_obs], or [n][S_obs] when obs_stride == 0 (every net on the same rows)
    size_t obs_stride;    // floats between two nets' observations
    int n, S_obs, nd;
    float* value;         // [n_nets][n]             (each may be NULL)
    float* dist;          // [n_nets][n][nd]
    float* raw;           // [n_nets][n][1 + nd]
};

template <int HP, int NREG>
__global__ __launch_bounds__(256, 1) void population_eval_kernel(KParams P, PopEval pe) {
    constexpr int NCH = head_chunks<HP>();
    __shared__ f32x4 s_parts[NCH * 64];
    __shared__ float s_obsT[128];   // [8 input rows][16 observations]
    __shared__ float s_bhead[16];
    __shared__ float s_ln[2 * 64];
    extern __shared__ f32x4 s_act[];   // two activation buffers of HP/16 tiles x 64 lanes
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int net = blockIdx.y;
    const size_t wofs = (size_t)net * P.net_wstride;
    if (tid < 16) s_bhead[tid] = P.bhead[wofs + tid];
    // this net's weights, read once: the first layer, and with NREG > 0 the hidden->hidden layers and the head (as rollout_kernel)
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
    const float* obs = pe.obs + (size_t)net * pe.obs_stride;
    const size_t out0 = (size_t)net * pe.n;   // this net's first output row
    float* value = pe.value ? pe.value + out0 : nullptr;
    float* dist = pe.dist ? pe.dist + out0 * pe.nd : nullptr;
    float* raw = pe.raw ? pe.raw + out0 * (pe.nd + 1) : nullptr;
    const int tiles = (pe.n + 15) / 16;
#ifdef AZG_STAMPS
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // (the trip count depends on blockIdx.x alone: every barrier below is reached by all four waves)
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // s_obsT of the previous tile was last read by mlp_forward's first layer, which every wave left before that call's closing barrier:
        // these stores come behind it
        if (tid < 128) {
            const int k = tid >> 4, row = tile * 16 + (tid & 15);
            s_obsT[tid] = (row < pe.n && k < pe.S_obs) ? obs[(size_t)row * pe.S_obs + k] : 0.0f;
        }
        // This barrier publishes s_obsT (and, in the first round, s_bhead), and it is the one that protects s_parts: wave 0 arrives here only
        // after its epilogue of the previous tile has read the head partials, and no wave stores new ones (the end of mlp_forward) before
        // it has passed.  The activation buffers and s_ln are ordered by the closing barrier, like s_obsT.
        __syncthreads();
        mlp_forward<HP, NREG, 4, 1, 64, WR, 16, true>(P, wr, s_obsT, s_act, s_act + HP / 16 * 64, s_parts, s_ln, wave, lane STAMP_ARG, nullptr, 0, wofs);
        // (mlp_forward's closing barrier: s_parts is complete)
        const int row = tile * 16 + tid;
        if (tid < 16 && row < pe.n) eval_write_row<NCH>(P, s_parts, s_bhead, tid, row, pe.nd, value, dist, raw);
    }
}

// Workgroups per net (*groups): one per tile up to a cap under which every workgroup of the launch is resident at once, over all nets --
// n_cus x (workgroups of this instantiation a CU holds: 1 for the forms that fill the register file, 2 or 3 for the small ones) /
// n_nets, at least 1.  More would only read the weights again behind the first round; fewer leave CUs, or the latency-hiding second
// workgroup of a CU, unused.  AZG_EVAL_GROUPS=g replaces the cap (tests).
template <int HP, int NREG>
static hipError_t population_eval_launch(azg_engine* e, const PopEval& pe, int* groups) {
    auto kern = population_eval_kernel<HP, NREG>;
    const size_t lds = (size_t)2 * HP * 64;
    static KernelAttrs attrs;
    int per_cu = 1;
    hipError_t rc = attrs.occupancy(e, (const void*)kern, 256, lds, &per_cu);
    if (rc != hipSuccess) return rc;
    const int tiles = (pe.n + 15) / 16;
    int cap = e->opt.eval_groups > 0 ? e->opt.eval_groups : e->n_cus * (per_cu > 1 ? per_cu : 1) / e->n_nets;
    if (cap < 1) cap = 1;
    *groups = tiles < cap ? tiles : cap;
    hipLaunchKernelGGL(kern, dim3((unsigned)*groups, (unsigned)e->n_nets), dim3(256), lds, e->stream, e->P, pe);
    return hipGetLastError();
}
