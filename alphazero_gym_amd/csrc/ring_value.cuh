// ring_value.cuh -- the value head of every net of a population on the stored observations of its own rows of the replay ring, in the
// ring where they lie (azg_selfplay_refresh_values, include/azgym_refresh.h): population_eval_kernel's ring form.
// Grid (groups, n_nets): workgroup (g, k) reads net k's weights ONCE, exactly as population_eval_kernel does (population_eval.cuh: the
// first layer, and with NREG > 0 the hidden->hidden layers and the head, into registers; NREG == 0 streams the hidden layers, HP = 512 /
// 1024 the first layer too), and walks the 16-row tiles g, g + groups, ... of net k's work: the n_slots * T rows r = i * T + j, T = B /
// n_nets -- slot s = slots ? slots[i] : i, tree t = k * T + j, ring row s * B + t.  Per tile the rows' first S_obs columns go to LDS
// (tiles straddle slot boundaries; rows past the end are zero-filled), mlp_forward runs with population_eval_kernel's template arguments
// and LDS plan -- a row's value has the bits of azg_mlp_eval -- and lanes 0..15 of wave 0 store (double)V, V the float32 value of
// eval_write_row, to the kept value column at s * B + t.  Nothing else is written.  One writer per output (a slot listed twice is written
// twice with equal bits); no atomics, no waiting between workgroups.  Every index is a size_t: the rows are not bounded by 2^24 or 2^31.
#pragma once
#include "records.h"
#include "mlp.cuh"

struct RingValue {
    const float* rows;    // the ring [capacity][B][row_len]; a row's observation: its first S_obs columns
    double* value;        // the kept value column [capacity][B]
    const int* slots;     // [n_slots] ring slots, or NULL: slot i is i
    size_t n_slots;
    int B, T, row_len, S_obs;
};

template <int HP, int NREG>
__global__ __launch_bounds__(256, 1) void ring_value_kernel(KParams P, RingValue rv) {
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
    // this net's weights, read once (as population_eval_kernel)
    typedef WRegs<HP, NREG, 4> WR;
    WR wr;
    constexpr int NTW = HP / 64;
    if constexpr (HP <= 256) {
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
    const size_t T = (size_t)rv.T, B = (size_t)rv.B;
    const size_t n = rv.n_slots * T;          // this net's rows
    const size_t tiles = (n + 15) / 16;
    const size_t tree0 = (size_t)net * T;     // this net's first tree
#ifdef AZG_STAMPS
    unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    // (the trip count depends on blockIdx.x alone: every barrier below is reached by all four waves)
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // s_obsT of the previous tile was last read by mlp_forward's first layer, which every wave left before that call's closing barrier:
        // these stores come behind it
        if (tid < 128) {
            const int c = tid >> 4;
            const size_t r = tile * 16 + (size_t)(tid & 15);
            float x = 0.0f;
            if (r < n && c < rv.S_obs) {
                const size_t i = r / T, j = r - i * T;
                const size_t s = rv.slots ? (size_t)rv.slots[i] : i;
                x = rv.rows[(s * B + tree0 + j) * (size_t)rv.row_len + (size_t)c];
            }
            s_obsT[tid] = x;
        }
        // publishes s_obsT (and, in the first round, s_bhead) and protects s_parts: wave 0 arrives only after its epilogue of the previous
        // tile has read the head partials, and no wave stores new ones (the end of mlp_forward) before it has passed
        __syncthreads();
        mlp_forward<HP, NREG, 4, 1, 64, WR, 16, true>(P, wr, s_obsT, s_act, s_act + HP / 16 * 64, s_parts, s_ln, wave, lane STAMP_ARG, nullptr, 0, wofs);
        // (mlp_forward's closing barrier: s_parts is complete)
        const size_t r = tile * 16 + (size_t)tid;
        if (tid < 16 && r < n) {
            const size_t i = r / T, j = r - i * T;
            const size_t s = rv.slots ? (size_t)rv.slots[i] : i;
            const float V = head_output<NCH, 64>(s_parts, s_bhead, tid, 0);   // (eval_write_row's value)
            rv.value[s * B + tree0 + j] = (double)V;
        }
    }
}

// Workgroups per net (*groups): population_eval_launch's rule -- one per tile up to the cap under which every workgroup of the launch is
// resident at once over all nets; AZG_EVAL_GROUPS=g replaces the cap (tests).
template <int HP, int NREG>
static hipError_t ring_value_launch(azg_engine* e, const RingValue& rv, int* groups) {
    auto kern = ring_value_kernel<HP, NREG>;
    const size_t lds = (size_t)2 * HP * 64;
    static KernelAttrs attrs;
    int per_cu = 1;
    hipError_t rc = attrs.occupancy(e, (const void*)kern, 256, lds, &per_cu);
    if (rc != hipSuccess) return rc;
    const size_t tiles = (rv.n_slots * (size_t)rv.T + 15) / 16;
    int cap = e->opt.eval_groups > 0 ? e->opt.eval_groups : e->n_cus * (per_cu > 1 ? per_cu : 1) / e->n_nets;
    if (cap < 1) cap = 1;
    *groups = tiles < (size_t)cap ? (int)tiles : cap;
    hipLaunchKernelGGL(kern, dim3((unsigned)*groups, (unsigned)e->n_nets), dim3(256), lds, e->stream, e->P, rv);
    return hipGetLastError();
}
