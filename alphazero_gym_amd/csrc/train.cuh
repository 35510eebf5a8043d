// train.cuh -- population training (include/azgym_train.h): forward, backward and RMSprop step of K small MLPs on
// v_mfma_f32_16x16x4_f32.  Parameters are read in state_dict order straight from the caller's [K][P] array; activations live in
// the trainer's scratch (global memory, L2-resident at these sizes), so every GEMM operand is addressed as element (row, k) of some
// array and one routine (mma_strip) serves Z = A W^T, dA = dZ W and dW = dZ^T A.
//
// Summation order (fixed; no atomics): an output element is one accumulator chain, bias first, then the k-blocks of 16 in order;
// inside a block, MFMA step s = 0..3 adds the products of k = kk + s, kk + 4 + s, kk + 8 + s, kk + 12 + s (the four lane groups).
// For dW the k axis is the batch row, so batch tiles are summed in tile order.  db sums rows r = 0, 4, 8, ... / 1, 5, ... / 2, ... /
// 3, ... in four float64 chains, combined (s0 + s1) + (s2 + s3) and rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/azg_math.h"
#include "../../include/azgym.h"

typedef float tr_f32x4 __attribute__((ext_vector_type(4)));

#define TR_MAX_LAYERS 3
#define TR_OBS_LD 8          // observations are kept padded to 8 columns
#define TR_BWD_THREADS 1024

struct TrainDims {
    int n_layers, in_dim, nd, NO, act;
    int H[TR_MAX_LAYERS];
    int offW[TR_MAX_LAYERS], offb[TR_MAX_LAYERS];   // parameter offsets of the trunk layers
    int offWv;                                      // value_head.weight; head row o starts at offWv + o * HL + (o > 0)
    int offbv, offbd;                               // value_head.bias, dist_head.bias
    int P;
    // scratch of one net, in floats: obs [Bmax][8], per layer A_l [Bmax][H_l] and D_l [Bmax][H_l] (act'(Z_l), later dZ_l in place)
    unsigned s_obs, s_A[TR_MAX_LAYERS], s_D[TR_MAX_LAYERS];
    size_t per_net;
};

struct TrainOpt {
    float lr, alpha, one_minus_alpha, eps, wd;
};

// act'(z) with torch's conventions at the kinks (a = act(z))
__device__ __forceinline__ float tr_dact(int act, float z, float a) {
    switch (act) {
        case AZG_ACT_ELU: return z > 0.0f ? 1.0f : a + 1.0f;                 // exp(z) = expm1(z) + 1
        case AZG_ACT_LEAKYRELU: return z > 0.0f ? 1.0f : 0.01f;
        case AZG_ACT_RELU6: return (z > 0.0f && z < 6.0f) ? 1.0f : 0.0f;
        case AZG_ACT_SILU: { const float s = 1.0f / (1.0f + azg_expf(-z)); return s * (1.0f + z * (1.0f - s)); }
        case AZG_ACT_HARDSWISH: return z < -3.0f ? 0.0f : (z <= 3.0f ? z / 3.0f + 0.5f : 1.0f);
        default: return z > 0.0f ? 1.0f : 0.0f;
    }
}

// acc[t] += sum_k a(k) * b(t, k) for the wave's 16 x (16 * nt) strip.  fa(k): element (m0 + lane%16, k) of the left operand;
// fb(t, k): element (n0 + 16 t + lane%16, k) of the right one.  Result layout: acc[t][i] = C[m0 + 4 * (lane / 16) + i][n0 + 16 t + lane % 16].
template <int NT, class FA, class FB>
__device__ __forceinline__ void mma_strip(tr_f32x4 (&acc)[NT], int nt, int kdim, FA fa, FB fb, int g) {
    for (int kk = 0; kk < kdim; kk += 16) {
        const int k = kk + 4 * g;
        const float a0 = fa(k), a1 = fa(k + 1), a2 = fa(k + 2), a3 = fa(k + 3);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t < nt) {
                const float b0 = fb(t, k), b1 = fb(t, k + 1), b2 = fb(t, k + 2), b3 = fb(t, k + 3);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc[t], 0, 0, 0);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
// grid (row tiles, nets), one wave per workgroup: the wave carries its 16 rows through every layer, so nothing crosses waves.
__global__ __launch_bounds__(64) void train_forward_kernel(TrainDims d, const float* params, const float* obs, int n_rows, float* raw,
                                                           float* scratch) {
    const int net = blockIdx.y, m0 = blockIdx.x * 16, lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const float* p = params + (size_t)net * d.P;
    float* sc = scratch + (size_t)net * d.per_net;
    float* s_obs = sc + d.s_obs;
    for (int i = lane; i < 16 * TR_OBS_LD; i += 64) {
        const int row = m0 + i / TR_OBS_LD, c = i % TR_OBS_LD;
        s_obs[(size_t)row * TR_OBS_LD + c] = (row < n_rows && c < d.in_dim) ? obs[((size_t)net * n_rows + row) * d.in_dim + c] : 0.0f;
    }
    __syncthreads();
    const float* Ain = s_obs;
    int lda = TR_OBS_LD, kin = d.in_dim;
    for (int l = 0; l < d.n_layers; ++l) {
        const int H = d.H[l];
        const float* W = p + d.offW[l];
        const float* bias = p + d.offb[l];
        float* A = sc + d.s_A[l];
        float* D = sc + d.s_D[l];
        const float* arow = Ain + (size_t)(m0 + r) * lda;
        for (int n0 = 0; n0 < H; n0 += 64) {
            const int nt = (H - n0) >= 64 ? 4 : (H - n0) / 16;
            tr_f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float b = t < nt ? bias[n0 + 16 * t + r] : 0.0f;
                acc[t] = tr_f32x4{b, b, b, b};
            }
            mma_strip<4>(acc, nt, kin,
                         [&](int k) { return k < kin ? arow[k] : 0.0f; },
                         [&](int t, int k) { return k < kin ? W[(size_t)(n0 + 16 * t + r) * kin + k] : 0.0f; }, g);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < nt) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float z = acc[t][i], a = azg_activation(d.act, z);
                        const size_t at = (size_t)(m0 + 4 * g + i) * H + n0 + 16 * t + r;
                        A[at] = a;
                        D[at] = tr_dact(d.act, z, a);
                    }
                }
            }
        }
        __syncthreads();
        Ain = A; lda = H; kin = H;
    }
    // heads: output o = 0 is the value head, 1 .. nd the distribution head
    const int HL = kin, NO = d.NO;
    const float* Wh = p + d.offWv;
    const float* arow = Ain + (size_t)(m0 + r) * lda;
    const int nt = (NO + 15) / 16;
    tr_f32x4 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = 16 * t + r;
        const float b = o == 0 ? p[d.offbv] : (o < NO ? p[d.offbd + o - 1] : 0.0f);
        acc[t] = tr_f32x4{b, b, b, b};
    }
    mma_strip<2>(acc, nt, HL, [&](int k) { return arow[k]; },
                 [&](int t, int k) { const int o = 16 * t + r; return o < NO ? Wh[(size_t)o * HL + (o > 0) + k] : 0.0f; }, g);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = 16 * t + r;
        if (t < nt && o < NO) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m0 + 4 * g + i;
                if (row < n_rows) raw[((size_t)net * n_rows + row) * NO + o] = acc[t][i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward + RMSprop
// torch.optim.RMSprop (momentum 0, not centered) on one parameter, from its gradient
__device__ __forceinline__ void tr_update(const TrainOpt& o, float* p, float* sq, float* grads, int idx, float grad) {
    if (grads) grads[idx] = grad;
    const float pv = p[idx];
    float gd = grad;
    if (o.wd != 0.0f) gd = gd + o.wd * pv;
    const float s = o.alpha * sq[idx] + (o.one_minus_alpha * gd) * gd;
    sq[idx] = s;
    p[idx] = pv - o.lr * (gd / (__builtin_sqrtf(s) + o.eps));
}

// sum over rows of one column, x(row): four interleaved float64 chains combined (s0 + s1) + (s2 + s3), rounded to float32 once
// (a bias gradient is a plain sum of B float32 values: in float64 it is exact to the last bit for any B the trainer takes)
template <class F>
__device__ __forceinline__ float tr_colsum(int rows, F x) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int rr = 0;
    for (; rr + 4 <= rows; rr += 4) { s0 = s0 + (double)x(rr); s1 = s1 + (double)x(rr + 1); s2 = s2 + (double)x(rr + 2); s3 = s3 + (double)x(rr + 3); }
    if (rr < rows) s0 = s0 + (double)x(rr);
    if (rr + 1 < rows) s1 = s1 + (double)x(rr + 1);
    if (rr + 2 < rows) s2 = s2 + (double)x(rr + 2);
    return (float)((s0 + s1) + (s2 + s3));
}

// One workgroup per net.  Per layer, from the heads down: (a) dA of the layer below = dZ W, times act' -> dZ of the layer below
// (in place over D); barrier; (b) dW = dZ^T A_below, db, and the optimiser step of this layer's parameters.  (a) reads the layer's
// weights before the barrier and (b) writes them after it; (b) of one layer and (a) of the next touch different arrays.
__global__ __launch_bounds__(TR_BWD_THREADS) void train_backward_kernel(TrainDims d, TrainOpt opt, float* params, const float* d_raw, int n_rows,
                                                                        float* square_avg, float* grads_all, float* scratch) {
    const int net = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int NWV = TR_BWD_THREADS / 64;
    float* p = params + (size_t)net * d.P;
    float* sq = square_avg + (size_t)net * d.P;
    float* grads = grads_all ? grads_all + (size_t)net * d.P : nullptr;
    float* sc = scratch + (size_t)net * d.per_net;
    const int Bpad = (n_rows + 15) / 16 * 16, MT = Bpad / 16;
    const int L = d.n_layers, NO = d.NO, NOT = (NO + 15) / 16;
    const float* dr = d_raw + (size_t)net * n_rows * NO;
    auto dzh = [&](int row, int o) { return (row < n_rows && o < NO) ? dr[(size_t)row * NO + o] : 0.0f; };

    for (int l = L; l >= 0; --l) {
        const bool head = l == L;
        const int Hl = head ? NO : d.H[l];                      // outputs of this layer
        const int MTl = head ? NOT : Hl / 16;                   // ... in tiles
        const int Hp = l > 0 ? d.H[l - 1] : d.in_dim;           // inputs of this layer
        const float* Aprev = l > 0 ? sc + d.s_A[l - 1] : sc + d.s_obs;
        const int lda = l > 0 ? Hp : TR_OBS_LD;
        const float* dZ = head ? nullptr : sc + d.s_D[l];       // [Bpad][Hl]
        float* W = p + (head ? d.offWv : d.offW[l]);
        if (l > 0) {
            // (a) dZ_{l-1}[row][j] = D_{l-1}[row][j] * sum_u dZ_l[row][u] W_l[u][j]
            float* Dp = sc + d.s_D[l - 1];
            const int ns = (Hp + 63) / 64, kdim = head ? NOT * 16 : Hl;
            for (int s = wave; s < MT * ns; s += NWV) {
                const int m0 = (s / ns) * 16, n0 = (s % ns) * 64;
                const int nt = (Hp - n0) >= 64 ? 4 : (Hp - n0) / 16;
                tr_f32x4 acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = tr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (head)
                    mma_strip<4>(acc, nt, kdim, [&](int k) { return dzh(m0 + r, k); },
                                 [&](int t, int k) { return k < NO ? W[(size_t)k * Hp + (k > 0) + n0 + 16 * t + r] : 0.0f; }, g);
                else
                    mma_strip<4>(acc, nt, kdim, [&](int k) { return dZ[(size_t)(m0 + r) * Hl + k]; },
                                 [&](int t, int k) { return W[(size_t)k * Hp + n0 + 16 * t + r]; }, g);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t < nt) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const size_t at = (size_t)(m0 + 4 * g + i) * Hp + n0 + 16 * t + r;
                            Dp[at] = acc[t][i] * Dp[at];
                        }
                    }
                }
            }
            __syncthreads();
        }
        // (b) dW_l[u][j] = sum_row dZ_l[row][u] A_{l-1}[row][j]: the k axis is the batch row
        const int ns = (Hp + 63) / 64;
        for (int s = wave; s < MTl * ns; s += NWV) {
            const int m0 = (s / ns) * 16, n0 = (s % ns) * 64;
            const int nt = (Hp - n0) >= 64 ? 4 : (Hp - n0 + 15) / 16;
            tr_f32x4 acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = tr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            auto fb = [&](int t, int k) { const int j = n0 + 16 * t + r; return j < Hp ? Aprev[(size_t)k * lda + j] : 0.0f; };
            if (head) mma_strip<4>(acc, nt, Bpad, [&](int k) { return dzh(k, m0 + r); }, fb, g);
            else mma_strip<4>(acc, nt, Bpad, [&](int k) { return dZ[(size_t)k * Hl + m0 + r]; }, fb, g);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < nt) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int u = m0 + 4 * g + i, j = n0 + 16 * t + r;
                        if (u < Hl && j < Hp) {
                            const int idx = head ? d.offWv + u * Hp + (u > 0) + j : d.offW[l] + u * Hp + j;
                            tr_update(opt, p, sq, grads, idx, acc[t][i]);
                        }
                    }
                }
            }
        }
        for (int u = tid; u < Hl; u += TR_BWD_THREADS) {
            float gsum;
            if (head) gsum = tr_colsum(n_rows, [&](int row) { return dr[(size_t)row * NO + u]; });
            else gsum = tr_colsum(Bpad, [&](int row) { return dZ[(size_t)row * Hl + u]; });
            const int idx = head ? (u == 0 ? d.offbv : d.offbd + u - 1) : d.offb[l] + u;
            tr_update(opt, p, sq, grads, idx, gsum);
        }
    }
}
