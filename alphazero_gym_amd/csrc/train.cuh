// train.cuh -- population training (include/azgym_train.h): forward, backward and optimiser step (RMSprop fused into the backward
// pass; or Adam / RMSprop with gradient clipping as a phase after it) of K small MLPs on
// v_mfma_f32_16x16x4_f32.  Parameters are read in state_dict order straight from the caller's [K][P] array; activations live in
// the trainer's scratch (global memory, L2-resident at these sizes), so every GEMM operand is addressed as element (row, k) of some
// array and one routine (mma_strip) serves Z = A W^T, dA = dZ W and dW = dZ^T A.
//
// Summation order (fixed; no atomics): an output element is one accumulator chain, bias first, then the k-blocks of 16 in order;
// inside a block, MFMA step s = 0..3 adds the products of k = kk + s, kk + 4 + s, kk + 8 + s, kk + 12 + s (the four lane groups).
// For dW the k axis is the batch row, so batch tiles are summed in tile order.  db sums rows r = 0, 4, 8, ... / 1, 5, ... / 2, ... /
// 3, ... in four float64 chains, combined (s0 + s1) + (s2 + s3) and rounded once.
//
// LayerNorm trunks (the LN = true instantiations; azg_trainer_create_ex).  After trunk layer m's A = act(Z): X = (A - mean) * rstd,
// Y = X * gamma + beta; Y is what the next layer, the heads and dW read, and takes A's place in the scratch; X, rstd and
// G = dZ_{m+1} W_{m+1} (the gradient by Y) have arrays of their own.  Every sum over the H columns of a row -- the mean, the variance
// of the centred values (biased, eps 1e-5), and backward the means of dx = G * gamma and of dx * X -- has one order: sixteen
// consecutive lanes share the row, lane c of them adds columns c, c + 16, c + 32, ... in that order in one float64 chain from the
// float32 values (A, dx; A - mean and dx * X are formed in float64), and the sixteen partials are combined by a butterfly,
// s = s + s[lane ^ 1], then ^ 2, ^ 4, ^ 8: the tree ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) + ..., in which every lane
// ends with the same bits because each step adds the same two numbers on both sides.  The sum is divided by H in float64 and rounded
// to float32 once (the mean, rstd = 1 / sqrt(var + eps), and the two backward means); the elementwise X, Y, dx and
// dA = rstd * ((dx - m1) - X * m2) are float32.  Which wave owns a row differs between the forward and the backward kernel and with
// the row's number; which lane takes which column and how the partials meet does not, so it depends on neither K nor n_rows.
// dgamma = sum over rows of G * X (the products exact in float64) and dbeta = sum over rows of G are db's four float64 chains.
//
// train_loss_kernel (the losses between the two): one lane per row computes the row's loss terms and its d_raw in float64 from the
// float32 inputs (d_raw rounded once per element); the sums over the rows are the same four float64 chains, rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/azg_math.h"
#include "../../include/azgym.h"
#include "../../include/azgym_train.h"
#include "gather_row.cuh"

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

// The LN = true kernels' argument: TrainDims and what a LayerNorm trunk adds (the LN = false kernels keep taking TrainDims itself, so
// their argument block and their code stay what they were).
struct TrainDimsLN : TrainDims {
    int layernorm;                                  // the descriptor's flag (0: a trainer made by create_ex for a plain trunk)
    int offG[TR_MAX_LAYERS], offB[TR_MAX_LAYERS];   // ln.weight, ln.bias of the trunk layers
    // per layer X_l [Bmax][H_l], G_l [Bmax][H_l] (d loss / d Y_l) and rstd_l [Bmax]; with LayerNorm s_A holds Y_l
    unsigned s_X[TR_MAX_LAYERS], s_G[TR_MAX_LAYERS], s_R[TR_MAX_LAYERS];
};
template <bool LN> struct TrainDimsOf { typedef TrainDims type; };
template <> struct TrainDimsOf<true> { typedef TrainDimsLN type; };
#define TR_LN_EPS 1e-5

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
        case AZG_ACT_HARDSWISH: return z <= -3.0f ? 0.0f : (z < 3.0f ? z / 3.0f + 0.5f : 1.0f);   // 0 at -3 and 1 at 3, not -0.5 and 1.5
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

// The sum of s over the sixteen lanes that share a row (lanes 16 g .. 16 g + 15 of the wave): the butterfly of the header comment.
__device__ __forceinline__ double tr_row16_sum(double s) {
    s = s + __shfl_xor(s, 1);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 4);
    s = s + __shfl_xor(s, 8);
    return s;
}

// LayerNorm of one row after the layer's strips are stored: a[0 .. H) holds A and leaves holding Y; x receives X, *rstd_out rstd.
// Called by all sixteen lanes c = 0 .. 15 of the row's group.  A row of equal values (a padded row) has var = 0 and rstd =
// 1 / sqrt(eps): finite.
__device__ __forceinline__ void tr_ln_row_forward(int H, int c, float* a, float* x, float* rstd_out, const float* gam, const float* bet) {
    double s = 0.0;
    for (int j = c; j < H; j += 16) s = s + (double)a[j];
    const double mean = tr_row16_sum(s) / (double)H;
    double v = 0.0;
    for (int j = c; j < H; j += 16) { const double dc = (double)a[j] - mean; v = v + dc * dc; }
    const double var = tr_row16_sum(v) / (double)H;
    const float mf = (float)mean, rstd = (float)(1.0 / sqrt(var + TR_LN_EPS));
    for (int j = c; j < H; j += 16) {
        const float xv = (a[j] - mf) * rstd;
        x[j] = xv;
        a[j] = xv * gam[j] + bet[j];
    }
    if (c == 0) *rstd_out = rstd;
}

// ------------------------------------------------------------------------------------------------ forward
// grid (row tiles, nets), one wave per workgroup: the wave carries its 16 rows through every layer, so nothing crosses waves.
// LN: after a layer's strips are stored the wave makes the row pass over its own 16 rows, four rows at a time.
template <bool LN>
__global__ __launch_bounds__(64) void train_forward_kernel(typename TrainDimsOf<LN>::type d, const float* params, const float* obs, int n_rows,
                                                           float* raw, float* scratch) {
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
        if constexpr (LN) {
            for (int q = 0; q < 4; ++q) {
                const size_t row = (size_t)(m0 + 4 * q + g);
                tr_ln_row_forward(H, r, A + row * H, sc + d.s_X[l] + row * H, sc + d.s_R[l] + row, p + d.offG[l], p + d.offB[l]);
            }
            __syncthreads();
        }
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
__device__ __forceinline__ double tr_colsum64(int rows, F x) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int rr = 0;
    for (; rr + 4 <= rows; rr += 4) { s0 = s0 + (double)x(rr); s1 = s1 + (double)x(rr + 1); s2 = s2 + (double)x(rr + 2); s3 = s3 + (double)x(rr + 3); }
    if (rr < rows) s0 = s0 + (double)x(rr);
    if (rr + 1 < rows) s1 = s1 + (double)x(rr + 1);
    if (rr + 2 < rows) s2 = s2 + (double)x(rr + 2);
    return (s0 + s1) + (s2 + s3);
}
template <class F>
__device__ __forceinline__ float tr_colsum(int rows, F x) { return (float)tr_colsum64(rows, x); }

// One workgroup per net.  Per layer, from the heads down: (a) dA of the layer below = dZ W, times act' -> dZ of the layer below
// (in place over D); barrier; (b) dW = dZ^T A_below, db, and the optimiser step of this layer's parameters.  (a) reads the layer's
// weights before the barrier and (b) writes them after it; (b) of one layer and (a) of the next touch different arrays.
// LN: (a) stores G = dZ W instead; barrier; the row pass reads G, gamma, X, rstd and turns D into dZ of the layer below; then the
// barrier that was there.  (b) also emits dgamma and dbeta of the layer below from G and X, so gamma, like W, is read in front of a
// barrier and stepped behind it, and G, X of one layer are not written again in this launch.
template <bool LN>
__global__ __launch_bounds__(TR_BWD_THREADS) void train_backward_kernel(typename TrainDimsOf<LN>::type d, TrainOpt opt, float* params,
                                                                        const float* d_raw, int n_rows, float* square_avg, float* grads_all,
                                                                        float* scratch) {
#define TR_EMIT(idx, grad) tr_update(opt, p, sq, grads, idx, grad)
#include "train_backward_layers.inc"
#undef TR_EMIT
}

// ------------------------------------------------------------------------------------------------ backward, then the optimiser
// torch.optim.Adam's single-tensor step (no amsgrad, not capturable) of one element in float64 from its float32 state: weight decay
// into the gradient, exp_avg by lerp, exp_avg_sq, then p -= (lr / bc1) * exp_avg / (sqrt(exp_avg_sq) / bc2_sqrt + eps) with
// bc1 = 1 - beta1^t and bc2_sqrt = sqrt(1 - beta2^t) of the step t being taken (host, float64).  exp_avg and exp_avg_sq are rounded
// to float32 once and stored; the caller rounds and stores p.  The loss kernel's log_alpha and the deferred backward kernel's
// parameters both step through it.
__device__ __forceinline__ void tr_adam(double& p, float* exp_avg, float* exp_avg_sq, double g, double lr, double b1, double b2, double eps,
                                        double wd, double bc1, double bc2_sqrt) {
    if (wd != 0.0) g = g + wd * p;
    const double m0 = (double)*exp_avg;
    const double m = m0 + (g - m0) * (1.0 - b1);
    const double s = b2 * (double)*exp_avg_sq + (1.0 - b2) * g * g;
    p = p - (lr / bc1) * (m / (sqrt(s) / bc2_sqrt + eps));
    *exp_avg = (float)m; *exp_avg_sq = (float)s;
}

// The deferred form's optimiser settings (azg_optim as the kernel takes it).
struct TrainOptD {
    TrainOpt rms;                       // AZG_OPT_RMSPROP: tr_update's
    int kind, want_norm;                // AZG_OPT_*; compute the norm (grad_clip != 0 or grad_norms given)
    float clip;                         // 0: off
    double lr, b1, b2, eps, wd, bc1, bc2_sqrt;   // AZG_OPT_ADAM: tr_adam's
};

// The same walk through the layers, the same GEMMs in the same order, with every gradient element stored to grads_all [K][P] and
// no parameter written.  Then, behind a workgroup barrier (the workgroup's own global stores are complete and visible to its own
// later loads), the optimiser as a phase of its own, thread t taking elements t, t + 1024, ...:
//   norm    each thread sums (double)g * (double)g of its elements in one float64 chain (the products are exact); the 1024 partials
//           are added pairwise through LDS, partner t + 512, t + 256, ... t + 1: a fixed tree.  total_norm = (float)sqrt(sum).
//   clip    torch's clip_grad_norm_: coef = min(clip / (total_norm + 1e-6f), 1) in float32, every gradient times coef (coef == 1
//           included).  grads_all keeps the gradients as they were before clipping and weight decay.
//   update  tr_update (RMSprop, float32, the fused form's own) or tr_adam (float64, rounded once) of every element.
// state0: square_avg / exp_avg_sq, state1: exp_avg.  norms (may be NULL): total_norm of every net.
template <bool LN>
__global__ __launch_bounds__(TR_BWD_THREADS) void train_backward_deferred_kernel(typename TrainDimsOf<LN>::type d, TrainOptD o, float* params,
                                                                                 const float* d_raw, int n_rows, float* state0, float* state1,
                                                                                 float* grads_all, float* norms, float* scratch) {
    {
        float* square_avg = state0;
#define TR_EMIT(idx, grad) ((void)sq, grads[idx] = (grad))
#include "train_backward_layers.inc"
#undef TR_EMIT
    }
    // every wave's gradient stores have completed before any wave passes the barrier and loads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int net = blockIdx.x, tid = threadIdx.x, P = d.P;
    float* p = params + (size_t)net * P;
    float* s0 = state0 + (size_t)net * P;
    float* grads = grads_all + (size_t)net * P;
    float coef = 1.0f;
    if (o.want_norm) {
        __shared__ double part[TR_BWD_THREADS];
        double acc = 0.0;
        for (int i = tid; i < P; i += TR_BWD_THREADS) { const double gd = (double)grads[i]; acc = acc + gd * gd; }
        part[tid] = acc;
        __syncthreads();
        for (int st = TR_BWD_THREADS / 2; st > 0; st >>= 1) {
            if (tid < st) part[tid] = part[tid] + part[tid + st];
            __syncthreads();
        }
        const float total = (float)sqrt(part[0]);
        if (norms && tid == 0) norms[net] = total;
        if (o.clip != 0.0f) { const float c = o.clip / (total + 1e-6f); coef = c < 1.0f ? c : 1.0f; }
    }
    const bool clipped = o.clip != 0.0f;
    if (o.kind == AZG_OPT_ADAM) {
        float* s1 = state1 + (size_t)net * P;
        for (int i = tid; i < P; i += TR_BWD_THREADS) {
            float g = grads[i];
            if (clipped) g = g * coef;
            double pv = (double)p[i];
            tr_adam(pv, s1 + i, s0 + i, (double)g, o.lr, o.b1, o.b2, o.eps, o.wd, o.bc1, o.bc2_sqrt);
            p[i] = (float)pv;
        }
    } else {
        for (int i = tid; i < P; i += TR_BWD_THREADS) {
            float g = grads[i];
            if (clipped) g = g * coef;
            tr_update(o.rms, p, s0, nullptr, i, g);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the optimiser, settings per net
// The *_nets entry points: every net has its own TrainOptD, element (minibatch, net) of a table in device memory that the host
// filled before the first launch.  A workgroup copies its net's entry once at entry -- the address is the same in every lane -- and
// from there on runs the deferred form's text with that copy in the kernel argument's place, so net k ends with the bits a one-net
// launch with entry k gives.  The kernels above are not touched by it: the per-net forms have their own copy of the optimiser phase
// (tr_optim_span, shared by this header's and train_wide.cuh's per-net kernel).

// Norm tree, clip and update of the elements i0 .. i1 - 1 of one net, thread tid taking i0 + tid, i0 + tid + 1024, ...: the phase
// behind train_backward_deferred_kernel's barrier, operation for operation.  my_part: this thread's partial chain of the squared
// gradients (read only if o.want_norm).  write_norm: this workgroup stores the net's norm.
__device__ __forceinline__ void tr_optim_span(const TrainOptD& o, double my_part, bool write_norm, float* norm_out, float* p, float* s0,
                                              float* s1, const float* grads, int i0, int i1) {
    const int tid = threadIdx.x;
    float coef = 1.0f;
    if (o.want_norm) {
        __shared__ double part[TR_BWD_THREADS];
        part[tid] = my_part;
        __syncthreads();
        for (int st = TR_BWD_THREADS / 2; st > 0; st >>= 1) {
            if (tid < st) part[tid] = part[tid] + part[tid + st];
            __syncthreads();
        }
        const float total = (float)sqrt(part[0]);
        if (norm_out && write_norm && tid == 0) *norm_out = total;
        if (o.clip != 0.0f) { const float c = o.clip / (total + 1e-6f); coef = c < 1.0f ? c : 1.0f; }
    }
    const bool clipped = o.clip != 0.0f;
    if (o.kind == AZG_OPT_ADAM) {
        for (int i = i0 + tid; i < i1; i += TR_BWD_THREADS) {
            float g = grads[i];
            if (clipped) g = g * coef;
            double pv = (double)p[i];
            tr_adam(pv, s1 + i, s0 + i, (double)g, o.lr, o.b1, o.b2, o.eps, o.wd, o.bc1, o.bc2_sqrt);
            p[i] = (float)pv;
        }
    } else {
        for (int i = i0 + tid; i < i1; i += TR_BWD_THREADS) {
            float g = grads[i];
            if (clipped) g = g * coef;
            tr_update(o.rms, p, s0, nullptr, i, g);
        }
    }
}

// train_backward_deferred_kernel with the settings of net blockIdx.x from table[blockIdx.x].
template <bool LN>
__global__ __launch_bounds__(TR_BWD_THREADS) void train_backward_deferred_nets_kernel(typename TrainDimsOf<LN>::type d,
                                                                                      const TrainOptD* __restrict__ table, float* params,
                                                                                      const float* d_raw, int n_rows, float* state0,
                                                                                      float* state1, float* grads_all, float* norms,
                                                                                      float* scratch) {
    const TrainOptD o = table[blockIdx.x];
    {
        float* square_avg = state0;
#define TR_EMIT(idx, grad) ((void)sq, grads[idx] = (grad))
#include "train_backward_layers.inc"
#undef TR_EMIT
    }
    // every wave's gradient stores have completed before any wave passes the barrier and loads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int net = blockIdx.x, tid = threadIdx.x, P = d.P;
    const float* grads = grads_all + (size_t)net * P;
    double acc = 0.0;
    if (o.want_norm)
        for (int i = tid; i < P; i += TR_BWD_THREADS) { const double gd = (double)grads[i]; acc = acc + gd * gd; }
    tr_optim_span(o, acc, true, norms ? norms + net : nullptr, params + (size_t)net * P, state0 + (size_t)net * P,
                  state1 ? state1 + (size_t)net * P : nullptr, grads, 0, P);
}

// ------------------------------------------------------------------------------------------------ losses
// agent/population_trainer.py's population_terms / population_loss as one kernel: per row the summands of the losses and
// d loss_k / d raw by hand, then per net the reductions over the rows and, for the tuned loss, the Adam step of log_alpha.
#define TR_LOSS_THREADS 256
#define TR_MAX_ACTIONS 16
#define TR_MAX_COMP 5

struct LossDims {
    int kind, head, nd, C, A, squashed;
    float lmin, lmax;
    double tau;
    double bpe, corr, ladj0;         // SquashedNormal: bound + epsilon, 1 + epsilon / bound, x.shape[-1] * log(bound)
    double cP, cV, cE;               // d loss / d (a row's policy term, squared error, entropy term), alpha not included
    // the reductions (float64): policy_coeff, value_coeff, 1/B or 1, the entropy's reduction factor, 1/B, alpha, target entropy
    double pc, vc, red, ent_red, inv_rows, alpha, target;
    // Adam of log_alpha: bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step) of the step being taken
    double lr, b1, b2, eps, wd, clip, bc1, bc2_sqrt;
};

// torch's softplus (beta 1, threshold 20)
__device__ __forceinline__ double tr_softplus(double t) { return t > 20.0 ? t : log1p(exp(t)); }

// One row: terms[0] the policy summand, terms[1] the squared value error, terms[2] the entropy summand; d[0 .. nd] = d loss / d raw.
// z = raw + 1 is the distribution head.  The row's arithmetic is float64 from the float32 inputs, every sum over its actions and
// components a chain in index order; d is rounded to float32 once per element.  (In float32 the row terms carry the 2^-24 of expf /
// logf into sums that the float32 PyTorch path sometimes happens to hit exactly: DESIGN section 3.)
//
// WT (the weighted losses, azgym_train_weighted.h): the row's weight w multiplies every element of d in float64 before its one
// rounding, (float)(w * x) with x the value the WT = false form rounds; terms stay unweighted (the caller multiplies them).  w = 1 gives
// the WT = false bits: 1.0 * x is exact.
template <bool WT>
__device__ __forceinline__ float tr_round_w(double w, double x) {
    if constexpr (WT) return (float)(w * x);
    else return (float)x;
}
template <bool WT>
__device__ __forceinline__ void tr_loss_row_t(const LossDims& c, double alpha, const float* raw, const float* act, const float* cnt, float v,
                                              double w_row, float* d, double (&terms)[3]) {
    const double dv = (double)raw[0] - (double)v;
    terms[1] = dv * dv;
    d[0] = tr_round_w<WT>(w_row, c.cV * (2.0 * dv));
    const float* z = raw + 1;
    const double aE = alpha * c.cE;
    if (c.head == AZG_HEAD_DISCRETE) {
        const int n = c.nd;
        float mf = z[0];
        for (int j = 1; j < n; ++j) mf = z[j] > mf ? z[j] : mf;
        const double m = (double)mf;
        double se = 0.0;
        for (int j = 0; j < n; ++j) se = se + exp((double)z[j] - m);
        const double lse = m + log(se);
        if (c.kind == AZG_LOSS_ALPHAZERO) {
            int t = 0;   // argmax of softmax(counts) = argmax of counts, the lowest index among equals
            for (int i = 1; i < c.A; ++i) if (cnt[i] > cnt[t]) t = i;
            terms[0] = -((double)z[t] - lse);
            terms[2] = 0.0;
            for (int j = 0; j < n; ++j) d[1 + j] = tr_round_w<WT>(w_row, c.cP * (exp((double)z[j] - lse) - (j == t ? 1.0 : 0.0)));
            return;
        }
        // log pi_i = lsm[a_i]; W[j] = the sum of the detached factors w_i = log pi_i - tau log(counts_i + 1) of the actions i with a_i = j
        double W[TR_MAX_ACTIONS];
#pragma unroll
        for (int j = 0; j < TR_MAX_ACTIONS; ++j) W[j] = 0.0;
        double pol = 0.0, wsum = 0.0;
        for (int i = 0; i < c.A; ++i) {
            int idx = (int)act[i];
            idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
            const double lp = (double)z[idx] - lse;
            const double w = lp - c.tau * log((double)cnt[i] + 1.0);
            pol = pol + w * lp;
            wsum = wsum + w;
#pragma unroll
            for (int j = 0; j < TR_MAX_ACTIONS; ++j) W[j] = W[j] + (j == idx ? w : 0.0);
        }
        double H = 0.0;
        for (int j = 0; j < n; ++j) { const double l = (double)z[j] - lse; H = H - exp(l) * l; }
        terms[0] = pol;
        terms[2] = H;
#pragma unroll
        for (int j = 0; j < TR_MAX_ACTIONS; ++j) {
            if (j < n) {
                const double l = (double)z[j] - lse, pj = exp(l);
                d[1 + j] = tr_round_w<WT>(w_row, c.cP * (W[j] - pj * wsum) - aE * (pj * (l + H)));
            }
        }
        return;
    }
    // squashed Normal (C = 1) or mixture of C of them: z = mu[C] | log_std[C] ( | log_coeff[C])
    const int C = c.C;
    const bool gmm = c.head == AZG_HEAD_GMM;
    double mu[TR_MAX_COMP], ls[TR_MAX_COMP], iv[TR_MAX_COMP], lmix[TR_MAX_COMP];
    double dmu[TR_MAX_COMP], dls[TR_MAX_COMP], dlc[TR_MAX_COMP];
    bool gate[TR_MAX_COMP];
    float lcm = 0.0f;
    if (gmm) { lcm = z[2 * C]; for (int k = 1; k < C; ++k) lcm = z[2 * C + k] > lcm ? z[2 * C + k] : lcm; }
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < TR_MAX_COMP; ++k) {
        const bool on = k < C;
        mu[k] = on ? (double)z[k] : 0.0;
        const float l = on ? z[C + k] : 0.0f;
        gate[k] = l >= c.lmin && l <= c.lmax;               // torch.clamp passes the gradient inside [min, max], ends included
        ls[k] = (double)(l < c.lmin ? c.lmin : (l > c.lmax ? c.lmax : l));
        iv[k] = exp(-2.0 * ls[k]);                          // 1 / sigma^2
        lmix[k] = (on && gmm) ? (double)z[2 * C + k] - (double)lcm : 0.0;
        if (on && gmm) se = se + exp(lmix[k]);
        dmu[k] = 0.0; dls[k] = 0.0; dlc[k] = 0.0;
    }
    const double lse = gmm ? log(se) : 0.0;
#pragma unroll
    for (int k = 0; k < TR_MAX_COMP; ++k) lmix[k] = (k < C && gmm) ? lmix[k] - lse : 0.0;
    double pol = 0.0, lpsum = 0.0;
    const double inv_A = 1.0 / (double)c.A;
    for (int i = 0; i < c.A; ++i) {
        double x = (double)act[i], ladj = 0.0;
        if (c.squashed) {
            x = atanh(x / c.bpe);
            const double cx = c.corr * x;
            ladj = c.ladj0 + 2.0 * ((0.693147180559945286 - cx) - tr_softplus(-2.0 * cx));
        }
        double s[TR_MAX_COMP], sm = -1.0e300;
#pragma unroll
        for (int k = 0; k < TR_MAX_COMP; ++k) {
            const double dx = x - mu[k];
            s[k] = (((-0.5 * (dx * dx * iv[k]) - ls[k]) - 0.918938533204672742) - ladj) + lmix[k];
            if (k < C) sm = s[k] > sm ? s[k] : sm;
        }
        double lp = s[0];
        if (gmm) {
            double e = 0.0;
#pragma unroll
            for (int k = 0; k < TR_MAX_COMP; ++k) if (k < C) e = e + exp(s[k] - sm);
            lp = sm + log(e);
        }
        const double w = lp - c.tau * log((double)cnt[i]);
        pol = pol + w * lp;
        lpsum = lpsum + lp;
        const double g = c.cP * w - aE * inv_A;   // d loss / d log pi_i: the policy term's detached factor, the entropy's -1/A
#pragma unroll
        for (int k = 0; k < TR_MAX_COMP; ++k) {
            if (k < C) {
                const double r = gmm ? exp(s[k] - lp) : 1.0;   // the component's responsibility
                const double dx = x - mu[k], q = dx * dx * iv[k];
                dmu[k] = dmu[k] + g * r * (dx * iv[k]);
                dls[k] = dls[k] + g * r * (q - 1.0);
                dlc[k] = dlc[k] + g * (r - exp(lmix[k]));
            }
        }
    }
    terms[0] = pol;
    terms[2] = -lpsum * inv_A;
#pragma unroll
    for (int k = 0; k < TR_MAX_COMP; ++k) {
        if (k < C) {
            d[1 + k] = tr_round_w<WT>(w_row, dmu[k]);
            d[1 + C + k] = gate[k] ? tr_round_w<WT>(w_row, dls[k]) : 0.0f;
            if (gmm) d[1 + 2 * C + k] = tr_round_w<WT>(w_row, dlc[k]);
        }
    }
}

__device__ __forceinline__ void tr_loss_row(const LossDims& c, double alpha, const float* raw, const float* act, const float* cnt, float v,
                                            float* d, double (&terms)[3]) {
    tr_loss_row_t<false>(c, alpha, raw, act, cnt, v, 1.0, d, terms);
}

// (TR_NO_SHARED_KERNELS: a second translation unit that wants this header's device routines and templates, not another copy of the
// three plain kernels below -- dispatch_train_wide.hip)
#ifndef TR_NO_SHARED_KERNELS
// One workgroup per net, one lane per row (rows tid, tid + 256, ...).  rows: the trainer's float64 [n_nets][3][stride] array of the
// rows' terms.  log_alpha[net] is read by every lane before the first barrier and written by lane 0 after the second.
__global__ __launch_bounds__(TR_LOSS_THREADS) void train_loss_kernel(LossDims c, const float* raw, const float* actions, const float* counts,
                                                                     const float* values, int n_rows, float* log_alpha, float* exp_avg,
                                                                     float* exp_avg_sq, float* d_raw, float* losses, double* rows, int stride) {
    const int net = blockIdx.x, tid = threadIdx.x, NO = 1 + c.nd;
    const bool tuned = c.kind == AZG_LOSS_A0C_TUNED;
    const float la = tuned ? log_alpha[net] : 0.0f;
    const double alpha = tuned ? exp((double)la) : c.alpha;
    double* rw = rows + (size_t)net * 3 * stride;
    for (int row = tid; row < n_rows; row += TR_LOSS_THREADS) {
        const size_t at = (size_t)net * n_rows + row;
        double terms[3];
        tr_loss_row(c, alpha, raw + at * NO, actions + at * c.A, counts + at * c.A, values[at], d_raw + at * NO, terms);
        rw[row] = terms[0]; rw[stride + row] = terms[1]; rw[2 * stride + row] = terms[2];
    }
    __syncthreads();
    __shared__ double sums[3];
    if (tid < 3) sums[tid] = tr_colsum64(n_rows, [&](int r) { return rw[(size_t)tid * stride + r]; });
    __syncthreads();
    if (tid != 0) return;
    float* out = losses + (size_t)net * AZG_LOSS_SLOTS;
    const double policy = c.pc * (sums[0] * c.red), value = c.vc * (sums[1] * c.red);
    if (c.kind == AZG_LOSS_ALPHAZERO) {
        out[AZG_LOSS_TOTAL] = (float)(policy + value); out[AZG_LOSS_POLICY] = (float)policy; out[AZG_LOSS_VALUE] = (float)value;
        out[AZG_LOSS_ENTROPY] = 0.0f; out[AZG_LOSS_ALPHA] = 0.0f;
        return;
    }
    const double a = alpha;
    const double entropy = a * (sums[2] * c.ent_red);
    out[AZG_LOSS_TOTAL] = (float)((policy + entropy) + value); out[AZG_LOSS_POLICY] = (float)policy; out[AZG_LOSS_VALUE] = (float)value;
    out[AZG_LOSS_ENTROPY] = (float)entropy;
    if (!tuned) { out[AZG_LOSS_ALPHA] = 0.0f; return; }
    // alpha_loss = mean(exp(log_alpha) * (entropy - target).detach()); its derivative by log_alpha is itself
    const double alpha_loss = a * (sums[2] * c.inv_rows - c.target);
    out[AZG_LOSS_ALPHA] = (float)alpha_loss;
    double g = alpha_loss;
    if (c.clip != 0.0) { const double f = c.clip / (fabs(g) + 1e-6); g = g * (f < 1.0 ? f : 1.0); }
    double p = (double)la;
    tr_adam(p, exp_avg + net, exp_avg_sq + net, g, c.lr, c.b1, c.b2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    log_alpha[net] = (float)p;
}

// train_loss_kernel with the settings of net blockIdx.x from table[blockIdx.x] (azg_trainer_loss_nets; kind, head and the squashing
// are the same in every entry).  The entry is copied once at entry; what follows is train_loss_kernel's own text, kept as a copy so
// that the kernel above compiles to the code it always was.
__global__ __launch_bounds__(TR_LOSS_THREADS) void train_loss_nets_kernel(const LossDims* __restrict__ table, const float* raw,
                                                                          const float* actions, const float* counts, const float* values,
                                                                          int n_rows, float* log_alpha, float* exp_avg, float* exp_avg_sq,
                                                                          float* d_raw, float* losses, double* rows, int stride) {
    const LossDims c = table[blockIdx.x];
    const int net = blockIdx.x, tid = threadIdx.x, NO = 1 + c.nd;
    const bool tuned = c.kind == AZG_LOSS_A0C_TUNED;
    const float la = tuned ? log_alpha[net] : 0.0f;
    const double alpha = tuned ? exp((double)la) : c.alpha;
    double* rw = rows + (size_t)net * 3 * stride;
    for (int row = tid; row < n_rows; row += TR_LOSS_THREADS) {
        const size_t at = (size_t)net * n_rows + row;
        double terms[3];
        tr_loss_row(c, alpha, raw + at * NO, actions + at * c.A, counts + at * c.A, values[at], d_raw + at * NO, terms);
        rw[row] = terms[0]; rw[stride + row] = terms[1]; rw[2 * stride + row] = terms[2];
    }
    __syncthreads();
    __shared__ double sums[3];
    if (tid < 3) sums[tid] = tr_colsum64(n_rows, [&](int r) { return rw[(size_t)tid * stride + r]; });
    __syncthreads();
    if (tid != 0) return;
    float* out = losses + (size_t)net * AZG_LOSS_SLOTS;
    const double policy = c.pc * (sums[0] * c.red), value = c.vc * (sums[1] * c.red);
    if (c.kind == AZG_LOSS_ALPHAZERO) {
        out[AZG_LOSS_TOTAL] = (float)(policy + value); out[AZG_LOSS_POLICY] = (float)policy; out[AZG_LOSS_VALUE] = (float)value;
        out[AZG_LOSS_ENTROPY] = 0.0f; out[AZG_LOSS_ALPHA] = 0.0f;
        return;
    }
    const double a = alpha;
    const double entropy = a * (sums[2] * c.ent_red);
    out[AZG_LOSS_TOTAL] = (float)((policy + entropy) + value); out[AZG_LOSS_POLICY] = (float)policy; out[AZG_LOSS_VALUE] = (float)value;
    out[AZG_LOSS_ENTROPY] = (float)entropy;
    if (!tuned) { out[AZG_LOSS_ALPHA] = 0.0f; return; }
    const double alpha_loss = a * (sums[2] * c.inv_rows - c.target);
    out[AZG_LOSS_ALPHA] = (float)alpha_loss;
    double g = alpha_loss;
    if (c.clip != 0.0) { const double f = c.clip / (fabs(g) + 1e-6); g = g * (f < 1.0 ? f : 1.0); }
    double p = (double)la;
    tr_adam(p, exp_avg + net, exp_avg_sq + net, g, c.lr, c.b1, c.b2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    log_alpha[net] = (float)p;
}

// ------------------------------------------------------------------------------------------------ a whole epoch
// azg_trainer_epoch's two kernels: the minibatch gather in front of every step, and the sum of the steps' losses after the last.
#define TR_GATHER_THREADS 256

struct GatherDims : GatherRow {     // (gather_row.cuh: the row's layout and its copy)
    int group, n_order;
    long long group_stride, net_stride;
};

// grid (ceil(n_rows / 4), nets): one wave per minibatch row, lane c takes float c of the row, so a row is read as one coalesced
// segment.  The row's number and address are the same for every lane of the wave (one computation per row, on the scalar unit).
// Writes obs [nets][n_rows][state_dim], actions and counts [nets][n_rows][A] and values [nets][n_rows]; the Q columns are skipped.
__global__ __launch_bounds__(TR_GATHER_THREADS) void train_gather_kernel(GatherDims g, const float* rows, const int* order, int first,
                                                                         int n_rows, float* obs, float* actions, float* counts,
                                                                         float* values) {
    const int net = blockIdx.y, lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TR_GATHER_THREADS / 64) + (threadIdx.x >> 6)));
    if (b >= n_rows) return;
    const int i = __builtin_amdgcn_readfirstlane(order[(size_t)net * g.n_order + first + b]);
    const long long at = (long long)(i / g.group) * g.group_stride + (long long)net * g.net_stride + (long long)(i % g.group);
    const float* src = rows + at * g.row_len;
    const size_t out = (size_t)net * n_rows + b;
    gather_row(g, src, out, lane, obs, actions, counts, values);
}

// One thread per (net, slot): table [n_minibatches][n_nets * AZG_LOSS_SLOTS] float32 -> sums [n_nets * AZG_LOSS_SLOTS] float64, the
// minibatches added in order in one chain from 0.0 (what Python's 0.0 + l0 + l1 + ... of the steps' losses gives).
__global__ __launch_bounds__(64) void train_loss_sum_kernel(const float* table, int n_minibatches, int n, double* sums) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int m = 0; m < n_minibatches; ++m) s = s + (double)table[(size_t)m * n + e];
    sums[e] = s;
}
// ------------------------------------------------------------------------------------------------ weighted losses
// include/azgym_train_weighted.h: a float32 weight per minibatch row, weights [n_nets][n_rows], multiplies the row's summands and its
// d_raw in float64 before the reductions, which stay what they are.  rows: a float64 [n_nets][4][stride] array of the weighted path's
// own -- the three weighted terms and, fourth, the weight itself, whose sum S_w the tuned loss's alpha_loss needs:
// alpha * (S_wH / n - target * (S_w / n)).  train_loss_kernel's text with those changes; weights of 1.0f give its bits (every product
// with 1.0 is exact and S_w / n is 1).
//
// ERR (include/azgym_train_errors.h): the row's value error e = (float)fabs((double)raw[0] - (double)z), the first two operations of
// tr_loss_row_t, also goes to errors[err_at[at]] -- err_at [n_nets][n_rows]: the element the epoch's gather staged beside the row -- or,
// with err_at NULL, to the dense errors[at]; and NULL weights stand for weights of 1.0f.  ERR = false is the text as it was: the two
// weighted kernels below compile to the code they had.
template <bool ERR>
__device__ __forceinline__ void tr_loss_weighted_body(const LossDims& c, const float* raw, const float* actions, const float* counts,
                                                      const float* values, const float* weights, int n_rows, float* log_alpha,
                                                      float* exp_avg, float* exp_avg_sq, float* d_raw, float* losses, double* rows,
                                                      int stride, const long long* err_at = nullptr, float* errors = nullptr) {
    const int net = blockIdx.x, tid = threadIdx.x, NO = 1 + c.nd;
    const bool tuned = c.kind == AZG_LOSS_A0C_TUNED;
    const float la = tuned ? log_alpha[net] : 0.0f;
    const double alpha = tuned ? exp((double)la) : c.alpha;
    double* rw = rows + (size_t)net * 4 * stride;
    for (int row = tid; row < n_rows; row += TR_LOSS_THREADS) {
        const size_t at = (size_t)net * n_rows + row;
        double w;
        if constexpr (ERR) {
            w = weights ? (double)weights[at] : 1.0;
            errors[err_at ? (size_t)err_at[at] : at] = (float)fabs((double)raw[at * NO] - (double)values[at]);
        } else {
            w = (double)weights[at];
        }
        double terms[3];
        tr_loss_row_t<true>(c, alpha, raw + at * NO, actions + at * c.A, counts + at * c.A, values[at], w, d_raw + at * NO, terms);
        rw[row] = w * terms[0]; rw[stride + row] = w * terms[1]; rw[2 * stride + row] = w * terms[2]; rw[3 * (size_t)stride + row] = w;
    }
    __syncthreads();
    __shared__ double sums[4];
    if (tid < 4) sums[tid] = tr_colsum64(n_rows, [&](int r) { return rw[(size_t)tid * stride + r]; });
    __syncthreads();
    if (tid != 0) return;
    float* out = losses + (size_t)net * AZG_LOSS_SLOTS;
    const double policy = c.pc * (sums[0] * c.red), value = c.vc * (sums[1] * c.red);
    if (c.kind == AZG_LOSS_ALPHAZERO) {
        out[AZG_LOSS_TOTAL] = (float)(policy + value); out[AZG_LOSS_POLICY] = (float)policy; out[AZG_LOSS_VALUE] = (float)value;
        out[AZG_LOSS_ENTROPY] = 0.0f; out[AZG_LOSS_ALPHA] = 0.0f;
        return;
    }
    const double a = alpha;
    const double entropy = a * (sums[2] * c.ent_red);
    out[AZG_LOSS_TOTAL] = (float)((policy + entropy) + value); out[AZG_LOSS_POLICY] = (float)policy; out[AZG_LOSS_VALUE] = (float)value;
    out[AZG_LOSS_ENTROPY] = (float)entropy;
    if (!tuned) { out[AZG_LOSS_ALPHA] = 0.0f; return; }
    // alpha_loss = mean(exp(log_alpha) * w * (entropy - target).detach())
    const double alpha_loss = a * (sums[2] * c.inv_rows - c.target * (sums[3] / (double)n_rows));
    out[AZG_LOSS_ALPHA] = (float)alpha_loss;
    double g = alpha_loss;
    if (c.clip != 0.0) { const double f = c.clip / (fabs(g) + 1e-6); g = g * (f < 1.0 ? f : 1.0); }
    double p = (double)la;
    tr_adam(p, exp_avg + net, exp_avg_sq + net, g, c.lr, c.b1, c.b2, c.eps, c.wd, c.bc1, c.bc2_sqrt);
    log_alpha[net] = (float)p;
}

__global__ __launch_bounds__(TR_LOSS_THREADS) void train_loss_weighted_kernel(LossDims c, const float* raw, const float* actions,
                                                                              const float* counts, const float* values, const float* weights,
                                                                              int n_rows, float* log_alpha, float* exp_avg, float* exp_avg_sq,
                                                                              float* d_raw, float* losses, double* rows, int stride) {
    tr_loss_weighted_body<false>(c, raw, actions, counts, values, weights, n_rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, rows, stride);
}

// ... with the settings of net blockIdx.x from table[blockIdx.x] (the *_nets_weighted entry points)
__global__ __launch_bounds__(TR_LOSS_THREADS) void train_loss_nets_weighted_kernel(const LossDims* __restrict__ table, const float* raw,
                                                                                   const float* actions, const float* counts,
                                                                                   const float* values, const float* weights, int n_rows,
                                                                                   float* log_alpha, float* exp_avg, float* exp_avg_sq,
                                                                                   float* d_raw, float* losses, double* rows, int stride) {
    const LossDims c = table[blockIdx.x];
    tr_loss_weighted_body<false>(c, raw, actions, counts, values, weights, n_rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, rows, stride);
}

// train_gather_kernel, and the wave that copies row `at` also stages weights[at] -- the weight array is addressed like the rows with
// a row length of 1 -- into wout [nets][n_rows].
__global__ __launch_bounds__(TR_GATHER_THREADS) void train_gather_weighted_kernel(GatherDims g, const float* rows, const float* weights,
                                                                                  const int* order, int first, int n_rows, float* obs,
                                                                                  float* actions, float* counts, float* values, float* wout) {
    const int net = blockIdx.y, lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TR_GATHER_THREADS / 64) + (threadIdx.x >> 6)));
    if (b >= n_rows) return;
    const int i = __builtin_amdgcn_readfirstlane(order[(size_t)net * g.n_order + first + b]);
    const long long at = (long long)(i / g.group) * g.group_stride + (long long)net * g.net_stride + (long long)(i % g.group);
    const float* src = rows + at * g.row_len;
    const size_t out = (size_t)net * n_rows + b;
    gather_row(g, src, out, lane, obs, actions, counts, values);
    if (lane == 0) wout[out] = weights[at];
}

// ------------------------------------------------------------------------------------------------ value errors out of the loss launch
// include/azgym_train_errors.h: the weighted loss kernels' ERR = true forms (weights may be NULL), and the gather that stages each
// row's element index `at` -- where its error goes in an array addressed like the rows with a row length of 1 -- beside the row.
__global__ __launch_bounds__(TR_LOSS_THREADS) void train_loss_errors_kernel(LossDims c, const float* raw, const float* actions,
                                                                            const float* counts, const float* values, const float* weights,
                                                                            int n_rows, float* log_alpha, float* exp_avg, float* exp_avg_sq,
                                                                            float* d_raw, float* losses, double* rows, int stride,
                                                                            const long long* err_at, float* errors) {
    tr_loss_weighted_body<true>(c, raw, actions, counts, values, weights, n_rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, rows, stride,
                                err_at, errors);
}

__global__ __launch_bounds__(TR_LOSS_THREADS) void train_loss_nets_errors_kernel(const LossDims* __restrict__ table, const float* raw,
                                                                                 const float* actions, const float* counts,
                                                                                 const float* values, const float* weights, int n_rows,
                                                                                 float* log_alpha, float* exp_avg, float* exp_avg_sq,
                                                                                 float* d_raw, float* losses, double* rows, int stride,
                                                                                 const long long* err_at, float* errors) {
    const LossDims c = table[blockIdx.x];
    tr_loss_weighted_body<true>(c, raw, actions, counts, values, weights, n_rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, rows, stride,
                                err_at, errors);
}

// train_gather_weighted_kernel, and the wave also stages `at` into at_out [nets][n_rows]; NULL weights stage 1.0f.
__global__ __launch_bounds__(TR_GATHER_THREADS) void train_gather_errors_kernel(GatherDims g, const float* rows, const float* weights,
                                                                                const int* order, int first, int n_rows, float* obs,
                                                                                float* actions, float* counts, float* values, float* wout,
                                                                                long long* at_out) {
    const int net = blockIdx.y, lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TR_GATHER_THREADS / 64) + (threadIdx.x >> 6)));
    if (b >= n_rows) return;
    const int i = __builtin_amdgcn_readfirstlane(order[(size_t)net * g.n_order + first + b]);
    const long long at = (long long)(i / g.group) * g.group_stride + (long long)net * g.net_stride + (long long)(i % g.group);
    const float* src = rows + at * g.row_len;
    const size_t out = (size_t)net * n_rows + b;
    gather_row(g, src, out, lane, obs, actions, counts, values);
    if (lane == 0) { wout[out] = weights ? weights[at] : 1.0f; at_out[out] = at; }
}
#endif  // TR_NO_SHARED_KERNELS
