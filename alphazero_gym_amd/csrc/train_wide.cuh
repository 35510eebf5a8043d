// train_wide.cuh -- the population trainer's kernels for nets beyond train.cuh's one-wave / one-workgroup forms: 1..8 hidden layers of
// widths up to 1024 (azg_trainer_create_wide).  A layer is one launch whose grid spreads (row tiles x column strips x nets) over the
// chip, one wave per strip; the hand-offs between layers are kernel boundaries on the trainer's stream (no grid-wide barrier, no
// spin wait, no atomics).  Scratch layout, parameter order and the arithmetic are train.cuh's: every output element is the same
// accumulator chain through the same mma_strip, db is tr_colsum, an element is stepped by tr_update / tr_adam, and the deferred form's
// norm is the same 1024 float64 chains and the same pairwise tree.  Which wave owns a strip and how many tiles a strip has change no
// bit, so a shape both trainers accept gives the bits of train.cuh's kernels, whatever n_nets.
//
// Launches of one step (L hidden layers): forward L + 1 (the layers, the heads); backward 2 L + 1: from the heads down, (a) dZ of
// the layer below, then (b) dW, db and the optimiser step (or the gradient store) of the layer.  (a) of layer l reads W_l and (b) of
// layer l rewrites it, in the next launch.  Deferred form: + the norm's partial chains (when a norm is wanted) + the update.
//
// LayerNorm trunks (azg_trainer_create_wide_ex; the LN = true instantiations and the two row-pass kernels): train.cuh's LayerNorm
// arithmetic with a launch where its kernels have a barrier.  Forward 2 L + 1: behind every layer's launch a row pass, sixteen lanes
// per row running tr_ln_row_forward itself, leaves Y in A's place and X, rstd in arrays of their own.  Backward 3 L + 1: per layer,
// from the heads down, (a) of layer l stores G = dZ_l W_l; the row pass of LayerNorm l - 1 reads G, gamma, X and rstd and turns D into
// dZ of the layer below; (b) of layer l also emits dgamma and dbeta of LayerNorm l - 1 from G and X in workgroups beside db's.  In this
// order gamma of layer l - 1, like W_l, is read in a launch before the one that steps it, and G, X of a layer are written once per
// step.  A row's sums keep train.cuh's order at every width: lane c of the row's sixteen adds columns c, c + 16, ... in one float64
// chain (64 links at width 1024), the partials meet in tr_row16_sum, one division by H and one rounding.
#pragma once
#include "train.cuh"

#define TW_MAX_LAYERS AZG_MAX_HIDDEN_LAYERS
#define TW_THREADS 256                 // four waves, one strip each
#define TW_WAVES (TW_THREADS / 64)
#define TW_NORM_CHAINS TR_BWD_THREADS  // the deferred norm's partial chains: train.cuh's one per thread of its workgroup
#define TW_UPDATE_SPAN 4096            // elements of one net that a workgroup of the update kernel steps
#define TW_ROW_AHEAD 8                 // links of a lane's row chain whose loads the backward row pass issues ahead of their additions

// the strip of wave `s`: row tile m0, first column n0, nt tiles of the `cols` columns (cols need not be a multiple of 16: dW_0)
template <int NT>
__device__ __forceinline__ void tw_strip_of(int s, int cols, int& m0, int& n0, int& nt) {
    const int ns = (cols + 16 * NT - 1) / (16 * NT);
    m0 = (s / ns) * 16;
    n0 = (s % ns) * (16 * NT);
    const int rem = (cols - n0 + 15) / 16;
    nt = rem >= NT ? NT : rem;
}

// ------------------------------------------------------------------------------------------------ forward
struct TwFwd {
    int H, kin, lda, in_dim, act, first;   // first: the layer reads the caller's obs (and leaves its padded copy in the scratch)
    int offW, offb, P;
    unsigned s_in, s_A, s_D;
    size_t per_net;
};

// grid (ceil(row tiles * strips / 4), nets): Z = A_in W^T + b, A = act(Z), D = act'(Z) of one layer.
template <int NT>
__global__ __launch_bounds__(TW_THREADS) void train_wide_forward_kernel(TwFwd a, const float* params, const float* obs, int n_rows,
                                                                        float* scratch) {
    const int net = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int MT = (n_rows + 15) / 16, H = a.H, kin = a.kin;
    const int s = blockIdx.x * TW_WAVES + wave;
    if (s >= MT * ((H + 16 * NT - 1) / (16 * NT))) return;
    int m0, n0, nt;
    tw_strip_of<NT>(s, H, m0, n0, nt);
    const float* p = params + (size_t)net * a.P;
    float* sc = scratch + (size_t)net * a.per_net;
    const float* W = p + a.offW;
    const float* bias = p + a.offb;
    float* A = sc + a.s_A;
    float* D = sc + a.s_D;
    tr_f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float b = t < nt ? bias[n0 + 16 * t + r] : 0.0f;
        acc[t] = tr_f32x4{b, b, b, b};
    }
    auto fb = [&](int t, int k) { return k < kin ? W[(size_t)(n0 + 16 * t + r) * kin + k] : 0.0f; };
    if (a.first) {
        const float* ob = obs + (size_t)net * n_rows * a.in_dim;
        if (n0 == 0) {   // the row tile's observations, padded to 8 columns and 16 rows: what dW of this layer reads
            float* s_obs = sc + a.s_in;
            for (int i = lane; i < 16 * TR_OBS_LD; i += 64) {
                const int row = m0 + i / TR_OBS_LD, c = i % TR_OBS_LD;
                s_obs[(size_t)row * TR_OBS_LD + c] = (row < n_rows && c < a.in_dim) ? ob[(size_t)row * a.in_dim + c] : 0.0f;
            }
        }
        const bool live = m0 + r < n_rows;
        const float* orow = ob + (size_t)(m0 + r) * a.in_dim;
        mma_strip<NT>(acc, nt, kin, [&](int k) { return (live && k < kin) ? orow[k] : 0.0f; }, fb, g);
    } else {
        const float* arow = sc + a.s_in + (size_t)(m0 + r) * a.lda;
        mma_strip<NT>(acc, nt, kin, [&](int k) { return arow[k]; }, fb, g);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float z = acc[t][i], av = azg_activation(a.act, z);
                const size_t at = (size_t)(m0 + 4 * g + i) * H + n0 + 16 * t + r;
                A[at] = av;
                D[at] = tr_dact(a.act, z, av);
            }
        }
    }
}

// The row pass of one LayerNorm, forward or backward: H columns, Bpad rows.
struct TwRow {
    int H, P;
    int offG, offB;
    unsigned s_A, s_D, s_X, s_G, s_R;
    size_t per_net;
};

// grid (row tiles, nets): wave w of the workgroup takes rows m0 + 4 w .. m0 + 4 w + 3, sixteen lanes each (padded rows included: a
// tile's sixteen rows lie below the padded row count together, so all 64 lanes of a wave meet in the butterfly).  A -> Y in place,
// X and rstd to their arrays: tr_ln_row_forward as train_forward_kernel<true> calls it.
__global__ __launch_bounds__(TW_THREADS) void train_wide_ln_forward_kernel(TwRow a, const float* params, float* scratch) {
    const int net = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const size_t row = (size_t)blockIdx.x * 16 + 4 * wave + g;
    const float* p = params + (size_t)net * a.P;
    float* sc = scratch + (size_t)net * a.per_net;
    tr_ln_row_forward(a.H, r, sc + a.s_A + row * a.H, sc + a.s_X + row * a.H, sc + a.s_R + row, p + a.offG, p + a.offB);
}

struct TwHead {
    int HL, NO, P;
    int offWv, offbv, offbd;
    unsigned s_in;
    size_t per_net;
};

// grid (row tiles, nets), one wave: output o = 0 is the value head, 1 .. nd the distribution head
__global__ __launch_bounds__(64) void train_wide_heads_kernel(TwHead a, const float* params, int n_rows, float* raw, const float* scratch) {
    const int net = blockIdx.y, m0 = blockIdx.x * 16, lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const float* p = params + (size_t)net * a.P;
    const int HL = a.HL, NO = a.NO;
    const float* Wh = p + a.offWv;
    const float* arow = scratch + (size_t)net * a.per_net + a.s_in + (size_t)(m0 + r) * HL;
    const int nt = (NO + 15) / 16;
    tr_f32x4 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = 16 * t + r;
        const float b = o == 0 ? p[a.offbv] : (o < NO ? p[a.offbd + o - 1] : 0.0f);
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

// ------------------------------------------------------------------------------------------------ backward
// One layer l of train_backward_layers.inc's walk (head: l = L, whose dZ is the caller's d_raw and whose weights are the two head
// matrices).  Hl / Hp: outputs / inputs of the layer.
struct TwBwd {
    int head, Hl, Hp, lda, NO, P;
    int offW, offb;          // trunk layer; the head's are offWv, offbv, offbd
    int offWv, offbv, offbd;
    int strip_blocks;        // (b): workgroups of the dW role; the rest take db
    unsigned s_dZ, s_Dp, s_Ap;
    size_t per_net;
};
// The LN = true forms' argument: TwBwd and the LayerNorm below the layer (the LN = false forms keep taking TwBwd itself, so their
// argument block and their code stay what they were).
struct TwBwdLN : TwBwd {
    int offGp, offBp;        // ln.weight, ln.bias of LayerNorm l - 1
    unsigned s_Gp, s_Xp;     // G_{l-1}, X_{l-1}
};
template <bool LN> struct TwBwdOf { typedef TwBwd type; };
template <> struct TwBwdOf<true> { typedef TwBwdLN type; };

// (a) grid (ceil(row tiles * strips / 4), nets): dZ_{l-1}[row][j] = D_{l-1}[row][j] * sum_u dZ_l[row][u] W_l[u][j]
// LN: G_{l-1}[row][j] = the sum alone (padded rows: dZ_l is 0 there, so their G is 0); the row pass below makes dZ_{l-1} of it.
template <int NT, bool LN = false>
__global__ __launch_bounds__(TW_THREADS) void train_wide_backward_a_kernel(typename TwBwdOf<LN>::type a, const float* params,
                                                                           const float* d_raw, int n_rows, float* scratch) {
    const int net = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int MT = (n_rows + 15) / 16, Hl = a.Hl, Hp = a.Hp, NO = a.NO;
    const int s = blockIdx.x * TW_WAVES + wave;
    if (s >= MT * ((Hp + 16 * NT - 1) / (16 * NT))) return;
    int m0, n0, nt;
    tw_strip_of<NT>(s, Hp, m0, n0, nt);
    const float* p = params + (size_t)net * a.P;
    float* sc = scratch + (size_t)net * a.per_net;
    float* Dp = sc + a.s_Dp;
    tr_f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = tr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (a.head) {
        const float* W = p + a.offWv;
        const float* dr = d_raw + (size_t)net * n_rows * NO;
        auto dzh = [&](int row, int o) { return (row < n_rows && o < NO) ? dr[(size_t)row * NO + o] : 0.0f; };
        mma_strip<NT>(acc, nt, (NO + 15) / 16 * 16, [&](int k) { return dzh(m0 + r, k); },
                      [&](int t, int k) { return k < NO ? W[(size_t)k * Hp + (k > 0) + n0 + 16 * t + r] : 0.0f; }, g);
    } else {
        const float* W = p + a.offW;
        const float* dZ = sc + a.s_dZ;
        mma_strip<NT>(acc, nt, Hl, [&](int k) { return dZ[(size_t)(m0 + r) * Hl + k]; },
                      [&](int t, int k) { return W[(size_t)k * Hp + n0 + 16 * t + r]; }, g);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t at = (size_t)(m0 + 4 * g + i) * Hp + n0 + 16 * t + r;
                if constexpr (LN) sc[a.s_Gp + at] = acc[t][i];
                else Dp[at] = acc[t][i] * Dp[at];
            }
        }
    }
}

// The row pass of LayerNorm l - 1, grid (row tiles, nets), rows to waves as in train_wide_ln_forward_kernel: the loop of
// train_backward_layers.inc restated, element for element and link for link (m1, m2 float64 chains rounded once; dA float32),
// D_{l-1} -> dZ_{l-1} in place.
__global__ __launch_bounds__(TW_THREADS) void train_wide_ln_backward_kernel(TwRow a, const float* params, float* scratch) {
    const int net = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int Hp = a.H;
    const size_t row = (size_t)blockIdx.x * 16 + 4 * wave + g;
    float* sc = scratch + (size_t)net * a.per_net;
    const float* gam = params + (size_t)net * a.P + a.offG;
    const float* Gp = sc + a.s_G;
    const float* Xp = sc + a.s_X;
    float* Dp = sc + a.s_D;
    const size_t base = row * Hp;
    // (a lane's links in the same order, the loads of eight of them issued ahead of their additions: at width 1024 a chain is 64
    // links, and one load round trip per link is what this launch would otherwise take)
    double s1 = 0.0, s2 = 0.0;
    int j = r;
    for (; j + 16 * (TW_ROW_AHEAD - 1) < Hp; j += 16 * TW_ROW_AHEAD) {
        float dx[TW_ROW_AHEAD], xv[TW_ROW_AHEAD];
#pragma unroll
        for (int q = 0; q < TW_ROW_AHEAD; ++q) { dx[q] = Gp[base + j + 16 * q] * gam[j + 16 * q]; xv[q] = Xp[base + j + 16 * q]; }
#pragma unroll
        for (int q = 0; q < TW_ROW_AHEAD; ++q) { s1 = s1 + (double)dx[q]; s2 = s2 + (double)dx[q] * (double)xv[q]; }
    }
    for (; j < Hp; j += 16) {
        const float dx = Gp[base + j] * gam[j];
        s1 = s1 + (double)dx;
        s2 = s2 + (double)dx * (double)Xp[base + j];
    }
    const float m1 = (float)(tr_row16_sum(s1) / (double)Hp), m2 = (float)(tr_row16_sum(s2) / (double)Hp);
    const float rstd = sc[a.s_R + row];
    j = r;
    for (; j + 16 * (TW_ROW_AHEAD - 1) < Hp; j += 16 * TW_ROW_AHEAD) {
        float dA[TW_ROW_AHEAD], dv[TW_ROW_AHEAD];
#pragma unroll
        for (int q = 0; q < TW_ROW_AHEAD; ++q) {
            const float dx = Gp[base + j + 16 * q] * gam[j + 16 * q];
            dA[q] = rstd * ((dx - m1) - Xp[base + j + 16 * q] * m2);
            dv[q] = Dp[base + j + 16 * q];
        }
#pragma unroll
        for (int q = 0; q < TW_ROW_AHEAD; ++q) Dp[base + j + 16 * q] = dA[q] * dv[q];
    }
    for (; j < Hp; j += 16) {
        const float dx = Gp[base + j] * gam[j];
        const float dA = rstd * ((dx - m1) - Xp[base + j] * m2);
        Dp[base + j] = dA * Dp[base + j];
    }
}

// (b) grid (strip_blocks + ceil(Hl / 256), nets): dW_l[u][j] = sum_row dZ_l[row][u] A_{l-1}[row][j] (the k axis is the batch row) in the
// first strip_blocks workgroups, db_l[u] one thread per column in the rest.  FUSED: every finished element is stepped by tr_update
// (and stored to grads when given); else it is stored to grads and no parameter is written.
// LN (layers above the first): behind db's workgroups ceil(Hp / 256) more for dgamma and as many for dbeta of LayerNorm l - 1, one
// thread per column: the sums over the rows of G X (the products exact in float64) and of G, through tr_colsum into the same emit.
template <int NT, bool FUSED, bool LN = false>
__global__ __launch_bounds__(TW_THREADS) void train_wide_backward_b_kernel(typename TwBwdOf<LN>::type a, TrainOpt opt, float* params,
                                                                           const float* d_raw, int n_rows, float* square_avg,
                                                                           float* grads_all, const float* scratch) {
    const int net = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int Bpad = (n_rows + 15) / 16 * 16, Hl = a.Hl, Hp = a.Hp, NO = a.NO;
    const bool head = a.head != 0;
    float* p = params + (size_t)net * a.P;
    float* sq = FUSED ? square_avg + (size_t)net * a.P : nullptr;
    float* grads = grads_all ? grads_all + (size_t)net * a.P : nullptr;
    const float* sc = scratch + (size_t)net * a.per_net;
    const float* dr = d_raw + (size_t)net * n_rows * NO;
    const float* dZ = sc + a.s_dZ;
    auto emit = [&](int idx, float grad) {
        if constexpr (FUSED) tr_update(opt, p, sq, grads, idx, grad);
        else grads[idx] = grad;
    };
    if ((int)blockIdx.x >= a.strip_blocks) {
        if constexpr (LN) {
            const int nb = (Hl + TW_THREADS - 1) / TW_THREADS, ng = (Hp + TW_THREADS - 1) / TW_THREADS;
            const int blk = (int)blockIdx.x - a.strip_blocks - nb;
            if (blk >= 0) {
                const bool beta = blk >= ng;
                const int j = (beta ? blk - ng : blk) * TW_THREADS + tid;
                if (j >= Hp) return;
                const float* Gq = sc + a.s_Gp;
                const float* Xq = sc + a.s_Xp;
                if (beta) emit(a.offBp + j, tr_colsum(Bpad, [&](int row) { return Gq[(size_t)row * Hp + j]; }));
                else emit(a.offGp + j, tr_colsum(Bpad, [&](int row) { return (double)Gq[(size_t)row * Hp + j] * (double)Xq[(size_t)row * Hp + j]; }));
                return;
            }
        }
        const int u = ((int)blockIdx.x - a.strip_blocks) * TW_THREADS + tid;
        if (u >= Hl) return;
        float gsum;
        if (head) gsum = tr_colsum(n_rows, [&](int row) { return dr[(size_t)row * NO + u]; });
        else gsum = tr_colsum(Bpad, [&](int row) { return dZ[(size_t)row * Hl + u]; });
        emit(head ? (u == 0 ? a.offbv : a.offbd + u - 1) : a.offb + u, gsum);
        return;
    }
    const int MTl = (Hl + 15) / 16;
    const int s = blockIdx.x * TW_WAVES + wave;
    if (s >= MTl * ((Hp + 16 * NT - 1) / (16 * NT))) return;
    int m0, n0, nt;
    tw_strip_of<NT>(s, Hp, m0, n0, nt);
    const float* Aprev = sc + a.s_Ap;
    const int lda = a.lda;
    tr_f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = tr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    auto fb = [&](int t, int k) { const int j = n0 + 16 * t + r; return j < Hp ? Aprev[(size_t)k * lda + j] : 0.0f; };
    if (head) {
        auto dzh = [&](int row, int o) { return (row < n_rows && o < NO) ? dr[(size_t)row * NO + o] : 0.0f; };
        mma_strip<NT>(acc, nt, Bpad, [&](int k) { return dzh(k, m0 + r); }, fb, g);
    } else {
        mma_strip<NT>(acc, nt, Bpad, [&](int k) { return dZ[(size_t)k * Hl + m0 + r]; }, fb, g);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t < nt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = m0 + 4 * g + i, j = n0 + 16 * t + r;
                if (u < Hl && j < Hp) emit(head ? a.offWv + u * Hp + (u > 0) + j : a.offW + u * Hp + j, acc[t][i]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the deferred form's optimiser
// grid (TW_NORM_CHAINS / 64, nets): partial chain t of net `net` adds (double)g * (double)g of elements t, t + 1024, ... in that order
// (train_backward_deferred_kernel's thread t), the loads of sixteen links issued ahead of their additions.
__global__ __launch_bounds__(64) void train_wide_norm_kernel(int P, const float* grads_all, double* partials) {
    const int net = blockIdx.y, t = blockIdx.x * 64 + threadIdx.x;
    const float* grads = grads_all + (size_t)net * P;
    double acc = 0.0;
    int i = t;
    for (; i + 15 * TW_NORM_CHAINS < P; i += 16 * TW_NORM_CHAINS) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = grads[i + q * TW_NORM_CHAINS];
#pragma unroll
        for (int q = 0; q < 16; ++q) { const double gd = (double)v[q]; acc = acc + gd * gd; }
    }
    for (; i < P; i += TW_NORM_CHAINS) { const double gd = (double)grads[i]; acc = acc + gd * gd; }
    partials[(size_t)net * TW_NORM_CHAINS + t] = acc;
}

// grid (ceil(P / TW_UPDATE_SPAN), nets), 1024 threads: every workgroup adds the net's 1024 partials by train.cuh's pairwise tree
// (partner t + 512, t + 256, ... t + 1; the same bits in every workgroup), takes the clip coefficient from it, and steps its span of
// the net's elements with tr_update or tr_adam.  Workgroup 0 of a net writes its norm.
__global__ __launch_bounds__(TR_BWD_THREADS) void train_wide_update_kernel(int P, TrainOptD o, float* params, float* state0, float* state1,
                                                                           const float* grads_all, float* norms, const double* partials) {
    const int net = blockIdx.y, tid = threadIdx.x;
    float* p = params + (size_t)net * P;
    float* s0 = state0 + (size_t)net * P;
    const float* grads = grads_all + (size_t)net * P;
    float coef = 1.0f;
    if (o.want_norm) {
        __shared__ double part[TR_BWD_THREADS];
        part[tid] = partials[(size_t)net * TW_NORM_CHAINS + tid];
        __syncthreads();
        for (int st = TR_BWD_THREADS / 2; st > 0; st >>= 1) {
            if (tid < st) part[tid] = part[tid] + part[tid + st];
            __syncthreads();
        }
        const float total = (float)sqrt(part[0]);
        if (norms && tid == 0 && blockIdx.x == 0) norms[net] = total;
        if (o.clip != 0.0f) { const float c = o.clip / (total + 1e-6f); coef = c < 1.0f ? c : 1.0f; }
    }
    const bool clipped = o.clip != 0.0f;
    const int i0 = blockIdx.x * TW_UPDATE_SPAN, i1 = i0 + TW_UPDATE_SPAN < P ? i0 + TW_UPDATE_SPAN : P;
    if (o.kind == AZG_OPT_ADAM) {
        float* s1 = state1 + (size_t)net * P;
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

// train_wide_update_kernel with the settings of net blockIdx.y from table[blockIdx.y] (the *_nets entry points): every workgroup of
// a net copies the same entry once at entry, then runs train.cuh's tr_optim_span -- the text above -- on its span.  A net that
// neither clips nor reports its norm never reads `partials`, whatever the other nets of the launch ask for.
__global__ __launch_bounds__(TR_BWD_THREADS) void train_wide_update_nets_kernel(int P, const TrainOptD* __restrict__ table, float* params,
                                                                                float* state0, float* state1, const float* grads_all,
                                                                                float* norms, const double* partials) {
    const TrainOptD o = table[blockIdx.y];
    const int net = blockIdx.y;
    const int i0 = blockIdx.x * TW_UPDATE_SPAN, i1 = i0 + TW_UPDATE_SPAN < P ? i0 + TW_UPDATE_SPAN : P;
    const double mine = o.want_norm ? partials[(size_t)net * TW_NORM_CHAINS + threadIdx.x] : 0.0;
    tr_optim_span(o, mine, blockIdx.x == 0, norms ? norms + net : nullptr, params + (size_t)net * P, state0 + (size_t)net * P,
                  state1 ? state1 + (size_t)net * P : nullptr, grads_all + (size_t)net * P, i0, i1);
}
