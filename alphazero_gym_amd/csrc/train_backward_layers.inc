// train_backward_layers.inc -- the backward kernels' walk through the layers (train.cuh includes it once per kernel form, so that
// both forms are the same text and the fused kernel compiles to the code it always was).  Expects the kernel's arguments d, params,
// d_raw, n_rows, square_avg, grads_all and scratch in scope, the kernel's template parameter LN, and TR_EMIT(idx, grad): what a
// finished gradient element goes into.
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
            float* Gp = nullptr;
            if constexpr (LN) Gp = sc + d.s_G[l - 1];
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
                            if constexpr (LN) Gp[at] = acc[t][i];
                            else Dp[at] = acc[t][i] * Dp[at];
                        }
                    }
                }
            }
            if constexpr (LN) {
                // the row pass of LayerNorm l - 1: sixteen lanes per row, four rows per wave at a time (Bpad is a multiple of 16, so
                // a wave's four rows are inside or outside together)
                __syncthreads();
                const float* gam = p + d.offG[l - 1];
                const float* Xp = sc + d.s_X[l - 1];
                const float* Rp = sc + d.s_R[l - 1];
                for (int row = 4 * wave + g; row < Bpad; row += 4 * NWV) {
                    const size_t base = (size_t)row * Hp;
                    double s1 = 0.0, s2 = 0.0;
                    for (int j = r; j < Hp; j += 16) {
                        const float dx = Gp[base + j] * gam[j];
                        s1 = s1 + (double)dx;
                        s2 = s2 + (double)dx * (double)Xp[base + j];
                    }
                    const float m1 = (float)(tr_row16_sum(s1) / (double)Hp), m2 = (float)(tr_row16_sum(s2) / (double)Hp);
                    const float rstd = Rp[row];
                    for (int j = r; j < Hp; j += 16) {
                        const float dx = Gp[base + j] * gam[j];
                        const float dA = rstd * ((dx - m1) - Xp[base + j] * m2);
                        Dp[base + j] = dA * Dp[base + j];
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
                            TR_EMIT(idx, acc[t][i]);
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
            TR_EMIT(idx, gsum);
        }
        if constexpr (LN) {
            // dgamma and dbeta of LayerNorm l - 1 (widths are at most 256: threads 256 .. and 512 .. take them beside db's 0 ..)
            if (l > 0) {
                const float* Gq = sc + d.s_G[l - 1];
                const float* Xq = sc + d.s_X[l - 1];
                for (int u = tid - 256; u >= 0 && u < Hp; u += TR_BWD_THREADS) {
                    const float gsum = tr_colsum(Bpad, [&](int row) { return (double)Gq[(size_t)row * Hp + u] * (double)Xq[(size_t)row * Hp + u]; });
                    TR_EMIT(d.offG[l - 1] + u, gsum);
                }
                for (int u = tid - 512; u >= 0 && u < Hp; u += TR_BWD_THREADS) {
                    const float gsum = tr_colsum(Bpad, [&](int row) { return Gq[(size_t)row * Hp + u]; });
                    TR_EMIT(d.offB[l - 1] + u, gsum);
                }
            }
        }
    }
