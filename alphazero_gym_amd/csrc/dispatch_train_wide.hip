// dispatch_train_wide.hip -- the wide trainer's launches (a TrainNet made by azg_trainer_create_wide or azg_trainer_create_wide_ex): the
// kernels of train_wide.cuh, one launch per layer and role (with LayerNorm: a row pass behind every layer's forward launch and between
// (a) and (b) of every layer above the first).  The C ABI, the descriptor checks and the layout are dispatch_train.hip's; a wide
// handle takes these launches where a narrow one takes train.cuh's.
#define TR_NO_SHARED_KERNELS
#include "train_wide.cuh"
#include "train_wide_host.h"

static_assert(TW_MAX_LAYERS == 8, "azg_mlp_desc.hidden has 8 entries");

// Tiles per strip: the widest strip (the fewest operand reads) that still gives the chip a few thousand waves; a narrow grid takes
// narrower strips.  (Which strip an element lies in changes none of its bits.)
static int pick_nt(int row_tiles, int cols, int n_nets) {
    const int tiles = (cols + 15) / 16;
    for (int nt = 4; nt > 1; nt >>= 1)
        if ((size_t)row_tiles * (size_t)((tiles + nt - 1) / nt) * (size_t)n_nets >= 2048) return nt;
    return 1;
}
static int strip_blocks(int row_tiles, int cols, int nt) {
    const int strips = row_tiles * ((cols + 16 * nt - 1) / (16 * nt));
    return (strips + TW_WAVES - 1) / TW_WAVES;
}

#define TW_BY_NT(nt, CALL) \
    do { if ((nt) == 4) { CALL(4); } else if ((nt) == 2) { CALL(2); } else { CALL(1); } } while (0)

// the row pass of LayerNorm l
static TwRow row_pass(const TrainNet& d, int l) {
    TwRow rw{};
    rw.H = d.H[l]; rw.P = d.P; rw.offG = d.offG[l]; rw.offB = d.offB[l];
    rw.s_A = d.s_A[l]; rw.s_D = d.s_D[l]; rw.s_X = d.s_X[l]; rw.s_G = d.s_G[l]; rw.s_R = d.s_R[l]; rw.per_net = d.per_net;
    return rw;
}

void tw_launch_forward(const TrainNet& d, hipStream_t stream, int n_nets, const float* params, const float* obs, int n_rows, float* raw,
                       float* scratch) {
    const int MT = (n_rows + 15) / 16;
    for (int l = 0; l < d.n_layers; ++l) {
        TwFwd a{};
        a.H = d.H[l]; a.kin = l ? d.H[l - 1] : d.in_dim; a.lda = l ? d.H[l - 1] : TR_OBS_LD; a.in_dim = d.in_dim; a.act = d.act; a.first = l == 0;
        a.offW = d.offW[l]; a.offb = d.offb[l]; a.P = d.P;
        a.s_in = l ? d.s_A[l - 1] : d.s_obs; a.s_A = d.s_A[l]; a.s_D = d.s_D[l]; a.per_net = d.per_net;
        const int nt = pick_nt(MT, a.H, n_nets);
        const dim3 grid(strip_blocks(MT, a.H, nt), n_nets);
#define TW_CALL(N) hipLaunchKernelGGL(train_wide_forward_kernel<N>, grid, dim3(TW_THREADS), 0, stream, a, params, obs, n_rows, scratch)
        TW_BY_NT(nt, TW_CALL);
#undef TW_CALL
        if (d.layernorm) {
            const TwRow rw = row_pass(d, l);
            hipLaunchKernelGGL(train_wide_ln_forward_kernel, dim3(MT, n_nets), dim3(TW_THREADS), 0, stream, rw, params, scratch);
        }
    }
    TwHead h{};
    h.HL = d.H[d.n_layers - 1]; h.NO = d.NO; h.P = d.P; h.offWv = d.offWv; h.offbv = d.offbv; h.offbd = d.offbd;
    h.s_in = d.s_A[d.n_layers - 1]; h.per_net = d.per_net;
    hipLaunchKernelGGL(train_wide_heads_kernel, dim3(MT, n_nets), dim3(64), 0, stream, h, params, n_rows, raw, scratch);
}

// The walk from the heads down.  FUSED: opt and square_avg are tr_update's; else the gradients go to grads.  LN: the trunk has
// LayerNorm; per layer above the first (a), the row pass of the LayerNorm below, (b).
template <bool FUSED, bool LN>
static void launch_layers(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOpt& opt, float* params, const float* d_raw,
                          int n_rows, float* square_avg, float* grads, float* scratch) {
    const int MT = (n_rows + 15) / 16, L = d.n_layers;
    for (int l = L; l >= 0; --l) {
        const bool head = l == L;
        typename TwBwdOf<LN>::type a{};
        a.head = head; a.Hl = head ? d.NO : d.H[l]; a.Hp = l > 0 ? d.H[l - 1] : d.in_dim; a.lda = l > 0 ? a.Hp : TR_OBS_LD; a.NO = d.NO; a.P = d.P;
        a.offW = head ? 0 : d.offW[l]; a.offb = head ? 0 : d.offb[l];
        a.offWv = d.offWv; a.offbv = d.offbv; a.offbd = d.offbd;
        a.s_dZ = head ? 0 : d.s_D[l]; a.s_Dp = l > 0 ? d.s_D[l - 1] : 0; a.s_Ap = l > 0 ? d.s_A[l - 1] : d.s_obs; a.per_net = d.per_net;
        if constexpr (LN) {
            if (l > 0) { a.offGp = d.offG[l - 1]; a.offBp = d.offB[l - 1]; a.s_Gp = d.s_G[l - 1]; a.s_Xp = d.s_X[l - 1]; }
        }
        if (l > 0) {
            const int nt = pick_nt(MT, a.Hp, n_nets);
            const dim3 grid(strip_blocks(MT, a.Hp, nt), n_nets);
#define TW_CALL(N) hipLaunchKernelGGL((train_wide_backward_a_kernel<N, LN>), grid, dim3(TW_THREADS), 0, stream, a, params, d_raw, n_rows, scratch)
            TW_BY_NT(nt, TW_CALL);
#undef TW_CALL
            if constexpr (LN) {
                const TwRow rw = row_pass(d, l - 1);
                hipLaunchKernelGGL(train_wide_ln_backward_kernel, dim3(MT, n_nets), dim3(TW_THREADS), 0, stream, rw, params, scratch);
            }
        }
        const int MTl = (a.Hl + 15) / 16;
        const int nt = pick_nt(MTl, a.Hp, n_nets);
        a.strip_blocks = strip_blocks(MTl, a.Hp, nt);
        const int ln_blocks = (LN && l > 0) ? 2 * ((a.Hp + TW_THREADS - 1) / TW_THREADS) : 0;   // dgamma, dbeta of LayerNorm l - 1
        const dim3 grid(a.strip_blocks + (a.Hl + TW_THREADS - 1) / TW_THREADS + ln_blocks, n_nets);
#define TW_CALL(N) hipLaunchKernelGGL((train_wide_backward_b_kernel<N, FUSED, LN>), grid, dim3(TW_THREADS), 0, stream, a, opt, params, d_raw, \
                                      n_rows, square_avg, grads, scratch)
        TW_BY_NT(nt, TW_CALL);
#undef TW_CALL
    }
}

void tw_launch_backward(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOpt& opt, float* params, const float* d_raw, int n_rows,
                        float* square_avg, float* grads, float* scratch) {
    if (d.layernorm) launch_layers<true, true>(d, stream, n_nets, opt, params, d_raw, n_rows, square_avg, grads, scratch);
    else launch_layers<true, false>(d, stream, n_nets, opt, params, d_raw, n_rows, square_avg, grads, scratch);
}

void tw_launch_backward_deferred(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOptD& opt, float* params, const float* d_raw,
                                 int n_rows, float* state0, float* state1, float* grads, float* norms, float* scratch, double* partials) {
    if (d.layernorm) launch_layers<false, true>(d, stream, n_nets, opt.rms, params, d_raw, n_rows, nullptr, grads, scratch);
    else launch_layers<false, false>(d, stream, n_nets, opt.rms, params, d_raw, n_rows, nullptr, grads, scratch);
    if (opt.want_norm)
        hipLaunchKernelGGL(train_wide_norm_kernel, dim3(TW_NORM_CHAINS / 64, n_nets), dim3(64), 0, stream, d.P, grads, partials);
    hipLaunchKernelGGL(train_wide_update_kernel, dim3((d.P + TW_UPDATE_SPAN - 1) / TW_UPDATE_SPAN, n_nets), dim3(TR_BWD_THREADS), 0, stream,
                       d.P, opt, params, state0, state1, grads, norms, partials);
}

void tw_launch_backward_deferred_nets(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOptD* table, bool any_norm, float* params,
                                      const float* d_raw, int n_rows, float* state0, float* state1, float* grads, float* norms,
                                      float* scratch, double* partials) {
    const TrainOpt unused{};   // (the layers' deferred form stores gradients and steps nothing)
    if (d.layernorm) launch_layers<false, true>(d, stream, n_nets, unused, params, d_raw, n_rows, nullptr, grads, scratch);
    else launch_layers<false, false>(d, stream, n_nets, unused, params, d_raw, n_rows, nullptr, grads, scratch);
    if (any_norm)
        hipLaunchKernelGGL(train_wide_norm_kernel, dim3(TW_NORM_CHAINS / 64, n_nets), dim3(64), 0, stream, d.P, grads, partials);
    hipLaunchKernelGGL(train_wide_update_nets_kernel, dim3((d.P + TW_UPDATE_SPAN - 1) / TW_UPDATE_SPAN, n_nets), dim3(TR_BWD_THREADS), 0, stream,
                       d.P, table, params, state0, state1, grads, norms, partials);
}
