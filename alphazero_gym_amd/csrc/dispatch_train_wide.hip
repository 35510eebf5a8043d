// dispatch_train_wide.hip -- the wide trainer (azg_trainer_create_wide, azg_trainer_create_wide_ex): its descriptor checks and layout,
// and the launches of train_wide.cuh, one per layer and role (with LayerNorm: a row pass behind every layer's forward launch and
// between (a) and (b) of every layer above the first).  The C ABI itself is dispatch_train.hip's; a wide handle takes these launches
// where a narrow one takes train.cuh's.
#include <cstdint>
#include <string>

#define TR_NO_SHARED_KERNELS
#include "train_wide.cuh"
#include "train_wide_host.h"

static_assert(TW_MAX_LAYERS == 8, "azg_mlp_desc.hidden has 8 entries");

struct TrainWide {
    TrainDimsW d{};
};

int tw_plan(const azg_mlp_desc* desc, int32_t max_batch, bool layernorm_ok, TrainWide** out, std::string* msg) {
    auto fail = [&](int code, const char* m) { *msg = std::string("azg_trainer_create_wide: ") + m; return code; };
    if (desc->layernorm && !layernorm_ok) return fail(AZG_E_UNSUPPORTED, "wide LayerNorm trunks are not trained on the device");
    if (desc->n_hidden < 1 || desc->n_hidden > TW_MAX_LAYERS) return fail(AZG_E_UNSUPPORTED, "1 to 8 hidden layers");
    if (desc->in_dim < 1 || desc->in_dim > TR_OBS_LD) return fail(AZG_E_UNSUPPORTED, "in_dim must be 1..8");
    if (desc->n_dist < 1 || desc->n_dist > 16) return fail(AZG_E_UNSUPPORTED, "n_dist must be 1..16");
    if (desc->activation < AZG_ACT_RELU || desc->activation > AZG_ACT_HARDSWISH) return fail(AZG_E_UNSUPPORTED, "unknown activation");
    for (int l = 0; l < desc->n_hidden; ++l)
        if (desc->hidden[l] < 16 || desc->hidden[l] > 1024 || desc->hidden[l] % 16)
            return fail(AZG_E_UNSUPPORTED, "hidden widths must be multiples of 16 up to 1024");
    TrainWide* w = new TrainWide();
    TrainDimsW& d = w->d;
    d.n_layers = desc->n_hidden; d.in_dim = desc->in_dim; d.nd = desc->n_dist; d.NO = 1 + desc->n_dist; d.act = desc->activation;
    d.layernorm = desc->layernorm ? 1 : 0;
    const size_t Bmax = ((size_t)max_batch + 15) / 16 * 16;
    // (at most 8 * 1024 * 1024 + ... parameters: off stays far below 2^31; the scratch offsets are checked as they are laid out)
    int off = 0, prev = d.in_dim;
    size_t so = 0;
    const size_t limit = (size_t)1 << 32;
    d.s_obs = (unsigned)so; so += Bmax * TR_OBS_LD;
    for (int l = 0; l < d.n_layers; ++l) {
        d.H[l] = desc->hidden[l];
        d.offW[l] = off; off += d.H[l] * prev;
        d.offb[l] = off; off += d.H[l];
        if (d.layernorm) { d.offG[l] = off; off += d.H[l]; d.offB[l] = off; off += d.H[l]; }
        const size_t need = d.layernorm ? 4 * Bmax * d.H[l] + Bmax : 2 * Bmax * d.H[l];
        if (so + need >= limit) { delete w; return fail(AZG_E_UNSUPPORTED, "max_batch too large"); }
        d.s_A[l] = (unsigned)so; so += Bmax * d.H[l];
        d.s_D[l] = (unsigned)so; so += Bmax * d.H[l];
        if (d.layernorm) {
            d.s_X[l] = (unsigned)so; so += Bmax * d.H[l];
            d.s_G[l] = (unsigned)so; so += Bmax * d.H[l];
            d.s_R[l] = (unsigned)so; so += Bmax;
        }
        prev = d.H[l];
    }
    d.offWv = off; off += prev;
    d.offbv = off; off += 1;
    off += d.nd * prev;            // dist_head.weight: head rows 1 .. nd
    d.offbd = off; off += d.nd;
    d.P = off;
    d.per_net = so;
    *out = w;
    return AZG_OK;
}

void tw_free(TrainWide* w) { delete w; }
int tw_param_count(const TrainWide* w) { return w->d.P; }
size_t tw_scratch_floats(const TrainWide* w) { return w->d.per_net; }

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
static TwRow row_pass(const TrainDimsW& d, int l) {
    TwRow rw{};
    rw.H = d.H[l]; rw.P = d.P; rw.offG = d.offG[l]; rw.offB = d.offB[l];
    rw.s_A = d.s_A[l]; rw.s_D = d.s_D[l]; rw.s_X = d.s_X[l]; rw.s_G = d.s_G[l]; rw.s_R = d.s_R[l]; rw.per_net = d.per_net;
    return rw;
}

void tw_launch_forward(const TrainWide* w, hipStream_t stream, int n_nets, const float* params, const float* obs, int n_rows, float* raw,
                       float* scratch) {
    const TrainDimsW& d = w->d;
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
static void launch_layers(const TrainDimsW& d, hipStream_t stream, int n_nets, const TrainOpt& opt, float* params, const float* d_raw,
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

void tw_launch_backward(const TrainWide* w, hipStream_t stream, int n_nets, const TrainOpt& opt, float* params, const float* d_raw, int n_rows,
                        float* square_avg, float* grads, float* scratch) {
    if (w->d.layernorm) launch_layers<true, true>(w->d, stream, n_nets, opt, params, d_raw, n_rows, square_avg, grads, scratch);
    else launch_layers<true, false>(w->d, stream, n_nets, opt, params, d_raw, n_rows, square_avg, grads, scratch);
}

void tw_launch_backward_deferred(const TrainWide* w, hipStream_t stream, int n_nets, const TrainOptD& opt, float* params, const float* d_raw,
                                 int n_rows, float* state0, float* state1, float* grads, float* norms, float* scratch, double* partials) {
    const TrainDimsW& d = w->d;
    if (d.layernorm) launch_layers<false, true>(d, stream, n_nets, opt.rms, params, d_raw, n_rows, nullptr, grads, scratch);
    else launch_layers<false, false>(d, stream, n_nets, opt.rms, params, d_raw, n_rows, nullptr, grads, scratch);
    if (opt.want_norm)
        hipLaunchKernelGGL(train_wide_norm_kernel, dim3(TW_NORM_CHAINS / 64, n_nets), dim3(64), 0, stream, d.P, grads, partials);
    hipLaunchKernelGGL(train_wide_update_kernel, dim3((d.P + TW_UPDATE_SPAN - 1) / TW_UPDATE_SPAN, n_nets), dim3(TR_BWD_THREADS), 0, stream,
                       d.P, opt, params, state0, state1, grads, norms, partials);
}

void tw_launch_backward_deferred_nets(const TrainWide* w, hipStream_t stream, int n_nets, const TrainOptD* table, bool any_norm, float* params,
                                      const float* d_raw, int n_rows, float* state0, float* state1, float* grads, float* norms,
                                      float* scratch, double* partials) {
    const TrainDimsW& d = w->d;
    const TrainOpt unused{};   // (the layers' deferred form stores gradients and steps nothing)
    if (d.layernorm) launch_layers<false, true>(d, stream, n_nets, unused, params, d_raw, n_rows, nullptr, grads, scratch);
    else launch_layers<false, false>(d, stream, n_nets, unused, params, d_raw, n_rows, nullptr, grads, scratch);
    if (any_norm)
        hipLaunchKernelGGL(train_wide_norm_kernel, dim3(TW_NORM_CHAINS / 64, n_nets), dim3(64), 0, stream, d.P, grads, partials);
    hipLaunchKernelGGL(train_wide_update_nets_kernel, dim3((d.P + TW_UPDATE_SPAN - 1) / TW_UPDATE_SPAN, n_nets), dim3(TR_BWD_THREADS), 0, stream,
                       d.P, table, params, state0, state1, grads, norms, partials);
}
