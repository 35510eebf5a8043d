// dispatch_train.hip -- the population trainer's C ABI (include/azgym_train.h): scratch, checks and the three launches of train.cuh;
// azg_trainer_epoch enqueues them for a whole epoch of minibatches behind a gather launch each.  The *_opt entry points take an
// azg_optim and choose the backward launch's form: fused RMSprop, or gradients first and norm, clip and update after the last layer.
// The *_nets entry points take one azg_optim / azg_loss_cfg per net: the same checks per entry, the launch-ready settings in a device
// table, and the per-net forms of the deferred backward, update and loss kernels, which read their net's entry from it.
// A trainer made by azg_trainer_create_wide(_ex) keeps its dims in `wide` and takes dispatch_train_wide.hip's launches (one per layer and
// role) wherever a narrow one takes train.cuh's; every check, buffer and synchronisation is the same code.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/azgym_train.h"
#include "hip_host.h"
#include "train.cuh"
#include "train_wide_host.h"

struct azg_trainer {
    int device_id = 0;
    int n_nets = 0, max_batch = 0;
    int fwd_rows = 0;            // rows of the last azg_trainer_forward (0: none)
    int step_rows = 0;           // rows of the d_raw the last azg_trainer_step left in d_raw_buf (0: none)
    int num_components = 0;
    float log_std_min = 0.0f, log_std_max = 0.0f;
    bool ln = false;             // the LN = true kernels (a LayerNorm descriptor through azg_trainer_create_ex)
    TrainDimsLN d{};
    TrainWide* wide = nullptr;   // azg_trainer_create_wide(_ex): d then holds only what the host reads (P, NO, nd, in_dim, n_layers)
    double* norm_part = nullptr; // ... and the deferred norm's partial chains [n_nets][1024]
    float* scratch = nullptr;
    float* grad_buf = nullptr;   // [n_nets][P]: where the deferred backward form keeps the gradients when the caller gives no grads
    // the loss kernel's: the rows' terms [n_nets][3][max_batch] (float64), and azg_trainer_step's raw and d_raw [n_nets][max_batch][NO]
    // (allocated by the first call that needs them)
    double* loss_rows = nullptr;
    float* raw_buf = nullptr;
    float* d_raw_buf = nullptr;
    // azg_trainer_epoch's, grown on demand: the uploaded order [n_nets][n_order], the minibatch staging arrays (obs [n_nets][B][in_dim] |
    // actions | counts [n_nets][B][A] | values [n_nets][B], laid out for max_batch rows) and the loss table [n_minibatches][n_nets][5]
    int* order_buf = nullptr;
    float* stage_buf = nullptr;
    float* loss_table = nullptr;
    size_t order_bytes = 0, stage_bytes = 0, table_bytes = 0;
    // the *_nets entry points': the launch-ready settings of every (minibatch, net), [M][n_nets] TrainOptD | [M][n_nets] LossDims (a
    // part the call has no entries for is empty), filled on the host for the whole call and uploaded in one copy; grown on demand
    std::vector<unsigned char> nets_host;
    unsigned char* nets_dev = nullptr;
    size_t nets_bytes = 0;
    size_t nets_loss_off = 0;    // where the LossDims part starts
    bool nets_any_norm = false;  // some net of the call clips or reports its norm
    hipStream_t stream = nullptr;
    std::string err;
};

// (azg_trainer_last_error(NULL) reads the calling thread's own last creation error)
static thread_local std::string g_trainer_create_err;

static int tfail(azg_trainer* t, int code, const std::string& msg) {
    if (t) t->err = msg; else g_trainer_create_err = msg;
    return code;
}

extern "C" {

const char* azg_trainer_last_error(const azg_trainer* t) { return t ? t->err.c_str() : g_trainer_create_err.c_str(); }

size_t azg_trainer_param_count(const azg_trainer* t) { return t ? (size_t)t->d.P : 0; }

void azg_trainer_destroy(azg_trainer* t) {
    if (!t) return;
    DeviceScope scope(t->device_id);
    if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
    if (t->scratch) (void)hipFree(t->scratch);
    if (t->grad_buf) (void)hipFree(t->grad_buf);
    if (t->loss_rows) (void)hipFree(t->loss_rows);
    if (t->raw_buf) (void)hipFree(t->raw_buf);
    if (t->d_raw_buf) (void)hipFree(t->d_raw_buf);
    if (t->order_buf) (void)hipFree(t->order_buf);
    if (t->stage_buf) (void)hipFree(t->stage_buf);
    if (t->loss_table) (void)hipFree(t->loss_table);
    if (t->norm_part) (void)hipFree(t->norm_part);
    if (t->nets_dev) (void)hipFree(t->nets_dev);
    if (t->wide) tw_free(t->wide);
    delete t;
}

// azg_trainer_create (layernorm_ok = false) and azg_trainer_create_ex
static int create_impl(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, bool layernorm_ok, azg_trainer** out) {
    if (desc->struct_size != (int32_t)sizeof(azg_mlp_desc)) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: azg_mlp_desc.struct_size mismatch");
    if (n_nets < 1 || max_batch < 1) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: n_nets and max_batch must be at least 1");
    if (desc->layernorm && !layernorm_ok) return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: LayerNorm trunks are not trained on the device");
    if (desc->n_hidden < 1 || desc->n_hidden > TR_MAX_LAYERS)
        return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: 1 to 3 hidden layers");
    if (desc->in_dim < 1 || desc->in_dim > TR_OBS_LD) return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: in_dim must be 1..8");
    if (desc->n_dist < 1 || desc->n_dist > 16) return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: n_dist must be 1..16");
    if (desc->activation < AZG_ACT_RELU || desc->activation > AZG_ACT_HARDSWISH)
        return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: unknown activation");
    for (int l = 0; l < desc->n_hidden; ++l)
        if (desc->hidden[l] < 16 || desc->hidden[l] > 256 || desc->hidden[l] % 16)
            return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: hidden widths must be multiples of 16 up to 256");
    azg_trainer* t = new azg_trainer();
    t->device_id = device_id;
    t->n_nets = n_nets;
    t->max_batch = max_batch;
    t->num_components = desc->num_components;
    t->log_std_min = desc->log_std_min;
    t->log_std_max = desc->log_std_max;
    TrainDimsLN& d = t->d;
    t->ln = desc->layernorm != 0;
    d.layernorm = t->ln ? 1 : 0;
    d.n_layers = desc->n_hidden; d.in_dim = desc->in_dim; d.nd = desc->n_dist; d.NO = 1 + desc->n_dist; d.act = desc->activation;
    const size_t Bmax = ((size_t)max_batch + 15) / 16 * 16;
    int off = 0, prev = d.in_dim;
    size_t so = 0;
    d.s_obs = (unsigned)so; so += Bmax * TR_OBS_LD;
    for (int l = 0; l < d.n_layers; ++l) {
        d.H[l] = desc->hidden[l];
        d.offW[l] = off; off += d.H[l] * prev;
        d.offb[l] = off; off += d.H[l];
        if (t->ln) { d.offG[l] = off; off += d.H[l]; d.offB[l] = off; off += d.H[l]; }
        d.s_A[l] = (unsigned)so; so += Bmax * d.H[l];
        d.s_D[l] = (unsigned)so; so += Bmax * d.H[l];
        if (t->ln) {
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
    if (so >= ((size_t)1 << 32)) { delete t; return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: max_batch too large"); }
    DeviceScope scope(device_id);
    if (!scope.ok) { delete t; return tfail(nullptr, AZG_E_DEVICE, "hipSetDevice failed"); }
    const size_t bytes = so * (size_t)n_nets * sizeof(float);
    // (not cleared: the forward launch writes every scratch element below its padded row count, and the backward launch of the
    // same n_rows reads nothing else)
    hipError_t rc = hipMalloc((void**)&t->scratch, bytes);
    if (rc == hipSuccess) rc = hipMalloc((void**)&t->grad_buf, (size_t)n_nets * (size_t)d.P * sizeof(float));
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (rc != hipSuccess) {
        const std::string msg = std::string("azg_trainer_create: ") + hipGetErrorString(rc);
        azg_trainer_destroy(t);
        return tfail(nullptr, AZG_E_DEVICE, msg);
    }
    *out = t;
    return AZG_OK;
}

int azg_trainer_create(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out) {
    if (!desc || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: NULL argument");
    *out = nullptr;
    return create_impl(device_id, desc, n_nets, max_batch, false, out);
}

int azg_trainer_create_ex(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const azg_trainer_options* opts,
                          azg_trainer** out) {
    if (!desc || !opts || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_ex: NULL argument");
    *out = nullptr;
    if (opts->struct_size != (int32_t)sizeof(azg_trainer_options))
        return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_ex: azg_trainer_options.struct_size mismatch");
    return create_impl(device_id, desc, n_nets, max_batch, opts->layernorm != 0, out);
}

// azg_trainer_create_wide (layernorm_ok = false) and azg_trainer_create_wide_ex, behind their NULL checks
static int create_wide_impl(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, bool layernorm_ok,
                            azg_trainer** out) {
    if (desc->struct_size != (int32_t)sizeof(azg_mlp_desc)) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide: azg_mlp_desc.struct_size mismatch");
    if (n_nets < 1 || max_batch < 1) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide: n_nets and max_batch must be at least 1");
    TrainWide* w = nullptr;
    std::string msg;
    if (int rc = tw_plan(desc, max_batch, layernorm_ok, &w, &msg)) return tfail(nullptr, rc, msg);
    azg_trainer* t = new azg_trainer();
    t->wide = w;
    t->device_id = device_id;
    t->n_nets = n_nets;
    t->max_batch = max_batch;
    t->num_components = desc->num_components;
    t->log_std_min = desc->log_std_min;
    t->log_std_max = desc->log_std_max;
    t->d.n_layers = desc->n_hidden; t->d.in_dim = desc->in_dim; t->d.nd = desc->n_dist; t->d.NO = 1 + desc->n_dist; t->d.act = desc->activation;
    t->d.P = tw_param_count(w);
    t->d.per_net = tw_scratch_floats(w);
    DeviceScope scope(device_id);
    if (!scope.ok) { azg_trainer_destroy(t); return tfail(nullptr, AZG_E_DEVICE, "hipSetDevice failed"); }
    // (the scratch is not cleared, for azg_trainer_create's reason)
    hipError_t rc = hipMalloc((void**)&t->scratch, t->d.per_net * (size_t)n_nets * sizeof(float));
    if (rc == hipSuccess) rc = hipMalloc((void**)&t->grad_buf, (size_t)n_nets * (size_t)t->d.P * sizeof(float));
    if (rc == hipSuccess) rc = hipMalloc((void**)&t->norm_part, (size_t)n_nets * TR_BWD_THREADS * sizeof(double));
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (rc != hipSuccess) {
        const std::string m = std::string("azg_trainer_create_wide: ") + hipGetErrorString(rc);
        (void)hipGetLastError();
        azg_trainer_destroy(t);
        return tfail(nullptr, AZG_E_DEVICE, m);
    }
    *out = t;
    return AZG_OK;
}

int azg_trainer_create_wide(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out) {
    if (!desc || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide: NULL argument");
    return create_wide_impl(device_id, desc, n_nets, max_batch, false, out);
}

int azg_trainer_create_wide_ex(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const azg_trainer_options* opts,
                               azg_trainer** out) {
    if (!desc || !opts || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide_ex: NULL argument");
    if (opts->struct_size != (int32_t)sizeof(azg_trainer_options))
        return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide_ex: azg_trainer_options.struct_size mismatch");
    return create_wide_impl(device_id, desc, n_nets, max_batch, opts->layernorm != 0, out);
}

// ---- each call in three parts: its checks (nothing launched, nothing written), its launch, and the public entry point ----

static int check_forward(azg_trainer* t, const char* who, const float* params, const float* obs, int32_t n_rows) {
    if (!params || !obs) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, std::string(who) + ": n_rows must be 1..max_batch");
    return AZG_OK;
}

static void launch_forward(azg_trainer* t, const float* params, const float* obs, int n_rows, float* raw) {
    if (t->wide) { tw_launch_forward(t->wide, t->stream, t->n_nets, params, obs, n_rows, raw, t->scratch); return; }
    const dim3 grid((n_rows + 15) / 16, t->n_nets);
    if (t->ln) hipLaunchKernelGGL(train_forward_kernel<true>, grid, dim3(64), 0, t->stream, t->d, params, obs, n_rows, raw, t->scratch);
    else hipLaunchKernelGGL(train_forward_kernel<false>, grid, dim3(64), 0, t->stream, (const TrainDims&)t->d, params, obs, n_rows, raw, t->scratch);
}

static int check_backward(azg_trainer* t, const char* who, const float* params, const azg_rmsprop* opt, const float* square_avg,
                          int32_t n_rows) {
    const std::string w(who);
    if (!params || !opt || !square_avg) return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    if (opt->struct_size != (int32_t)sizeof(azg_rmsprop)) return tfail(t, AZG_E_INVALID, w + ": azg_rmsprop.struct_size mismatch");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": n_rows must be 1..max_batch");
    if (opt->momentum != 0.0 || opt->centered) return tfail(t, AZG_E_UNSUPPORTED, w + ": RMSprop with momentum or centered is not built");
    if (opt->grad_clip != 0.0) return tfail(t, AZG_E_UNSUPPORTED, w + ": gradient clipping is not built (a per-net global norm needs a pass of its own)");
    return AZG_OK;
}

static void launch_backward(azg_trainer* t, float* params, const float* d_raw, int n_rows, const azg_rmsprop* opt, float* square_avg,
                            float* grads) {
    TrainOpt o;
    o.lr = (float)opt->lr; o.alpha = (float)opt->alpha; o.one_minus_alpha = (float)(1.0 - opt->alpha); o.eps = (float)opt->eps;
    o.wd = (float)opt->weight_decay;
    if (t->wide) { tw_launch_backward(t->wide, t->stream, t->n_nets, o, params, d_raw, n_rows, square_avg, grads, t->scratch); return; }
    if (t->ln)
        hipLaunchKernelGGL(train_backward_kernel<true>, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream, t->d, o, params, d_raw, n_rows,
                           square_avg, grads, t->scratch);
    else
        hipLaunchKernelGGL(train_backward_kernel<false>, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream, (const TrainDims&)t->d, o, params,
                           d_raw, n_rows, square_avg, grads, t->scratch);
}

// An azg_optim as the launch takes it: the fused kernel with the old settings (plain RMSprop, nothing asked of the gradients as a
// whole), or the deferred kernel's TrainOptD for the step opt->step + step_add + 1.
struct OptPlan {
    bool fused;
    azg_rmsprop rms;
    TrainOptD o;
};

static int check_optim(azg_trainer* t, const char* who, const float* params, const azg_optim* opt, int32_t n_rows, int step_add,
                       OptPlan* out) {
    const std::string w(who);
    if (!params || !opt) return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    if (opt->struct_size != (int32_t)sizeof(azg_optim)) return tfail(t, AZG_E_INVALID, w + ": azg_optim.struct_size mismatch");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": n_rows must be 1..max_batch");
    if (opt->kind != AZG_OPT_RMSPROP && opt->kind != AZG_OPT_ADAM) return tfail(t, AZG_E_UNSUPPORTED, w + ": unknown optimiser kind");
    const bool adam = opt->kind == AZG_OPT_ADAM;
    if (!opt->state0 || (adam && !opt->state1)) return tfail(t, AZG_E_INVALID, w + ": NULL state pointer in azg_optim");
    if (!(opt->lr >= 0.0) || !(opt->eps >= 0.0)) return tfail(t, AZG_E_INVALID, w + ": lr and eps must be >= 0");
    if (!(opt->grad_clip >= 0.0)) return tfail(t, AZG_E_INVALID, w + ": grad_clip must be >= 0");
    if (opt->step < 0 || opt->step > INT32_MAX - 1 - step_add) return tfail(t, AZG_E_INVALID, w + ": azg_optim.step must be >= 0 (and fit with the epoch's steps)");
    if (adam && !(opt->beta1 >= 0.0 && opt->beta1 < 1.0 && opt->beta2 >= 0.0 && opt->beta2 < 1.0))
        return tfail(t, AZG_E_INVALID, w + ": Adam's betas must lie in [0, 1)");
    OptPlan pl{};
    pl.fused = !adam && opt->grad_clip == 0.0 && !opt->grad_norms;
    pl.rms.struct_size = (int32_t)sizeof(azg_rmsprop);
    pl.rms.lr = opt->lr; pl.rms.alpha = opt->alpha; pl.rms.eps = opt->eps; pl.rms.weight_decay = opt->weight_decay;
    TrainOptD& o = pl.o;
    o.rms.lr = (float)opt->lr; o.rms.alpha = (float)opt->alpha; o.rms.one_minus_alpha = (float)(1.0 - opt->alpha);
    o.rms.eps = (float)opt->eps; o.rms.wd = (float)opt->weight_decay;
    o.kind = opt->kind;
    o.clip = (float)opt->grad_clip;
    o.want_norm = (opt->grad_clip != 0.0 || opt->grad_norms) ? 1 : 0;
    if (adam) {
        const double step = (double)opt->step + (double)step_add + 1.0;
        o.lr = opt->lr; o.b1 = opt->beta1; o.b2 = opt->beta2; o.eps = opt->eps; o.wd = opt->weight_decay;
        o.bc1 = 1.0 - std::pow(o.b1, step);
        o.bc2_sqrt = std::sqrt(1.0 - std::pow(o.b2, step));
    }
    *out = pl;
    return AZG_OK;
}

// The optimiser argument of a step or an epoch in either form: (azg_rmsprop, square_avg) of the first entry points, or an azg_optim.
struct OptArg {
    bool opt_form;
    const azg_rmsprop* rms;
    float* square_avg;
    const azg_optim* opt;
};

static int check_opt_arg(azg_trainer* t, const char* who, const float* params, const OptArg& a, int32_t n_rows, int step_add, OptPlan* pl) {
    if (a.opt_form) return check_optim(t, who, params, a.opt, n_rows, step_add, pl);
    if (int rc = check_backward(t, who, params, a.rms, a.square_avg, n_rows)) return rc;
    pl->fused = true;
    pl->rms = *a.rms;
    return AZG_OK;
}

static void launch_backward_arg(azg_trainer* t, float* params, const float* d_raw, int n_rows, const OptPlan& pl, const OptArg& a,
                                float* grads) {
    if (pl.fused) { launch_backward(t, params, d_raw, n_rows, &pl.rms, a.opt_form ? a.opt->state0 : a.square_avg, grads); return; }
    float* gr = grads ? grads : t->grad_buf;
    if (t->wide) {
        tw_launch_backward_deferred(t->wide, t->stream, t->n_nets, pl.o, params, d_raw, n_rows, a.opt->state0, a.opt->state1, gr,
                                    a.opt->grad_norms, t->scratch, t->norm_part);
        return;
    }
    if (t->ln)
        hipLaunchKernelGGL(train_backward_deferred_kernel<true>, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream, t->d, pl.o, params, d_raw,
                           n_rows, a.opt->state0, a.opt->state1, gr, a.opt->grad_norms, t->scratch);
    else
        hipLaunchKernelGGL(train_backward_deferred_kernel<false>, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream, (const TrainDims&)t->d,
                           pl.o, params, d_raw, n_rows, a.opt->state0, a.opt->state1, gr, a.opt->grad_norms, t->scratch);
}

// The loss settings as the kernel takes them; every refusal of azg_trainer_loss.
static int check_loss(azg_trainer* t, const char* who, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfg,
                      const azg_alpha_state* st, LossDims* out) {
    const std::string w(who);
    if (!cfg) return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    if (cfg->struct_size != (int32_t)sizeof(azg_loss_cfg)) return tfail(t, AZG_E_INVALID, w + ": azg_loss_cfg.struct_size mismatch");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": n_rows must be 1..max_batch");
    if (n_actions < 1 || n_actions > TR_MAX_ACTIONS) return tfail(t, AZG_E_INVALID, w + ": n_actions must be 1..16");
    if (cfg->kind != AZG_LOSS_ALPHAZERO && cfg->kind != AZG_LOSS_A0C && cfg->kind != AZG_LOSS_A0C_TUNED)
        return tfail(t, AZG_E_UNSUPPORTED, w + ": unknown loss kind");
    if (cfg->head != AZG_HEAD_DISCRETE && cfg->head != AZG_HEAD_NORMAL && cfg->head != AZG_HEAD_GMM)
        return tfail(t, AZG_E_UNSUPPORTED, w + ": unknown head kind");
    if (cfg->reduction != AZG_REDUCE_MEAN && cfg->reduction != AZG_REDUCE_SUM) return tfail(t, AZG_E_UNSUPPORTED, w + ": reduction must be mean or sum");
    if (cfg->kind == AZG_LOSS_ALPHAZERO && cfg->head != AZG_HEAD_DISCRETE)
        return tfail(t, AZG_E_UNSUPPORTED, w + ": AlphaZeroLoss needs a discrete head");
    const int nd = t->d.nd;
    int C = 1;
    if (cfg->head == AZG_HEAD_GMM) {
        C = t->num_components;
        if (C > TR_MAX_COMP) return tfail(t, AZG_E_UNSUPPORTED, w + ": at most 5 mixture components");
        if (C < 1 || nd != 3 * C) return tfail(t, AZG_E_UNSUPPORTED, w + ": a mixture head needs n_dist = 3 * num_components (one-dimensional actions)");
    }
    if (cfg->head == AZG_HEAD_NORMAL && nd != 2) return tfail(t, AZG_E_UNSUPPORTED, w + ": a Normal head needs n_dist = 2 (one-dimensional actions)");
    if (cfg->kind == AZG_LOSS_ALPHAZERO && n_actions != nd) return tfail(t, AZG_E_INVALID, w + ": AlphaZeroLoss needs n_actions = n_dist");
    if (!(cfg->action_bound >= 0.0)) return tfail(t, AZG_E_INVALID, w + ": action_bound must be >= 0");
    const bool tuned = cfg->kind == AZG_LOSS_A0C_TUNED;
    if (tuned) {
        if (!st) return tfail(t, AZG_E_INVALID, w + ": A0CLossTuned needs an azg_alpha_state");
        if (st->struct_size != (int32_t)sizeof(azg_alpha_state)) return tfail(t, AZG_E_INVALID, w + ": azg_alpha_state.struct_size mismatch");
        if (!st->log_alpha || !st->exp_avg || !st->exp_avg_sq) return tfail(t, AZG_E_INVALID, w + ": NULL pointer in azg_alpha_state");
        if (st->step < 0) return tfail(t, AZG_E_INVALID, w + ": azg_alpha_state.step must be >= 0");
    }
    LossDims c{};
    c.kind = cfg->kind; c.head = cfg->head; c.nd = nd; c.C = C; c.A = n_actions;
    c.squashed = cfg->head != AZG_HEAD_DISCRETE && cfg->action_bound > 0.0;
    c.tau = cfg->tau; c.lmin = t->log_std_min; c.lmax = t->log_std_max;
    if (c.squashed) {
        const double eps = 1e-6, b = cfg->action_bound;   // SquashedNormal's epsilon
        c.bpe = b + eps;
        c.corr = 1.0 + eps / b;
        // log|det J| counts log(bound) x.shape[-1] times: the row's actions for the Normal head, 1 for the mixture's components
        c.ladj0 = (cfg->head == AZG_HEAD_NORMAL ? (double)n_actions : 1.0) * std::log(b);
    }
    const bool mean = cfg->reduction == AZG_REDUCE_MEAN;
    const double B = (double)n_rows;
    c.pc = cfg->policy_coeff; c.vc = cfg->value_coeff;
    c.red = mean ? 1.0 / B : 1.0;
    c.inv_rows = 1.0 / B;
    // the discrete head's entropy is [B][A], every action of a row carrying the row's entropy: its mean is the mean over the rows,
    // its sum A times their sum
    c.ent_red = mean ? 1.0 / B : (cfg->head == AZG_HEAD_DISCRETE ? (double)n_actions : 1.0);
    c.cP = c.pc * c.red; c.cV = c.vc * c.red; c.cE = cfg->kind == AZG_LOSS_ALPHAZERO ? 0.0 : c.ent_red;
    c.alpha = cfg->alpha; c.target = cfg->target_entropy;
    if (tuned) {
        const double step = (double)st->step + 1.0;
        c.lr = cfg->alpha_lr; c.b1 = cfg->alpha_beta1; c.b2 = cfg->alpha_beta2; c.eps = cfg->alpha_eps; c.wd = cfg->alpha_weight_decay;
        c.clip = cfg->alpha_clip;
        c.bc1 = 1.0 - std::pow(c.b1, step);
        c.bc2_sqrt = std::sqrt(1.0 - std::pow(c.b2, step));
    }
    *out = c;
    return AZG_OK;
}

static int ensure(azg_trainer* t, void** buf, size_t bytes) {
    if (*buf) return AZG_OK;
    const hipError_t rc = hipMalloc(buf, bytes);
    if (rc != hipSuccess) { *buf = nullptr; return tfail(t, AZG_E_DEVICE, std::string("azg_trainer: ") + hipGetErrorString(rc)); }
    return AZG_OK;
}

// (for buffers whose size depends on the call: a larger one replaces the old one; the stream is idle between calls)
static int grow(azg_trainer* t, void** buf, size_t* have, size_t bytes) {
    if (*buf && *have >= bytes) return AZG_OK;
    void* p = nullptr;
    const hipError_t rc = hipMalloc(&p, bytes);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer: ") + hipGetErrorString(rc));
    if (*buf) (void)hipFree(*buf);
    *buf = p;
    *have = bytes;
    return AZG_OK;
}

static void launch_loss(azg_trainer* t, const LossDims& c, const float* raw, const float* actions, const float* counts, const float* values,
                        int n_rows, const azg_alpha_state* st, float* d_raw, float* losses) {
    const bool tuned = c.kind == AZG_LOSS_A0C_TUNED;
    hipLaunchKernelGGL(train_loss_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, c, raw, actions, counts, values, n_rows,
                       tuned ? st->log_alpha : nullptr, tuned ? st->exp_avg : nullptr, tuned ? st->exp_avg_sq : nullptr, d_raw, losses,
                       t->loss_rows, t->max_batch);
}

// ---- the *_nets entry points: one azg_optim and / or one azg_loss_cfg per net ----

static int nets_differ(azg_trainer* t, const char* who, const char* field, int k) {
    return tfail(t, AZG_E_INVALID, std::string(who) + ": " + field + " of net " + std::to_string(k) + " differs from net 0's (it must be equal in every entry)");
}

// (check_optim / check_loss, called without a name, refused entry k: their message behind the entry point's name and the net)
static int net_refused(azg_trainer* t, const char* who, int k, int rc) {
    t->err = std::string(who) + " (net " + std::to_string(k) + ")" + t->err;
    return rc;
}

// Entry 0 has passed the *_opt call's checks.  Here: entries 1 .. n_nets - 1 equal entry 0 where they must; then every entry goes
// through check_optim / check_loss for every minibatch (count[m] rows, Adam steps + m) -- the expressions of the one-net call, so
// the bias corrections and every derived factor are that call's -- and what they return fills the host table.  (They are called with
// an empty name, which a refusal gets from net_refused: a call that passes builds no message string per net.)  opts or cfgs may be
// NULL (a call without that kind of entry).  Nothing is launched or written to the device.
static int plan_nets(azg_trainer* t, const char* who, const float* params, const azg_optim* opts, const azg_loss_cfg* cfgs,
                     const azg_alpha_state* alpha_state, bool stepped, int32_t n_actions, const int* count, int M) {
    const int K = t->n_nets;
    for (int k = 1; k < K; ++k) {
        if (opts) {
            const azg_optim &a = opts[0], &b = opts[k];
            if (b.struct_size != a.struct_size) return nets_differ(t, who, "azg_optim.struct_size", k);
            if (b.kind != a.kind) return nets_differ(t, who, "azg_optim.kind", k);
            if (b.state0 != a.state0) return nets_differ(t, who, "azg_optim.state0", k);
            if (b.state1 != a.state1) return nets_differ(t, who, "azg_optim.state1", k);
            if (b.grad_norms != a.grad_norms) return nets_differ(t, who, "azg_optim.grad_norms", k);
            if (b.step != a.step) return nets_differ(t, who, "azg_optim.step", k);
        }
        if (cfgs) {
            const azg_loss_cfg &a = cfgs[0], &b = cfgs[k];
            if (b.struct_size != a.struct_size) return nets_differ(t, who, "azg_loss_cfg.struct_size", k);
            if (b.kind != a.kind) return nets_differ(t, who, "azg_loss_cfg.kind", k);
            if (b.head != a.head) return nets_differ(t, who, "azg_loss_cfg.head", k);
            if (b.reduction != a.reduction) return nets_differ(t, who, "azg_loss_cfg.reduction", k);
            if (!(b.action_bound == a.action_bound)) return nets_differ(t, who, "azg_loss_cfg.action_bound", k);
        }
    }
    const size_t n = (size_t)M * (size_t)K;
    t->nets_loss_off = opts ? n * sizeof(TrainOptD) : 0;
    t->nets_host.resize(t->nets_loss_off + (cfgs ? n * sizeof(LossDims) : 0));
    TrainOptD* od = reinterpret_cast<TrainOptD*>(t->nets_host.data());
    LossDims* ld = reinterpret_cast<LossDims*>(t->nets_host.data() + t->nets_loss_off);
    t->nets_any_norm = false;
    for (int m = 0; m < M; ++m) {
        azg_alpha_state st{};
        if (stepped) { st = *alpha_state; st.step += m; }
        for (int k = 0; k < K; ++k) {
            if (opts) {
                OptPlan pl;
                if (int rc = check_optim(t, "", params, &opts[k], count[m], m, &pl)) return net_refused(t, who, k, rc);
                od[(size_t)m * K + k] = pl.o;
                t->nets_any_norm = t->nets_any_norm || pl.o.want_norm;
            }
            if (cfgs) {
                if (int rc = check_loss(t, "", count[m], n_actions, &cfgs[k], stepped ? &st : alpha_state, &ld[(size_t)m * K + k]))
                    return net_refused(t, who, k, rc);
            }
        }
    }
    return AZG_OK;
}

// The table to the device: one asynchronous copy on the trainer's stream, in front of the call's first launch.  nets_host stays as
// it is until the call's synchronisation.
static int upload_nets(azg_trainer* t, const char* who) {
    const size_t bytes = t->nets_host.size();
    if (int rc = grow(t, (void**)&t->nets_dev, &t->nets_bytes, bytes)) return rc;
    const hipError_t up = hipMemcpyAsync(t->nets_dev, t->nets_host.data(), bytes, hipMemcpyHostToDevice, t->stream);
    if (up != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string(who) + ": " + hipGetErrorString(up));
    return AZG_OK;
}

// minibatch m's launches with every net's own entry
static void launch_loss_nets(azg_trainer* t, int m, int kind, const float* raw, const float* actions, const float* counts, const float* values,
                             int n_rows, const azg_alpha_state* st, float* d_raw, float* losses) {
    const bool tuned = kind == AZG_LOSS_A0C_TUNED;
    const LossDims* table = reinterpret_cast<const LossDims*>(t->nets_dev + t->nets_loss_off) + (size_t)m * t->n_nets;
    hipLaunchKernelGGL(train_loss_nets_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, table, raw, actions, counts, values, n_rows,
                       tuned ? st->log_alpha : nullptr, tuned ? st->exp_avg : nullptr, tuned ? st->exp_avg_sq : nullptr, d_raw, losses,
                       t->loss_rows, t->max_batch);
}

static void launch_backward_nets(azg_trainer* t, int m, float* params, const float* d_raw, int n_rows, const azg_optim* opts, float* grads) {
    const TrainOptD* table = reinterpret_cast<const TrainOptD*>(t->nets_dev) + (size_t)m * t->n_nets;
    float* gr = grads ? grads : t->grad_buf;
    if (t->wide) {
        tw_launch_backward_deferred_nets(t->wide, t->stream, t->n_nets, table, t->nets_any_norm, params, d_raw, n_rows, opts->state0,
                                         opts->state1, gr, opts->grad_norms, t->scratch, t->norm_part);
        return;
    }
    if (t->ln)
        hipLaunchKernelGGL(train_backward_deferred_nets_kernel<true>, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream, t->d, table, params,
                           d_raw, n_rows, opts->state0, opts->state1, gr, opts->grad_norms, t->scratch);
    else
        hipLaunchKernelGGL(train_backward_deferred_nets_kernel<false>, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream,
                           (const TrainDims&)t->d, table, params, d_raw, n_rows, opts->state0, opts->state1, gr, opts->grad_norms, t->scratch);
}

static int finish(azg_trainer* t, const char* who) {
    hipError_t rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string(who) + ": " + hipGetErrorString(rc));
    return AZG_OK;
}

int azg_trainer_forward(azg_trainer* t, const float* params, const float* obs, int32_t n_rows, float* raw) {
    if (!t) return AZG_E_INVALID;
    if (!raw) return tfail(t, AZG_E_INVALID, "azg_trainer_forward: NULL pointer");
    if (int rc = check_forward(t, "azg_trainer_forward", params, obs, n_rows)) return rc;
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    t->fwd_rows = 0;
    launch_forward(t, params, obs, (int)n_rows, raw);
    if (int rc = finish(t, "azg_trainer_forward")) return rc;
    t->fwd_rows = n_rows;
    return AZG_OK;
}

int azg_trainer_backward_step(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_rmsprop* opt, float* square_avg,
                              float* grads) {
    if (!t) return AZG_E_INVALID;
    if (!d_raw) return tfail(t, AZG_E_INVALID, "azg_trainer_backward_step: NULL pointer");
    if (int rc = check_backward(t, "azg_trainer_backward_step", params, opt, square_avg, n_rows)) return rc;
    if (t->fwd_rows != n_rows) return tfail(t, AZG_E_STATE, "azg_trainer_backward_step: needs azg_trainer_forward of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    t->fwd_rows = 0;   // the scratch is consumed: dZ overwrites the activation derivatives
    launch_backward(t, params, d_raw, (int)n_rows, opt, square_avg, grads);
    return finish(t, "azg_trainer_backward_step");
}

int azg_trainer_backward_step_opt(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_optim* opt, float* grads) {
    if (!t) return AZG_E_INVALID;
    if (!d_raw) return tfail(t, AZG_E_INVALID, "azg_trainer_backward_step_opt: NULL pointer");
    OptPlan pl;
    if (int rc = check_optim(t, "azg_trainer_backward_step_opt", params, opt, n_rows, 0, &pl)) return rc;
    if (t->fwd_rows != n_rows) return tfail(t, AZG_E_STATE, "azg_trainer_backward_step_opt: needs azg_trainer_forward of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    t->fwd_rows = 0;
    launch_backward_arg(t, params, d_raw, (int)n_rows, pl, OptArg{true, nullptr, nullptr, opt}, grads);
    return finish(t, "azg_trainer_backward_step_opt");
}

int azg_trainer_loss(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values, int32_t n_rows,
                     int32_t n_actions, const azg_loss_cfg* cfg, const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    if (!t) return AZG_E_INVALID;
    if (!raw || !actions || !counts || !values || !d_raw || !losses) return tfail(t, AZG_E_INVALID, "azg_trainer_loss: NULL pointer");
    LossDims c;
    if (int rc = check_loss(t, "azg_trainer_loss", n_rows, n_actions, cfg, alpha_state, &c)) return rc;
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    if (int rc = ensure(t, (void**)&t->loss_rows, (size_t)t->n_nets * 3 * t->max_batch * sizeof(double))) return rc;
    launch_loss(t, c, raw, actions, counts, values, (int)n_rows, alpha_state, d_raw, losses);
    return finish(t, "azg_trainer_loss");
}

static int step_impl(azg_trainer* t, const char* who, float* params, const float* obs, const float* actions, const float* counts,
                     const float* values, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg,
                     const azg_alpha_state* alpha_state, const OptArg& oa, float* grads, float* raw_out, float* losses,
                     bool nets = false) {
    if (!t) return AZG_E_INVALID;
    if (!actions || !counts || !values || !losses) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    if (int rc = check_forward(t, who, params, obs, n_rows)) return rc;
    LossDims c;
    if (int rc = check_loss(t, who, n_rows, n_actions, loss_cfg, alpha_state, &c)) return rc;
    OptPlan pl;
    if (int rc = check_opt_arg(t, who, params, oa, n_rows, 0, &pl)) return rc;
    const int rows1 = n_rows;
    if (nets) { if (int rc = plan_nets(t, who, params, oa.opt, loss_cfg, alpha_state, false, n_actions, &rows1, 1)) return rc; }
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const size_t per = (size_t)t->n_nets * t->max_batch * t->d.NO;
    if (int rc = ensure(t, (void**)&t->loss_rows, (size_t)t->n_nets * 3 * t->max_batch * sizeof(double))) return rc;
    if (int rc = ensure(t, (void**)&t->d_raw_buf, per * sizeof(float))) return rc;
    if (!raw_out) { if (int rc = ensure(t, (void**)&t->raw_buf, per * sizeof(float))) return rc; }
    float* raw = raw_out ? raw_out : t->raw_buf;
    if (nets) { if (int rc = upload_nets(t, who)) return rc; }
    t->fwd_rows = 0;
    t->step_rows = 0;
    launch_forward(t, params, obs, (int)n_rows, raw);
    if (nets) {
        launch_loss_nets(t, 0, c.kind, raw, actions, counts, values, (int)n_rows, alpha_state, t->d_raw_buf, losses);
        launch_backward_nets(t, 0, params, t->d_raw_buf, (int)n_rows, oa.opt, grads);
    } else {
        launch_loss(t, c, raw, actions, counts, values, (int)n_rows, alpha_state, t->d_raw_buf, losses);
        launch_backward_arg(t, params, t->d_raw_buf, (int)n_rows, pl, oa, grads);
    }
    if (int rc = finish(t, who)) return rc;
    t->step_rows = n_rows;
    return AZG_OK;
}

int azg_trainer_step(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                     int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                     const azg_rmsprop* opt, float* square_avg, float* grads, float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step", params, obs, actions, counts, values, n_rows, n_actions, loss_cfg, alpha_state,
                     OptArg{false, opt, square_avg, nullptr}, grads, raw_out, losses);
}

int azg_trainer_step_opt(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                         int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                         const azg_optim* opt, float* grads, float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step_opt", params, obs, actions, counts, values, n_rows, n_actions, loss_cfg, alpha_state,
                     OptArg{true, nullptr, nullptr, opt}, grads, raw_out, losses);
}

static int epoch_impl(azg_trainer* t, const char* who, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                      int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const OptArg& oa,
                      double* loss_sums, int32_t* n_minibatches, bool nets = false) {
    if (!t) return AZG_E_INVALID;
    const std::string w(who);
    const bool no_opt = oa.opt_form ? !oa.opt : (!oa.rms || !oa.square_avg);
    if (!params || !rows || !order || !loss_cfg || no_opt || !loss_sums || !n_minibatches)
        return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    if (rows->struct_size != (int32_t)sizeof(azg_epoch_rows)) return tfail(t, AZG_E_INVALID, w + ": azg_epoch_rows.struct_size mismatch");
    if (!rows->rows) return tfail(t, AZG_E_INVALID, w + ": NULL pointer in azg_epoch_rows");
    if (batch_size < 1 || n_order < 1) return tfail(t, AZG_E_INVALID, w + ": batch_size and n_order must be at least 1");
    const int A = rows->n_actions;
    if (A < 1 || A > TR_MAX_ACTIONS) return tfail(t, AZG_E_INVALID, w + ": n_actions must be 1..16");
    if (rows->state_dim != t->d.in_dim) return tfail(t, AZG_E_INVALID, w + ": state_dim must be the trainer's in_dim");
    if (rows->row_len != rows->state_dim + 3 * A + 1) return tfail(t, AZG_E_INVALID, w + ": row_len must be state_dim + 3 * n_actions + 1");
    if (rows->rows_per_net < 1 || rows->group < 1) return tfail(t, AZG_E_INVALID, w + ": rows_per_net and group must be at least 1");
    if (rows->group_stride < 0 || rows->net_stride < 0) return tfail(t, AZG_E_INVALID, w + ": strides must be >= 0");
    // the minibatches: train_on_rows's rule, the last one absorbing the remainder
    std::vector<int> first, count;
    int largest = 0;
    for (int64_t i = 0; i < n_order;) {
        const int64_t j = i + 2 * (int64_t)batch_size > n_order ? (int64_t)n_order : i + batch_size;
        first.push_back((int)i);
        count.push_back((int)(j - i));
        largest = (int)(j - i) > largest ? (int)(j - i) : largest;
        i = j;
    }
    const int M = (int)first.size();
    if (largest > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": the largest minibatch exceeds max_batch");
    // every refusal of azg_trainer_step, for every minibatch's row count and Adam step
    const bool stepped = alpha_state && loss_cfg->struct_size == (int32_t)sizeof(azg_loss_cfg) && loss_cfg->kind == AZG_LOSS_A0C_TUNED &&
                         alpha_state->struct_size == (int32_t)sizeof(azg_alpha_state);
    if (stepped && alpha_state->step > INT32_MAX - M) return tfail(t, AZG_E_INVALID, w + ": azg_alpha_state.step too large");
    std::vector<LossDims> dims((size_t)M);
    std::vector<OptPlan> plans((size_t)M);
    for (int m = 0; m < M; ++m) {
        azg_alpha_state st{};
        if (stepped) { st = *alpha_state; st.step += m; }
        if (int rc = check_loss(t, who, count[m], A, loss_cfg, stepped ? &st : alpha_state, &dims[m])) return rc;
        if (int rc = check_opt_arg(t, who, params, oa, count[m], m, &plans[m])) return rc;
    }
    if (nets) { if (int rc = plan_nets(t, who, params, oa.opt, loss_cfg, alpha_state, stepped, A, count.data(), M)) return rc; }
    const size_t K = (size_t)t->n_nets;
    for (size_t e = 0; e < K * (size_t)n_order; ++e)
        if (order[e] < 0 || order[e] >= rows->rows_per_net) return tfail(t, AZG_E_INVALID, w + ": an order entry is outside 0 .. rows_per_net - 1");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const size_t mb = (size_t)t->max_batch, per = K * mb * t->d.NO, in_dim = (size_t)t->d.in_dim;
    if (int rc = ensure(t, (void**)&t->loss_rows, K * 3 * mb * sizeof(double))) return rc;
    if (int rc = ensure(t, (void**)&t->d_raw_buf, per * sizeof(float))) return rc;
    if (int rc = ensure(t, (void**)&t->raw_buf, per * sizeof(float))) return rc;
    if (int rc = grow(t, (void**)&t->order_buf, &t->order_bytes, K * (size_t)n_order * sizeof(int32_t))) return rc;
    if (int rc = grow(t, (void**)&t->stage_buf, &t->stage_bytes, K * mb * (in_dim + 2 * (size_t)A + 1) * sizeof(float))) return rc;
    if (int rc = grow(t, (void**)&t->loss_table, &t->table_bytes, (size_t)M * K * AZG_LOSS_SLOTS * sizeof(float))) return rc;
    float* obs = t->stage_buf;
    float* actions = obs + K * mb * in_dim;
    float* counts = actions + K * mb * (size_t)A;
    float* values = counts + K * mb * (size_t)A;
    GatherDims g{};
    g.row_len = rows->row_len; g.state_dim = rows->state_dim; g.A = A; g.group = rows->group; g.n_order = n_order;
    g.group_stride = rows->group_stride; g.net_stride = rows->net_stride;
    t->fwd_rows = 0;
    t->step_rows = 0;
    if (nets) { if (int rc = upload_nets(t, who)) return rc; }
    const hipError_t up = hipMemcpyAsync(t->order_buf, order, K * (size_t)n_order * sizeof(int32_t), hipMemcpyHostToDevice, t->stream);
    if (up != hipSuccess) return tfail(t, AZG_E_DEVICE, w + ": " + hipGetErrorString(up));
    for (int m = 0; m < M; ++m) {
        const int B = count[m];
        hipLaunchKernelGGL(train_gather_kernel, dim3((B + TR_GATHER_THREADS / 64 - 1) / (TR_GATHER_THREADS / 64), t->n_nets),
                           dim3(TR_GATHER_THREADS), 0, t->stream, g, rows->rows, t->order_buf, first[m], B, obs, actions, counts, values);
        launch_forward(t, params, obs, B, t->raw_buf);
        float* mb_losses = t->loss_table + (size_t)m * K * AZG_LOSS_SLOTS;
        if (nets) {
            launch_loss_nets(t, m, dims[m].kind, t->raw_buf, actions, counts, values, B, alpha_state, t->d_raw_buf, mb_losses);
            launch_backward_nets(t, m, params, t->d_raw_buf, B, oa.opt, nullptr);
        } else {
            launch_loss(t, dims[m], t->raw_buf, actions, counts, values, B, alpha_state, t->d_raw_buf, mb_losses);
            launch_backward_arg(t, params, t->d_raw_buf, B, plans[m], oa, nullptr);
        }
    }
    const int n_sums = t->n_nets * AZG_LOSS_SLOTS;
    hipLaunchKernelGGL(train_loss_sum_kernel, dim3((n_sums + 63) / 64), dim3(64), 0, t->stream, t->loss_table, M, n_sums, loss_sums);
    if (int rc = finish(t, who)) return rc;
    t->step_rows = count[M - 1];
    *n_minibatches = M;
    return AZG_OK;
}

int azg_trainer_epoch(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                      int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_rmsprop* opt,
                      float* square_avg, double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch", params, rows, order, n_order, batch_size, loss_cfg, alpha_state,
                      OptArg{false, opt, square_avg, nullptr}, loss_sums, n_minibatches);
}

int azg_trainer_epoch_opt(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                          int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_optim* opt,
                          double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_opt", params, rows, order, n_order, batch_size, loss_cfg, alpha_state,
                      OptArg{true, nullptr, nullptr, opt}, loss_sums, n_minibatches);
}

int azg_trainer_backward_step_nets(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_optim* opts, float* grads) {
    if (!t) return AZG_E_INVALID;
    const char* who = "azg_trainer_backward_step_nets";
    if (!d_raw) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    OptPlan pl;
    if (int rc = check_optim(t, who, params, opts, n_rows, 0, &pl)) return rc;
    const int rows1 = n_rows;
    if (int rc = plan_nets(t, who, params, opts, nullptr, nullptr, false, 0, &rows1, 1)) return rc;
    if (t->fwd_rows != n_rows) return tfail(t, AZG_E_STATE, std::string(who) + ": needs azg_trainer_forward of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    if (int rc = upload_nets(t, who)) return rc;
    t->fwd_rows = 0;
    launch_backward_nets(t, 0, params, d_raw, (int)n_rows, opts, grads);
    return finish(t, who);
}

int azg_trainer_loss_nets(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values, int32_t n_rows,
                          int32_t n_actions, const azg_loss_cfg* cfgs, const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    if (!t) return AZG_E_INVALID;
    const char* who = "azg_trainer_loss_nets";
    if (!raw || !actions || !counts || !values || !d_raw || !losses) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    LossDims c;
    if (int rc = check_loss(t, who, n_rows, n_actions, cfgs, alpha_state, &c)) return rc;
    const int rows1 = n_rows;
    if (int rc = plan_nets(t, who, nullptr, nullptr, cfgs, alpha_state, false, n_actions, &rows1, 1)) return rc;
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    if (int rc = ensure(t, (void**)&t->loss_rows, (size_t)t->n_nets * 3 * t->max_batch * sizeof(double))) return rc;
    if (int rc = upload_nets(t, who)) return rc;
    launch_loss_nets(t, 0, c.kind, raw, actions, counts, values, (int)n_rows, alpha_state, d_raw, losses);
    return finish(t, who);
}

int azg_trainer_step_nets(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                          int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state,
                          const azg_optim* opts, float* grads, float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step_nets", params, obs, actions, counts, values, n_rows, n_actions, loss_cfgs, alpha_state,
                     OptArg{true, nullptr, nullptr, opts}, grads, raw_out, losses, true);
}

int azg_trainer_epoch_nets(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                           int32_t batch_size, const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state, const azg_optim* opts,
                           double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_nets", params, rows, order, n_order, batch_size, loss_cfgs, alpha_state,
                      OptArg{true, nullptr, nullptr, opts}, loss_sums, n_minibatches, true);
}

int azg_trainer_read_d_raw(azg_trainer* t, int32_t n_rows, float* d_raw) {
    if (!t) return AZG_E_INVALID;
    if (!d_raw) return tfail(t, AZG_E_INVALID, "azg_trainer_read_d_raw: NULL pointer");
    if (n_rows < 1 || t->step_rows != n_rows) return tfail(t, AZG_E_STATE, "azg_trainer_read_d_raw: needs an azg_trainer_step of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const hipError_t rc = hipMemcpyAsync(d_raw, t->d_raw_buf, (size_t)t->n_nets * n_rows * t->d.NO * sizeof(float), hipMemcpyDeviceToDevice, t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer_read_d_raw: ") + hipGetErrorString(rc));
    return finish(t, "azg_trainer_read_d_raw");
}

}  // extern "C"
