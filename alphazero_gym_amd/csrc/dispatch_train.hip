// dispatch_train.hip -- the population trainer's C ABI (include/azgym_train.h).
// Creation: one routine checks the descriptor against the entry point's limits and lays out parameters and scratch (describe_net);
// all four azg_trainer_create* make their handle through create_trainer.  The handle keeps that one TrainNet, the narrow kernels'
// TrainDimsLN copied from it once, and owns its device memory: what lives as long as the handle in a DeviceAllocs, what a call may
// need larger in a DeviceBuffer each.
// Calls: each entry point's checks (nothing launched, nothing written) fill one TrainPlan -- the backward launch's form (fused RMSprop;
// gradients first and norm, clip and update after the last layer; or that with every net's own entry of a device table), the state
// pointers, and per minibatch the launch-ready TrainOptD and LossDims -- before the device scope is entered.  launch_forward,
// launch_loss and launch_backward are the only places that choose between the forms and between train.cuh's kernels (plain,
// LayerNorm) and dispatch_train_wide.hip's launches; a step is an epoch's minibatch body with one minibatch.  The online epoch
// (include/azgym_train_online.h) is an errors epoch whose gather is the engine's refresh, draw and gather (online_ring.h).
// An attached moving average of the parameters (include/azgym_train_ema.h, train_ema.cuh) follows launch_backward, the one place every
// optimiser step leaves through.
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/azgym_train.h"
#include "../../include/azgym_train_weighted.h"
#include "../../include/azgym_train_errors.h"
#include "../../include/azgym_train_online.h"
#include "../../include/azgym_train_ema.h"
#include "hip_host.h"
#include "online_ring.h"
#include "train.cuh"
#include "train_ema.cuh"
#include "train_wide_host.h"

struct azg_trainer {
    int device_id = 0;
    int n_nets = 0, max_batch = 0;
    int fwd_rows = 0;            // rows of the last azg_trainer_forward (0: none)
    int step_rows = 0;           // rows of the d_raw the last azg_trainer_step left in d_raw_buf (0: none)
    int num_components = 0;
    float log_std_min = 0.0f, log_std_max = 0.0f;
    TrainNet net{};
    TrainDimsLN dims{};          // a narrow trainer's kernel argument: net's first TR_MAX_LAYERS layers (the LN = false kernels take its base)
    DeviceAllocs mem;            // everything below up to d_raw_buf
    float* scratch = nullptr;
    float* grad_buf = nullptr;   // [n_nets][P]: where the deferred backward form keeps the gradients when the caller gives no grads
    double* norm_part = nullptr; // a wide trainer's: the deferred norm's partial chains [n_nets][1024]
    // the loss kernel's: the rows' terms [n_nets][3][max_batch] (float64), and azg_trainer_step's raw and d_raw [n_nets][max_batch][NO]
    // (allocated by the first call that needs them)
    double* loss_rows = nullptr;
    double* loss_rows_w = nullptr;   // the weighted loss kernels' own: [n_nets][4][max_batch], allocated by the first weighted call
    float* raw_buf = nullptr;
    float* d_raw_buf = nullptr;
    // azg_trainer_epoch's, grown on demand: the uploaded order [n_nets][n_order], the minibatch staging arrays (obs [n_nets][B][in_dim] |
    // actions | counts [n_nets][B][A] | values [n_nets][B], laid out for max_batch rows) and the loss table [n_minibatches][n_nets][5]
    DeviceBuffer order_buf, stage_buf, loss_table;
    DeviceBuffer stage_w;        // a weighted epoch's staged weights [n_nets][max_batch]
    DeviceBuffer stage_at;       // an errors epoch's staged element indices [n_nets][max_batch] (int64): where each row's error goes
    // the *_nets entry points': the launch-ready settings of every (minibatch, net), [M][n_nets] TrainOptD | [M][n_nets] LossDims (a
    // part the call has no entries for is empty), filled on the host for the whole call and uploaded in one copy; grown on demand
    std::vector<unsigned char> nets_host;
    DeviceBuffer nets_dev;
    // azg_trainer_set_ema: the caller's average [n_nets][P] (NULL: none attached), the device table om[n_nets] = 1 - decay (allocated
    // by the first attach), and the optimiser steps and kernel launches since the attach
    float* ema = nullptr;
    float* ema_om = nullptr;
    int ema_every = 1;
    int64_t ema_steps = 0, ema_updates = 0;
    hipStream_t stream = nullptr;
    std::string err;
};

// (azg_trainer_last_error(NULL) reads the calling thread's own last creation error)
static thread_local std::string g_trainer_create_err;

static int tfail(azg_trainer* t, int code, const std::string& msg) {
    if (t) t->err = msg; else g_trainer_create_err = msg;
    return code;
}

// What an entry point accepts of a descriptor, and how it says no.
struct TrainLimits {
    int max_layers, max_width;
    const char* who;            // the message prefix: azg_trainer_create also for _ex, azg_trainer_create_wide also for _wide_ex
    const char* ln_refusal;     // the refusal of a LayerNorm descriptor where layernorm_ok is false
    bool layernorm_ok;
    bool wide;
};

// Checks the descriptor against the limits and lays out parameters and scratch.  AZG_OK and *out, or a code and the creation error.
static int describe_net(const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const TrainLimits& lim, TrainNet* out) {
    const std::string w = std::string(lim.who) + ": ";
    if (desc->struct_size != (int32_t)sizeof(azg_mlp_desc)) return tfail(nullptr, AZG_E_INVALID, w + "azg_mlp_desc.struct_size mismatch");
    if (n_nets < 1 || max_batch < 1) return tfail(nullptr, AZG_E_INVALID, w + "n_nets and max_batch must be at least 1");
    if (desc->layernorm && !lim.layernorm_ok) return tfail(nullptr, AZG_E_UNSUPPORTED, w + lim.ln_refusal);
    if (desc->n_hidden < 1 || desc->n_hidden > lim.max_layers)
        return tfail(nullptr, AZG_E_UNSUPPORTED, w + "1 to " + std::to_string(lim.max_layers) + " hidden layers");
    if (desc->in_dim < 1 || desc->in_dim > TR_OBS_LD) return tfail(nullptr, AZG_E_UNSUPPORTED, w + "in_dim must be 1..8");
    if (desc->n_dist < 1 || desc->n_dist > 16) return tfail(nullptr, AZG_E_UNSUPPORTED, w + "n_dist must be 1..16");
    if (desc->activation < AZG_ACT_RELU || desc->activation > AZG_ACT_HARDSWISH) return tfail(nullptr, AZG_E_UNSUPPORTED, w + "unknown activation");
    for (int l = 0; l < desc->n_hidden; ++l)
        if (desc->hidden[l] < 16 || desc->hidden[l] > lim.max_width || desc->hidden[l] % 16)
            return tfail(nullptr, AZG_E_UNSUPPORTED, w + "hidden widths must be multiples of 16 up to " + std::to_string(lim.max_width));
    TrainNet d{};
    d.wide = lim.wide;
    d.n_layers = desc->n_hidden; d.in_dim = desc->in_dim; d.nd = desc->n_dist; d.NO = 1 + desc->n_dist; d.act = desc->activation;
    d.layernorm = desc->layernorm ? 1 : 0;
    const size_t Bmax = ((size_t)max_batch + 15) / 16 * 16;
    // (at most 8 * 1024 * 1024 + ... parameters: off stays far below 2^31; so, in 64 bits, stays below 2^47 and is checked at the end)
    int off = 0, prev = d.in_dim;
    size_t so = 0;
    d.s_obs = (unsigned)so; so += Bmax * TR_OBS_LD;
    for (int l = 0; l < d.n_layers; ++l) {
        d.H[l] = desc->hidden[l];
        d.offW[l] = off; off += d.H[l] * prev;
        d.offb[l] = off; off += d.H[l];
        if (d.layernorm) { d.offG[l] = off; off += d.H[l]; d.offB[l] = off; off += d.H[l]; }
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
    if (so >= ((size_t)1 << 32)) return tfail(nullptr, AZG_E_UNSUPPORTED, w + "max_batch too large");   // the kernels' offsets are 32 bits
    *out = d;
    return AZG_OK;
}

// the narrow kernels' argument
static TrainDimsLN narrow_dims(const TrainNet& n) {
    TrainDimsLN d{};
    d.n_layers = n.n_layers; d.in_dim = n.in_dim; d.nd = n.nd; d.NO = n.NO; d.act = n.act;
    d.offWv = n.offWv; d.offbv = n.offbv; d.offbd = n.offbd; d.P = n.P;
    d.s_obs = n.s_obs; d.per_net = n.per_net; d.layernorm = n.layernorm;
    for (int l = 0; l < TR_MAX_LAYERS; ++l) {
        d.H[l] = n.H[l]; d.offW[l] = n.offW[l]; d.offb[l] = n.offb[l]; d.s_A[l] = n.s_A[l]; d.s_D[l] = n.s_D[l];
        d.offG[l] = n.offG[l]; d.offB[l] = n.offB[l]; d.s_X[l] = n.s_X[l]; d.s_G[l] = n.s_G[l]; d.s_R[l] = n.s_R[l];
    }
    return d;
}

extern "C" {

const char* azg_trainer_last_error(const azg_trainer* t) { return t ? t->err.c_str() : g_trainer_create_err.c_str(); }

size_t azg_trainer_param_count(const azg_trainer* t) { return t ? (size_t)t->net.P : 0; }

// (the handle's owners free its device memory, with its device current)
void azg_trainer_destroy(azg_trainer* t) {
    if (!t) return;
    DeviceScope scope(t->device_id);
    if (t->stream) { (void)hipStreamSynchronize(t->stream); (void)hipStreamDestroy(t->stream); }
    delete t;
}

}  // extern "C"

namespace { struct TrainerDestroy { void operator()(azg_trainer* t) const { azg_trainer_destroy(t); } }; }

// The four azg_trainer_create*, behind their NULL and struct_size checks.
static int create_trainer(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const TrainLimits& lim,
                          azg_trainer** out) {
    TrainNet net;
    if (int rc = describe_net(desc, n_nets, max_batch, lim, &net)) return rc;
    std::unique_ptr<azg_trainer, TrainerDestroy> t(new azg_trainer());   // (a failure below leaves through azg_trainer_destroy)
    t->net = net;
    if (!lim.wide) t->dims = narrow_dims(net);
    t->device_id = device_id;
    t->n_nets = n_nets;
    t->max_batch = max_batch;
    t->num_components = desc->num_components;
    t->log_std_min = desc->log_std_min;
    t->log_std_max = desc->log_std_max;
    DeviceScope scope(device_id);
    if (!scope.ok) return tfail(nullptr, AZG_E_DEVICE, "hipSetDevice failed");
    // (the scratch is not cleared: the forward launch writes every scratch element below its padded row count, and the backward
    // launch of the same n_rows reads nothing else)
    const size_t K = (size_t)n_nets;
    hipError_t rc = hipSuccess;
    if (!(t->scratch = t->mem.alloc<float>(t->net.per_net * K)) || !(t->grad_buf = t->mem.alloc<float>(K * (size_t)t->net.P)) ||
        (lim.wide && !(t->norm_part = t->mem.alloc<double>(K * TR_BWD_THREADS))))
        rc = t->mem.last;
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (rc != hipSuccess) {
        (void)hipGetLastError();   // (not left for a later call's finish to report)
        return tfail(nullptr, AZG_E_DEVICE, std::string(lim.who) + ": " + hipGetErrorString(rc));
    }
    *out = t.release();
    return AZG_OK;
}

static TrainLimits narrow_limits(bool layernorm_ok) {
    return TrainLimits{TR_MAX_LAYERS, 256, "azg_trainer_create", "LayerNorm trunks are not trained on the device", layernorm_ok, false};
}
static TrainLimits wide_limits(bool layernorm_ok) {
    return TrainLimits{AZG_MAX_HIDDEN_LAYERS, 1024, "azg_trainer_create_wide", "wide LayerNorm trunks are not trained on the device",
                       layernorm_ok, true};
}

extern "C" {

int azg_trainer_create(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out) {
    if (!desc || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: NULL argument");
    *out = nullptr;
    return create_trainer(device_id, desc, n_nets, max_batch, narrow_limits(false), out);
}

int azg_trainer_create_ex(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const azg_trainer_options* opts,
                          azg_trainer** out) {
    if (!desc || !opts || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_ex: NULL argument");
    *out = nullptr;
    if (opts->struct_size != (int32_t)sizeof(azg_trainer_options))
        return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_ex: azg_trainer_options.struct_size mismatch");
    return create_trainer(device_id, desc, n_nets, max_batch, narrow_limits(opts->layernorm != 0), out);
}

// (the wide entry points leave *out untouched on an error, as their header says; the first two clear it)
int azg_trainer_create_wide(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out) {
    if (!desc || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide: NULL argument");
    return create_trainer(device_id, desc, n_nets, max_batch, wide_limits(false), out);
}

int azg_trainer_create_wide_ex(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, const azg_trainer_options* opts,
                               azg_trainer** out) {
    if (!desc || !opts || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide_ex: NULL argument");
    if (opts->struct_size != (int32_t)sizeof(azg_trainer_options))
        return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create_wide_ex: azg_trainer_options.struct_size mismatch");
    return create_trainer(device_id, desc, n_nets, max_batch, wide_limits(opts->layernorm != 0), out);
}

}  // extern "C"

// ---- what a call launches ----

// The weights argument of a call: `asked` for the *_weighted entry points (whose NULL is a refusal), w the caller's device array.
// The *_errors entry points (azgym_train_errors.h): err_asked, whose NULL `errors` is a refusal and whose NULL w means unweighted; they
// run the weighted path's errors kernels either way.
struct RowWeights {
    bool asked = false;
    const float* w = nullptr;
    bool err_asked = false;
    float* errors = nullptr;
    bool weighted_path() const { return asked || err_asked; }
    bool refused() const { return (asked && !w) || (err_asked && !errors); }
};
static const RowWeights kNoWeights{};
static RowWeights with_errors(const float* w, float* errors) { return RowWeights{false, w, true, errors}; }

enum class OptForm { fused, deferred, table };

struct Minibatch {
    int first = 0, rows = 0;     // its rows of the epoch's order
    TrainOptD o{};               // fused: o.rms is the kernel's TrainOpt
    LossDims c{};                // (table: entry 0's, for its kind)
};

// Seeded by the entry point with the form its name implies (fused for the azg_rmsprop ones, which never leave it; table for *_nets)
// and filled by the checks below.
struct TrainPlan {
    OptForm form = OptForm::fused;
    float* state0 = nullptr;     // square_avg, or Adam's exp_avg_sq
    float* state1 = nullptr;     // Adam's exp_avg
    float* grad_norms = nullptr;
    const azg_alpha_state* alpha = nullptr;   // the tuned loss's state
    // table: where the LossDims part starts in nets_host / nets_dev, and whether some net of the call clips or reports its norm
    size_t loss_off = 0;
    bool any_norm = false;
    std::vector<Minibatch> mb;
    explicit TrainPlan(OptForm f, int n_rows = 0) : form(f), mb(1) { mb[0].rows = n_rows; }
};

// ---- the checks: nothing launched, nothing written ----

static int check_forward(azg_trainer* t, const char* who, const float* params, const float* obs, int32_t n_rows) {
    if (!params || !obs) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, std::string(who) + ": n_rows must be 1..max_batch");
    return AZG_OK;
}

static TrainOpt rmsprop_step(double lr, double alpha, double eps, double weight_decay) {
    TrainOpt o;
    o.lr = (float)lr; o.alpha = (float)alpha; o.one_minus_alpha = (float)(1.0 - alpha); o.eps = (float)eps;
    o.wd = (float)weight_decay;
    return o;
}

// The (azg_rmsprop, square_avg) of the first entry points: always the fused form.
static int check_backward(azg_trainer* t, const char* who, const float* params, const azg_rmsprop* opt, float* square_avg, int32_t n_rows,
                          TrainPlan* plan, TrainOptD* out) {
    const std::string w(who);
    if (!params || !opt || !square_avg) return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    if (opt->struct_size != (int32_t)sizeof(azg_rmsprop)) return tfail(t, AZG_E_INVALID, w + ": azg_rmsprop.struct_size mismatch");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": n_rows must be 1..max_batch");
    if (opt->momentum != 0.0 || opt->centered) return tfail(t, AZG_E_UNSUPPORTED, w + ": RMSprop with momentum or centered is not built");
    if (opt->grad_clip != 0.0) return tfail(t, AZG_E_UNSUPPORTED, w + ": gradient clipping is not built (a per-net global norm needs a pass of its own)");
    plan->state0 = square_avg;
    out->rms = rmsprop_step(opt->lr, opt->alpha, opt->eps, opt->weight_decay);
    return AZG_OK;
}

// An azg_optim as the launch takes it, for the step opt->step + step_add + 1: with plain RMSprop and nothing asked of the gradients
// as a whole the fused kernel (out->rms), else the deferred one.  plan: the form (unless the call's is the table) and the state
// pointers; NULL for the entries of a table, which entry 0 has set.
static int check_optim(azg_trainer* t, const char* who, const float* params, const azg_optim* opt, int32_t n_rows, int step_add,
                       TrainPlan* plan, TrainOptD* out) {
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
    TrainOptD o{};
    o.rms = rmsprop_step(opt->lr, opt->alpha, opt->eps, opt->weight_decay);
    o.kind = opt->kind;
    o.clip = (float)opt->grad_clip;
    o.want_norm = (opt->grad_clip != 0.0 || opt->grad_norms) ? 1 : 0;
    if (adam) {
        const double step = (double)opt->step + (double)step_add + 1.0;
        o.lr = opt->lr; o.b1 = opt->beta1; o.b2 = opt->beta2; o.eps = opt->eps; o.wd = opt->weight_decay;
        o.bc1 = 1.0 - std::pow(o.b1, step);
        o.bc2_sqrt = std::sqrt(1.0 - std::pow(o.b2, step));
    }
    if (plan) {
        if (plan->form != OptForm::table) plan->form = (!adam && !o.want_norm) ? OptForm::fused : OptForm::deferred;
        plan->state0 = opt->state0; plan->state1 = opt->state1; plan->grad_norms = opt->grad_norms;
    }
    *out = o;
    return AZG_OK;
}

// The optimiser of minibatch m, in the form the caller gave it: (rms, square_avg), or opt (entry 0 of a table).
static int check_optimiser(azg_trainer* t, const char* who, const float* params, const azg_rmsprop* rms, float* square_avg,
                           const azg_optim* opt, TrainPlan* plan, int m) {
    Minibatch& mb = plan->mb[m];
    if (rms || square_avg) return check_backward(t, who, params, rms, square_avg, mb.rows, plan, &mb.o);
    return check_optim(t, who, params, opt, mb.rows, m, plan, &mb.o);
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
    const int nd = t->net.nd;
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

static int nets_differ(azg_trainer* t, const char* who, const char* field, int k) {
    return tfail(t, AZG_E_INVALID, std::string(who) + ": " + field + " of net " + std::to_string(k) + " differs from net 0's (it must be equal in every entry)");
}

// (check_optim / check_loss, called without a name, refused entry k: their message behind the entry point's name and the net)
static int net_refused(azg_trainer* t, const char* who, int k, int rc) {
    t->err = std::string(who) + " (net " + std::to_string(k) + ")" + t->err;
    return rc;
}

// Entry 0 has passed the *_opt call's checks.  Here: entries 1 .. n_nets - 1 equal entry 0 where they must; then every entry goes
// through check_optim / check_loss for every minibatch (its rows, Adam steps + m) -- the expressions of the one-net call, so
// the bias corrections and every derived factor are that call's -- and what they return fills the host table.  (They are called with
// an empty name, which a refusal gets from net_refused: a call that passes builds no message string per net.)  opts or cfgs may be
// NULL (a call without that kind of entry).  Nothing is launched or written to the device.
static int plan_nets(azg_trainer* t, const char* who, const float* params, const azg_optim* opts, const azg_loss_cfg* cfgs, bool stepped,
                     int32_t n_actions, TrainPlan* plan) {
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
    const size_t M = plan->mb.size(), n = M * (size_t)K;
    plan->loss_off = opts ? n * sizeof(TrainOptD) : 0;
    t->nets_host.resize(plan->loss_off + (cfgs ? n * sizeof(LossDims) : 0));
    TrainOptD* od = reinterpret_cast<TrainOptD*>(t->nets_host.data());
    LossDims* ld = reinterpret_cast<LossDims*>(t->nets_host.data() + plan->loss_off);
    plan->any_norm = false;
    for (size_t m = 0; m < M; ++m) {
        const int rows = plan->mb[m].rows;
        azg_alpha_state st{};
        if (stepped) { st = *plan->alpha; st.step += (int)m; }
        for (int k = 0; k < K; ++k) {
            if (opts) {
                TrainOptD& o = od[m * K + k];
                if (int rc = check_optim(t, "", params, &opts[k], rows, (int)m, nullptr, &o)) return net_refused(t, who, k, rc);
                plan->any_norm = plan->any_norm || o.want_norm;
            }
            if (cfgs) {
                if (int rc = check_loss(t, "", rows, n_actions, &cfgs[k], stepped ? &st : plan->alpha, &ld[m * K + k]))
                    return net_refused(t, who, k, rc);
            }
        }
    }
    return AZG_OK;
}

// ---- the launches ----

template <typename T>
static int ensure(azg_trainer* t, T*& buf, size_t n) {
    if (buf) return AZG_OK;
    buf = t->mem.alloc<T>(n);
    if (!buf) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer: ") + hipGetErrorString(t->mem.last));
    return AZG_OK;
}

static int grow(azg_trainer* t, DeviceBuffer& buf, size_t bytes) {
    if (!buf.reserve(bytes)) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer: ") + hipGetErrorString(buf.last));
    return AZG_OK;
}

// A table plan's settings to the device: one asynchronous copy on the trainer's stream, in front of the call's first launch.
// nets_host stays as it is until the call's synchronisation.
static int upload_nets(azg_trainer* t, const char* who, const TrainPlan& plan) {
    if (plan.form != OptForm::table) return AZG_OK;
    const size_t bytes = t->nets_host.size();
    if (int rc = grow(t, t->nets_dev, bytes)) return rc;
    const hipError_t up = hipMemcpyAsync(t->nets_dev.p, t->nets_host.data(), bytes, hipMemcpyHostToDevice, t->stream);
    if (up != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string(who) + ": " + hipGetErrorString(up));
    return AZG_OK;
}

// the loss kernels' float64 rows: the unweighted path's three columns, or the weighted path's four in an array of its own
static int ensure_loss_rows(azg_trainer* t, const RowWeights& wt) {
    if (wt.weighted_path()) return ensure(t, t->loss_rows_w, (size_t)t->n_nets * 4 * t->max_batch);
    return ensure(t, t->loss_rows, (size_t)t->n_nets * 3 * t->max_batch);
}

static void launch_forward(azg_trainer* t, const float* params, const float* obs, int n_rows, float* raw) {
    if (t->net.wide) { tw_launch_forward(t->net, t->stream, t->n_nets, params, obs, n_rows, raw, t->scratch); return; }
    const dim3 grid((n_rows + 15) / 16, t->n_nets);
    if (t->net.layernorm) hipLaunchKernelGGL(train_forward_kernel<true>, grid, dim3(64), 0, t->stream, t->dims, params, obs, n_rows, raw, t->scratch);
    else hipLaunchKernelGGL(train_forward_kernel<false>, grid, dim3(64), 0, t->stream, (const TrainDims&)t->dims, params, obs, n_rows, raw, t->scratch);
}

// minibatch m's losses: with the plan's LossDims, or every net with its own entry of the table
// (weights: [n_nets][rows] or NULL; the weighted kernels keep their rows' terms in loss_rows_w.  errors: NULL, or where the errors
// forms of the weighted kernels write each row's value error: errors[err_at[.]], dense with err_at NULL)
static void launch_loss(azg_trainer* t, const TrainPlan& plan, int m, const float* raw, const float* actions, const float* counts,
                        const float* values, const float* weights, float* d_raw, float* losses, const long long* err_at = nullptr,
                        float* errors = nullptr) {
    const Minibatch& mb = plan.mb[m];
    const bool tuned = mb.c.kind == AZG_LOSS_A0C_TUNED;
    float* log_alpha = tuned ? plan.alpha->log_alpha : nullptr;
    float* exp_avg = tuned ? plan.alpha->exp_avg : nullptr;
    float* exp_avg_sq = tuned ? plan.alpha->exp_avg_sq : nullptr;
    if (errors) {
        if (plan.form == OptForm::table) {
            const LossDims* table = reinterpret_cast<const LossDims*>((const unsigned char*)t->nets_dev.p + plan.loss_off) + (size_t)m * t->n_nets;
            hipLaunchKernelGGL(train_loss_nets_errors_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, table, raw, actions, counts,
                               values, weights, mb.rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, t->loss_rows_w, t->max_batch, err_at, errors);
        } else {
            hipLaunchKernelGGL(train_loss_errors_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, mb.c, raw, actions, counts,
                               values, weights, mb.rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, t->loss_rows_w, t->max_batch, err_at, errors);
        }
        return;
    }
    if (weights) {
        if (plan.form == OptForm::table) {
            const LossDims* table = reinterpret_cast<const LossDims*>((const unsigned char*)t->nets_dev.p + plan.loss_off) + (size_t)m * t->n_nets;
            hipLaunchKernelGGL(train_loss_nets_weighted_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, table, raw, actions, counts,
                               values, weights, mb.rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, t->loss_rows_w, t->max_batch);
        } else {
            hipLaunchKernelGGL(train_loss_weighted_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, mb.c, raw, actions, counts,
                               values, weights, mb.rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, t->loss_rows_w, t->max_batch);
        }
        return;
    }
    if (plan.form == OptForm::table) {
        const LossDims* table = reinterpret_cast<const LossDims*>((const unsigned char*)t->nets_dev.p + plan.loss_off) + (size_t)m * t->n_nets;
        hipLaunchKernelGGL(train_loss_nets_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, table, raw, actions, counts, values,
                           mb.rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, t->loss_rows, t->max_batch);
    } else {
        hipLaunchKernelGGL(train_loss_kernel, dim3(t->n_nets), dim3(TR_LOSS_THREADS), 0, t->stream, mb.c, raw, actions, counts, values,
                           mb.rows, log_alpha, exp_avg, exp_avg_sq, d_raw, losses, t->loss_rows, t->max_batch);
    }
}

// The attached average after one more optimiser step: its kernel on the trainer's stream when the step's number is a multiple of `every`
static void launch_ema(azg_trainer* t, const float* params) {
    if (++t->ema_steps % t->ema_every) return;
    const unsigned P = (unsigned)t->net.P;
    const size_t N = (size_t)t->n_nets * P;
    const bool aligned = (((uintptr_t)params | (uintptr_t)t->ema) & 15) == 0 && P >= 4;
    const size_t n4 = aligned ? N / 4 : 0;
    const size_t work = n4 ? n4 : N;
    size_t blocks = (work + TR_EMA_THREADS - 1) / TR_EMA_THREADS;
    if (blocks > TR_EMA_MAX_BLOCKS) blocks = TR_EMA_MAX_BLOCKS;
    hipLaunchKernelGGL(train_ema_kernel, dim3((unsigned)blocks), dim3(TR_EMA_THREADS), 0, t->stream, params, t->ema, t->ema_om, P, n4, N);
    ++t->ema_updates;
}

// minibatch m's backward pass and optimiser step, in the plan's form (a deferred form without the caller's grads keeps them in grad_buf)
static void launch_backward(azg_trainer* t, const TrainPlan& plan, int m, float* params, const float* d_raw, float* grads) {
    const Minibatch& mb = plan.mb[m];
    const int K = t->n_nets, n_rows = mb.rows;
    const dim3 grid(K), block(TR_BWD_THREADS);
    const bool wide = t->net.wide, ln = t->net.layernorm != 0;
    const TrainDimsLN& d = t->dims;
    const TrainDims& d0 = t->dims;
    float *s0 = plan.state0, *s1 = plan.state1, *norms = plan.grad_norms;
    float* gr = grads ? grads : t->grad_buf;
    switch (plan.form) {
    case OptForm::fused:
        if (wide) tw_launch_backward(t->net, t->stream, K, mb.o.rms, params, d_raw, n_rows, s0, grads, t->scratch);
        else if (ln) hipLaunchKernelGGL(train_backward_kernel<true>, grid, block, 0, t->stream, d, mb.o.rms, params, d_raw, n_rows, s0, grads, t->scratch);
        else hipLaunchKernelGGL(train_backward_kernel<false>, grid, block, 0, t->stream, d0, mb.o.rms, params, d_raw, n_rows, s0, grads, t->scratch);
        break;
    case OptForm::deferred:
        if (wide) tw_launch_backward_deferred(t->net, t->stream, K, mb.o, params, d_raw, n_rows, s0, s1, gr, norms, t->scratch, t->norm_part);
        else if (ln) hipLaunchKernelGGL(train_backward_deferred_kernel<true>, grid, block, 0, t->stream, d, mb.o, params, d_raw, n_rows, s0, s1, gr, norms, t->scratch);
        else hipLaunchKernelGGL(train_backward_deferred_kernel<false>, grid, block, 0, t->stream, d0, mb.o, params, d_raw, n_rows, s0, s1, gr, norms, t->scratch);
        break;
    case OptForm::table: {
        const TrainOptD* table = reinterpret_cast<const TrainOptD*>(t->nets_dev.p) + (size_t)m * K;
        if (wide) tw_launch_backward_deferred_nets(t->net, t->stream, K, table, plan.any_norm, params, d_raw, n_rows, s0, s1, gr, norms, t->scratch, t->norm_part);
        else if (ln) hipLaunchKernelGGL(train_backward_deferred_nets_kernel<true>, grid, block, 0, t->stream, d, table, params, d_raw, n_rows, s0, s1, gr, norms, t->scratch);
        else hipLaunchKernelGGL(train_backward_deferred_nets_kernel<false>, grid, block, 0, t->stream, d0, table, params, d_raw, n_rows, s0, s1, gr, norms, t->scratch);
        break;
    }
    }
    if (t->ema) launch_ema(t, params);
}

// one minibatch: forward, losses (d_raw to d_raw_buf), backward and step
static void launch_minibatch(azg_trainer* t, const TrainPlan& plan, int m, float* params, const float* obs, const float* actions,
                             const float* counts, const float* values, const float* weights, float* raw, float* grads, float* losses,
                             const long long* err_at = nullptr, float* errors = nullptr) {
    launch_forward(t, params, obs, plan.mb[m].rows, raw);
    launch_loss(t, plan, m, raw, actions, counts, values, weights, t->d_raw_buf, losses, err_at, errors);
    launch_backward(t, plan, m, params, t->d_raw_buf, grads);
}

static int finish(azg_trainer* t, const char* who) {
    hipError_t rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string(who) + ": " + hipGetErrorString(rc));
    return AZG_OK;
}

// ---- the entry points: one body per family; form = what the entry point's name implies (TrainPlan) ----

static int backward_step_impl(azg_trainer* t, const char* who, OptForm form, float* params, const float* d_raw, int32_t n_rows,
                              const azg_rmsprop* rms, float* square_avg, const azg_optim* opt, float* grads) {
    if (!t) return AZG_E_INVALID;
    if (!d_raw) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    TrainPlan plan(form, n_rows);
    if (int rc = check_optimiser(t, who, params, rms, square_avg, opt, &plan, 0)) return rc;
    if (form == OptForm::table) { if (int rc = plan_nets(t, who, params, opt, nullptr, false, 0, &plan)) return rc; }
    if (t->fwd_rows != n_rows) return tfail(t, AZG_E_STATE, std::string(who) + ": needs azg_trainer_forward of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    if (int rc = upload_nets(t, who, plan)) return rc;
    t->fwd_rows = 0;   // the scratch is consumed: dZ overwrites the activation derivatives
    launch_backward(t, plan, 0, params, d_raw, grads);
    return finish(t, who);
}

static int loss_impl(azg_trainer* t, const char* who, OptForm form, const float* raw, const float* actions, const float* counts,
                     const float* values, const RowWeights& wt, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfg,
                     const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    if (!t) return AZG_E_INVALID;
    if (!raw || !actions || !counts || !values || !d_raw || !losses || wt.refused())
        return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    TrainPlan plan(form, n_rows);
    plan.alpha = alpha_state;
    if (int rc = check_loss(t, who, n_rows, n_actions, cfg, alpha_state, &plan.mb[0].c)) return rc;
    if (form == OptForm::table) { if (int rc = plan_nets(t, who, nullptr, nullptr, cfg, false, n_actions, &plan)) return rc; }
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    if (int rc = ensure_loss_rows(t, wt)) return rc;
    if (int rc = upload_nets(t, who, plan)) return rc;
    launch_loss(t, plan, 0, raw, actions, counts, values, wt.w, d_raw, losses, nullptr, wt.errors);
    return finish(t, who);
}

static int step_impl(azg_trainer* t, const char* who, OptForm form, float* params, const float* obs, const float* actions,
                     const float* counts, const float* values, const RowWeights& wt, int32_t n_rows, int32_t n_actions,
                     const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_rmsprop* rms, float* square_avg,
                     const azg_optim* opt, float* grads, float* raw_out, float* losses) {
    if (!t) return AZG_E_INVALID;
    if (!actions || !counts || !values || !losses || (wt.asked && !wt.w)) return tfail(t, AZG_E_INVALID, std::string(who) + ": NULL pointer");
    if (int rc = check_forward(t, who, params, obs, n_rows)) return rc;
    TrainPlan plan(form, n_rows);
    plan.alpha = alpha_state;
    if (int rc = check_loss(t, who, n_rows, n_actions, loss_cfg, alpha_state, &plan.mb[0].c)) return rc;
    if (int rc = check_optimiser(t, who, params, rms, square_avg, opt, &plan, 0)) return rc;
    if (form == OptForm::table) { if (int rc = plan_nets(t, who, params, opt, loss_cfg, false, n_actions, &plan)) return rc; }
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const size_t per = (size_t)t->n_nets * t->max_batch * t->net.NO;
    if (int rc = ensure_loss_rows(t, wt)) return rc;
    if (int rc = ensure(t, t->d_raw_buf, per)) return rc;
    if (!raw_out) { if (int rc = ensure(t, t->raw_buf, per)) return rc; }
    if (int rc = upload_nets(t, who, plan)) return rc;
    t->fwd_rows = 0;
    t->step_rows = 0;
    launch_minibatch(t, plan, 0, params, obs, actions, counts, values, wt.w, raw_out ? raw_out : t->raw_buf, grads, losses);
    if (int rc = finish(t, who)) return rc;
    t->step_rows = n_rows;
    return AZG_OK;
}

static int epoch_impl(azg_trainer* t, const char* who, OptForm form, float* params, const azg_epoch_rows* rows, const RowWeights& wt,
                      const int32_t* order, int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                      const azg_rmsprop* rms, float* square_avg, const azg_optim* opt, double* loss_sums, int32_t* n_minibatches) {
    if (!t) return AZG_E_INVALID;
    const std::string w(who);
    if (!params || !rows || !order || !loss_cfg || !(opt || (rms && square_avg)) || !loss_sums || !n_minibatches || wt.refused())
        return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    if (rows->struct_size != (int32_t)sizeof(azg_epoch_rows)) return tfail(t, AZG_E_INVALID, w + ": azg_epoch_rows.struct_size mismatch");
    if (!rows->rows) return tfail(t, AZG_E_INVALID, w + ": NULL pointer in azg_epoch_rows");
    if (batch_size < 1 || n_order < 1) return tfail(t, AZG_E_INVALID, w + ": batch_size and n_order must be at least 1");
    const int A = rows->n_actions;
    if (A < 1 || A > TR_MAX_ACTIONS) return tfail(t, AZG_E_INVALID, w + ": n_actions must be 1..16");
    if (rows->state_dim != t->net.in_dim) return tfail(t, AZG_E_INVALID, w + ": state_dim must be the trainer's in_dim");
    if (rows->row_len != rows->state_dim + 3 * A + 1) return tfail(t, AZG_E_INVALID, w + ": row_len must be state_dim + 3 * n_actions + 1");
    if (rows->rows_per_net < 1 || rows->group < 1) return tfail(t, AZG_E_INVALID, w + ": rows_per_net and group must be at least 1");
    if (rows->group_stride < 0 || rows->net_stride < 0) return tfail(t, AZG_E_INVALID, w + ": strides must be >= 0");
    // the minibatches: train_on_rows's rule, the last one absorbing the remainder
    TrainPlan plan(form);
    plan.alpha = alpha_state;
    plan.mb.clear();
    int largest = 0;
    for (int64_t i = 0; i < n_order;) {
        const int64_t j = i + 2 * (int64_t)batch_size > n_order ? (int64_t)n_order : i + batch_size;
        Minibatch mb;
        mb.first = (int)i;
        mb.rows = (int)(j - i);
        plan.mb.push_back(mb);
        largest = mb.rows > largest ? mb.rows : largest;
        i = j;
    }
    const int M = (int)plan.mb.size();
    if (largest > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": the largest minibatch exceeds max_batch");
    // every refusal of azg_trainer_step, for every minibatch's row count and Adam step
    const bool stepped = alpha_state && loss_cfg->struct_size == (int32_t)sizeof(azg_loss_cfg) && loss_cfg->kind == AZG_LOSS_A0C_TUNED &&
                         alpha_state->struct_size == (int32_t)sizeof(azg_alpha_state);
    if (stepped && alpha_state->step > INT32_MAX - M) return tfail(t, AZG_E_INVALID, w + ": azg_alpha_state.step too large");
    for (int m = 0; m < M; ++m) {
        azg_alpha_state st{};
        if (stepped) { st = *alpha_state; st.step += m; }
        if (int rc = check_loss(t, who, plan.mb[m].rows, A, loss_cfg, stepped ? &st : alpha_state, &plan.mb[m].c)) return rc;
        if (int rc = check_optimiser(t, who, params, rms, square_avg, opt, &plan, m)) return rc;
    }
    if (form == OptForm::table) { if (int rc = plan_nets(t, who, params, opt, loss_cfg, stepped, A, &plan)) return rc; }
    const size_t K = (size_t)t->n_nets;
    for (size_t e = 0; e < K * (size_t)n_order; ++e)
        if (order[e] < 0 || order[e] >= rows->rows_per_net) return tfail(t, AZG_E_INVALID, w + ": an order entry is outside 0 .. rows_per_net - 1");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const size_t mb = (size_t)t->max_batch, per = K * mb * t->net.NO, in_dim = (size_t)t->net.in_dim;
    if (int rc = ensure_loss_rows(t, wt)) return rc;
    if (wt.weighted_path()) { if (int rc = grow(t, t->stage_w, K * mb * sizeof(float))) return rc; }
    if (wt.err_asked) { if (int rc = grow(t, t->stage_at, K * mb * sizeof(long long))) return rc; }
    if (int rc = ensure(t, t->d_raw_buf, per)) return rc;
    if (int rc = ensure(t, t->raw_buf, per)) return rc;
    if (int rc = grow(t, t->order_buf, K * (size_t)n_order * sizeof(int32_t))) return rc;
    if (int rc = grow(t, t->stage_buf, K * mb * (in_dim + 2 * (size_t)A + 1) * sizeof(float))) return rc;
    if (int rc = grow(t, t->loss_table, (size_t)M * K * AZG_LOSS_SLOTS * sizeof(float))) return rc;
    int* order_dev = (int*)t->order_buf.p;
    float* loss_table = (float*)t->loss_table.p;
    float* obs = (float*)t->stage_buf.p;
    float* actions = obs + K * mb * in_dim;
    float* counts = actions + K * mb * (size_t)A;
    float* values = counts + K * mb * (size_t)A;
    float* staged_w = wt.weighted_path() ? (float*)t->stage_w.p : nullptr;
    long long* staged_at = wt.err_asked ? (long long*)t->stage_at.p : nullptr;
    GatherDims g{};
    g.row_len = rows->row_len; g.state_dim = rows->state_dim; g.A = A; g.group = rows->group; g.n_order = n_order;
    g.group_stride = rows->group_stride; g.net_stride = rows->net_stride;
    t->fwd_rows = 0;
    t->step_rows = 0;
    if (int rc = upload_nets(t, who, plan)) return rc;
    const hipError_t up = hipMemcpyAsync(order_dev, order, K * (size_t)n_order * sizeof(int32_t), hipMemcpyHostToDevice, t->stream);
    if (up != hipSuccess) return tfail(t, AZG_E_DEVICE, w + ": " + hipGetErrorString(up));
    for (int m = 0; m < M; ++m) {
        const int B = plan.mb[m].rows;
        const dim3 ggrid((B + TR_GATHER_THREADS / 64 - 1) / (TR_GATHER_THREADS / 64), t->n_nets);
        if (wt.err_asked)
            hipLaunchKernelGGL(train_gather_errors_kernel, ggrid, dim3(TR_GATHER_THREADS), 0, t->stream, g, rows->rows, wt.w, order_dev,
                               plan.mb[m].first, B, obs, actions, counts, values, staged_w, staged_at);
        else if (wt.asked)
            hipLaunchKernelGGL(train_gather_weighted_kernel, ggrid, dim3(TR_GATHER_THREADS), 0, t->stream, g, rows->rows, wt.w, order_dev,
                               plan.mb[m].first, B, obs, actions, counts, values, staged_w);
        else
            hipLaunchKernelGGL(train_gather_kernel, ggrid, dim3(TR_GATHER_THREADS), 0, t->stream, g, rows->rows, order_dev, plan.mb[m].first, B,
                               obs, actions, counts, values);
        launch_minibatch(t, plan, m, params, obs, actions, counts, values, staged_w, t->raw_buf, nullptr,
                         loss_table + (size_t)m * K * AZG_LOSS_SLOTS, staged_at, wt.errors);
    }
    const int n_sums = t->n_nets * AZG_LOSS_SLOTS;
    hipLaunchKernelGGL(train_loss_sum_kernel, dim3((n_sums + 63) / 64), dim3(64), 0, t->stream, loss_table, M, n_sums, loss_sums);
    if (int rc = finish(t, who)) return rc;
    t->step_rows = plan.mb[M - 1].rows;
    *n_minibatches = M;
    return AZG_OK;
}

// include/azgym_train_online.h: an errors epoch of M whole minibatches over the engine's ring whose gather is the ring's refresh,
// draw and gather (online_ring.h).  The checks are the loop's: the ring's, then epoch_impl's for M minibatches of batch_size rows.
static int epoch_online_impl(azg_trainer* t, const char* who, OptForm form, azg_engine* e, float* params, const azg_online_epoch* cfg,
                             const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_optim* opt, double* loss_sums) {
    if (!t) return AZG_E_INVALID;
    const std::string w(who);
    if (!e || !cfg) return tfail(t, AZG_E_INVALID, w + ": engine and cfg must not be NULL");
    if (cfg->struct_size != (int32_t)sizeof(azg_online_epoch)) return tfail(t, AZG_E_INVALID, w + ": azg_online_epoch.struct_size mismatch");
    if (cfg->n_minibatches < 1) return tfail(t, AZG_E_INVALID, w + ": n_minibatches must be at least 1");
    if (cfg->batch_size < 1 || cfg->batch_size > t->max_batch) return tfail(t, AZG_E_INVALID, w + ": batch_size must be 1..max_batch");
    if (!params || !loss_cfg || !opt || !loss_sums) return tfail(t, AZG_E_INVALID, w + ": NULL pointer");
    OnlineRingShape ring;
    if (int rc = online_ring_check(e, &cfg->prio, cfg->beta, &ring)) return tfail(t, rc, w + ": " + azg_last_error(e));
    if (ring.device_id != t->device_id) return tfail(t, AZG_E_INVALID, w + ": the engine and the trainer are on different devices");
    if (ring.n_nets != t->n_nets) return tfail(t, AZG_E_INVALID, w + ": the engine's n_nets is not the trainer's");
    if (ring.obs_dim != t->net.in_dim) return tfail(t, AZG_E_INVALID, w + ": the engine's observation width must be the trainer's in_dim");
    const int A = ring.n_actions, M = cfg->n_minibatches, B = cfg->batch_size;
    if (A < 1 || A > TR_MAX_ACTIONS) return tfail(t, AZG_E_INVALID, w + ": the engine's action count must be 1..16");
    // every refusal of azg_trainer_step, for every minibatch's Adam step (epoch_impl's)
    TrainPlan plan(form);
    plan.alpha = alpha_state;
    plan.mb.assign((size_t)M, Minibatch{});
    const bool stepped = alpha_state && loss_cfg->struct_size == (int32_t)sizeof(azg_loss_cfg) && loss_cfg->kind == AZG_LOSS_A0C_TUNED &&
                         alpha_state->struct_size == (int32_t)sizeof(azg_alpha_state);
    if (stepped && alpha_state->step > INT32_MAX - M) return tfail(t, AZG_E_INVALID, w + ": azg_alpha_state.step too large");
    for (int m = 0; m < M; ++m) {
        plan.mb[m].first = m * B; plan.mb[m].rows = B;
        azg_alpha_state st{};
        if (stepped) { st = *alpha_state; st.step += m; }
        if (int rc = check_loss(t, who, B, A, loss_cfg, stepped ? &st : alpha_state, &plan.mb[m].c)) return rc;
        if (int rc = check_optimiser(t, who, params, nullptr, nullptr, opt, &plan, m)) return rc;
    }
    if (form == OptForm::table) { if (int rc = plan_nets(t, who, params, opt, loss_cfg, stepped, A, &plan)) return rc; }
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const RowWeights wt = with_errors(nullptr, ring.err);
    const size_t K = (size_t)t->n_nets, mb = (size_t)t->max_batch, per = K * mb * t->net.NO, in_dim = (size_t)t->net.in_dim;
    const size_t n_drawn = (size_t)M * K * (size_t)B;
    if (int rc = ensure_loss_rows(t, wt)) return rc;
    if (int rc = grow(t, t->stage_w, K * mb * sizeof(float))) return rc;
    if (int rc = grow(t, t->stage_at, K * mb * sizeof(long long))) return rc;
    if (int rc = ensure(t, t->d_raw_buf, per)) return rc;
    if (int rc = ensure(t, t->raw_buf, per)) return rc;
    if (int rc = grow(t, t->order_buf, n_drawn * sizeof(int32_t))) return rc;
    if (int rc = grow(t, t->stage_buf, K * mb * (in_dim + 2 * (size_t)A + 1) * sizeof(float))) return rc;
    if (int rc = grow(t, t->loss_table, (size_t)M * K * AZG_LOSS_SLOTS * sizeof(float))) return rc;
    if (int rc = online_ring_enter(e)) return tfail(t, rc, w + ": " + azg_last_error(e));
    float* loss_table = (float*)t->loss_table.p;
    OnlineStage st;
    st.n_rows = B;
    st.obs = (float*)t->stage_buf.p;
    st.actions = st.obs + K * mb * in_dim;
    st.counts = st.actions + K * mb * (size_t)A;
    st.values = st.counts + K * mb * (size_t)A;
    st.w = (float*)t->stage_w.p;
    st.at = (long long*)t->stage_at.p;
    t->fwd_rows = 0;
    t->step_rows = 0;
    if (int rc = upload_nets(t, who, plan)) return rc;
    for (int m = 0; m < M; ++m) {
        st.drawn = (int*)t->order_buf.p + (size_t)m * K * B;
        const hipError_t rc = online_ring_refresh(e, t->stream, cfg->prio, cfg->beta, cfg->sample_index + (uint32_t)m, st);
        if (rc != hipSuccess) { (void)hipStreamSynchronize(t->stream); return tfail(t, AZG_E_DEVICE, w + ": " + hipGetErrorString(rc)); }
        launch_minibatch(t, plan, m, params, st.obs, st.actions, st.counts, st.values, st.w, t->raw_buf, nullptr,
                         loss_table + (size_t)m * K * AZG_LOSS_SLOTS, st.at, wt.errors);
    }
    const int n_sums = t->n_nets * AZG_LOSS_SLOTS;
    hipLaunchKernelGGL(train_loss_sum_kernel, dim3((n_sums + 63) / 64), dim3(64), 0, t->stream, loss_table, M, n_sums, loss_sums);
    if (cfg->drawn) {
        const hipError_t down = hipMemcpyAsync(cfg->drawn, t->order_buf.p, n_drawn * sizeof(int32_t), hipMemcpyDeviceToHost, t->stream);
        if (down != hipSuccess) { (void)hipStreamSynchronize(t->stream); return tfail(t, AZG_E_DEVICE, w + ": " + hipGetErrorString(down)); }
    }
    if (int rc = finish(t, who)) return rc;
    t->step_rows = B;
    return AZG_OK;
}

extern "C" {

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
    return backward_step_impl(t, "azg_trainer_backward_step", OptForm::fused, params, d_raw, n_rows, opt, square_avg, nullptr, grads);
}

int azg_trainer_backward_step_opt(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_optim* opt, float* grads) {
    return backward_step_impl(t, "azg_trainer_backward_step_opt", OptForm::fused, params, d_raw, n_rows, nullptr, nullptr, opt, grads);
}

int azg_trainer_backward_step_nets(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_optim* opts, float* grads) {
    return backward_step_impl(t, "azg_trainer_backward_step_nets", OptForm::table, params, d_raw, n_rows, nullptr, nullptr, opts, grads);
}

int azg_trainer_loss(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values, int32_t n_rows,
                     int32_t n_actions, const azg_loss_cfg* cfg, const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    return loss_impl(t, "azg_trainer_loss", OptForm::fused, raw, actions, counts, values, kNoWeights, n_rows, n_actions, cfg, alpha_state, d_raw, losses);
}

int azg_trainer_loss_nets(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values, int32_t n_rows,
                          int32_t n_actions, const azg_loss_cfg* cfgs, const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    return loss_impl(t, "azg_trainer_loss_nets", OptForm::table, raw, actions, counts, values, kNoWeights, n_rows, n_actions, cfgs, alpha_state, d_raw, losses);
}

int azg_trainer_step(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                     int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                     const azg_rmsprop* opt, float* square_avg, float* grads, float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step", OptForm::fused, params, obs, actions, counts, values, kNoWeights, n_rows, n_actions, loss_cfg, alpha_state,
                     opt, square_avg, nullptr, grads, raw_out, losses);
}

int azg_trainer_step_opt(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                         int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                         const azg_optim* opt, float* grads, float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step_opt", OptForm::fused, params, obs, actions, counts, values, kNoWeights, n_rows, n_actions, loss_cfg, alpha_state,
                     nullptr, nullptr, opt, grads, raw_out, losses);
}

int azg_trainer_step_nets(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts, const float* values,
                          int32_t n_rows, int32_t n_actions, const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state,
                          const azg_optim* opts, float* grads, float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step_nets", OptForm::table, params, obs, actions, counts, values, kNoWeights, n_rows, n_actions, loss_cfgs,
                     alpha_state, nullptr, nullptr, opts, grads, raw_out, losses);
}

int azg_trainer_epoch(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                      int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_rmsprop* opt,
                      float* square_avg, double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch", OptForm::fused, params, rows, kNoWeights, order, n_order, batch_size, loss_cfg, alpha_state, opt, square_avg,
                      nullptr, loss_sums, n_minibatches);
}

int azg_trainer_epoch_opt(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                          int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_optim* opt,
                          double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_opt", OptForm::fused, params, rows, kNoWeights, order, n_order, batch_size, loss_cfg, alpha_state, nullptr,
                      nullptr, opt, loss_sums, n_minibatches);
}

int azg_trainer_epoch_nets(azg_trainer* t, float* params, const azg_epoch_rows* rows, const int32_t* order, int32_t n_order,
                           int32_t batch_size, const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state, const azg_optim* opts,
                           double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_nets", OptForm::table, params, rows, kNoWeights, order, n_order, batch_size, loss_cfgs, alpha_state, nullptr,
                      nullptr, opts, loss_sums, n_minibatches);
}

// ---- the weighted forms (include/azgym_train_weighted.h): the namesake's body with the weights

int azg_trainer_loss_weighted(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                              const float* weights, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfg,
                              const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    return loss_impl(t, "azg_trainer_loss_weighted", OptForm::fused, raw, actions, counts, values, RowWeights{true, weights}, n_rows, n_actions,
                     cfg, alpha_state, d_raw, losses);
}

int azg_trainer_loss_nets_weighted(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                                   const float* weights, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfgs,
                                   const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    return loss_impl(t, "azg_trainer_loss_nets_weighted", OptForm::table, raw, actions, counts, values, RowWeights{true, weights}, n_rows,
                     n_actions, cfgs, alpha_state, d_raw, losses);
}

int azg_trainer_step_opt_weighted(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts,
                                  const float* values, const float* weights, int32_t n_rows, int32_t n_actions,
                                  const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state, const azg_optim* opt, float* grads,
                                  float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step_opt_weighted", OptForm::fused, params, obs, actions, counts, values, RowWeights{true, weights}, n_rows,
                     n_actions, loss_cfg, alpha_state, nullptr, nullptr, opt, grads, raw_out, losses);
}

int azg_trainer_step_nets_weighted(azg_trainer* t, float* params, const float* obs, const float* actions, const float* counts,
                                   const float* values, const float* weights, int32_t n_rows, int32_t n_actions,
                                   const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state, const azg_optim* opts, float* grads,
                                   float* raw_out, float* losses) {
    return step_impl(t, "azg_trainer_step_nets_weighted", OptForm::table, params, obs, actions, counts, values, RowWeights{true, weights}, n_rows,
                     n_actions, loss_cfgs, alpha_state, nullptr, nullptr, opts, grads, raw_out, losses);
}

int azg_trainer_epoch_opt_weighted(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, const int32_t* order,
                                   int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfg, const azg_alpha_state* alpha_state,
                                   const azg_optim* opt, double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_opt_weighted", OptForm::fused, params, rows, RowWeights{true, weights}, order, n_order, batch_size,
                      loss_cfg, alpha_state, nullptr, nullptr, opt, loss_sums, n_minibatches);
}

int azg_trainer_epoch_nets_weighted(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, const int32_t* order,
                                    int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state,
                                    const azg_optim* opts, double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_nets_weighted", OptForm::table, params, rows, RowWeights{true, weights}, order, n_order, batch_size,
                      loss_cfgs, alpha_state, nullptr, nullptr, opts, loss_sums, n_minibatches);
}

// ---- the errors forms (include/azgym_train_errors.h): the weighted namesake's body, the rows' value errors written by the loss launch

int azg_trainer_loss_errors(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                            const float* weights, float* errors, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfg,
                            const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    return loss_impl(t, "azg_trainer_loss_errors", OptForm::fused, raw, actions, counts, values, with_errors(weights, errors), n_rows, n_actions,
                     cfg, alpha_state, d_raw, losses);
}

int azg_trainer_loss_nets_errors(azg_trainer* t, const float* raw, const float* actions, const float* counts, const float* values,
                                 const float* weights, float* errors, int32_t n_rows, int32_t n_actions, const azg_loss_cfg* cfgs,
                                 const azg_alpha_state* alpha_state, float* d_raw, float* losses) {
    return loss_impl(t, "azg_trainer_loss_nets_errors", OptForm::table, raw, actions, counts, values, with_errors(weights, errors), n_rows,
                     n_actions, cfgs, alpha_state, d_raw, losses);
}

int azg_trainer_epoch_opt_errors(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, float* errors,
                                 const int32_t* order, int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfg,
                                 const azg_alpha_state* alpha_state, const azg_optim* opt, double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_opt_errors", OptForm::fused, params, rows, with_errors(weights, errors), order, n_order, batch_size,
                      loss_cfg, alpha_state, nullptr, nullptr, opt, loss_sums, n_minibatches);
}

int azg_trainer_epoch_nets_errors(azg_trainer* t, float* params, const azg_epoch_rows* rows, const float* weights, float* errors,
                                  const int32_t* order, int32_t n_order, int32_t batch_size, const azg_loss_cfg* loss_cfgs,
                                  const azg_alpha_state* alpha_state, const azg_optim* opts, double* loss_sums, int32_t* n_minibatches) {
    return epoch_impl(t, "azg_trainer_epoch_nets_errors", OptForm::table, params, rows, with_errors(weights, errors), order, n_order, batch_size,
                      loss_cfgs, alpha_state, nullptr, nullptr, opts, loss_sums, n_minibatches);
}

// ---- the online epoch (include/azgym_train_online.h): an errors epoch whose every minibatch is redrawn from the engine's ring

int azg_trainer_epoch_online(azg_trainer* t, azg_engine* e, float* params, const azg_online_epoch* cfg, const azg_loss_cfg* loss_cfg,
                             const azg_alpha_state* alpha_state, const azg_optim* opt, double* loss_sums) {
    return epoch_online_impl(t, "azg_trainer_epoch_online", OptForm::fused, e, params, cfg, loss_cfg, alpha_state, opt, loss_sums);
}

int azg_trainer_epoch_online_nets(azg_trainer* t, azg_engine* e, float* params, const azg_online_epoch* cfg,
                                  const azg_loss_cfg* loss_cfgs, const azg_alpha_state* alpha_state, const azg_optim* opts,
                                  double* loss_sums) {
    return epoch_online_impl(t, "azg_trainer_epoch_online_nets", OptForm::table, e, params, cfg, loss_cfgs, alpha_state, opts, loss_sums);
}

// ---- the moving average of the parameters (include/azgym_train_ema.h)

int azg_trainer_set_ema(azg_trainer* t, const azg_ema_cfg* cfg) {
    if (!t) return AZG_E_INVALID;
    const std::string w("azg_trainer_set_ema");
    if (!cfg) {   // (the table stays with the handle; the stream is idle between calls)
        t->ema = nullptr;
        t->ema_every = 1;
        t->ema_steps = t->ema_updates = 0;
        return AZG_OK;
    }
    if (cfg->struct_size != (int32_t)sizeof(azg_ema_cfg)) return tfail(t, AZG_E_INVALID, w + ": azg_ema_cfg.struct_size mismatch");
    if (!cfg->ema || !cfg->decay) return tfail(t, AZG_E_INVALID, w + ": NULL pointer in azg_ema_cfg");
    if (cfg->n_decay != 1 && cfg->n_decay != t->n_nets) return tfail(t, AZG_E_INVALID, w + ": n_decay must be 1 or the trainer's n_nets");
    if (cfg->every < 1) return tfail(t, AZG_E_INVALID, w + ": every must be at least 1");
    std::vector<float> om((size_t)t->n_nets);
    for (int k = 0; k < t->n_nets; ++k) {
        const double d = cfg->decay[cfg->n_decay == 1 ? 0 : k];
        if (!std::isfinite(d) || d < 0.0 || !(d < 1.0))
            return tfail(t, AZG_E_INVALID, w + ": decay of net " + std::to_string(k) + " must be finite and in [0, 1)");
        om[k] = (float)(1.0 - d);
    }
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    if (int rc = ensure(t, t->ema_om, (size_t)t->n_nets)) return rc;
    // (no launch of an earlier attach is in flight: every entry point ends with the stream's synchronisation)
    hipError_t rc = hipMemcpyAsync(t->ema_om, om.data(), om.size() * sizeof(float), hipMemcpyHostToDevice, t->stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, w + ": " + hipGetErrorString(rc));
    t->ema = cfg->ema;
    t->ema_every = cfg->every;
    t->ema_steps = t->ema_updates = 0;
    return AZG_OK;
}

int azg_trainer_ema_info(const azg_trainer* t, int64_t* steps_seen, int64_t* updates_made) {
    if (!t) return AZG_E_INVALID;
    if (steps_seen) *steps_seen = t->ema_steps;
    if (updates_made) *updates_made = t->ema_updates;
    return AZG_OK;
}

int azg_trainer_read_d_raw(azg_trainer* t, int32_t n_rows, float* d_raw) {
    if (!t) return AZG_E_INVALID;
    if (!d_raw) return tfail(t, AZG_E_INVALID, "azg_trainer_read_d_raw: NULL pointer");
    if (n_rows < 1 || t->step_rows != n_rows) return tfail(t, AZG_E_STATE, "azg_trainer_read_d_raw: needs an azg_trainer_step of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    const hipError_t rc = hipMemcpyAsync(d_raw, t->d_raw_buf, (size_t)t->n_nets * n_rows * t->net.NO * sizeof(float), hipMemcpyDeviceToDevice, t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer_read_d_raw: ") + hipGetErrorString(rc));
    return finish(t, "azg_trainer_read_d_raw");
}

}  // extern "C"
