// dispatch_train.hip -- the population trainer's C ABI (include/azgym_train.h): scratch, checks and the two launches of train.cuh.
#include <string>

#include "../../include/azgym_train.h"
#include "hip_host.h"
#include "train.cuh"

struct azg_trainer {
    int device_id = 0;
    int n_nets = 0, max_batch = 0;
    int fwd_rows = 0;            // rows of the last azg_trainer_forward (0: none)
    TrainDims d{};
    float* scratch = nullptr;
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
    delete t;
}

int azg_trainer_create(int32_t device_id, const azg_mlp_desc* desc, int32_t n_nets, int32_t max_batch, azg_trainer** out) {
    if (!desc || !out) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(azg_mlp_desc)) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: azg_mlp_desc.struct_size mismatch");
    if (n_nets < 1 || max_batch < 1) return tfail(nullptr, AZG_E_INVALID, "azg_trainer_create: n_nets and max_batch must be at least 1");
    if (desc->layernorm) return tfail(nullptr, AZG_E_UNSUPPORTED, "azg_trainer_create: LayerNorm trunks are not trained on the device");
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
    TrainDims& d = t->d;
    d.n_layers = desc->n_hidden; d.in_dim = desc->in_dim; d.nd = desc->n_dist; d.NO = 1 + desc->n_dist; d.act = desc->activation;
    const size_t Bmax = ((size_t)max_batch + 15) / 16 * 16;
    int off = 0, prev = d.in_dim;
    size_t so = 0;
    d.s_obs = (unsigned)so; so += Bmax * TR_OBS_LD;
    for (int l = 0; l < d.n_layers; ++l) {
        d.H[l] = desc->hidden[l];
        d.offW[l] = off; off += d.H[l] * prev;
        d.offb[l] = off; off += d.H[l];
        d.s_A[l] = (unsigned)so; so += Bmax * d.H[l];
        d.s_D[l] = (unsigned)so; so += Bmax * d.H[l];
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
    if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (rc != hipSuccess) {
        const std::string msg = std::string("azg_trainer_create: ") + hipGetErrorString(rc);
        azg_trainer_destroy(t);
        return tfail(nullptr, AZG_E_DEVICE, msg);
    }
    *out = t;
    return AZG_OK;
}

int azg_trainer_forward(azg_trainer* t, const float* params, const float* obs, int32_t n_rows, float* raw) {
    if (!t) return AZG_E_INVALID;
    if (!params || !obs || !raw) return tfail(t, AZG_E_INVALID, "azg_trainer_forward: NULL pointer");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, "azg_trainer_forward: n_rows must be 1..max_batch");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    t->fwd_rows = 0;
    hipLaunchKernelGGL(train_forward_kernel, dim3((n_rows + 15) / 16, t->n_nets), dim3(64), 0, t->stream, t->d, params, obs, (int)n_rows, raw,
                       t->scratch);
    hipError_t rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer_forward: ") + hipGetErrorString(rc));
    t->fwd_rows = n_rows;
    return AZG_OK;
}

int azg_trainer_backward_step(azg_trainer* t, float* params, const float* d_raw, int32_t n_rows, const azg_rmsprop* opt, float* square_avg,
                              float* grads) {
    if (!t) return AZG_E_INVALID;
    if (!params || !d_raw || !opt || !square_avg) return tfail(t, AZG_E_INVALID, "azg_trainer_backward_step: NULL pointer");
    if (opt->struct_size != (int32_t)sizeof(azg_rmsprop)) return tfail(t, AZG_E_INVALID, "azg_trainer_backward_step: azg_rmsprop.struct_size mismatch");
    if (n_rows < 1 || n_rows > t->max_batch) return tfail(t, AZG_E_INVALID, "azg_trainer_backward_step: n_rows must be 1..max_batch");
    if (opt->momentum != 0.0 || opt->centered) return tfail(t, AZG_E_UNSUPPORTED, "azg_trainer_backward_step: RMSprop with momentum or centered is not built");
    if (opt->grad_clip != 0.0) return tfail(t, AZG_E_UNSUPPORTED, "azg_trainer_backward_step: gradient clipping is not built (a per-net global norm needs a pass of its own)");
    if (t->fwd_rows != n_rows) return tfail(t, AZG_E_STATE, "azg_trainer_backward_step: needs azg_trainer_forward of the same n_rows first");
    DeviceScope scope(t->device_id);
    if (!scope.ok) return tfail(t, AZG_E_DEVICE, "hipSetDevice failed");
    TrainOpt o;
    o.lr = (float)opt->lr; o.alpha = (float)opt->alpha; o.one_minus_alpha = (float)(1.0 - opt->alpha); o.eps = (float)opt->eps;
    o.wd = (float)opt->weight_decay;
    t->fwd_rows = 0;   // the scratch is consumed: dZ overwrites the activation derivatives
    hipLaunchKernelGGL(train_backward_kernel, dim3(t->n_nets), dim3(TR_BWD_THREADS), 0, t->stream, t->d, o, params, d_raw, (int)n_rows,
                       square_avg, grads, t->scratch);
    hipError_t rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipStreamSynchronize(t->stream);
    if (rc != hipSuccess) return tfail(t, AZG_E_DEVICE, std::string("azg_trainer_backward_step: ") + hipGetErrorString(rc));
    return AZG_OK;
}

}  // extern "C"
