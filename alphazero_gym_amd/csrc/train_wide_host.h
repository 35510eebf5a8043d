// train_wide_host.h -- what dispatch_train.hip (the trainer's C ABI) asks of dispatch_train_wide.hip (the wide trainer's checks and
// launches).  Include after train.cuh (TrainOpt, TrainOptD).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include <hip/hip_runtime.h>

#include "../../include/azgym_train.h"

struct TrainWide;   // the dims of a wide trainer (train_wide.cuh: TrainDimsW); host memory only

// Checks the descriptor against azg_trainer_create_wide's accepted set (layernorm_ok: azg_trainer_create_wide_ex's, which also has
// LayerNorm trunks) and lays out parameters and scratch.  AZG_OK and *out, or a code and *msg (nothing allocated).
int tw_plan(const azg_mlp_desc* desc, int32_t max_batch, bool layernorm_ok, TrainWide** out, std::string* msg);
void tw_free(TrainWide* w);
int tw_param_count(const TrainWide* w);
size_t tw_scratch_floats(const TrainWide* w);   // per net

// Enqueue on `stream` (a LayerNorm plan: with the row passes): the forward launches; the backward launches with the fused RMSprop step; the backward launches that store the
// gradients, then norm (partials: [n_nets][1024] float64 of the trainer), clip and update.
void tw_launch_forward(const TrainWide* w, hipStream_t stream, int n_nets, const float* params, const float* obs, int n_rows, float* raw,
                       float* scratch);
void tw_launch_backward(const TrainWide* w, hipStream_t stream, int n_nets, const TrainOpt& opt, float* params, const float* d_raw, int n_rows,
                        float* square_avg, float* grads, float* scratch);
void tw_launch_backward_deferred(const TrainWide* w, hipStream_t stream, int n_nets, const TrainOptD& opt, float* params, const float* d_raw,
                                 int n_rows, float* state0, float* state1, float* grads, float* norms, float* scratch, double* partials);
// ... with every net's own settings: table = [n_nets] TrainOptD in device memory, filled by a copy enqueued on `stream` before this;
// any_norm = some entry has want_norm set (the norm launch is made for all nets then).
void tw_launch_backward_deferred_nets(const TrainWide* w, hipStream_t stream, int n_nets, const TrainOptD* table, bool any_norm, float* params,
                                      const float* d_raw, int n_rows, float* state0, float* state1, float* grads, float* norms,
                                      float* scratch, double* partials);
