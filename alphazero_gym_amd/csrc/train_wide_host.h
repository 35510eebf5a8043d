// train_wide_host.h -- what dispatch_train.hip (the trainer's C ABI, its checks and its layout) asks of dispatch_train_wide.hip: the wide
// nets' launches, one per layer and role.  Include after train.cuh (TrainOpt, TrainOptD).
#pragma once
#include <hip/hip_runtime.h>

#include "train_net.h"

// Enqueue on `stream` (a LayerNorm net: with the row passes): the forward launches; the backward launches with the fused RMSprop
// step; the backward launches that store the gradients, then norm (partials: [n_nets][1024] float64 of the trainer), clip and update.
void tw_launch_forward(const TrainNet& d, hipStream_t stream, int n_nets, const float* params, const float* obs, int n_rows, float* raw,
                       float* scratch);
void tw_launch_backward(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOpt& opt, float* params, const float* d_raw, int n_rows,
                        float* square_avg, float* grads, float* scratch);
void tw_launch_backward_deferred(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOptD& opt, float* params, const float* d_raw,
                                 int n_rows, float* state0, float* state1, float* grads, float* norms, float* scratch, double* partials);
// ... with every net's own settings: table = [n_nets] TrainOptD in device memory, filled by a copy enqueued on `stream` before this;
// any_norm = some entry has want_norm set (the norm launch is made for all nets then).
void tw_launch_backward_deferred_nets(const TrainNet& d, hipStream_t stream, int n_nets, const TrainOptD* table, bool any_norm, float* params,
                                      const float* d_raw, int n_rows, float* state0, float* state1, float* grads, float* norms,
                                      float* scratch, double* partials);
