// online_ring.h -- what the trainer's online epoch (dispatch_train.hip: azg_trainer_epoch_online) takes of an engine's replay ring
// (engine_selfplay.hip, which owns the ring, its scratch and priority_online.cuh's kernels).  The trainer checks, then enqueues on
// its own stream: online_ring_check (nothing written), online_ring_enter (scratch, the engine's stream idle, the ring's marks), and
// per minibatch online_ring_refresh.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/azgym_priority.h"

// what the trainer compares with its own handle, and the errors array its loss launches write
struct OnlineRingShape {
    int device_id = 0, n_nets = 0, obs_dim = 0, n_actions = 0;
    float* err = nullptr;    // [capacity_steps][n_trees]
};

// a minibatch's staging arrays on the trainer's side, [n_nets][n_rows][.] each, and its block of the draw log [n_nets][n_rows]
struct OnlineStage {
    int n_rows = 0;
    float *obs = nullptr, *actions = nullptr, *counts = nullptr, *values = nullptr, *w = nullptr;
    long long* at = nullptr;
    int* drawn = nullptr;
};

// Every refusal azg_selfplay_priorities_trained, azg_selfplay_sample_rows and azg_selfplay_is_weights would make over the loop, with
// their codes, and an empty ring (AZG_E_STATE); the message is the engine's last error.  Nothing is written or launched.
int online_ring_check(azg_engine* e, const azg_trained_priority_config* prio, float beta, OnlineRingShape* shape);
// After every check of the call: the minima's scratch (azg_selfplay_is_weights' own block), the engine's stream synchronised, and
// the ring's marks as the loop leaves them but for the weights -- q counts as computed, the weight array as not.
int online_ring_enter(azg_engine* e);
// Minibatch m's refresh, draw and gather on `stream`: 3 launches, 5 under AZG_UNSEEN_MAX.  Returns hipGetLastError's code.
hipError_t online_ring_refresh(azg_engine* e, hipStream_t stream, const azg_trained_priority_config& prio, float beta,
                               uint32_t sample_index, const OnlineStage& stage);
