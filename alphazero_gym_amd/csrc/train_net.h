// train_net.h -- the trainer's one host-side description of its net: dims, parameter offsets (state_dict order) and the scratch layout
// of one net.  dispatch_train.hip checks a descriptor and lays it out once at creation, for either kind of trainer; the narrow kernels'
// TrainDimsLN argument is a copy of its first three layers, and a wide launch gets the slice it needs as one of train_wide.cuh's
// argument structs.  Host memory only.
#pragma once
#include <cstddef>

#include "../../include/azgym.h"

struct TrainNet {
    bool wide;                                      // made by azg_trainer_create_wide(_ex): dispatch_train_wide.hip's launches
    int n_layers, in_dim, nd, NO, act;
    int H[AZG_MAX_HIDDEN_LAYERS];
    int offW[AZG_MAX_HIDDEN_LAYERS], offb[AZG_MAX_HIDDEN_LAYERS];   // parameter offsets of the trunk layers
    int offWv, offbv, offbd;                        // value_head.weight (head row o starts at offWv + o * HL + (o > 0)) and the head biases
    int P;
    // scratch of one net, in floats: obs [Bmax][8], per layer A_l [Bmax][H_l] and D_l [Bmax][H_l] (act'(Z_l), later dZ_l in place)
    unsigned s_obs, s_A[AZG_MAX_HIDDEN_LAYERS], s_D[AZG_MAX_HIDDEN_LAYERS];
    size_t per_net;
    // LayerNorm trunks: the descriptor's flag, ln.weight / ln.bias of the trunk layers, and per layer X_l [Bmax][H_l],
    // G_l [Bmax][H_l] (d loss / d Y_l) and rstd_l [Bmax]; s_A then holds Y_l
    int layernorm;
    int offG[AZG_MAX_HIDDEN_LAYERS], offB[AZG_MAX_HIDDEN_LAYERS];
    unsigned s_X[AZG_MAX_HIDDEN_LAYERS], s_G[AZG_MAX_HIDDEN_LAYERS], s_R[AZG_MAX_HIDDEN_LAYERS];
};
