// persistent search kernels with per-net MCTS settings (search_kernel_nets), MountainCarContinuous (continuous MCTS), hidden widths 512 and 1024
#include "dispatch.cuh"
template hipError_t azg_persistent_search_nets_wide<AZG_ENV_MOUNTAINCAR_CONT>(azg_engine*);
