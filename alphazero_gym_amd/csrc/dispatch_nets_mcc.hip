// persistent search kernels with per-net MCTS settings (search_kernel_nets), MountainCarContinuous (continuous MCTS)
#include "dispatch.cuh"
template hipError_t azg_persistent_search_nets<AZG_ENV_MOUNTAINCAR_CONT, false>(azg_engine*);
template hipError_t azg_persistent_search_nets<AZG_ENV_MOUNTAINCAR_CONT, true>(azg_engine*);
