// persistent search kernels with per-net MCTS settings (search_kernel_nets), Acrobot-v1 (discrete MCTS)
#include "dispatch.cuh"
template hipError_t azg_persistent_search_nets<AZG_ENV_ACROBOT, false>(azg_engine*);
template hipError_t azg_persistent_search_nets<AZG_ENV_ACROBOT, true>(azg_engine*);
