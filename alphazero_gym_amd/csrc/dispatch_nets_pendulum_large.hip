// persistent search kernels with per-net MCTS settings (search_kernel_nets), Pendulum (continuous MCTS), hidden width 256
#include "dispatch.cuh"
template hipError_t azg_persistent_search_nets<AZG_ENV_PENDULUM_V1, true>(azg_engine*);
