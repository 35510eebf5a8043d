// persistent search kernels with per-net MCTS settings (search_kernel_nets), CartPole / MountainCar (discrete MCTS)
#include "dispatch.cuh"
template hipError_t azg_persistent_search_nets<AZG_ENV_CARTPOLE, false>(azg_engine*);
template hipError_t azg_persistent_search_nets<AZG_ENV_CARTPOLE, true>(azg_engine*);
