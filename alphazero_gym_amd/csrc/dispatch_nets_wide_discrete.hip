// persistent search kernels with per-net MCTS settings (search_kernel_nets), CartPole / MountainCar and Acrobot-v1 (discrete MCTS), hidden
// widths 512 and 1024
#include "dispatch.cuh"
template hipError_t azg_persistent_search_nets_wide<AZG_ENV_CARTPOLE>(azg_engine*);
template hipError_t azg_persistent_search_nets_wide<AZG_ENV_ACROBOT>(azg_engine*);
