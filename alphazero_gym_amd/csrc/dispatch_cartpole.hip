// persistent search kernels, CartPole (discrete MCTS)
#include "dispatch.cuh"
template hipError_t azg_persistent_search<AZG_ENV_CARTPOLE, false>(azg_engine*);
template hipError_t azg_persistent_search<AZG_ENV_CARTPOLE, true>(azg_engine*);
