// persistent search kernels, Pendulum (continuous MCTS), hidden widths 256 and up
#include "dispatch.cuh"
template hipError_t azg_persistent_search<AZG_ENV_PENDULUM_V1, true>(azg_engine*);
