// persistent search kernels, Pendulum (continuous MCTS), hidden widths up to 128
#include "dispatch.cuh"
template hipError_t azg_persistent_search<AZG_ENV_PENDULUM_V1, false>(azg_engine*);
