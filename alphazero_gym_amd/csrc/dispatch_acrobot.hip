// persistent search kernels, Acrobot-v1 (discrete MCTS, three actions, six observations), all hidden widths
#include "dispatch.cuh"
template hipError_t azg_persistent_search<AZG_ENV_ACROBOT, false>(azg_engine*);
template hipError_t azg_persistent_search<AZG_ENV_ACROBOT, true>(azg_engine*);
