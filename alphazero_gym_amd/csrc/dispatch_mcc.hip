// persistent search kernels, MountainCarContinuous (continuous MCTS whose traces can end in terminal nodes), all hidden widths
#include "dispatch.cuh"
template hipError_t azg_persistent_search<AZG_ENV_MOUNTAINCAR_CONT, false>(azg_engine*);
template hipError_t azg_persistent_search<AZG_ENV_MOUNTAINCAR_CONT, true>(azg_engine*);
