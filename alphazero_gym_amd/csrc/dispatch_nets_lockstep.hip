// per-layer launches with per-net MCTS settings (ls_tree_kernel_nets) for wide networks, the CartPole and Pendulum families
#include "ls_dispatch.cuh"
template hipError_t azg_lockstep_search_nets<AZG_ENV_CARTPOLE>(azg_engine*);
template hipError_t azg_lockstep_search_nets<AZG_ENV_PENDULUM_V1>(azg_engine*);
