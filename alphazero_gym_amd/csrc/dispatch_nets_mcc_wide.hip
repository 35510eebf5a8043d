// per-layer launches and persistent team kernel with per-net MCTS settings for wide networks, MountainCarContinuous
#include "ls_dispatch.cuh"
#include "team_dispatch.cuh"
template hipError_t azg_lockstep_search_nets<AZG_ENV_MOUNTAINCAR_CONT>(azg_engine*);
template hipError_t azg_team_search_nets<AZG_ENV_MOUNTAINCAR_CONT>(azg_engine*);
