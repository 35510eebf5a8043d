// lock-step path and persistent team kernel for wide networks, MountainCarContinuous
#include "ls_dispatch.cuh"
#include "team_dispatch.cuh"
template hipError_t azg_lockstep_search<AZG_ENV_MOUNTAINCAR_CONT>(azg_engine*);
template hipError_t azg_team_search<AZG_ENV_MOUNTAINCAR_CONT>(azg_engine*);
