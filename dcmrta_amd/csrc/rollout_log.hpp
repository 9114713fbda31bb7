// rollout_log.hpp -- the logging forms of the persistent rollout (dcm_set_rollout_log: every agent_step of dcm_rollout_random /
// dcm_rollout_policy appends (task id, arrival time) to the acting agent's row).
// Included by dcmrta_env.hip inside its anonymous namespace, after rollout_fast.hpp, in the translation unit of the logging forms only
// (-DDCM_TU_L, or a one-unit developer build).
//
// The forms are the existing kernel texts compiled once more, as the greedy forms are:
//   k_lg_rollout_fast   / k_lgrn_rollout_fast    from k_rollout_fast.inc   (Fast<>::decide_logged, apply<true>)   one-chunk layouts
//   k_lg_rollout_random / k_lgrn_rollout_random  from k_rollout_random.inc (Sim<>::apply_and_advance's RouteLog)   every other launch
// with two more arguments: `policy`, wave-uniform and here covering DCM_POLICY_RANDOM as well, so that the random policy does not
// double the kernel count, and the log.  k_lgrn_* renew a uniform generated batch's instances at episode restarts like k_rn_*; there
// is no size-renewing form (the host refuses that launch), no wave-priority (PRIO) instantiation, and no logging form of
// k_rollout_fast_mc / k_rollout_fast_g: their shapes take k_lg_rollout_random (plan::form_rollout_kind).
#pragma once

#define DCM_LOG 1
#include "k_rollout_forms.inc"
#undef DCM_LOG
