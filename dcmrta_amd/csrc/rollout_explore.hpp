// rollout_explore.hpp -- the epsilon-greedy forms of the persistent rollout (dcm_rollout_explore: a base policy DCM_POLICY_FIRST /
// DCM_POLICY_NEAREST, and explore_q32 in [0, 2^32]).
// Included by dcmrta_env.hip inside its anonymous namespace, after rollout_fast.hpp, in the translation unit of these forms only
// (-DDCM_TU_E, or a one-unit developer build).
//
// Choice protocol: with key_1 = mix64(seed_e + GAMMA (d + 1)), decision d EXPLORES iff
//     mix64(key_1 ^ EXPLORE_SALT) >> 32  <  explore_q32
// and then takes the random policy's action (protocol slot 1); every other decision takes the base policy's pick and does not consume
// slot 1.  explore_q32 = 0 is the greedy policy, 2^32 the random one, bit for bit, through these same kernels.
//
// The forms are the existing kernel texts compiled once more, as the greedy and the logging forms are:
//   k_ex_rollout_fast   / k_exrn_rollout_fast    from k_rollout_fast.inc   (Fast<>::decide_logged, apply<true>)   one-chunk layouts
//   k_ex_rollout_random / k_exrn_rollout_random  from k_rollout_random.inc (pick_random_action / pick_policy_action)  every other launch
// They are the logging forms with one more argument: ONE set serves the launches with the rollout log set (the plan) and without it
// (return sampling on large batches; the log then has cap 0 and a null length array, which costs the decision loop one compare of
// two registers and a skipped branch).  k_exrn_* renew a uniform generated batch's instances at episode restarts like k_rn_*; there is
// no size-renewing form (the host refuses that launch), no wave-priority (PRIO) instantiation, and no form of k_rollout_fast_mc /
// k_rollout_fast_g: their shapes take k_ex_rollout_random (plan::form_rollout_kind).
#pragma once

// (EXPLORE_SALT: common.hpp, beside the protocol's other constants)
#define DCM_EXPLORE 1
#include "k_rollout_forms.inc"
#undef DCM_EXPLORE
