// rollout_policy.hpp -- the greedy device policies of the persistent rollout (dcm_rollout_policy: DCM_POLICY_FIRST, DCM_POLICY_NEAREST).
// Included by dcmrta_env.hip inside its anonymous namespace, after rollout_fast.hpp, in the translation unit of the greedy forms only
// (-DDCM_TU_P, or a one-unit developer build).
//
// The forms are the existing kernel texts compiled once more ("two kernels from one text leave them as they were"):
//   k_hp_rollout_fast   / k_hprn_rollout_fast    from k_rollout_fast.inc   (Fast<>::decide_policy)     one-chunk layouts
//   k_hp_rollout_random / k_hprn_rollout_random  from k_rollout_random.inc (Sim<>::pick_policy_action)  every other launch
// with one more wave-uniform argument, `policy`.  A kernel argument rather than a template argument: the two policies differ by one
// distance chain and one wave minimum in front of the same ballot, and half as many kernels are compiled.  k_hprn_* renew a uniform
// generated batch's instances at episode restarts like k_rn_*; there is no size-renewing form (the host refuses that launch), no
// wave-priority (PRIO) instantiation -- its estimate of the work left is calibrated on the random policy's episodes -- and no greedy
// form of k_rollout_fast_mc / k_rollout_fast_g: their shapes take k_hp_rollout_random (plan::form_rollout_kind).
#pragma once

#define DCM_POLICY 1
#include "k_rollout_forms.inc"
#undef DCM_POLICY
