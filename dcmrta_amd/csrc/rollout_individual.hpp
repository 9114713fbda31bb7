// rollout_individual.hpp -- the individual-selection forms of the persistent rollout (dcm_rollout_individual: any of the three device
// policies, explore_q32 in [0, 2^32], on a handle created with DCM_PARAM_NO_GROUPING).
// Included by dcmrta_env.hip inside its anonymous namespace, in the translation unit of these forms only (-DDCM_TU_I, or a one-unit
// developer build).
//
// The reference's second evaluation protocol, Worker.run_test_IS (worker.py:159-198): the deciders of an event are not grouped by
// location (no get_unique_group); they act one by one in ascending id, each alone through agent_step, and a depot action moves that
// one agent only.  A decision is therefore ONE agent's agent_step: steps_out, the budgets and Hdr::d count those.
//
// Choice protocol: decision d has key_1 = mix64(seed_e + GAMMA (d + 1)) as everywhere.  Slot 0 (the leader draw) and the
// follower keys key_2.. are never consumed; slot 1 is consumed by DCM_POLICY_RANDOM and by an exploring decision
// (mix64(key_1 ^ EXPLORE_SALT) >> 32 < explore_q32), as in the epsilon-greedy forms.
//
// The forms are the general kernel text compiled once more:
//   k_is_rollout_random / k_isrn_rollout_random   from k_rollout_random.inc, every shape (the register-resident texts hold the grouping
//                                                 and the follower draws in their hot loops: no form of them)
// The epsilon-greedy loop with three call sites changed (k_rollout_random.inc): pick_leader(..., lowest), and no_grouping into
// apply_and_advance and into both advance calls -- code Sim<> already has for the lockstep kernel k_step.  The log rides along as in
// the epsilon-greedy forms (lg.len null: no log).  k_isrn_* renews a uniform generated batch's instances at episode restarts like
// k_rn_*; there is no size-renewing, best-keeping or lookahead form (the host refuses those launches).
#pragma once

#define DCM_INDIVIDUAL 1
#define DCM_RENEW 0
#include "k_rollout_random.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_rollout_random.inc"
#undef DCM_RENEW
#undef DCM_INDIVIDUAL
