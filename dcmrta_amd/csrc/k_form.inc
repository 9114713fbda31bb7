// k_form.inc -- the forms of a kernel text: one text, compiled once per form, each time under another name and with that form's
// arguments.  A text (k_step.inc, k_step_fast.inc, k_rollout_random.inc, k_rollout_fast.inc, k_rollout_fast_mc.inc,
// k_rollout_fast_g.inc) says
//     #define KBASE rollout_fast         its name without the prefix
//     #define KPOLICY_FORMS 1            only if it has the forms of the second table
//     #include "k_form.inc"
// in front of its kernel, declares it as KNAME(..., KSIZES, ... int retcap KRENEW_PARAM KPOLICY_PARAM), and ends with
// #include "k_form_end.inc".  Whoever includes the text sets DCM_RENEW and at most one of DCM_POLICY, DCM_LOG, DCM_EXPLORE, DCM_BEST,
// DCM_LOOKAHEAD, DCM_INDIVIDUAL.
//
//   DCM_RENEW   KNAME          launched                                            KRENEW_PARAM   KSIZES
//   0           k_<base>       without a renewal stride                            --             const int32_t* sizes
//   1           k_rn_<base>    with a stride (dcm_set_instance_renewal), uniform   , Renew rn     const int32_t* sizes
//   2           k_rs_<base>    with a stride, ragged (DCM_PARAM_RENEW_SIZES)       , Renew rn     int32_t* sizes
// k_rn_*: an env that restarts an episode first replaces its instance (wave_renew_instance, instgen.hpp).  k_rs_*, for the
// instantiations that read per-env sizes: the restarting env draws its next SIZES with its next instance
// (wave_renew_instance_sized), writes them to the handle's size table and carries on as an env of those sizes: everything the kernel
// derived from the old ones at its head is derived again at the restart.
//
//   macro         KNAME (DCM_RENEW 0 / 1)        entry point                          KPOLICY_PARAM
//   DCM_POLICY    k_hp_<base> / k_hprn_<base>    dcm_rollout_policy, FIRST / NEAREST  , int policy
//   DCM_LOG       k_lg_<base> / k_lgrn_<base>    either, dcm_set_rollout_log set      , int policy, RouteLog lg
//   DCM_EXPLORE   k_ex_<base> / k_exrn_<base>    dcm_rollout_explore                  , int policy, uint64_t explore_q32, RouteLog lg
//   DCM_BEST      k_bs_<base> / --               any of the three, dcm_set_best_log   , int policy, uint64_t explore_q32, RouteLog lg, BestLog best
//   DCM_LOOKAHEAD k_la_<base> / k_larn_<base>    dcm_rollout_lookahead[_width]        , int policy, RouteLog lg, unsigned char* snap,
//                                                                                       int width, int64_t* inner_out
//   DCM_INDIVIDUAL k_is_<base> / k_isrn_<base>   dcm_rollout_individual               , int policy, uint64_t explore_q32, RouteLog lg
// Greedy: the action comes from `policy` (wave-uniform) instead of protocol slot 1.  Logging: `policy` covers all three policies
// (DCM_POLICY_RANDOM takes slot 1 as the plain form does) and every agent_step is appended to the log.  Epsilon-greedy: the logging
// form with explore_q32; the log may be unset there (lg.len null).  These forms exist for k_rollout_fast and k_rollout_random only,
// each set in a translation unit of its own (rollout_policy.hpp, rollout_log.hpp, rollout_explore.hpp), and none of them has a
// size-renewing form: the host refuses that launch (plan::form_ok).
// Best-keeping (rollout_best.hpp): the epsilon-greedy form with the log always set and `policy` covering all three as in the logging
// form (explore_q32 = 0 under dcm_rollout_random / dcm_rollout_policy: their k_lg_* decisions and budget rule), plus ONE hook where the
// text sees a freshly finished episode: keep_best (rollout_best.hpp) copies the env's summary row and its rows of the log to the best
// log if the episode beats the kept one.  No renewing form at all: the host refuses a best-keeping launch while a stride is set.
// Lookahead (rollout_lookahead.hpp): every decision is chosen by one-step lookahead over the base `policy` (any of the three) -- the
// wave snapshots its env into its slice of `snap`, plays one inner episode per unmasked action and restores -- and the logging code
// rides along as in the epsilon-greedy forms (lg.len null: no log).  `width` (0: all) limits the valued actions to the nearest ones;
// `inner_out` (null: not wanted) takes per env the inner episodes' decisions.  k_rollout_random only; no size-renewing form.
// Individual selection (rollout_individual.hpp): the epsilon-greedy form's arguments, `policy` covering all three as in the logging
// form, with the deciders of an event taken one by one in ascending id instead of grouped by location: no leader draw, no
// followers, the depot action moves the deciding agent alone (Worker.run_test_IS).  k_rollout_random only; no size-renewing form.
// KEXPLORES (defined here, for the texts): the form draws explore words -- DCM_EXPLORE or DCM_BEST.
//
// Two kernels from one text leave the first as it was: a form holds nothing of the others and compiles to the code it had before
// they existed (DESIGN 4, 6).  A new form: one #elif here, its rollout_<form>.hpp, one DCM_FORM_LAUNCHERS line in dcmrta_env.hip
// (DCM_PLAIN_FORM_LAUNCHERS for a form without renewing kernels).
#ifndef KBASE
#error "k_form.inc: the including text sets KBASE"
#endif
#if defined(DCM_POLICY) + defined(DCM_LOG) + defined(DCM_EXPLORE) + defined(DCM_BEST) + defined(DCM_LOOKAHEAD) > 1
#error "at most one of DCM_POLICY, DCM_LOG, DCM_EXPLORE, DCM_BEST, DCM_LOOKAHEAD"
#endif
#if (defined(DCM_POLICY) || defined(DCM_LOG) || defined(DCM_EXPLORE) || defined(DCM_BEST)) && !defined(KPOLICY_FORMS)
#error "this kernel text has no greedy, logging, epsilon-greedy or best-keeping form"
#endif
#if defined(DCM_INDIVIDUAL) && (defined(DCM_POLICY) || defined(DCM_LOG) || defined(DCM_EXPLORE) || defined(DCM_BEST) || defined(DCM_LOOKAHEAD))
#error "DCM_INDIVIDUAL stands alone: no other form macro beside it"
#endif
#if defined(DCM_INDIVIDUAL) && !defined(KINDIVIDUAL_FORM)
#error "the individual-selection form exists for k_rollout_random only"
#endif
#if defined(DCM_INDIVIDUAL) && DCM_RENEW == 2
#error "no size-renewing individual-selection form"
#endif
#if defined(DCM_LOOKAHEAD) && !defined(KLOOKAHEAD_FORM)
#error "the lookahead form exists for k_rollout_random only"
#endif
#if defined(DCM_LOOKAHEAD) && DCM_RENEW == 2
#error "no size-renewing lookahead form"
#endif
#if defined(DCM_BEST) && DCM_RENEW != 0
#error "no renewing best-keeping form"
#endif
#if (defined(DCM_LOG) || defined(DCM_EXPLORE)) && DCM_RENEW == 2
#error "no size-renewing logging form"
#endif
#if defined(DCM_POLICY) && DCM_RENEW == 2
#error "no size-renewing greedy form"
#endif

#if DCM_RENEW
#define KFORM_PICK(plain, renewing) renewing
#define KRENEW_PARAM , Renew rn
#else
#define KFORM_PICK(plain, renewing) plain
#define KRENEW_PARAM
#endif
#if DCM_RENEW == 2
#define KSIZES int32_t* sizes
#else
#define KSIZES const int32_t* sizes
#endif

#if defined(DCM_POLICY)
#define KPREFIX KFORM_PICK(k_hp_, k_hprn_)
#define KPOLICY_PARAM , int policy
#elif defined(DCM_LOG)
#define KPREFIX KFORM_PICK(k_lg_, k_lgrn_)
#define KPOLICY_PARAM , int policy, RouteLog lg
#elif defined(DCM_EXPLORE)
#define KPREFIX KFORM_PICK(k_ex_, k_exrn_)
#define KPOLICY_PARAM , int policy, uint64_t explore_q32, RouteLog lg
#elif defined(DCM_BEST)
#define KPREFIX k_bs_
#define KPOLICY_PARAM , int policy, uint64_t explore_q32, RouteLog lg, BestLog best
#elif defined(DCM_LOOKAHEAD)
#define KPREFIX KFORM_PICK(k_la_, k_larn_)
#define KPOLICY_PARAM , int policy, RouteLog lg, unsigned char* snap, int width, int64_t* inner_out
#elif defined(DCM_INDIVIDUAL)
#define KPREFIX KFORM_PICK(k_is_, k_isrn_)
#define KPOLICY_PARAM , int policy, uint64_t explore_q32, RouteLog lg
#elif DCM_RENEW == 2
#define KPREFIX k_rs_
#define KPOLICY_PARAM
#else
#define KPREFIX KFORM_PICK(k_, k_rn_)
#define KPOLICY_PARAM
#endif
#if defined(DCM_EXPLORE) || defined(DCM_BEST)
#define KEXPLORES 1
#endif
#define KFORM_PASTE_(prefix, base) prefix##base
#define KFORM_PASTE(prefix, base) KFORM_PASTE_(prefix, base)
#define KNAME KFORM_PASTE(KPREFIX, KBASE)
