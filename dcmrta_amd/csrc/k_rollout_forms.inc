// k_rollout_forms.inc -- the plain and the renewing form of the two kernel texts that have greedy, logging and epsilon-greedy forms,
// under whichever of DCM_POLICY, DCM_LOG, DCM_EXPLORE the including rollout_<form>.hpp has defined (k_form.inc)
#define DCM_RENEW 0
#include "k_rollout_random.inc"
#include "k_rollout_fast.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_rollout_random.inc"
#include "k_rollout_fast.inc"
#undef DCM_RENEW
