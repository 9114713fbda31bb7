// plan.hpp -- which kernels serve a handle: the one statement of the dispatch policy.  Plain functions of plain integers, no HIP
// and no handle, so that a host compiler alone can build it (tests/test_host.py pins dcmrta_amd/roofline.py to it that way).
// dcmrta_env.hip and dcmrta_replay.hip map the answers to template arguments and decide nothing themselves.
#pragma once
#include <cstdint>

#include "../../include/dcmrta_env.h"

namespace dcm::plan {

constexpr int LANES = 64;   // one wavefront per env: a lane chunk of agents or tasks

// What the policy reads of a handle: batch dims, per-env sizes (dcm_load_instances_ragged), DCM_PARAM_WIDE_MEMBERS, and
// max_waiting_time > 0.  The register-resident kernels skip the task_update pass of a QUIET join on the ground that a member who
// has just joined has not waited max_waiting_time yet (env/task_env.py:269), which needs max_waiting_time > 0 (the reference's
// 10 / 100): a handle with max_waiting_time <= 0 (or NaN) takes the general kernels, which evaluate the rule literally.
// inrange: every env's squared distance between any two of its T + 1 points (the depot and its tasks; fma(dy, dy, dx * dx) as dist2
// forms it) is 0 or >= 2^-767.  Fast<>::apply takes the square root without the range scaling that smaller arguments need
// (common.hpp, dist2_inrange): a handle that holds a smaller square takes the general kernels.  True by construction for instances
// made on the device (coordinates are multiples of 2^-53), checked on the device for loaded ones (dcmrta_env.hip, k_points_inrange).
struct Shape { int A, T; bool ragged, wide, quiet; bool inrange = true; };

// Record layout dims: Lay{20,50} for every shape inside the reference's training range A <= 20, T <= 50 (parameters.py:15-16),
// Lay{64,64} for the other shapes with one lane per agent / task, so that those shapes share constant-offset kernel instantiations;
// the batch's own dims otherwise, and always on a wide handle (sixteen member slots instead of five).
struct LayDims { int A, T, C; };
inline LayDims layout_dims(int A, int T, bool wide) {
    if (wide) return {A, T, DCM_MAX_MEMBERS_WIDE};
    if (A <= 20 && T <= 50) return {20, 50, DCM_MAX_MEMBERS};
    if (A <= LANES && T <= LANES) return {LANES, LANES, DCM_MAX_MEMBERS};
    return {A, T, DCM_MAX_MEMBERS};
}

// Sim<CA, CT, RS[, MC]> instantiations: the three BASELINE shapes exactly; <20,50> / <64,64> with runtime sizes (_RS: uniform or
// ragged) for every other shape of those layouts; <128,256> with runtime sizes and layout for the mid sizes (generate_env takes any
// size, env/task_env.py:57-65); <0,0> for the rest; <0,0,false,MW> (two id words, runtime-size code) for a wide handle.
enum class SimKind { S20x50, S20x50_RS, S64x64_RS, S50x200, S100x500, S128x256_RS, Runtime, RuntimeWide };
inline SimKind sim_kind(const Shape& s) {
    const bool uniform = !s.ragged;
    if (s.wide) return SimKind::RuntimeWide;
    if (s.A <= 20 && s.T <= 50) return (uniform && s.A == 20 && s.T == 50) ? SimKind::S20x50 : SimKind::S20x50_RS;
    if (s.A <= LANES && s.T <= LANES) return SimKind::S64x64_RS;
    if (uniform && s.A == 50 && s.T == 200) return SimKind::S50x200;
    if (uniform && s.A == 100 && s.T == 500) return SimKind::S100x500;
    if (s.A <= 2 * LANES && s.T <= 4 * LANES) return SimKind::S128x256_RS;   // mid sizes: bounded trip counts, own layout
    return SimKind::Runtime;
}

// The one-chunk register-resident kernels (k_step_fast, k_terminal_flush, k_rollout_fast) need one lane per agent and per task,
// with lane 63 free for the depot; sim_kind is then one of the first three.  (dcm_step adds its call-shape conditions.)
// They are the kernels of Fast<>, persistent and lockstep: in-range distances only (Shape::inrange).
inline bool one_chunk_ok(const Shape& s) { return s.quiet && s.inrange && !s.wide && s.A <= LANES && s.T <= LANES - 1; }

// Instance renewal (dcm_set_instance_renewal with a non-zero stride): the handle's instances must have come from
// dcm_generate_instances (`generated`: the handle then holds the seeds and scalar arguments the next instances are drawn from), and the
// batch must be uniform -- on a ragged one an env's sizes would change inside a launch, which the k_rn_* forms do not do.
inline bool renewal_ok(const Shape& s, bool generated) { return generated && !s.ragged; }
// ... unless the handle opted in at dcm_create (DCM_PARAM_RENEW_SIZES): a ragged batch made by dcm_generate_instances then renews
// its sizes with its instances.  (A loaded ragged batch has no seeds to draw from; a uniform batch is renewal_ok's.)
inline bool renewal_sizes_ok(const Shape& s, bool generated, bool opted_in) { return generated && opted_in && s.ragged; }
// Which form of a restarting kernel a launch takes: the plain one (k_*) without a stride, the renewing one (k_rn_*) with a stride
// on a uniform batch, the size-renewing one (k_rs_*) with a stride on a ragged batch -- which dcm_set_instance_renewal only
// accepts on a handle that opted in; the flag is asked again here so that an unflagged handle can never reach that form.
// A ragged batch runs a runtime-size instantiation (sim_kind: *_RS, Runtime, RuntimeWide; rollout_kind: Fast, FastG or General,
// never FastMc), and the k_rs_* forms exist for exactly those.
enum class RenewForm { Plain, Instance, Sizes };
inline RenewForm renew_form(const Shape& s, bool stride_set, bool opted_in) {
    if (!stride_set) return RenewForm::Plain;
    return (s.ragged && opted_in) ? RenewForm::Sizes : RenewForm::Instance;
}
// Deferred terminal metrics (k_step_fast parks the final record, k_terminal_flush computes its summary row later with the env's sizes
// from the handle's size table): not for a size-renewing launch, after which the table holds the NEXT episode's sizes -- those
// launches compute the metrics inline, as under stream capture.
// (captured: a dcm_step of the handle has been captured into a graph; the caller has dealt with a capture in progress)
inline bool defer_terminal(bool captured, RenewForm form) { return !captured && form != RenewForm::Sizes; }
// k_step_fast restarts an auto-resetting env from a copy of the record dcm_reset left (dcm_env::init) when it has one and the terminal
// metrics are deferred.  The copy describes the instance dcm_reset saw: with renewal on the kernel gets none and computes the
// restart (reset_state + the first event) on the new instance.
// (renewal: any renewing form, RenewForm::Instance or RenewForm::Sizes)
inline bool step_restart_image(bool image_valid, bool deferred_terminal, bool renewal) { return image_valid && deferred_terminal && !renewal; }

// dcm_rollout_random.  obs_all_or_none: all three observation buffers given, or none (a template argument of the fast kernels)
enum class Rollout { Fast, FastMc, FastG, General };
inline Rollout rollout_kind(const Shape& s, bool obs_all_or_none) {
    if (!s.quiet || s.wide || !obs_all_or_none) return Rollout::General;
    if (one_chunk_ok(s)) return Rollout::Fast;                                            // rollout_fast.hpp
    if (!s.ragged && s.A == 50 && s.T == 200) return Rollout::FastMc;                     // BASELINE configs[3]: rollout_fast_mc.hpp
    const bool one_chunk_layout = s.A <= LANES && s.T <= LANES;                           // (T = 64: no free depot lane)
    if (s.A <= 2 * LANES && s.T <= 4 * LANES && !one_chunk_layout) return Rollout::FastG;  // the mid-size class: rollout_fast_g.hpp
    return Rollout::General;
}
// The forms of the persistent kernels beside the plain and the renewing ones (k_form.inc): greedy (dcm_rollout_policy with
// DCM_POLICY_FIRST / DCM_POLICY_NEAREST; DCM_POLICY_RANDOM is dcm_rollout_random and asks rollout_kind), logging (a launch of either
// while dcm_set_rollout_log is set, under any of the three policies) and epsilon-greedy (dcm_rollout_explore).  They exist for the
// one-chunk register-resident kernel and for the general one only: where rollout_kind says FastMc or FastG (50A/200T, the mid sizes)
// such a launch takes the general kernel.
// The lookahead form (dcm_rollout_lookahead) exists for the general kernel only: its launches do not ask this function, every shape
// takes k_la_rollout_random.
inline Rollout form_rollout_kind(const Shape& s, bool obs_all_or_none) {
    return rollout_kind(s, obs_all_or_none) == Rollout::Fast ? Rollout::Fast : Rollout::General;
}
// ... and there is no size-renewing form of them: a launch that would take the k_rs_* form is refused under a greedy or an
// epsilon-greedy policy and while the log is set
inline bool form_ok(RenewForm form) { return form != RenewForm::Sizes; }
// A greedy policy on a handle with max_waiting_time <= 0 does not end its episodes in general: a member that has waited 0 is dropped
// at once (env/task_env.py:269), decides again at the same time and, the policy being a function of the state, takes the same task
// again -- in the reference as here.  Such a launch must carry a decision budget (the scalar one, or per-env budgets); so must an
// epsilon-greedy one, whose budget rule is the base policy's.
inline bool policy_needs_budget(const Shape& s) { return !s.quiet; }
// k_rollout_fast_g<NAC, NTC>: lane chunks of agents (1..2) and of tasks (2..4) from the batch dims
inline int fast_g_agent_chunks(int A) { return A > LANES ? 2 : 1; }
inline int fast_g_task_chunks(int T) { return T > 3 * LANES ? 4 : (T > 2 * LANES ? 3 : 2); }

// dcm_execute_routes.  The LIVE tasks of a replay: all of them without dynamic arrivals, tasks 1..cap with them (an agent is never
// sent to a task that is not visible yet, and visible <= cap: env/task_env.py:567,578-584).
inline int replay_live_tasks(int T, bool reactive, int vis_cap) { return (reactive && vis_cap < T) ? vis_cap : T; }
// The register-resident kernel (replay_fast.hpp) for every replay whose agents and live tasks fit two lane chunks each and whose
// member slots fit one id word: BASELINE config 5 (100A/500T at the reference's cap of 100) and every small shape.  An explicit
// replay placement (1 / 2) asks for the general kernel, whose scratch block it places; route_cap < 32768 because the cursor and the
// length share a word; fast_lds_bytes is what the kernel would ask for (replay_fast_lds_bytes), within the default 64 KiB.
enum class Replay { Fast, General };
inline Replay replay_kind(int A, int T, int member_cap, bool reactive, int vis_cap, int placement, int route_cap,
                          uint32_t fast_lds_bytes) {
    const bool fits = A <= 2 * LANES && replay_live_tasks(T, reactive, vis_cap) <= 2 * LANES && member_cap <= 8;
    return (placement == 0 && fits && fast_lds_bytes <= 64u * 1024u && route_cap < 32768) ? Replay::Fast : Replay::General;
}
// k_replay<100, 500, 5> serves BASELINE config 5 exactly, k_replay<0, 0, 0> everything else
inline bool replay_exact_100x500(int A, int T, int member_cap) { return A == 100 && T == 500 && member_cap == 5; }
// Where the general kernel's scratch block lives: in LDS (lds_in_bytes: the kernel's need with the block inside) when the whole batch
// is resident with at most one wave per SIMD anyway (<= 4 envs per CU) and it fits a quarter of the CU's LDS, else in HBM (14 instead
// of 4 resident waves per CU at 100A/500T).  Placement 1 forces LDS (when it fits at all), 2 forces HBM.
inline bool replay_scratch_in_lds(int placement, uint32_t lds_in_bytes, int n_envs, int cus) {
    if (placement == 1) return lds_in_bytes <= 160u * 1024u;
    if (placement == 2) return false;
    return lds_in_bytes <= 40u * 1024u && n_envs <= 4 * cus;
}

}  // namespace dcm::plan
