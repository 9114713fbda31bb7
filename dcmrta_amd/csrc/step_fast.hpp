// step_fast.hpp -- the lockstep kernel of the one-chunk layouts for the PLAIN call shape of dcm_step: no injected leader /
// followers, no route log, all five outputs, grouping on (what a policy in the loop calls: worker.py:54-76 once per env).
// Included by dcmrta_env.hip after rollout_fast.hpp.
//
// k_step runs the general Sim<> code on the LDS image: ~500 VALU + ~650 scalar + ~100 LDS instructions per step in a dozen dependent
// LDS round trips, and at a machine-filling batch its rate is (resident workgroups) / (workgroup lifetime), not HBM bandwidth
// (profiles/r03_lockstep: 53 % of the wave time parked on s_waitcnt).  Here the step itself runs on the register-resident
// simulator of rollout_fast.hpp -- record -> LDS (coalesced), lane-owned fields -> registers, one decision with the HOST's
// action, registers -> LDS, dirty sections -> HBM -- whenever that action is one the device policy could have taken (the depot,
// or an unmasked task: every action of a mask-respecting policy).  Anything else (a masked or out-of-range action, an event at
// which nobody can decide, the end of an episode, auto-reset) takes the general code on the same LDS image, exactly as k_step.
// The observation of the next decision is built from the registers when they hold the env, from the LDS image otherwise.
#pragma once
#ifndef DCM_STEP_WAVES
#define DCM_STEP_WAVES 4       // minimum waves per SIMD asked of the compiler for k_step_fast
#endif

// The terminal metrics' scratch (calculate_waiting_time: 3.6 KB at 20A/50T) sits in LDS behind the removal table when 16 workgroups
// per CU -- all that the kernel's VGPRs allow -- still fit: the env whose episode ends in a launch is that launch's slowest wave,
// and with the scratch in HBM every write -> WSYNC -> read phase of the metrics is a global-memory round trip.
template <int CA, int CT>
constexpr bool step_scratch_in_lds() { return Lay{CA, CT}.lds_bytes() + DUMMY_SLOT_BYTES <= 10240u; }
// dynamic LDS of a k_step_fast / k_terminal_flush launch: the record image, the removal table (DUMMY_SLOT_BYTES), the scratch when it sits in LDS
template <int CA, int CT, bool RS>
constexpr uint32_t step_fast_lds_bytes(Lay L) {
    return Sim<CA, CT, RS, false>::lds_image_bytes(L) + DUMMY_SLOT_BYTES + (step_scratch_in_lds<CA, CT>() ? L.scratch_bytes() : 0u);
}

// k_step_fast and its renewing form k_rn_step_fast: see k_step_fast.inc
#define DCM_RENEW 0
#include "k_step_fast.inc"
#undef DCM_RENEW
#define DCM_RENEW 1
#include "k_step_fast.inc"
#undef DCM_RENEW
#define DCM_RENEW 2   // the size-renewing form (k_rs_*): runtime-size instantiations only
#include "k_step_fast.inc"
#undef DCM_RENEW


// Reward + perf metrics (env/task_env.py:344-364,420-425, worker.py:103-108) of the episodes whose final records k_step_fast parked
// (dcm_env::side): one workgroup per env, those without a waiting snapshot leave at once.
template <int CA, int CT, bool RS>
__global__ __launch_bounds__(WAVE, DCM_STEP_WAVES) void k_terminal_flush(int A, int T, int PA, int PT, KP P, const unsigned char* side, uint32_t side_pitch,
                                                        uint32_t* pendq, double* summary, const int32_t* sizes, unsigned char* gscr) {
    const int e = env_of_workgroup(), lane = threadIdx.x;
    if (uni(pendq[e]) == 0u) return;
    int eA, eT;
    env_dims<CA, CT, RS>(sizes, e, A, T, eA, eT);
    using SimT = Sim<CA, CT, RS, false>;
    SimT S{eA, eT, PA, PT, smem, nullptr};
    const Lay L = S.L();
    S.scr = step_scratch_in_lds<CA, CT>() ? smem + SimT::lds_image_bytes(L) + 512u : gscr + (size_t)e * L.scratch_bytes();
    const unsigned char* sp = side + (size_t)e * side_pitch;
    typename SimT::XY xy;
    S.template load_record<false>(sp, lane, xy);                 // (every load in flight before the first LDS write)
    if (lane == 0) {                                             // the image's pointers: this snapshot's abandonment rows, nothing else
        *(const uint16_t**)(smem + S.aux_off()) = (const uint16_t*)(sp + L.rec_bytes());
        *(uint8_t**)(smem + S.aux_off() + 16) = nullptr;         // (a log that overflowed into the count table is never deferred)
        *(double**)(smem + S.aux_off() + 32) = nullptr;
    }
    WSYNC();
    const double now = uni(((const Hdr*)smem)->now);
    (void)SimT::terminal_metrics(S, now, P.mwt, lane, summary + (size_t)e * 8);
    if (lane == 0) pendq[e] = 0u;
}
