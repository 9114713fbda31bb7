// fork_envs.hpp -- the per-env gather of dcm_fork_envs: env b of a destination handle becomes env src_index[b] of a source handle --
// its record (header, mutable part, instance part), its dcm_summary row, its abandonment log and its overflow count table -- so that
// B envs fan out to B x K branches, or a batch is permuted or compacted, without the state leaving its handles.
// Included by dcmrta_env.hip inside its anonymous namespace, next to best_reduce.hpp; launched by the host API only, so the
// device-only translation units (-DDCM_TU_*) do not emit it.
//
// It is an HBM copy: 2 x (rec_bytes + 32 A + align16(2 A T) + 64) bytes per copied env, every byte read once and written once,
// nothing computed.  No LDS, no atomics, plain loads and plain stores (the next kernel reads the records: the lines stay in L2).
// Every section of an env is a multiple of 16 bytes at a 16-byte aligned address -- the record by Lay::rec_bytes, the log row
// u16[A][AB_CAP] = 32 A bytes, the count row by abcnt_pitch, which rounds u16[A][T] up so that the row's padding travels with it (it
// is part of the dcm_clone_state blob) and no narrower tail is left -- so all of them go through fork_copy16.
#pragma once

static_assert(Lay{20, 50}.rec_bytes() % 16 == 0 && Lay{64, 64}.rec_bytes() % 16 == 0 && Lay{50, 200}.rec_bytes() % 16 == 0 &&
              Lay{20, 50, MW}.rec_bytes() % 16 == 0 && Lay{DCM_MAX_AGENTS, DCM_MAX_TASKS}.rec_bytes() % 16 == 0,
              "records are copied in 16-byte pieces");
static_assert(AB_CAP * sizeof(uint16_t) % 16 == 0 && abcnt_pitch(1, 1) % 16 == 0 && abcnt_pitch(3, 7) % 16 == 0 &&
              abcnt_pitch(DCM_MAX_AGENTS, DCM_MAX_TASKS) % 16 == 0, "side rows are copied in 16-byte pieces");

constexpr int FORK_IN_FLIGHT = 4;   // 16-byte loads per lane issued before the first store: 4 KiB per wave, 16 VGPRs

// n16 16-byte pieces global -> global through registers, lane-coalesced; with `patch`, bytes 8..15 of piece 0 (Hdr::seed of a record)
// are replaced by `seed` in lane 0's register before the store, so the header's piece is written once, with its final value
__device__ __forceinline__ void fork_copy16(unsigned char* dst, const unsigned char* src, uint32_t n16, int lane, bool patch, uint64_t seed) {
    const u32x4* s = (const u32x4*)src;
    u32x4* d = (u32x4*)dst;
    for (uint32_t base = 0; base < n16; base += FORK_IN_FLIGHT * WAVE) {        // (n16, base: wave-uniform)
        u32x4 r[FORK_IN_FLIGHT];
#pragma unroll
        for (int c = 0; c < FORK_IN_FLIGHT; c++) {
            const uint32_t i = base + c * WAVE + lane;
            if (i < n16) r[c] = s[i];
        }
        if (patch && base == 0 && lane == 0) { r[0].z = (uint32_t)seed; r[0].w = (uint32_t)(seed >> 32); }
#pragma unroll
        for (int c = 0; c < FORK_IN_FLIGHT; c++) {
            const uint32_t i = base + c * WAVE + lane;
            if (i < n16) d[i] = r[c];
        }
    }
}
static_assert(offsetof(Hdr, seed) == 8, "fork_copy16 patches the seed in the second half of the record's first 16 bytes");

// grid = B_dst workgroups of one wave.  in_place: dst and src are one handle (the *_src and *_dst pointers are equal).
// rec16 / log16 / cnt16: 16-byte pieces of a record, of an env's log row, of an env's count row.  seeds_in / ok_out: nullable.
// Everything that decides what the wave does -- the index, its validity, the in-place rule -- is wave-uniform (uni()).
// In place a copied env reads a source that no workgroup copies INTO: src_index[s] == s is checked here, with one more 4-byte load, and
// such an s is at most given a new seed by its own workgroup, an 8-byte store into a field this wave replaces by seeds_in[b] before
// it stores (seeds_in is given for all envs or for none): every byte that ends up in memory is determined, whatever the order.
__global__ __launch_bounds__(WAVE) void k_fork_envs(int B_src, bool in_place, uint32_t rec16, uint32_t log16, uint32_t cnt16,
                                                    unsigned char* state_dst, const unsigned char* state_src, double* summary_dst,
                                                    const double* summary_src, unsigned char* log_dst, const unsigned char* log_src,
                                                    unsigned char* cnt_dst, const unsigned char* cnt_src,
                                                    const int32_t* __restrict__ src_index, const uint64_t* __restrict__ seeds_in,
                                                    uint8_t* __restrict__ ok_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int s = uni(src_index[b]);
    if (s == -1) {                                                               // left alone
        if (ok_out && lane == 0) ok_out[b] = 1;
        return;
    }
    bool ok = s >= 0 && s < B_src;
    if (ok && in_place && s != b) ok = uni(src_index[s]) == s;                   // (s < B_src == B_dst: inside src_index)
    if (ok_out && lane == 0) ok_out[b] = ok ? 1 : 0;
    if (!ok) return;                                                             // refused: untouched
    const bool reseed = seeds_in != nullptr;
    const uint64_t seed = reseed ? seeds_in[b] : 0;
    const size_t rec_bytes = (size_t)rec16 * 16;
    if (in_place && s == b) {                                                    // its own source: only the seed may change
        if (reseed && lane == 0) ((Hdr*)(state_dst + (size_t)b * rec_bytes))->seed = seed;
        return;
    }
    fork_copy16(state_dst + (size_t)b * rec_bytes, state_src + (size_t)s * rec_bytes, rec16, lane, reseed, seed);
    fork_copy16(log_dst + (size_t)b * log16 * 16, log_src + (size_t)s * log16 * 16, log16, lane, false, 0);
    fork_copy16(cnt_dst + (size_t)b * cnt16 * 16, cnt_src + (size_t)s * cnt16 * 16, cnt16, lane, false, 0);
    if (lane < 8) summary_dst[(size_t)b * 8 + lane] = summary_src[(size_t)s * 8 + lane];
}
