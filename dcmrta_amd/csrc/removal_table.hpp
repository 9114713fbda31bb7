// removal_table.hpp -- the compaction table of Fast<>::task_update's member-removal path (rollout_fast.hpp), and what a host program
// needs to replay an entry.  Plain C++: the kernels and tests/removal_table_host.cpp include the same text.
//
// A task with n <= 5 listed members loses the slots of the 5-bit mask `drop` (at least one).  Where every surviving slot goes, which
// bytes of the old id word make the new one, and how many members remain are functions of keep = ((1 << n) - 1) & ~drop alone:
// 32 entries of 16 bytes, built once per workgroup by lanes 0..31 (nothing is loaded for it) and read with one 128-bit LDS load.
//   perm      the byte selector of v_perm_b32 over the id word's halves {ids >> 32, ids}: byte k of the result = the id byte of
//             the k-th surviving slot, zero (selector 0x0c) behind the survivors.  At most four survive a removal, so the result is
//             the whole new id word; entry 31 (nobody leaves) is never read by the removal path and keeps its first four.
//   off[j]    16 bits each: the byte offset, from the task's slot 0, at which slot j's arrival is written: rank * stride for a
//             survivor (its rank among the survivors; stride = the bytes between two slots of one task), 5 * stride for a leaver --
//             "slot 5", the first word behind the five arrival rows, which the caller must be free to overwrite.
//   left      popcount(keep): the members that remain.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DCM_RT_HD __host__ __device__
#else
#define DCM_RT_HD
#endif

namespace dcm {

constexpr int RT_SLOTS = 5;                      // member slots of an ordinary handle (DCM_MAX_MEMBERS)
constexpr uint32_t RT_ENTRIES = 1u << RT_SLOTS;
constexpr uint32_t RT_BYTES = 16u * RT_ENTRIES;  // 512
constexpr uint32_t RT_PERM_ZERO = 0x0cu;         // v_perm_b32: selector bytes 0x0c give 0x00

struct RemovalEntry {
    uint32_t perm;       // byte selector for the new id word
    uint32_t off01;      // off[0] | off[1] << 16
    uint32_t off23;      // off[2] | off[3] << 16
    uint32_t off4_left;  // off[4] | left << 16
};
static_assert(sizeof(RemovalEntry) * RT_ENTRIES == RT_BYTES, "16-byte entries");

// the entry of `keep` for slots `stride` bytes apart (5 * stride < 65536)
DCM_RT_HD constexpr RemovalEntry removal_entry(uint32_t keep, uint32_t stride) {
    uint32_t perm = RT_PERM_ZERO * 0x01010101u;
    uint32_t off[RT_SLOTS] = {0, 0, 0, 0, 0};
    uint32_t k = 0;                                                      // survivors below slot j
    for (int j = 0; j < RT_SLOTS; j++) {
        const bool kp = (keep >> j) & 1u;
        off[j] = (kp ? k : (uint32_t)RT_SLOTS) * stride;
        if (kp && k < 4u) perm = (perm & ~(0xFFu << (8u * k))) | ((uint32_t)j << (8u * k));
        k += kp ? 1u : 0u;
    }
    return RemovalEntry{perm, off[0] | (off[1] << 16), off[2] | (off[3] << 16), off[4] | (k << 16)};
}
DCM_RT_HD constexpr uint32_t removal_offset(const RemovalEntry& e, int j) {
    const uint32_t w = j < 2 ? e.off01 : (j < 4 ? e.off23 : e.off4_left);
    return (j & 1) ? (w >> 16) : (w & 0xFFFFu);                         // (j == 4: the low half)
}
DCM_RT_HD constexpr uint32_t removal_left(const RemovalEntry& e) { return e.off4_left >> 16; }

// v_perm_b32 restated for the selectors the table holds (0..7: byte of {hi, lo}; 0x0c: zero) -- what the kernel's one instruction
// computes, for host code
DCM_RT_HD constexpr uint32_t removal_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t s = (sel >> (8 * k)) & 0xFFu;
        out |= (s < 8u ? (uint32_t)(src >> (8u * s)) & 0xFFu : 0u) << (8 * k);
    }
    return out;
}

}  // namespace dcm
