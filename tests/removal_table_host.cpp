// Host program (own main, no GPU, no HIP): the compaction table of the member-removal path, csrc/removal_table.hpp, against plain
// "erase the listed elements in order".  Built and run by tests/test_removal_table_host.py (with -fsanitize=address,undefined where
// the host compiler has the runtimes).
//
// All 57 cases -- every n in 1..5 and every non-empty drop within {0..n-1} -- for the two slot strides the kernels use (8 * 50 and
// 8 * 64 bytes), each with five distinct ids and five distinct arrivals.  The steps are the kernel's (Fast<>::task_update): vacate
// the five slots, read the entry of keep, write all five arrivals at the entry's offsets, one byte permute for the id word, the OR
// of 1 << id over the leavers, the entry's count.  Exit status 0 and "57 cases x 2 strides ok" when everything agrees.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../dcmrta_amd/csrc/removal_table.hpp"

using namespace dcm;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            failures++;                                   \
            std::printf("FAIL %s: ", #cond);              \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static int run_case(uint32_t stride, int n, uint32_t drop, const RemovalEntry* table) {
    const int before = failures;
    // five distinct ids below 64 (the first n are listed, the id word holds zero above them) and five distinct arrivals
    uint32_t id[RT_SLOTS];
    double arrival[RT_SLOTS];
    uint64_t ids = 0, listed = 0;
    for (int j = 0; j < RT_SLOTS; j++) {
        id[j] = (uint32_t)((11 * j + 7 * n + 3 * (int)drop + 1) % 64);
        for (int i = 0; i < j; i++) if (id[i] == id[j]) { id[j] = (id[j] + 1) % 64; i = -1; }
        arrival[j] = 10.5 + 1.25 * j + 0.03125 * n + 0.001 * drop;
        if (j < n) { ids |= (uint64_t)id[j] << (8 * j); listed |= 1ull << id[j]; }
    }
    // the task's slots, `stride` bytes apart, + slot 5 behind them + a guard slot that nothing may touch
    std::vector<unsigned char> mem((RT_SLOTS + 2) * (size_t)stride, 0xEE);
    const double nan = std::nan("");
    double av[RT_SLOTS];
    for (int j = 0; j < RT_SLOTS; j++) {
        av[j] = j < n ? arrival[j] : nan;                                 // unused slots hold NaN
        std::memcpy(&mem[j * (size_t)stride], &av[j], 8);
    }
    // ---- the kernel's steps
    const uint32_t keep = ((1u << n) - 1u) & ~drop;
    const RemovalEntry e = table[keep];
    for (int j = 0; j < RT_SLOTS; j++) std::memcpy(&mem[j * (size_t)stride], &nan, 8);
    uint64_t gone = 0;
    for (int j = 0; j < RT_SLOTS; j++) {
        const uint32_t off = removal_offset(e, j);
        CHECK(off % stride == 0 && off / stride <= (uint32_t)RT_SLOTS, "n %d drop %u slot %d offset %u", n, drop, j, off);
        if (off / stride > (uint32_t)RT_SLOTS) continue;
        const bool leaves = (drop >> j) & 1u;
        if (leaves || j >= n) CHECK(off == RT_SLOTS * stride, "n %d drop %u: slot %d is not kept but is written to slot %u", n, drop, j, off / stride);
        std::memcpy(&mem[off], &av[j], 8);
        gone |= (uint64_t)((drop >> j) & 1u) << ((j < 4 ? (uint32_t)ids >> (8 * j) : (uint32_t)(ids >> 32)) & 0xFFu);
    }
    const uint64_t new_ids = removal_perm((uint32_t)(ids >> 32), (uint32_t)ids, e.perm);
    const int nn = (int)removal_left(e);
    // ---- erase the listed elements in order
    std::vector<uint32_t> want_id;
    std::vector<double> want_arr;
    uint64_t want_gone = 0;
    for (int j = 0; j < n; j++) {
        if ((drop >> j) & 1u) want_gone |= 1ull << id[j];
        else { want_id.push_back(id[j]); want_arr.push_back(arrival[j]); }
    }
    CHECK(nn == (int)want_id.size(), "n %d drop %u: %d left, want %zu", n, drop, nn, want_id.size());
    uint64_t want_ids = 0;
    for (size_t k = 0; k < want_id.size(); k++) want_ids |= (uint64_t)want_id[k] << (8 * k);
    CHECK(new_ids == want_ids, "n %d drop %u: ids %llx want %llx", n, drop, (unsigned long long)new_ids, (unsigned long long)want_ids);
    CHECK(gone == want_gone && (gone & ~listed) == 0, "n %d drop %u: gone %llx want %llx", n, drop, (unsigned long long)gone, (unsigned long long)want_gone);
    for (int j = 0; j < RT_SLOTS; j++) {
        double got;
        std::memcpy(&got, &mem[j * (size_t)stride], 8);
        if (j < (int)want_arr.size()) CHECK(same_bits(got, want_arr[j]), "n %d drop %u: slot %d holds %g want %g", n, drop, j, got, want_arr[j]);
        else CHECK(same_bits(got, nan), "n %d drop %u: slot %d holds %g want NaN", n, drop, j, got);
    }
    // nothing but the six 8-byte words was written
    for (size_t b = 0; b < mem.size(); b++) {
        const bool word = b % stride < 8 && b / stride <= (size_t)RT_SLOTS;
        if (!word) CHECK(mem[b] == 0xEE, "n %d drop %u: byte %zu written", n, drop, b);
        if (!word && mem[b] != 0xEE) break;
    }
    return failures - before;
}

int main() {
    int cases = 0;
    for (uint32_t stride : {8u * 50u, 8u * 64u}) {
        RemovalEntry table[RT_ENTRIES];
        for (uint32_t k = 0; k < RT_ENTRIES; k++) table[k] = removal_entry(k, stride);      // one entry per lane in the kernel
        // every entry: the count is the popcount, survivors' offsets ascend by one stride from 0
        for (uint32_t k = 0; k < RT_ENTRIES; k++) {
            uint32_t rank = 0;
            for (int j = 0; j < RT_SLOTS; j++)
                if ((k >> j) & 1u) { CHECK(removal_offset(table[k], j) == rank * stride, "keep %u slot %d", k, j); rank++; }
            CHECK(removal_left(table[k]) == rank, "keep %u: left %u", k, removal_left(table[k]));
        }
        for (int n = 1; n <= RT_SLOTS; n++)
            for (uint32_t drop = 1; drop < (1u << n); drop++) { run_case(stride, n, drop, table); cases++; }
    }
    static_assert(removal_entry(0b01101u, 400u).perm == 0x0c030200u, "a constant expression; survivors 0, 2, 3");
    static_assert(removal_perm(0x00000055u, 0x44332211u, 0x0c0c0401u) == 0x00005522u, "bytes 1 and 4 of {hi, lo}");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("%d cases x 2 strides ok\n", cases / 2);
    return cases == 2 * 57 ? 0 : 1;
}
