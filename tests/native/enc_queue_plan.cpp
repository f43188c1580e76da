// enc_queue_plan.cpp -- the LDS-DMA encode's task list on the host (kernels.hpp enc_task, the
// function the kernel itself calls): for a range of stripe counts and call shapes, the queue
// positions 0 .. ntasks-1 of each launch must cover every (stripe, row of planes) exactly once --
// whole stripes in one launch, or the level-1 rows (0..6, `per` rows per task) in a first launch
// and the level-2 rows (7..9) only in a second -- and every task must start and end on an even
// plane (the ring slot parity the cross-stripe prefetch relies on) with at least 10 planes.
#include <cstdio>
#include <vector>
#include "kernels.hpp"

using namespace tec;

static int bad = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            if (bad++ < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                              \
    } while (0)

// marks rows of launch `a` into seen[stripe * 10 + row] (+1 per visit); returns its task count
static uint64_t walk(const EncArgs &a, std::vector<int> &seen, uint32_t row_lo, uint32_t row_hi) {
    const uint64_t nt = enc_task_count(a);
    std::vector<int> pos(nt, 0);
    for (uint32_t t = 0; t < nt; t++) {
        const uint32_t tile = enc_xcd_tile(t, (uint32_t)nt);
        CHECK(tile < nt);
        if (tile < nt) pos[tile]++;
        const EncTask k = enc_task(t, (uint32_t)nt, a.z0_first, a.z0_count, a.z0_split, a.z0_limit);
        CHECK(k.job < a.njobs);
        CHECK(k.z0b < k.z0e && k.z0e <= 10);
        CHECK(k.z0b >= row_lo && k.z0e <= row_hi);
        CHECK((k.z0b * 10) % 2 == 0 && (k.z0e * 10) % 2 == 0 && (k.z0e - k.z0b) * 10 >= 10);
        if (k.job < a.njobs)
            for (uint32_t r = k.z0b; r < k.z0e && r < 10; r++) seen[k.job * 10 + r]++;
    }
    for (uint64_t i = 0; i < nt; i++) CHECK(pos[i] == 1);  // the XCD remap is a permutation
    return nt;
}

int main() {
    long launches = 0;
    for (uint32_t stripes = 1; stripes <= 70; stripes++) {
        {  // whole stripes: one launch
            EncArgs a{};
            a.njobs = stripes;
            std::vector<int> seen(stripes * 10, 0);
            CHECK(walk(a, seen, 0, 10) == stripes);
            for (int v : seen) CHECK(v == 1);
            launches++;
        }
        for (uint32_t per = 1; per <= 7; per++) {  // split: level 1 in parts of `per` rows, then level 2
            EncArgs a{};
            a.njobs = stripes;
            a.z0_first = 0; a.z0_count = per; a.z0_split = (7 + per - 1) / per; a.z0_limit = 7;
            std::vector<int> l1(stripes * 10, 0), l2(stripes * 10, 0);
            CHECK(walk(a, l1, 0, 7) == (uint64_t)stripes * a.z0_split);
            a.z0_limit = 0; a.z0_first = 7; a.z0_count = 3; a.z0_split = 1;
            CHECK(walk(a, l2, 7, 10) == stripes);
            for (uint32_t i = 0; i < stripes * 10; i++) {
                const bool lvl2 = i % 10 >= 7;
                CHECK(l1[i] == (lvl2 ? 0 : 1));  // every level-1 row once, in the first launch only
                CHECK(l2[i] == (lvl2 ? 1 : 0));  // every level-2 range once, in the second only
            }
            launches += 2;
        }
    }
    // workgroups of a launch: min(tasks, slots); slots 0 = one per task
    CHECK(enc_grid(5120, 512) == 512 && enc_grid(300, 512) == 300 && enc_grid(512, 512) == 512);
    CHECK(enc_grid(5120, 0) == 5120 && enc_grid(1, 3) == 1);
    printf("launches %ld bad %d\n", launches, bad);
    return bad ? 1 : 0;
}
