// Stand-alone check of tape_amd/csrc/win_plan.hpp (tests/test_win_plan.py): the window cuts, the
// copy-run coalescing and the verify workspace's layout.  Exit status = number of failed checks.
#include <cstdio>
#include <map>
#include <random>
#include "win_plan.hpp"

using namespace tec;

static int bad = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            if (bad++ < 20) printf("line %d: %s\n", __LINE__, #x); \
        }                                                          \
    } while (0)

static uint64_t win_sum(const std::vector<uint64_t> &b, size_t a, size_t e) {
    uint64_t s = 0;
    for (size_t i = a; i < e; i++) s += b[i];
    return s;
}

static void check_cuts(const std::vector<uint64_t> &bytes, size_t window_bytes) {
    std::vector<size_t> cuts;
    window_cuts(bytes, window_bytes, cuts);
    const size_t n = bytes.size();
    const uint64_t cap = window_bytes ? window_bytes : (uint64_t)128 << 20;
    CHECK(!cuts.empty() && cuts.front() == 0);
    if (n == 0) {
        CHECK(cuts.size() == 1);  // no window
        return;
    }
    CHECK(cuts.size() >= 2 && cuts.back() == n);
    for (size_t w = 0; w + 1 < cuts.size(); w++) {
        const size_t a = cuts[w], e = cuts[w + 1];
        CHECK(a < e);  // strictly increasing
        if (a >= e || e > n) return;
        CHECK(win_sum(bytes, a, e) <= cap || e - a == 1);  // fits, or a single object
        if (e < n) CHECK(win_sum(bytes, a, e) + bytes[e] > cap);  // greedy: the successor's first object did not fit
    }
}

static void test_cuts() {
    std::mt19937_64 rng(0x77696e63757473ull);
    for (int t = 0; t < 400; t++) {
        const size_t n = (size_t)(rng() % 40);
        const size_t window = (size_t)(1 + rng() % 5000);
        std::vector<uint64_t> bytes(n);
        for (auto &b : bytes) {
            const unsigned kind = (unsigned)(rng() % 8);
            b = kind == 0 ? 0 : kind == 1 ? window + rng() % 3000 : rng() % (window / 2 + 2);  // zero, oversize, ordinary
        }
        check_cuts(bytes, window);
    }
    check_cuts({}, 1000);
    check_cuts({}, 0);
    check_cuts({5000}, 1000);                // one oversize object alone
    check_cuts({10, 5000, 10}, 1000);        // ... and between others: a window of its own
    check_cuts({0, 0, 0, 0}, 1000);          // all-zero sizes: one window
    check_cuts({0, 0, 0}, 0);
    {
        std::vector<size_t> cuts;
        window_cuts({10, 5000, 10}, 1000, cuts);
        CHECK((cuts == std::vector<size_t>{0, 1, 2, 3}));
        window_cuts({0, 0, 0, 0}, 1000, cuts);
        CHECK((cuts == std::vector<size_t>{0, 4}));
    }
    // window_bytes == 0: the 128 MiB default
    const uint64_t M = 1ull << 20;
    const std::vector<uint64_t> big = {64 * M, 64 * M, 1, 128 * M, 129 * M, 100 * M, 28 * M};
    check_cuts(big, 0);
    std::vector<size_t> c0, c1;
    window_cuts(big, 0, c0);
    window_cuts(big, (size_t)(128 * M), c1);
    CHECK(c0 == c1);
    CHECK((c0 == std::vector<size_t>{0, 2, 3, 4, 5, 7}));
}

// host byte -> device byte of a run list
static std::map<uint64_t, uint64_t> expand(const std::vector<CopyRun> &v) {
    std::map<uint64_t, uint64_t> m;
    for (const CopyRun &r : v)
        for (uint64_t i = 0; i < r.len; i++) m[r.host + i] = r.dev + i;
    return m;
}

static void test_add_run() {
    std::mt19937_64 rng(0x6164645f72756eull);
    for (int t = 0; t < 300; t++) {
        std::vector<CopyRun> raw, co;
        uint64_t host = rng() % 64, dev = rng() % 64;
        const int n = (int)(rng() % 30);
        uint64_t bytes = 0;
        for (int i = 0; i < n; i++) {
            // pieces ascending on both sides (as the pipelines place them), gaps on either side or none
            const unsigned gap = (unsigned)(rng() % 4);
            if (gap & 1u) host += 1 + rng() % 32;
            if (gap & 2u) dev += 1 + rng() % 32;
            const uint64_t len = rng() % 4 == 0 ? 0 : 1 + rng() % 48;
            raw.push_back({host, dev, len});
            add_run(co, host, dev, len);
            host += len;
            dev += len;
            bytes += len;
        }
        CHECK(expand(raw) == expand(co));
        uint64_t sum = 0;
        for (size_t i = 0; i < co.size(); i++) {
            CHECK(co[i].len != 0);  // zero lengths are skipped
            sum += co[i].len;
            if (i)  // whatever could merge did
                CHECK(!(co[i - 1].host + co[i - 1].len == co[i].host && co[i - 1].dev + co[i - 1].len == co[i].dev));
        }
        CHECK(sum == bytes);
        CHECK(co.size() <= raw.size());
    }
    std::vector<CopyRun> v;
    add_run(v, 100, 0, 0);
    CHECK(v.empty());
    add_run(v, 100, 0, 16);
    add_run(v, 116, 16, 0);  // zero length after a run: skipped, nothing merged
    CHECK(v.size() == 1 && v[0].len == 16);
    add_run(v, 116, 16, 16);  // contiguous on both sides: merged
    CHECK(v.size() == 1 && v[0].host == 100 && v[0].dev == 0 && v[0].len == 32);
    add_run(v, 132, 48, 16);  // contiguous on the host only (the device copy is aligned up)
    CHECK(v.size() == 2);
    add_run(v, 200, 64, 16);  // contiguous on the device only
    CHECK(v.size() == 3);
    add_run(v, 216, 80, 8);
    CHECK(v.size() == 3 && v[2].len == 24);
}

static void test_align16() {
    CHECK(align16(0) == 0 && align16(1) == 16 && align16(15) == 16 && align16(16) == 16 && align16(17) == 32);
    CHECK(align16((1ull << 40) + 1) == (1ull << 40) + 16);
}

static void check_layout(const VerLayout &L) {
    // ordered and disjoint: expected | peer digests | result digests | mask arrays
    CHECK(L.dig_off(0) == L.exp_b);
    CHECK(L.dig_off(1) == L.dig_off(0) + L.dig_p);
    CHECK(L.mask_off(0) == L.dig_off(1) + L.dig_o);
    for (size_t a = 1; a < L.narr; a++) CHECK(L.mask_off((int)a) == L.mask_off((int)a - 1) + L.mask_b);
    CHECK(L.total() == L.mask_off(0) + L.narr * L.mask_b);
    CHECK(L.h_mask(0) == L.exp_b);
    for (size_t a = 1; a < L.narr; a++) CHECK(L.h_mask((int)a) == L.h_mask((int)a - 1) + L.mask_b);
    CHECK(L.h_total() == L.h_mask(0) + L.narr * L.mask_b);
    for (int w = 0; w < 2; w++) CHECK(L.dig_off(w) % 4 == 0);
    for (size_t a = 0; a < L.narr; a++) CHECK(L.mask_off((int)a) % 4 == 0 && L.h_mask((int)a) % 4 == 0);
}

static void test_layout() {
    std::mt19937_64 rng(0x7665726c61796full);
    for (int t = 0; t < 300; t++) {
        const size_t nobj = (size_t)(1 + rng() % 200), n = (size_t)(1 + rng() % 32), nitems = (size_t)(1 + rng() % (nobj * n));
        // a read window: no result digests, one mask array -- the offsets verify_wait used
        const size_t exp_b = nobj * n * 32, dig_b = nitems * 32, mask_b = nobj * sizeof(uint32_t);
        const VerLayout R{exp_b, dig_b, 0, mask_b, 1};
        check_layout(R);
        CHECK(R.dig_off(0) == exp_b);
        CHECK(R.mask_off(0) == exp_b + dig_b);
        CHECK(R.total() == exp_b + dig_b + mask_b);
        CHECK(R.h_mask(0) == exp_b);
        CHECK(R.h_total() == exp_b + mask_b);
        // a rebuild window: peers' and rebuilt slices' digests, two mask arrays
        const VerLayout B{exp_b, dig_b, nobj * 32, mask_b, 2};
        check_layout(B);
        CHECK(B.dig_off(1) == exp_b + dig_b);
        CHECK(B.mask_off(1) == exp_b + dig_b + nobj * 32 + mask_b);
        CHECK(B.total() == exp_b + dig_b + nobj * 32 + 2 * mask_b);
        CHECK(B.h_mask(1) == exp_b + mask_b);
        CHECK(B.h_total() == exp_b + 2 * mask_b);
        // a repair window: no peers
        check_layout(VerLayout{exp_b, 0, nobj * 32, mask_b, 2});
    }
}

int main() {
    test_cuts();
    test_add_run();
    test_align16();
    test_layout();
    printf("win_plan bad %d\n", bad);
    return bad ? 1 : 0;
}
