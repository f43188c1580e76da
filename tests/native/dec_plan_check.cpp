// Stand-alone check of tape_amd/csrc/dec_plan.hpp (tests/test_dec_plan.py): the stripe plan of a
// decode call (full, raw, ranged, chunk path, node recover), the pattern keys, the group key's
// order, the staged-geometry rule and the class routing, for Clay(20,7,16).  The base pointers are
// fake and never dereferenced.  Exit status = number of failed checks.
#include <cstdio>
#include <random>
#include <set>
#include "dec_plan.hpp"

using namespace tec;

static int bad = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            if (bad++ < 20) printf("line %d: %s\n", __LINE__, #x); \
        }                                                          \
    } while (0)

static ClayHost H;
static constexpr int N = 20, K = 7;
static const uint8_t *const SL = reinterpret_cast<const uint8_t *>(0x100000000000ull);
static uint8_t *const OUT = reinterpret_cast<uint8_t *>(0x200000000000ull);
static uint64_t addr(const void *p) { return (uint64_t) reinterpret_cast<uintptr_t>(p); }

// the rotation and the padded erasure set, restated (slicer.rs:34-54)
static uint32_t ref_slice(int rot, uint64_t st, uint32_t shard) { return rot ? (uint32_t)((shard + st * 7 % N) % N) : shard; }
static uint32_t ref_shard(int rot, uint64_t st, uint32_t slice) { return rot ? (uint32_t)((slice + N - st * 7 % N) % N) : slice; }
static uint64_t ref_emask(int rot, uint32_t avail, uint64_t st) {
    uint64_t e = 0;
    for (uint32_t sh = 0; sh < (uint32_t)N; sh++)
        if (!((avail >> ref_slice(rot, st, sh)) & 1u)) e |= 1ull << sh;  // nu = 0: internal = external
    return H.pad_erasures(e);
}
static uint32_t random_avail(std::mt19937_64 &rng, int present) {
    uint32_t a = 0;
    while (__builtin_popcount(a) < present) a |= 1u << (rng() % N);
    return a;
}
static DecItem item(uint64_t S, uint64_t cs, uint64_t blob_len, uint32_t avail, uint64_t in_base, uint64_t out_off) {
    DecItem it{};
    it.in_base = in_base;
    it.blob_len = blob_len;
    it.stripe = S;
    it.cs = cs;
    it.ns = (blob_len + S - 1) / S;
    it.slice_len = it.ns * cs + 48;
    it.out_off = out_off;
    it.avail = avail;
    return it;
}
// jobs in walk order when every item shares one group
static const std::vector<GpeJob> &only_group(const DecGroups &g) {
    static const std::vector<GpeJob> none;
    CHECK(g.size() <= 1);
    return g.empty() ? none : g.begin()->second;
}
// keys distinct and numbered in first-seen order along `jobs`
static void check_keys(const DecPlan &P, const std::vector<GpeJob> &jobs) {
    CHECK(std::set<uint64_t>(P.keys.begin(), P.keys.end()).size() == P.keys.size());
    uint32_t next = 0;
    for (const GpeJob &g : jobs) {
        CHECK(g.pattern <= next && g.pattern < P.keys.size());
        if (g.pattern == next) next++;
    }
    CHECK(next == P.keys.size());
}

static void test_full_and_raw() {
    std::mt19937_64 rng(0x66756c6cull);
    for (int t = 0; t < 200; t++) {
        const int rot = (int)(rng() % 2);
        const uint64_t S = 5000, cs = 800, blob = 1 + rng() % (6 * S), in_base = rng() % 100000, out_off = rng() % 100000;
        const uint32_t avail = random_avail(rng, 7 + (int)(rng() % 6));
        const DecItem it = item(S, cs, t == 0 ? 3 * S : blob, avail, in_base, out_off);  // t == 0: a whole last stripe
        const DecPlan P = dec_plan(H, rot, false, &it, 1, SL, OUT);
        const std::vector<GpeJob> &jobs = only_group(P.groups);
        CHECK(jobs.size() == it.ns && P.copies.empty() && P.chunk_groups.empty() && !P.fused && !P.ranged_call);
        CHECK(P.touched == 0 && P.copied == 0 && P.decoded == 0 && P.rebuilt == 0);
        CHECK(P.groups.begin()->first == (DecGroupKey{cs, it.slice_len}));
        for (uint64_t st = 0; st < jobs.size(); st++) {
            const GpeJob &g = jobs[st];
            CHECK(addr(g.in) == addr(SL) + in_base + st * cs && g.in_len == ~0ull);
            CHECK(addr(g.out) == addr(OUT) + out_off + st * S && g.out_lo == 0);
            CHECK(g.out_len == (st + 1 == it.ns ? it.blob_len - st * S : S));  // the last stripe clipped to blob_len
            CHECK(g.rot == (rot ? st * TE_ROTATION_STEP % N : 0));
            CHECK(P.keys[g.pattern] == dec_key(ref_emask(rot, avail, st), -1));
        }
        check_keys(P, jobs);
    }
    // raw (te_clay_decode): one stripe of k chunks, never rotated by the caller
    DecItem it{};
    it.slice_len = it.cs = 800;
    it.blob_len = it.stripe = 7 * 800;
    it.ns = 1;
    it.avail = 0xfe000u;
    const DecPlan P = dec_plan(H, 0, true, &it, 1, SL, OUT);
    const std::vector<GpeJob> &jobs = only_group(P.groups);
    CHECK(jobs.size() == 1);
    if (jobs.size() == 1) CHECK(jobs[0].out == OUT && jobs[0].out_len == 5600 && jobs[0].rot == 0 && jobs[0].in == SL);
}

// One ranged item: the copies and the jobs' windows tile [0, w_len) exactly once.
static void check_ranged(int rot, uint32_t avail, uint64_t blob, uint64_t start, uint64_t len, bool chunk) {
    const uint64_t S = 5000, cs = 800, in_base = 4096, out_off = 512;
    DecItem it = item(S, cs, blob, avail, in_base, out_off);
    it.ranged = true;
    it.w_start = start;
    it.w_len = len;
    it.chunk = chunk;
    uint64_t sb = 0, se = 0;
    if (len) { sb = start / S; se = (start + len - 1) / S + 1; }
    it.in_skew = sb * cs;  // the staging of te_slicer_decode_range starts at the first touched stripe
    const DecPlan P = dec_plan(H, rot, false, &it, 1, SL, OUT);
    CHECK(P.ranged_call && !P.fused);
    std::vector<uint8_t> map(len, 0);
    const uint64_t base = addr(OUT) + out_off;
    auto cover = [&](uint64_t a, uint64_t b) {  // output addresses [a, b)
        CHECK(a >= base && b <= base + len && a <= b);
        for (uint64_t x = a; x < b && x >= base && x < base + len; x++) map[x - base]++;
    };
    // what each touched stripe must be, from the mask itself
    std::vector<int> kind(se - sb, 0);  // 0 copy, 1 decode, 2 chunk
    std::vector<uint32_t> miss_x(se - sb, 0);
    uint64_t n_copy = 0, n_dec = 0, n_chunk = 0, n_chunk_pieces = 0, chunk_bytes = 0;
    for (uint64_t st = sb; st < se; st++) {
        const uint64_t lo = std::max(start, st * S) - st * S, hi = std::min({start + len, (st + 1) * S, blob}) - st * S;
        uint32_t miss = 0, pieces = 0;
        for (uint64_t x = lo / cs; x * cs < hi; x++) {
            pieces++;
            if (!((avail >> ref_slice(rot, st, (uint32_t)x)) & 1u)) { miss++; miss_x[st - sb] = (uint32_t)x; }
        }
        kind[st - sb] = miss == 0 ? 0 : (chunk && miss == 1) ? 2 : 1;
        n_copy += miss == 0;
        n_dec += kind[st - sb] == 1;
        if (kind[st - sb] == 2) {
            n_chunk++;
            n_chunk_pieces += pieces - 1;
            const uint64_t x0 = miss_x[st - sb] * cs;
            chunk_bytes += std::min(hi, x0 + cs) - std::max(lo, x0);
        }
    }
    CHECK(P.touched == se - sb && P.copied == n_copy && P.decoded == n_dec && P.rebuilt == n_chunk);
    CHECK(P.chunk_gather == n_chunk_pieces && P.bytes_stored == chunk_bytes);
    for (const CopyJob &cj : P.copies) {
        CHECK(cj.len == cj.valid && cj.len > 0);
        cover(addr(cj.dst), addr(cj.dst) + cj.len);
        const uint64_t b0 = addr(cj.dst) - base + start, b1 = b0 + cj.len - 1;  // object bytes
        const uint64_t st = b0 / S, x = b0 % S / cs;
        CHECK(b1 / S == st && b1 % S / cs == x);  // one data chunk of one stripe
        if (st < sb || st >= se) continue;
        CHECK(kind[st - sb] == 0 || (kind[st - sb] == 2 && x != miss_x[st - sb]));  // a present chunk of a copy or chunk stripe
        const uint32_t sl = ref_slice(rot, st, (uint32_t)x);
        CHECK((avail >> sl) & 1u);
        CHECK(addr(cj.src) == addr(SL) + in_base + sl * it.slice_len + st * cs - it.in_skew + b0 % S % cs);
    }
    std::vector<int> seen(se - sb, 0);
    for (const GpeJob &g : only_group(P.groups)) {
        const uint64_t st = (addr(g.out) - base + start) / S;  // `out` is the address of stripe byte 0
        CHECK(addr(g.out) == base + st * S - start && st >= sb && st < se);
        if (st < sb || st >= se) continue;
        CHECK(kind[st - sb] == 1 && !seen[st - sb]++);
        CHECK(g.out_lo == std::max(start, st * S) - st * S && g.out_len == std::min({start + len, (st + 1) * S, blob}) - st * S);
        cover(addr(g.out) + g.out_lo, addr(g.out) + g.out_len);
        CHECK(addr(g.in) == addr(SL) + in_base + st * cs - it.in_skew);
        CHECK(P.keys[g.pattern] == dec_key(ref_emask(rot, avail, st), -1));
        CHECK(g.rot == (rot ? st * TE_ROTATION_STEP % N : 0));
    }
    for (const GpeJob &g : only_group(P.chunk_groups)) {
        const uint64_t c0 = addr(g.out) - base + start;  // object byte of the erased chunk's byte 0
        const uint64_t st = c0 / S, x = c0 % S / cs;
        CHECK(c0 % S % cs == 0 && st >= sb && st < se);
        if (st < sb || st >= se) continue;
        CHECK(kind[st - sb] == 2 && x == miss_x[st - sb] && !seen[st - sb]++);
        CHECK(g.out_len <= cs && g.out_lo < g.out_len);  // clipped to the chunk
        cover(addr(g.out) + g.out_lo, addr(g.out) + g.out_len);
        CHECK(P.keys[g.pattern] == dec_key(ref_emask(rot, avail, st), (int)x));  // the output node is that shard
        CHECK(addr(g.in) == addr(SL) + in_base + st * cs - it.in_skew);
    }
    for (uint64_t i = 0; i < se - sb; i++) CHECK(seen[i] == (kind[i] != 0));
    for (uint64_t i = 0; i < len; i++)
        if (map[i] != 1) { CHECK(!"every byte of the window exactly once"); break; }
    if (!chunk) CHECK(P.chunk_groups.empty());
    std::vector<GpeJob> all = only_group(P.groups);
    if (P.chunk_groups.empty()) check_keys(P, all);
}

static void test_ranged() {
    std::mt19937_64 rng(0x72616e6765ull);
    const uint64_t S = 5000, cs = 800, blob = 4 * S + 1234;  // a last partial stripe
    for (int rot = 0; rot < 2; rot++)
        for (int chunk = 0; chunk < 2; chunk++) {
            const uint32_t some[] = {0xfffffu, 0xfffffu & ~(1u << 2), 0xfffffu & ~((1u << 2) | (1u << 9)), 0xfe000u,
                                     random_avail(rng, 7), random_avail(rng, 12), random_avail(rng, 18)};
            for (uint32_t avail : some) {
                // starts and ends on a chunk boundary, one byte inside it, one byte across it
                for (int64_t ds = -1; ds <= 1; ds++)
                    for (int64_t de = -1; de <= 1; de++) {
                        const uint64_t a = S + 2 * cs + (uint64_t)ds, b = S + 5 * cs + (uint64_t)de;
                        check_ranged(rot, avail, blob, a, b - a, chunk);
                    }
                check_ranged(rot, avail, blob, 2 * S + cs + 10, 300, chunk);            // inside one chunk
                check_ranged(rot, avail, blob, 2 * S - 100, 200, chunk);                // over a stripe boundary
                check_ranged(rot, avail, blob, S - 1, 2 * S + 2, chunk);                // four stripes
                check_ranged(rot, avail, blob, 4 * S + 100, 1134, chunk);               // the last partial stripe, to the end
                check_ranged(rot, avail, blob, 0, blob, chunk);                         // the whole object
                check_ranged(rot, avail, blob, 777, 0, chunk);                          // len == 0
                for (int t = 0; t < 30; t++) {
                    const uint64_t a = rng() % blob, l = rng() % (blob - a + 1);
                    check_ranged(rot, avail, blob, a, l, chunk);
                }
            }
        }
    // two absent chunks in the window: a decode stripe even with the chunk path on
    {
        DecItem it = item(S, cs, blob, 0xfffffu & ~((1u << 1) | (1u << 3)), 0, 0);
        it.ranged = it.chunk = true;
        it.w_start = 0;
        it.w_len = S;
        DecPlan P = dec_plan(H, 0, false, &it, 1, SL, OUT);
        CHECK(P.chunk_groups.empty() && P.decoded == 1 && P.rebuilt == 0 && P.copies.empty());
        it.avail = 0xfffffu & ~(1u << 3);  // ... and one: a chunk stripe with gather pieces for the six present chunks
        P = dec_plan(H, 0, false, &it, 1, SL, OUT);
        CHECK(P.groups.empty() && P.rebuilt == 1 && P.copies.size() == 6 && P.chunk_gather == 6 && P.bytes_stored == cs);
        CHECK(only_group(P.chunk_groups).size() == 1 && dec_key_out_node(P.keys[0]) == 3);
    }
}

static void test_recover() {
    std::mt19937_64 rng(0x7265636f76ull);
    for (int t = 0; t < 100; t++) {
        const int rot = (int)(rng() % 2);
        const uint64_t S = 5000, cs = 800, blob = 1 + rng() % (30 * S), out_off = rng() % 100000;
        const int32_t lost = (int32_t)(rng() % N);
        uint32_t avail = random_avail(rng, 7 + (int)(rng() % 6)) & ~(1u << lost);
        while (__builtin_popcount(avail) < K) avail |= random_avail(rng, 1) & ~(1u << lost);
        DecItem it = item(S, cs, blob, avail, 64, out_off);
        it.lost = lost;
        const DecPlan P = dec_plan(H, rot, false, &it, 1, SL, OUT);
        const std::vector<GpeJob> &jobs = only_group(P.groups);
        CHECK(P.fused && jobs.size() == it.ns && P.copies.empty());
        for (uint64_t st = 0; st < jobs.size(); st++) {
            const GpeJob &g = jobs[st];
            CHECK(addr(g.out) == addr(OUT) + out_off + st * cs && g.out_len == cs && g.out_lo == 0);
            CHECK(P.keys[g.pattern] == dec_key(ref_emask(rot, avail, st), (int)ref_shard(rot, st, (uint32_t)lost)));
        }
        check_keys(P, jobs);
    }
}

static void test_keys_and_groups() {
    for (int node = -1; node < N; node++)
        for (uint64_t e : {0x1fffull, 0xfffffull, 0xabcdeull}) {
            const uint64_t k = dec_key(e, node);
            CHECK(dec_key_emask(k) == e && dec_key_out_node(k) == node);
            CHECK(k == (e | (uint64_t)(node + 1) * 281474976710656ull));
        }
    // the struct's order is the order of the integer key (cs << 32) ^ slice_len for slices below 4 GiB
    const DecGroupKey ks[] = {{800, 848}, {800, 1648}, {800, 0xffffffffull}, {14300, 14348}, {14300, 848},
                              {142900, 142948}, {100, 148}, {1428600, 1428648}, {1428600, 0xfffffff0ull}};
    for (const DecGroupKey &a : ks)
        for (const DecGroupKey &b : ks) {
            const uint64_t ia = (a.cs << 32) ^ a.slice_len, ib = (b.cs << 32) ^ b.slice_len;
            CHECK((a < b) == (ia < ib) && (a == b) == (ia == ib));
        }
    // items of two geometries: one group each
    DecItem two[2] = {item(5000, 800, 12000, 0xfe000u, 0, 0), item(100000, 14300, 250000, 0xfe000u, 1 << 20, 1 << 20)};
    const DecPlan P = dec_plan(H, 1, false, two, 2, SL, OUT);
    CHECK(P.groups.size() == 2 && P.groups.begin()->first.cs == 800 && P.groups.begin()->second.size() == 3);
    CHECK(P.groups.rbegin()->first == (DecGroupKey{14300, 3 * 14300 + 48}) && P.groups.rbegin()->second.size() == 3);
}

static void test_geometry() {
    // Clay(20,7,16): alpha = 100
    CHECK(!dec_geom_staged(H, 700, 748) && dec_geom_staged(H, 800, 848));  // sub-chunk 7 / 8
    CHECK(dec_geom_staged(H, 800, 107374182) && !dec_geom_staged(H, 800, 107374183));  // 20 * slice_len around 2^31 - 1
    CHECK(dec_geom_staged(H, 306783300, 848) && !dec_geom_staged(H, 306783400, 848));  // 7 * cs around 2^31 - 1
    // the bounds themselves (2^31 - 1 is prime): a profile of n = k = alpha = 1
    ClayHost one;
    one.n = one.k = one.alpha = 1;
    CHECK(dec_geom_staged(one, 8, 0x7ffffffeull) && !dec_geom_staged(one, 8, 0x7fffffffull));
    CHECK(dec_geom_staged(one, 0x7ffffffeull, 8) && !dec_geom_staged(one, 0x7fffffffull, 8));
    CHECK(!dec_geom_staged(one, 7, 8) && dec_geom_staged(one, 8, 8));
}

// for each (class, count): a new pattern of that class and `count` jobs of it, appended to g
static void add_jobs(std::vector<GpeJob> &g, std::vector<int> &pat_class, const std::vector<std::pair<int, size_t>> &count) {
    for (const auto &cc : count) {
        GpeJob j{};
        j.pattern = (uint32_t)pat_class.size();
        pat_class.push_back(cc.first);
        for (size_t i = 0; i < cc.second; i++) {
            j.out_len = g.size();  // a tag: where the job stood
            g.push_back(j);
        }
    }
}
static bool all_linked(int) { return true; }

static void test_route() {
    const DecGroupKey A{14300, 14348}, B{14300, 28648}, Tiny{700, 748};
    struct Knobs { bool class_on; int streams; bool small; };
    const Knobs on{true, 4, false}, off{false, 4, false};
    auto route = [](bool staged, const std::vector<int> &pc, auto linked, DecGroups &g, const DecGroups &ch, const Knobs &k) {
        return dec_route(H, staged, pc, linked, g, ch, k.class_on, k.streams, k.small);
    };
    // the fold-back rule: more class groups than streams, < 1,024 class stripes, > 64 stripes in the call
    struct Case { int ngroups; size_t per, rest; bool folded; };
    const Case cases[] = {
        {4, 25, 0, false}, {5, 20, 0, true},                     // class groups == streams / one more
        {5, 204, 3, true}, {5, 205, 0, false},                   // 1,020 (+ 3 table) and 1,025 class stripes
        {5, 12, 4, false}, {5, 12, 5, true}, {5, 13, 0, true},   // 64 and 65 stripes in the call
    };
    for (const Case &c : cases) {
        DecGroups g, none;
        std::vector<int> pc;
        std::vector<std::pair<int, size_t>> cnt;
        for (int i = 0; i < c.ngroups; i++) cnt.push_back({i, c.per});
        if (c.rest) cnt.push_back({-1, c.rest});
        add_jobs(g[A], pc, cnt);
        const size_t total = g[A].size();
        const DecRoute R = route(true, pc, all_linked, g, none, on);
        CHECK(R.err == TE_OK && R.folded == c.folded && !R.cls_small);
        CHECK(R.cls.size() == (c.folded ? 0u : (size_t)c.ngroups));
        CHECK(g[A].size() == (c.folded ? total : c.rest));
        if (c.folded) {  // the table jobs first, then the classes' in class order
            size_t at = 0;
            for (size_t i = 0; i < c.rest; i++) CHECK(pc[g[A][at++].pattern] == -1);
            for (int k = 0; k < c.ngroups; k++)
                for (size_t i = 0; i < c.per; i++) CHECK(pc[g[A][at++].pattern] == k);
        }
    }
    // exactly 1,023 and 1,024 class stripes
    for (size_t last : {203u, 204u}) {
        DecGroups g, none;
        std::vector<int> pc;
        add_jobs(g[A], pc, {{0, 205}, {1, 205}, {2, 205}, {3, 205}, {4, last}});
        const DecRoute R = route(true, pc, all_linked, g, none, on);
        CHECK(R.folded == (last == 203));
    }
    {   // class groups: per group key in key order, first seen first inside a key; the rest stays in order
        DecGroups g, none;
        std::vector<int> pc;
        add_jobs(g[B], pc, {{5, 2}, {-1, 1}, {3, 1}, {5, 1}});
        add_jobs(g[A], pc, {{4, 1}, {2, 2}, {6, 1}, {4, 1}, {-1, 2}});
        add_jobs(g[Tiny], pc, {{3, 2}});  // sub-chunks of 7 bytes: not a staged group
        const DecRoute R = route(true, pc, [](int id) { return id != 6; }, g, none, on);
        const int ids[] = {4, 2, 5, 3};
        const size_t sizes[] = {2, 2, 3, 1};
        CHECK(R.cls.size() == 4 && !R.folded && R.err == TE_OK);
        for (size_t i = 0; i < R.cls.size() && i < 4; i++) {
            CHECK(R.cls[i].id == ids[i] && R.cls[i].jobs.size() == sizes[i] && R.cls[i].key == (i < 2 ? A : B));
            for (size_t j = 1; j < R.cls[i].jobs.size(); j++) CHECK(R.cls[i].jobs[j - 1].out_len < R.cls[i].jobs[j].out_len);
        }
        CHECK(g[A].size() == 3 && pc[g[A][0].pattern] == 6 && g[B].size() == 1 && g[Tiny].size() == 2);  // class 6 is not linked
    }
    {   // class off, or a pattern without a plane program: every stripe stays in its table group
        for (int v = 0; v < 2; v++) {
            DecGroups g, none;
            std::vector<int> pc;
            add_jobs(g[A], pc, {{0, 3}, {1, 3}});
            const DecRoute R = route(v == 0, pc, all_linked, g, none, v == 0 ? off : on);
            CHECK(R.cls.empty() && g[A].size() == 6 && R.err == TE_OK && !R.folded);
        }
    }
    {   // TEC_DEC_CLASS_SMALL=1: class stripes of one round of per-call workgroups never fold back
        DecGroups g, none;
        std::vector<int> pc;
        add_jobs(g[A], pc, {{0, 20}, {1, 20}, {2, 20}, {3, 20}, {4, 20}});
        const DecRoute R = route(true, pc, all_linked, g, none, Knobs{true, 4, true});
        CHECK(R.cls_small && !R.folded && R.cls.size() == 5);
    }
    {   // chunk groups: the windowed kernel of the recover class 8 + 2 a0, after the decode classes
        DecGroups g, ch;
        std::vector<int> pc;
        add_jobs(g[A], pc, {{3, 2}});
        add_jobs(ch[A], pc, {{8, 1}, {14, 2}, {8, 1}});
        DecRoute R = route(true, pc, all_linked, g, ch, on);
        CHECK(R.err == TE_OK && R.cls.size() == 3);
        if (R.cls.size() == 3) {
            CHECK(R.cls[0].id == 3 && R.cls[1].id == kDecClasses + 0 && R.cls[2].id == kDecClasses + 3);
            CHECK(R.cls[1].jobs.size() == 2 && R.cls[2].jobs.size() == 2);
        }
        CHECK(ch[A].size() == 4);  // the chunk groups themselves are left alone
        // the windowed kernel not linked; the class kernels off; no plane program
        CHECK(route(true, pc, [](int id) { return id < kDecClasses; }, g, ch, on).err == TE_ERR_UNSUPPORTED);
        CHECK(route(true, pc, all_linked, g, ch, off).err == TE_ERR_UNSUPPORTED);
        CHECK(route(false, pc, all_linked, g, ch, on).err == TE_ERR_UNSUPPORTED);
        // a class without a windowed kernel: a column-1 recover class, a decode class, none
        for (int c : {9, 3, -1}) {
            DecGroups ch2;
            std::vector<int> pc2;
            add_jobs(ch2[A], pc2, {{8, 1}, {c, 1}});
            DecGroups g2;
            CHECK(route(true, pc2, all_linked, g2, ch2, on).err == TE_ERR_UNSUPPORTED);
        }
        DecGroups ch3, g3;  // a geometry the class kernels cannot address
        std::vector<int> pc3;
        add_jobs(ch3[Tiny], pc3, {{8, 1}});
        CHECK(route(true, pc3, all_linked, g3, ch3, on).err == TE_ERR_UNSUPPORTED);
    }
}

int main() {
    if (H.init(20, 7, 16)) return 99;
    test_full_and_raw();
    test_ranged();
    test_recover();
    test_keys_and_groups();
    test_geometry();
    test_route();
    printf("dec_plan bad %d\n", bad);
    return bad > 255 ? 255 : bad;
}
