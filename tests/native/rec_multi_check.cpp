// Host check of the multi-output rebuild's host side (tape_amd/csrc/rec_multi_plan.hpp), built and
// run by tests/test_rec_multi_host.py.
//   values  a fixed-seed sample of (survivor set, lost subset) pairs of Clay(20,7,16) -- every
//           a0 = 0..7 known column-0 nodes, lost sets of 2, 3, 7 and 13 slices, in either column
//           and across both, identity and rotated layouts at several stripe indices: the split
//           rule's sub-masks, each one's program (ClayHost::dec_prog with the sub-mask as out_mask)
//           interpreted byte by byte with the pattern's own matrix tables, every output row sent
//           through the job's node -> slot table, must rebuild every lost slice's chunk of a
//           stripe encoded by the oracle (oracle/clay_oracle.c), and store nothing else.
//   split   for one survivor set per a0 and every lost-set size 1..13: the sub-masks partition
//           the lost nodes, each compiles and fits (recover_multi_fits = decode_stage_fits of the
//           direct-output kernel, and kDecMaxOut items a step), a set that fits whole is one part.
//   args    rec_multi_check and rec_multi_route at their edges; rec_route, the route of every object:
//           Clay(20,7,16) and Clay(12,8,11), one and several lost slices, an empty blob, staged and
//           unstaged geometries; Clay(20,8,17), (20,9,18), (20,10,19): the kernel from two lost slices
//           on at a staged geometry, the generic path below 8-byte sub-chunks, one lost the class path.
// Run with no argument it is Clay(20,7,16), all three parts.  `<k>` (8, 9 or 10; 7 too) runs the
// values and split parts and the rec_route edges of Clay(20,k,k+9): a0 from max(0, k - 10) to
// min(k, 10), lost sets of 2, 3, ceil((n - k) / 2) and n - k slices.  `report k:avail:lost:rot:st ...`
// (masks in hex, by slice) prints what the engine builds for each named case -- the passes of the
// stripe and per pass nslots, nscratch, max_out, the LDS rows, the finish steps that store both rows
// of a pair and those that store one -- for tests/test_recover_multi_geometry_cases.py.
// Exit status = number of failed checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "rec_multi_plan.hpp"

extern "C" {
int oc_clay_sizeof(void);
int oc_clay_init(void *c, int n, int k, int d);
size_t oc_chunk_size_for(const void *c, size_t input_len);
int oc_clay_encode(const void *c, const uint8_t *data, size_t len, uint8_t *out);
}

using namespace tec;

static int bad = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            if (bad++ < 20) printf("line %d: %s\n", __LINE__, #x); \
        }                                                          \
    } while (0)

static constexpr int N = 20;
static int K = 7;  // the profile: Clay(20, K, K + 9)
static ClayHost H;

static uint8_t mul4(const uint32_t t[4], uint8_t x) {  // PermTab4 product, one byte
    uint8_t r = 0;
    for (int f = 0; f < 4; f++) r ^= (uint8_t)(t[f] >> (8 * ((x >> (2 * f)) & 3)));
    return r;
}
static uint8_t mul5(const PermTab &t, uint8_t x) {  // PermTab product (fields of 3, 3 and 2 bits), one byte
    auto at = [&](int w0, uint32_t j) { return (uint8_t)(t.t[w0 + (j >> 2)] >> (8 * (j & 3))); };
    return (uint8_t)(at(0, x & 7u) ^ at(2, (x >> 3) & 7u) ^ at(4, x >> 6));
}
// The pattern's matrix entry times x: the tables the kernel reads (D), and where the pattern has
// them (13 x 7: Clay(20,7,16)) the class kernels' D4, which must agree
static uint8_t mulD(const GpePattern &P, int e, int j, uint8_t x) {
    const uint8_t r = mul5(P.D[e][j], x);
    if (P.nerased <= (uint32_t)kClsMaxE && P.nknown <= (uint32_t)kClsMaxK) CHECK(mul4(P.D4[e][j], x) == r);
    return r;
}
static uint8_t pft3(uint8_t a, uint8_t b) { return (uint8_t)(a ^ gf_mul(2, (uint8_t)(a ^ b))); }

// Interpret one program (decode_stage.hip's step semantics) over the stripe's chunks (by node),
// every output row through `tab` into out (slot-major: slot s at out + s * cs).  rows: rows stored.
static void run(const GpePattern &P, const std::vector<DecStep> &steps, const uint8_t *chunks, size_t cs, size_t sc,
                const RmSlots &tab, std::vector<uint8_t> &out, std::vector<int> &written, long &rows) {
    const int NK = (int)P.nknown, NE = (int)P.nerased;
    auto kidx = [&](int node) {
        for (int j = 0; j < NK; j++)
            if ((int)P.known[j] == node) return j;
        CHECK(!"partner is a known node");
        return 0;
    };
    auto in = [&](int node, int z, size_t b) { return chunks[(size_t)node * cs + (size_t)z * sc + b]; };
    uint8_t slot[512], scr[512];
    bool slot_ok[512], scr_ok[512];
    for (size_t b = 0; b < sc; b++) {
        memset(slot_ok, 0, sizeof slot_ok);
        memset(scr_ok, 0, sizeof scr_ok);
        for (const DecStep &S : steps) {
            const int z = (int)S.z;
            auto put = [&](uint32_t loc, uint8_t v) {
                if (loc == kLocNone) return;
                const uint32_t ty = loc >> 24, ix = loc & 0xffffffu;
                if (ty == kLocStage) {
                    CHECK(ix < S.nout && S.nout <= (uint32_t)kDecMaxOut);
                    const uint32_t it = S.out[ix], node = it & 0xffu, zz = it >> 8;
                    CHECK(node < (uint32_t)N && zz < 100);
                    const uint8_t s = tab.slot[node];
                    if (s == kRmNoSlot) return;  // the kernel drops it
                    out[(size_t)s * cs + zz * sc + b] = v;
                    written[(size_t)s * cs + zz * sc + b]++;
                    rows += b == 0;
                } else {
                    CHECK(ix < 512);
                    (ty == kLocSlot ? slot : scr)[ix] = v;
                    (ty == kLocSlot ? slot_ok : scr_ok)[ix] = true;
                }
            };
            auto get = [&](uint32_t loc) {
                const uint32_t ty = loc >> 24, ix = loc & 0xffffffu;
                CHECK(ix < 512 && (ty == kLocSlot ? slot_ok : scr_ok)[ix]);
                return (ty == kLocSlot ? slot : scr)[ix];
            };
            uint8_t u[kDecMaxK], v[kDecMaxE] = {};
            for (int j = 0; j < NK; j++) {
                const uint8_t o = in((int)P.known[j], z, b);
                CHECK(S.kout[j] == kLocNone);  // a survivor is never an output
                if (S.kk[j] == kKnRed) u[j] = o;
                else if (S.kk[j] == kKnInput) u[j] = pft3(o, in((int)P.known[kidx((int)(S.kp[j] & 0xffu))], (int)(S.kp[j] >> 8), b));
                else if (S.kk[j] == kKnLoc) u[j] = pft3(o, get(S.kp[j]));
                else CHECK(!"known kind of the table kernel");
            }
            for (int e = 0; e < NE; e++)
                if (S.ek[e] == kErFinish) v[e] = get(S.ep[e]);
            for (int e = 0; e < NE; e++) {
                if (S.ek[e] == kErSkip) continue;
                uint8_t a = 0;
                for (int j = 0; j < NK; j++) a ^= mulD(P, e, j, u[j]);
                switch (S.ek[e]) {
                    case kErRed: put(S.ed0[e], a); break;
                    case kErType1: {
                        const uint8_t k = in((int)P.known[kidx((int)(S.ep[e] & 0xffu))], (int)(S.ep[e] >> 8), b);
                        const uint8_t w = (uint8_t)(gf_mul(kPft.t_u[0], (uint8_t)(a ^ k)) ^ k);
                        put(S.ed0[e], w);
                        put(S.ed1[e], w);
                        break;
                    }
                    case kErPark: put(S.ep[e], a); break;
                    case kErFinish:
                        put(S.ed0[e], pft3(a, v[e]));
                        put(S.epd[e], pft3(v[e], a));
                        break;
                    default: CHECK(!"erased kind of the table kernel");
                }
            }
        }
    }
}

static uint32_t pick(std::mt19937_64 &rng, uint32_t from, int count) {  // `count` random bits of `from`
    uint32_t m = 0;
    while (__builtin_popcount(m) < count) {
        const uint32_t b = 1u << (rng() % N);
        if (from & b) m |= b;
    }
    return m;
}
// survivor shards with a0 of them in column 0
static uint32_t survivors(std::mt19937_64 &rng, int a0) { return pick(rng, 0x3ffu, a0) | pick(rng, 0xffc00u, K - a0); }

static void check_split(const GpePattern &P, uint64_t lost, const std::vector<uint64_t> &subs, long &nsplit) {
    CHECK(!subs.empty());
    uint64_t seen = 0;
    for (uint64_t s : subs) {
        CHECK(s != 0 && !(s & seen) && !(s & ~lost));
        seen |= s;
        RecMultiProg R;
        CHECK(rec_multi_compile(H, P, s, R));
        CHECK(recover_multi_fits(R.H.nslots, R.H.max_out) && R.H.max_out <= (uint32_t)kDecMaxOut);
        CHECK(R.steps.size() == 102 && R.H.nsteps == 100);
    }
    CHECK(seen == lost);
    RecMultiProg whole;
    const bool fits = rec_multi_compile(H, P, lost, whole);
    CHECK(fits == (subs.size() == 1));  // a set that fits whole is not split; a split one does not fit
    nsplit += subs.size() > 1;
}

// rec_route of Clay(20,k,k+9), k = 8..10 (the profiles the class kernels do not serve, with plane
// programs all the same): two or more lost slices are the multi-output kernel at a staged geometry
// and the generic path below sub-chunks of 8 bytes; one lost slice is the class path (decode_enqueue
// with DecItem::lost), an empty blob included.
static void route_edges(int k) {
    ClayHost h;
    if (h.init(N, k, k + 9) != 0) {
        CHECK(!"profile");
        return;
    }
    for (uint32_t nl = 2; nl <= (uint32_t)(N - k); nl++) {
        CHECK(rec_route(h, nl, 1, 800, 848) == kRecKernel && rec_multi_route(h, nl, 1, 800, 848) == kRecMultiKernel);
        CHECK(rec_route(h, nl, 3, 14400, 3 * 14400 + 48) == kRecKernel);
        CHECK(rec_route(h, nl, 1, 600, 648) == kRecGeneric);  // sub-chunks of 6 bytes
        CHECK(rec_route(h, nl, 1, 200, 248) == kRecGeneric);
        CHECK(rec_route(h, nl, 0, 0, 248) == kRecClass);  // an empty blob
        CHECK(rec_route(h, nl, 1, 110000000, 110000048) == kRecGeneric);  // past the 31-bit offsets
    }
    CHECK(rec_route(h, 1, 1, 800, 848) == kRecClass && rec_multi_route(h, 1, 1, 800, 848) == kRecMultiSingle);
    CHECK(rec_route(h, 1, 1, 600, 648) == kRecGeneric && rec_route(h, 1, 0, 0, 248) == kRecClass);
    CHECK(rec_single_class(h, 1, 800, 848) && !rec_single_class(h, 1, 700, 748));
}

// One line per case and per pass of it, as the engine builds them (recover_multi_enqueue: the
// stripe's padded erasure mask and lost nodes, rec_multi_split, a job and a slot table per part)
static int report(int argc, char **argv) {
    for (int i = 2; i < argc; i++) {
        unsigned k = 0, avail = 0, lost = 0, rot = 0, st = 0;
        if (sscanf(argv[i], "%u:%x:%x:%u:%u", &k, &avail, &lost, &rot, &st) != 5 || k < 7 || k > 10) return 2;
        ClayHost h;
        if (h.init(N, (int)k, (int)k + 9) != 0) return 2;
        if (rec_multi_check(N, (int)k, avail, lost) != TE_OK || __builtin_popcount(avail) < (int)k) return 2;
        const uint64_t emask = stripe_emask(h, (int)rot, avail, st), lostn = rec_multi_lost_nodes(h, (int)rot, lost, st);
        GpePattern P;
        std::vector<uint16_t> pool;
        if (!h.gpe_pattern(emask, P, pool)) return 2;
        const std::vector<uint64_t> subs = rec_multi_split(h, P, lostn);
        printf("case %s passes %zu emask %05llx lostn %05llx\n", argv[i], subs.size(), (unsigned long long)emask,
               (unsigned long long)lostn);
        for (uint64_t sub : subs) {
            RecMultiProg R;
            std::vector<DecStep> raw;
            if (!rec_multi_compile(h, P, sub, R, &raw)) return 2;
            const RmSlots tab = rec_multi_slots(h, (int)rot, lost, sub, st);
            int noslot = 0, both = 0, one = 0;
            for (int node = 0; node < N; node++) noslot += ((lostn >> node) & 1ull) && tab.slot[node] == kRmNoSlot;
            for (const DecStep &S : raw)
                for (uint32_t e = 0; e < P.nerased; e++)
                    if (S.ek[e] == kErFinish) {
                        const int stored = (S.ed0[e] != kLocNone) + (S.epd[e] != kLocNone);
                        both += stored == 2;
                        one += stored == 1;
                    }
            printf("pass sub %05llx nslots %u nscratch %u max_out %u rows %u noslot %d finish_both %d finish_one %d\n",
                   (unsigned long long)sub, R.H.nslots, R.H.nscratch, R.H.max_out, recover_multi_rows(R.H.nslots), noslot, both,
                   one);
        }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "report")) return report(argc, argv);
    const bool full = argc < 2;  // no argument: Clay(20,7,16), every part, as before the profile argument
    if (!full) K = atoi(argv[1]);
    if (K < 7 || K > 10) return 2;
    const int E = N - K, a0_min = K > 10 ? K - 10 : 0, a0_max = K < 10 ? K : 10;
    if (H.init(N, K, K + 9) != 0) return 2;
    std::vector<uint8_t> oc((size_t)oc_clay_sizeof());
    oc_clay_init(oc.data(), N, K, K + 9);
    const size_t len = (size_t)400 * K;  // sc = 2 bytes: chunk 200 B
    const size_t cs = oc_chunk_size_for(oc.data(), len), sc = cs / 100;
    std::vector<uint8_t> data(len), chunks(N * cs);
    std::mt19937_64 rng(0x726d756c7469ull);
    for (auto &x : data) x = (uint8_t)rng();
    if (oc_clay_encode(oc.data(), data.data(), len, chunks.data()) != 0) return 2;
    std::vector<uint16_t> pool;

    // ---- values ----
    long pairs = 0, passes = 0, nsplit = 0, rows_total = 0;
    bool col_only[2] = {false, false}, col_both = false, rot_seen[2] = {false, false};
    const int sizes[4] = {2, 3, (E + 1) / 2, E};  // Clay(20,7,16): 2, 3, 7, 13
    for (int a0 = a0_min; a0 <= a0_max; a0++)
        for (int size : sizes)
            for (int rep = 0; rep < 16; rep++) {
                const int rotated = (int)(rng() % 2);
                const uint64_t st = rng() % 23;
                // the survivor shards of this stripe as slices, the lost slices among the rest
                const uint32_t surv_sh = survivors(rng, a0);
                uint32_t avail = 0;
                for (uint32_t sh = 0; sh < (uint32_t)N; sh++)
                    if ((surv_sh >> sh) & 1u) avail |= 1u << shard_to_slice(rotated, N, (uint32_t)st, sh);
                const uint32_t all = (1u << N) - 1u;
                uint32_t lost_sh = pick(rng, all & ~surv_sh, size);
                // the small sizes also within one column each, where the erased nodes allow
                if (size <= 3 && rep % 4 == 1 && __builtin_popcount(~surv_sh & 0x3ffu) >= size) lost_sh = pick(rng, ~surv_sh & 0x3ffu, size);
                if (size <= 3 && rep % 4 == 2 && __builtin_popcount(~surv_sh & 0xffc00u) >= size) lost_sh = pick(rng, ~surv_sh & 0xffc00u, size);
                uint32_t lost = 0;
                for (uint32_t sh = 0; sh < (uint32_t)N; sh++)
                    if ((lost_sh >> sh) & 1u) lost |= 1u << shard_to_slice(rotated, N, (uint32_t)st, sh);
                CHECK(rec_multi_check(N, K, avail, lost) == TE_OK);
                const uint64_t emask = stripe_emask(H, rotated, avail, st);
                const uint64_t lostn = rec_multi_lost_nodes(H, rotated, lost, st);
                CHECK(lostn == lost_sh && !(lostn & ~emask) && emask == (all & ~surv_sh));
                col_only[0] = col_only[0] || !(lostn & 0xffc00u);
                col_only[1] = col_only[1] || !(lostn & 0x3ffu);
                col_both = col_both || ((lostn & 0x3ffu) && (lostn & 0xffc00u));
                rot_seen[rotated] = true;
                GpePattern P;
                pool.clear();
                if (!H.gpe_pattern(emask, P, pool)) return 2;
                const std::vector<uint64_t> subs = rec_multi_split(H, P, lostn);
                check_split(P, lostn, subs, nsplit);
                // all n - k erased nodes never fit one pass (tests/test_gpu_recover_multi.py's split case and
                // tests/recover_multi_geometry_cases.py's rely on it)
                CHECK(size != E || subs.size() >= 2);
                std::vector<uint8_t> out((size_t)size * cs, 0xEE);
                std::vector<int> written((size_t)size * cs, 0);
                long rows = 0;
                for (uint64_t sub : subs) {
                    RecMultiProg R;
                    std::vector<DecStep> raw;
                    if (!rec_multi_compile(H, P, sub, R, &raw)) continue;  // counted by check_split
                    const RmSlots tab = rec_multi_slots(H, rotated, lost, sub, st);
                    for (int node = 0; node < 32; node++)
                        CHECK((tab.slot[node] != kRmNoSlot) == (node < N && ((sub >> node) & 1ull)));
                    run(P, raw, chunks.data(), cs, sc, tab, out, written, rows);
                    passes++;
                }
                CHECK(rows == (long)size * 100);  // alpha rows per lost node, each once
                uint32_t j = 0;
                for (uint32_t sl = 0; sl < (uint32_t)N; sl++) {
                    if (!((lost >> sl) & 1u)) continue;
                    const uint32_t sh = slice_to_shard(rotated, N, (uint32_t)st, sl);
                    const bool same = memcmp(out.data() + (size_t)j * cs, chunks.data() + (size_t)sh * cs, cs) == 0;
                    if (!same) printf("FAIL a0 %d size %d avail %05x lost %05x rot %d st %d slot %u\n", a0, size, avail, lost, rotated, (int)st, j);
                    CHECK(same);
                    j++;
                }
                for (int w : written) CHECK(w == 1);
                rows_total += rows;
                pairs++;
            }
    CHECK(pairs == 64 * (a0_max - a0_min + 1) && col_only[0] && col_only[1] && col_both && rot_seen[0] && rot_seen[1]);
    // the check can fail: a table that sends a node to another slot must not reproduce the slices
    {
        const uint64_t emask = 0xfffffull & ~(K == 7 ? 0x0c07cull : ((1ull << K) - 1ull) << 2);  // nodes 0 and 1 erased
        GpePattern P;
        pool.clear();
        if (!H.gpe_pattern(emask, P, pool)) return 2;
        const uint64_t lostn = 0x3ull;
        RecMultiProg R;
        std::vector<DecStep> raw;
        CHECK(rec_multi_compile(H, P, lostn, R, &raw));
        RmSlots tab = rec_multi_slots(H, 0, 0x3u, lostn, 0);
        std::swap(tab.slot[0], tab.slot[1]);
        std::vector<uint8_t> out(2 * cs, 0xEE);
        std::vector<int> written(2 * cs, 0);
        long rows = 0;
        run(P, raw, chunks.data(), cs, sc, tab, out, written, rows);
        CHECK(memcmp(out.data(), chunks.data(), 2 * cs) != 0 && memcmp(out.data(), chunks.data() + cs, cs) == 0);
    }

    // ---- split rule: one survivor set per a0, every lost-set size ----
    long split_sets = 0, split_found = 0, whole_found = 0;
    for (int a0 = a0_min; a0 <= a0_max; a0++) {
        const uint32_t surv = survivors(rng, a0), er = ((1u << N) - 1u) & ~surv;
        GpePattern P;
        pool.clear();
        if (!H.gpe_pattern(er, P, pool)) return 2;
        for (int size = 1; size <= E; size++)
            for (int rep = 0; rep < (size == E ? 1 : 24); rep++) {
                const uint64_t lostn = pick(rng, er, size);
                long ns = 0;
                check_split(P, lostn, rec_multi_split(H, P, lostn), ns);
                split_found += ns;
                whole_found += !ns;
                split_sets++;
            }
    }
    CHECK(split_found > 0 && whole_found > 0);  // both outcomes are exercised

    if (!full) {
        route_edges(K);
        printf("rec_multi k %d pairs %ld passes %ld split %ld rows %ld split_sets %ld (split %ld whole %ld) bad %d\n", K, pairs,
               passes, nsplit, rows_total, split_sets, split_found, whole_found, bad);
        return bad > 255 ? 255 : bad;
    }

    // ---- arguments and routing ----
    for (int k = 8; k <= 10; k++) route_edges(k);
    CHECK(rec_multi_check(N, K, 0x7f, 0) == TE_ERR_INVALID_ARG);
    CHECK(rec_multi_check(N, K, 0x7f, 1u << 20) == TE_ERR_INVALID_ARG);
    CHECK(rec_multi_check(N, K, 0x7f, 0x40) == TE_ERR_INVALID_ARG);
    CHECK(rec_multi_check(N, K, 0x7f, 0x80) == TE_OK);
    CHECK(rec_multi_check(N, K, 0x7f, 0xfff80) == TE_OK);
    CHECK(rec_multi_check(N, K, 0x3f, 0xfffc0) == TE_ERR_INVALID_ARG);  // 14 lost slices
    CHECK(rec_multi_check(N, K, 0x3f, 0x80) == TE_OK);                  // too few survivors is the decode's check
    CHECK(rec_multi_route(H, 1, 3, 3000, 9048) == kRecMultiSingle);
    CHECK(rec_multi_route(H, kRecMultiMinLost, 3, 3000, 9048) == kRecMultiKernel);
    CHECK(rec_multi_route(H, kRecMultiMinLost - 1, 3, 3000, 9048) == kRecMultiSingle);
    CHECK(rec_multi_route(H, 13, 0, 0, 248) == kRecMultiSingle);        // an empty blob
    CHECK(rec_multi_route(H, 2, 1, 700, 748) == kRecMultiGeneric);      // sub-chunks of 7 bytes
    CHECK(rec_multi_route(H, 2, 1, 800, 848) == kRecMultiKernel);
    ClayHost h2;
    if (h2.init(14, 10, 13) != 0) return 2;
    CHECK(rec_multi_route(h2, 2, 1, 25600, 25648) == kRecMultiGeneric);  // no plane programs

    // ---- the route of every object (rec_route): a lost index is a lost mask of one bit ----
    // Clay(20,7,16), chunk sizes by the oracle's rule.  A staged geometry: one slice the class path,
    // several the multi-output kernel.
    CHECK(rec_route(H, 1, 3, 3000, 9048) == kRecClass);
    CHECK(rec_route(H, 2, 3, 3000, 9048) == kRecKernel);
    CHECK(rec_route(H, 13, 3, 3000, 9048) == kRecKernel);
    // an unstaged one (999 bytes: sub-chunks of 2 bytes): the generic path whatever the count
    const size_t cs999 = oc_chunk_size_for(oc.data(), 999);
    CHECK(cs999 == 200 && !dec_geom_staged(H, cs999, cs999 + 48));
    CHECK(rec_route(H, 1, 1, cs999, cs999 + 48) == kRecGeneric);
    CHECK(rec_route(H, 2, 1, cs999, cs999 + 48) == kRecGeneric);
    // every length below the first staged one is unstaged: chunks come in steps of 200 bytes per 1,400
    // of the object, so 4,201 bytes are the first with sub-chunks of 8
    size_t first_staged = 0;
    for (size_t ln = 1; ln <= 6000 && !first_staged; ln++) {
        const size_t c1 = oc_chunk_size_for(oc.data(), ln);
        if (dec_geom_staged(H, c1, c1 + 48)) first_staged = ln;
        else CHECK(rec_route(H, 1, 1, c1, c1 + 48) == kRecGeneric && rec_route(H, 3, 1, c1, c1 + 48) == kRecGeneric);
    }
    CHECK(first_staged == 4201 && rec_route(H, 1, 1, 800, 848) == kRecClass);
    // an empty blob (ns = 0): nothing to decode, the class path's zero chunk whatever the count
    CHECK(rec_route(H, 1, 0, 0, 248) == kRecClass && rec_route(H, 13, 0, 0, 248) == kRecClass);
    CHECK(rec_single_class(H, 0, 0, 248) && rec_single_class(H, 1, 800, 848) && !rec_single_class(H, 1, 700, 748));
    // a slice range past the 31-bit offsets is unstaged as well
    CHECK(rec_route(H, 1, 1, 110000000, 110000048) == kRecGeneric && rec_route(H, 2, 1, 110000000, 110000048) == kRecGeneric);
    // Clay(12,8,11) has no plane programs: the generic path, an empty blob included
    ClayHost h3;
    if (h3.init(12, 8, 11) != 0) return 2;
    std::vector<uint8_t> oc3((size_t)oc_clay_sizeof());
    oc_clay_init(oc3.data(), 12, 8, 11);
    const size_t cs3 = oc_chunk_size_for(oc3.data(), 250001);
    CHECK(cs3 % (size_t)h3.alpha == 0 && dec_geom_staged(h3, cs3, cs3 + 48));  // the geometry is not what rules it out
    for (uint32_t nl : {1u, 2u, 4u}) {
        CHECK(rec_route(h3, nl, 1, cs3, cs3 + 48) == kRecGeneric);
        CHECK(rec_route(h3, nl, 1, (size_t)h3.alpha, (size_t)h3.alpha + 48) == kRecGeneric);  // unstaged too
        CHECK(rec_route(h3, nl, 0, 0, (size_t)h3.alpha + 48) == kRecGeneric);
    }
    CHECK(!rec_single_class(h3, 0, 0, 248) && !rec_single_class(h2, 1, 25600, 25648));
    // rec_each_lost: ascending slices, the j-th set bit is output slot j
    {
        std::vector<uint32_t> got;
        rec_each_lost(0x80025u, [&](uint32_t sl, uint64_t j) { CHECK(j == got.size()); got.push_back(sl); });
        CHECK((got == std::vector<uint32_t>{0, 2, 5, 19}));
        rec_each_lost(0u, [&](uint32_t, uint64_t) { CHECK(!"no lost slice"); });
    }

    printf("rec_multi pairs %ld passes %ld split %ld rows %ld split_sets %ld (split %ld whole %ld) bad %d\n", pairs, passes,
           nsplit, rows_total, split_sets, split_found, whole_found, bad);
    return bad > 255 ? 255 : bad;
}
