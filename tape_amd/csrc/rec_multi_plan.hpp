// The host side of a multi-output rebuild (engine.cpp's te_recover_multi_batch_device): the
// argument rules, which path an object takes, a stripe's lost nodes and output table, the program
// of a lost set and the rule that splits a set the kernel cannot take whole.  Host-only and pure,
// like dec_plan.hpp: tests/test_rec_multi_host.py builds this header into a stand-alone check
// (tests/native/rec_multi_check.cpp).
#pragma once
#include <vector>
#include "dec_plan.hpp"

namespace tec {

// ---- routing: stated once, here ----
// A lost index is a lost mask of one bit: every recover entry point routes its objects by rec_route.
// An object with fewer than kRecMultiMinLost lost slices is a single-slice object (rec_multi_route):
// a one-slice request through a multi entry point is the single entry point's request, launch for
// launch.  From kRecMultiMinLost on it runs the multi-output kernel (recover_multi.hip) when the
// profile has plane programs (q = 10, t = 2, nu = 0) and the staged kernels address its geometry
// (dec_geom_staged); any other object decodes on the existing decode path and re-encodes (the
// generic path), keeping the lost slices.  An empty blob has nothing to decode and is a
// single-slice object whatever its lost count.
// The threshold is 2, the smallest count the kernel exists for; scripts/recover_multi_bench.py
// measures the crossover and DESIGN §4.13 records it.
constexpr uint32_t kRecMultiMinLost = 2;
enum RecMultiPath { kRecMultiSingle = 0, kRecMultiKernel = 1, kRecMultiGeneric = 2 };
inline RecMultiPath rec_multi_route(const ClayHost &h, uint32_t nlost, uint64_t ns, uint64_t cs, uint64_t slice_len) {
    if (nlost < kRecMultiMinLost || ns == 0) return kRecMultiSingle;
    const bool planes = h.q == kRepQ && h.t == 2 && h.nu == 0 && h.k >= 7 && h.k <= kDecMaxK;
    return planes && dec_geom_staged(h, cs, slice_len) ? kRecMultiKernel : kRecMultiGeneric;
}
// A single-slice object runs the class path (decode_enqueue with DecItem::lost: the staged decode
// whose program outputs only the lost node's chunk, an item per lost slice) when the profile has
// plane programs and the object is an empty blob (no stripe to decode: its one chunk is zeros) or
// the staged kernels address its geometry; any other takes the generic path.  No bound on k here:
// a profile the staged kernels do not compile for is decode_enqueue's TE_ERR_UNSUPPORTED, answered
// before anything is enqueued, and its objects then take the generic path too.
inline bool rec_single_class(const ClayHost &h, uint64_t ns, uint64_t cs, uint64_t slice_len) {
    const bool planes = h.q == kRepQ && h.t == 2 && h.nu == 0;
    return planes && (ns == 0 || dec_geom_staged(h, cs, slice_len));
}
// The route of one object: ns and cs as decode_validate gives them (an empty blob: ns = 0)
enum RecPath { kRecClass = 0, kRecKernel = 1, kRecGeneric = 2 };
inline RecPath rec_route(const ClayHost &h, uint32_t nlost, uint64_t ns, uint64_t cs, uint64_t slice_len) {
    switch (rec_multi_route(h, nlost, ns, cs, slice_len)) {
        case kRecMultiKernel: return kRecKernel;
        case kRecMultiGeneric: return kRecGeneric;
        default: return rec_single_class(h, ns, cs, slice_len) ? kRecClass : kRecGeneric;
    }
}
// One call of f(slice, j) per lost slice of a mask, ascending: the j-th set bit is output slot j
template <class F>
inline void rec_each_lost(uint32_t lost, F f) {
    for (uint64_t j = 0; lost; lost &= lost - 1u) f((uint32_t)__builtin_ctz(lost), j++);
}

// ---- arguments (te_recover_multi_object) ----
// lost_mask: 1..n-k slices, all below n, none of them available.  Fewer than k available slices is
// decode_validate's TE_ERR_NOT_ENOUGH_SLICES, checked after this.
inline int rec_multi_check(int n, int k, uint32_t avail, uint32_t lost) {
    const uint32_t all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    if (lost == 0 || (lost & ~all) || (lost & avail)) return TE_ERR_INVALID_ARG;
    if (__builtin_popcount(lost) > n - k) return TE_ERR_INVALID_ARG;
    return TE_OK;
}

// ---- the host pipeline's windows (te_recover_multi_window_plan) ----
// What an object counts towards window_cuts' limit (win_plan.hpp): its present slices in and its
// lost slices out, a slice length each.  Bits at or above n count for nothing.
inline uint64_t rec_multi_object_bytes(int n, uint32_t avail, uint32_t lost, uint64_t slice_len) {
    const uint32_t all = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    return ((uint64_t)__builtin_popcount(avail & all) + (uint64_t)__builtin_popcount(lost & all)) * slice_len;
}

// ---- a stripe's lost nodes and output table ----
// The internal nodes the lost slices hold in stripe st (the rotation moves them per stripe).  The
// survivors follow the decode's rule (stripe_emask: the absent shards padded by A7 to n - k
// erasures), so every lost node is in the erased set.
inline uint64_t rec_multi_lost_nodes(const ClayHost &h, int rotated, uint32_t lost, uint64_t st) {
    uint64_t nodes = 0;
    for (int sl = 0; sl < h.n; sl++)
        if ((lost >> sl) & 1u) nodes |= 1ull << h.ext_to_int((int)slice_to_shard(rotated, (uint32_t)h.n, (uint32_t)st, (uint32_t)sl));
    return nodes;
}
// The job's table for the output nodes `sub` (a subset of the stripe's lost nodes): node -> the
// rank of its slice among the lost slices (the j-th set bit of lost_mask is output slot j)
inline RmSlots rec_multi_slots(const ClayHost &h, int rotated, uint32_t lost, uint64_t sub, uint64_t st) {
    RmSlots t;
    for (uint8_t &s : t.slot) s = (uint8_t)kRmNoSlot;
    for (int node = 0; node < h.qt && node < (int)sizeof(t.slot); node++) {
        if (!((sub >> node) & 1ull)) continue;
        const int sh = h.int_to_ext(node);
        if (sh < 0) continue;
        const uint32_t sl = shard_to_slice(rotated, (uint32_t)h.n, (uint32_t)st, (uint32_t)sh);
        if ((lost >> sl) & 1u) t.slot[node] = (uint8_t)__builtin_popcount(lost & ((1u << sl) - 1u));
    }
    return t;
}

// ---- the program of an output set ----
struct RecMultiProg {
    DecProgHdr H{};
    std::vector<DecStepP> steps;  // packed, + 2 blank steps (the kernel reads two ahead)
    int orient = 0;
};
// ClayHost::dec_prog(P, orient, H, steps, -1, out) in the orientation with fewer scratch rows
// (two workgroups per CU first, as compile_pattern picks), packed.  false: `out` does not fit --
// a step with more than kDecMaxOut flush items, more LDS rows than recover_multi_fits allows, or a
// location past the packed form -- or is not a set of erased nodes.
inline bool rec_multi_compile(const ClayHost &h, const GpePattern &P, uint64_t out, RecMultiProg &R,
                              std::vector<DecStep> *raw = nullptr) {
    if (out == 0 || (out & ~P.erased_mask)) return false;
    bool found = false;
    auto cost = [](const DecProgHdr &x) { return (recover_multi_rows(x.nslots) > 53 ? 1u << 20 : 0u) + x.nscratch; };
    for (int orient = 0; orient < 2; orient++) {
        DecProgHdr H;
        std::vector<DecStep> st;
        if (!h.dec_prog(P, orient, H, st, -1, out) || !recover_multi_fits(H.nslots, H.max_out)) continue;
        if (found && cost(H) >= cost(R.H)) continue;
        std::vector<DecStepP> packed(st.size());
        bool ok = true;
        for (size_t i = 0; i < st.size() && ok; i++) {
            ok = ClayHost::dec_pack(st[i], packed[i]);
            for (int j = 0; j < kDecMaxK; j++) ok = ok && st[i].kout[j] == kLocNone;  // survivors are never outputs
        }
        if (!ok) continue;
        packed.resize(packed.size() + 2);
        R.H = H;
        R.steps.swap(packed);
        R.orient = orient;
        if (raw) raw->swap(st);
        found = true;
    }
    return found;
}

// ---- the split rule ----
// The sub-masks one pass each stores, for the lost nodes `lost` of pattern P.  A set that compiles
// whole is one pass.  Otherwise the nodes, ascending, are dealt into p = 2, 3, ... balanced parts,
// first as contiguous runs, then round-robin, and the first p at which every part of one dealing
// compiles is taken: the fewest passes among balanced dealings (an exhaustive search over all
// partitions is exponential and its gain is at most a pass).  p = |lost| is single nodes, which
// have at most two flush items a step; should even one of those not fit the result is empty and
// the caller takes the generic path -- a valid request is never refused for fit.  progs: each
// part's program.
inline std::vector<uint64_t> rec_multi_split(const ClayHost &h, const GpePattern &P, uint64_t lost,
                                             std::vector<RecMultiProg> *progs = nullptr) {
    std::vector<RecMultiProg> got(1);
    auto done = [&](std::vector<uint64_t> parts) {
        if (progs) progs->swap(got);
        return parts;
    };
    if (rec_multi_compile(h, P, lost, got[0])) return done({lost});
    std::vector<int> nodes;
    for (int i = 0; i < 64; i++)
        if ((lost >> i) & 1ull) nodes.push_back(i);
    const size_t L = nodes.size();
    for (size_t p = 2; p <= L; p++)
        for (int deal = 0; deal < 2; deal++) {
            std::vector<uint64_t> parts(p, 0);
            for (size_t i = 0; i < L; i++) parts[deal ? i % p : i * p / L] |= 1ull << nodes[i];
            got.assign(p, RecMultiProg{});
            bool ok = true;
            for (size_t j = 0; j < p && ok; j++) ok = rec_multi_compile(h, P, parts[j], got[j]);
            if (ok) return done(parts);
        }
    got.clear();
    return done({});
}

// A program's key in the handle's caches and the device pattern store: the padded erasure mask
// under the output set, above every dec_key (those stay below 2^55)
constexpr uint64_t kRecMultiKey = 1ull << 62;
inline uint64_t rec_multi_key(uint64_t emask, uint64_t out) { return kRecMultiKey | emask | out << 20; }

}  // namespace tec
