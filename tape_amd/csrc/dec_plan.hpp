// The host side of a decode call (engine.cpp's decode_enqueue): which stripes run, their windows
// and jobs, the pattern keys, and which kernel family each stripe goes to.  Host-only and pure: no
// HIP call, no handle -- tests/test_dec_plan.py builds this header into a stand-alone check
// (tests/native/dec_plan_check.cpp).
#pragma once
#include <algorithm>
#include <map>
#include <unordered_map>
#include <vector>
#include "../../include/tape_ec.h"
#include "dec_class.hpp"

namespace tec {

// Slicer's rotation (slicer.rs:34-54): te_shard_to_slice / te_slice_to_shard
inline uint32_t shard_to_slice(int rotated, uint32_t n, uint32_t stripe, uint32_t shard) {
    if (!rotated || n == 0) return shard;
    return (shard + (uint32_t)(((uint64_t)stripe * TE_ROTATION_STEP) % n)) % n;
}
inline uint32_t slice_to_shard(int rotated, uint32_t n, uint32_t stripe, uint32_t slice) {
    if (!rotated || n == 0) return slice;
    return (slice + n - (uint32_t)(((uint64_t)stripe * TE_ROTATION_STEP) % n)) % n;
}

struct DecItem {          // one object, host-validated
    uint64_t in_base;     // offset in d_slices of slice 0
    uint64_t slice_len, blob_len, stripe, ns, cs, out_off;
    uint32_t avail;
    int32_t lost = -1;    // >= 0: output = that slice's chunks at out_off + stripe * cs (node recover)
    // ranged read: only object bytes [w_start, w_start + w_len) are written, at out_off
    bool ranged = false;
    uint64_t w_start = 0, w_len = 0;
    uint64_t in_skew = 0;  // the slices at in_base start at slice byte in_skew (te_slicer_decode_range's staging)
    // ranged read: a stripe whose window holds exactly one erased data chunk rebuilds that chunk
    // alone (TE_RANGE_CHUNK: the handle's knob, and range_chunk_ok of the object)
    bool chunk = false;
};

// Ranged reads (te_slicer_range_plan): the stripes a window touches, [sb, se)
inline void range_stripes(uint64_t S, uint64_t start, uint64_t len, uint64_t &sb, uint64_t &se) {
    sb = se = 0;
    if (len == 0 || S == 0) return;
    sb = start / S;
    se = (start + len - 1) / S + 1;
}
// ... and the window inside stripe st, [lo, hi) in stripe bytes.  copy: every data chunk it
// intersects (chunk x = stripe bytes [x cs, (x + 1) cs), shard x) is a present slice's -- decided
// from the mask itself, not from the padded erasure set -- so nothing needs decoding.
// miss: the absent chunks among them, and the last one (the only one when miss == 1).
struct RangeWin { uint64_t lo, hi; bool copy; uint32_t miss = 0, miss_x = 0; };
inline RangeWin range_window(int n, int rotated, uint32_t avail, uint64_t blob_len, uint64_t S, uint64_t cs,
                             uint64_t st, uint64_t start, uint64_t len) {
    const uint64_t base = st * S, end = std::min({start + len, base + S, blob_len});
    RangeWin w;
    w.lo = start > base ? start - base : 0;
    w.hi = end - base;
    w.copy = true;
    for (uint64_t x = w.lo / cs; x * cs < w.hi; x++)
        if (!((avail >> shard_to_slice(rotated, (uint32_t)n, (uint32_t)st, (uint32_t)x)) & 1u)) {
            w.copy = false;
            w.miss++;
            w.miss_x = (uint32_t)x;
        }
    return w;
}
inline bool range_is_chunk(const DecItem &it, const RangeWin &w) { return it.chunk && w.miss == 1; }
// every touched stripe's window, stripe sb + i at [i]
inline std::vector<RangeWin> range_windows(int n, int rotated, uint32_t avail, uint64_t blob_len, uint64_t S,
                                           uint64_t cs, uint64_t start, uint64_t len) {
    uint64_t sb, se;
    range_stripes(S, start, len, sb, se);
    std::vector<RangeWin> w;
    for (uint64_t st = sb; st < se; st++) w.push_back(range_window(n, rotated, avail, blob_len, S, cs, st, start, len));
    return w;
}
// The padded erasure set of stripe st as internal nodes: the shards whose slices are missing,
// padded to n - k erasures (the decode then reads exactly the k nodes left).
inline uint64_t stripe_emask(const ClayHost &h, int rotated, uint32_t avail, uint64_t st) {
    uint64_t emask = 0;
    for (int sh = 0; sh < h.n; sh++)
        if (!((avail >> shard_to_slice(rotated, (uint32_t)h.n, (uint32_t)st, (uint32_t)sh)) & 1u))
            emask |= 1ull << h.ext_to_int(sh);
    return h.pad_erasures(emask);
}
// check a window against the object (the argument rules of the ranged entry points)
inline bool range_valid(uint64_t blob_len, uint64_t start, uint64_t len) {
    return start + len >= start && start + len <= blob_len;
}

// A pattern's key: its padded erasure mask (48 bits) under its output node + 1 (-1: all data chunks)
constexpr uint64_t kDecKeyNode = 1ull << 48;
inline uint64_t dec_key(uint64_t emask, int out_node) { return emask | (uint64_t)(out_node + 1) * kDecKeyNode; }
inline uint64_t dec_key_emask(uint64_t key) { return key % kDecKeyNode; }
inline int dec_key_out_node(uint64_t key) { return (int)(key / kDecKeyNode) - 1; }

// The staged and class kernels read sub-chunks of >= 8 bytes and address a stripe's slices and its
// output share with 31-bit offsets: decode_enqueue, range_chunk_ok and rec_route answer from this.
inline bool dec_geom_staged(const ClayHost &h, uint64_t cs, uint64_t slice_len) {
    constexpr uint64_t lim = 0x7fffffffull;
    return cs / (uint64_t)h.alpha >= 8 && (uint64_t)h.n * slice_len < lim && cs * (uint64_t)h.k < lim;
}

// Measurement option TEC_DEBUG_KNOBS=1 TEC_DEC_CLASS=0: no class kernels (the table-driven one instead)
inline bool dec_class_on() {
    static const bool on = [] {
        const char *e = tec_knob("TEC_DEC_CLASS");
        return !(e && e[0] == '0');
    }();
    return on;
}

// A decode call of at most this many stripes is a per-call decode: one wave per workgroup.
constexpr size_t kDecSmallStripes = 64;

// The output node of stripe st (internal): node recover's lost slice's shard, a chunk stripe's
// erased data shard, else -1 (the stripe's data chunks).
inline int stripe_out_node(const ClayHost &h, int rotated, const DecItem &it, uint64_t st, bool chunk, uint32_t miss_x) {
    if (it.lost >= 0) return h.ext_to_int((int)slice_to_shard(rotated, (uint32_t)h.n, (uint32_t)st, (uint32_t)it.lost));
    return chunk ? h.ext_to_int((int)miss_x) : -1;
}

// Jobs that share a launch: one chunk size and one stride between slices.  Ordered by cs, then
// slice_len -- the order fixes the launch order and the arena layout.
struct DecGroupKey {
    uint64_t cs, slice_len;
    bool operator<(const DecGroupKey &o) const { return cs != o.cs ? cs < o.cs : slice_len < o.slice_len; }
    bool operator==(const DecGroupKey &o) const { return cs == o.cs && slice_len == o.slice_len; }
};
using DecGroups = std::map<DecGroupKey, std::vector<GpeJob>>;

struct DecPlan {
    std::vector<uint64_t> keys;  // distinct dec_key values, first seen first: a job's `pattern` indexes it
    DecGroups groups;            // a decode stripe's job (a ranged one carries its window [out_lo, out_len))
    DecGroups chunk_groups;      // a chunk stripe's erased chunk: a windowed recover job (the rest joins the gather)
    std::vector<CopyJob> copies;  // ranged reads: a copy stripe's window, gathered from the present data chunks
    bool fused = false, ranged_call = false;
    // te_range_launch_stats / te_range_chunk_stats of the walk
    uint64_t touched = 0, copied = 0, decoded = 0, rebuilt = 0, chunk_gather = 0, bytes_stored = 0;
};

// Walk a call's items once: every stripe (a ranged item's touched stripes) becomes gather pieces
// or a job in its group.  The base pointers are only offset, never read.
inline DecPlan dec_plan(const ClayHost &h, int rotated, bool raw, const DecItem *items, size_t nitems,
                        const uint8_t *d_slices, uint8_t *d_out) {
    const int n = h.n;
    DecPlan P;
    std::unordered_map<uint64_t, uint32_t> pat_index;  // dec_key -> pattern id
    for (size_t i = 0; i < nitems; i++) {
        const DecItem &it = items[i];
        uint64_t sb = 0, se = it.ns;
        if (it.ranged) range_stripes(it.stripe, it.w_start, it.w_len, sb, se);
        P.ranged_call = P.ranged_call || it.ranged;
        // a ranged or chunk job's `out` may lie below the caller's range: computed as an integer
        const uintptr_t obase = reinterpret_cast<uintptr_t>(d_out) + it.out_off;
        for (uint64_t st = sb; st < se; st++) {
            RangeWin win{0, 0, false};
            bool chunk = false;  // rebuild chunk win.miss_x alone
            if (it.ranged) {
                win = range_window(n, rotated, it.avail, it.blob_len, it.stripe, it.cs, st, it.w_start, it.w_len);
                chunk = range_is_chunk(it, win);
                P.touched++;
                if (win.copy || chunk) {
                    (chunk ? P.rebuilt : P.copied)++;
                    for (uint64_t x = win.lo / it.cs; x * it.cs < win.hi; x++) {
                        if (chunk && x == win.miss_x) continue;
                        const uint64_t a = std::max(win.lo, x * it.cs), b = std::min(win.hi, (x + 1) * it.cs);
                        const uint32_t sl = shard_to_slice(rotated, (uint32_t)n, (uint32_t)st, (uint32_t)x);
                        CopyJob cj{};
                        cj.src = d_slices + it.in_base + sl * it.slice_len + (st * it.cs - it.in_skew) + (a - x * it.cs);
                        cj.dst = d_out + it.out_off + (st * it.stripe + a - it.w_start);
                        cj.len = cj.valid = b - a;
                        P.copies.push_back(cj);
                        P.chunk_gather += chunk;
                    }
                    if (!chunk) continue;
                } else {
                    P.decoded++;
                }
            }
            const int onode = stripe_out_node(h, rotated, it, st, chunk, win.miss_x);
            P.fused = P.fused || it.lost >= 0;
            const uint64_t pkey = dec_key(stripe_emask(h, rotated, it.avail, st), onode);
            const auto f = pat_index.emplace(pkey, (uint32_t)P.keys.size());
            if (f.second) P.keys.push_back(pkey);
            GpeJob g{};
            g.in = d_slices + it.in_base + (st * it.cs - it.in_skew);
            g.in_len = ~0ull;
            if (chunk) {
                // `out` is the address of the erased chunk's byte 0 (below the caller's range when
                // the window starts inside the chunk), the window [out_lo, out_len) in chunk bytes
                const uint64_t x0 = win.miss_x * it.cs;
                g.out = reinterpret_cast<uint8_t *>(obase + st * it.stripe + x0 - it.w_start);
                g.out_lo = std::max(win.lo, x0) - x0;
                g.out_len = std::min(win.hi, x0 + it.cs) - x0;
                P.bytes_stored += g.out_len - g.out_lo;
            } else if (onode >= 0) {  // the lost slice's chunk of this stripe, whole
                g.out = d_out + it.out_off + st * it.cs;
                g.out_len = it.cs;
            } else if (it.ranged) {
                // `out` stays the address of stripe byte 0: for a window's first stripe that is
                // below the caller's range by out_lo bytes, which the kernels never store to
                g.out = reinterpret_cast<uint8_t *>(obase + st * it.stripe - it.w_start);
                g.out_lo = win.lo;
                g.out_len = win.hi;
            } else {
                g.out = d_out + it.out_off + st * (raw ? 0 : it.stripe);
                g.out_len = raw ? it.cs * (uint64_t)h.k : (st + 1 == it.ns ? it.blob_len - st * it.stripe : it.stripe);
            }
            g.rot = rotated ? (uint32_t)((st * TE_ROTATION_STEP) % n) : 0u;
            g.pattern = f.first->second;
            (chunk ? P.chunk_groups : P.groups)[DecGroupKey{it.cs, it.slice_len}].push_back(g);
        }
    }
    return P;
}

// One class launch: the jobs of one group whose survivor sets share a class kernel (`id`: its
// registry id, a windowed kernel's for a chunk group).  off: decode_enqueue's arena offset.
struct DecClassGrp { DecGroupKey key; int id; std::vector<GpeJob> jobs; size_t off = 0; };
struct DecRoute {
    std::vector<DecClassGrp> cls;  // the decode groups' classes (group order, first seen first), then the chunk groups'
    bool cls_small = false;        // the class stripes fit one round of per-call workgroups
    bool folded = false;           // the fold-back rule sent the class stripes back to their table groups
    int err = TE_OK;               // TE_ERR_UNSUPPORTED: a chunk stripe without a windowed class kernel
};

// Decode class kernels (decode_class.hip, dec_class.hpp): the stripes of every Clay(20,7,16)
// survivor set run the ahead-of-time kernel of the set's class -- the program's control compiled in,
// the set's slices, planes and decoding matrix read at run time.  pat_class[p]: pattern p's class
// (dec_class_of, -1: none); linked(id): the kernel is in the library; staged: every pattern of the
// call has a plane program.  What stays in `groups` runs the table-driven (or generic) kernel.
// Knobs: class_on (dec_class_on), streams the class groups run on side by side, small (TEC_DEC_CLASS_SMALL=1).
template <class Linked>
inline DecRoute dec_route(const ClayHost &h, bool staged, const std::vector<int> &pat_class, Linked linked,
                          DecGroups &groups, const DecGroups &chunk_groups, bool class_on, int streams, bool small) {
    DecRoute R;
    auto add = [&R](int *at, const DecGroupKey &key, int id, const GpeJob &g) {
        if (at[id] < 0) {
            at[id] = (int)R.cls.size();
            R.cls.push_back(DecClassGrp{key, id, {}});
        }
        R.cls[(size_t)at[id]].jobs.push_back(g);
    };
    int at[kDecClassKernels];
    if (staged && class_on) {
        for (auto &kv : groups) {
            if (!dec_geom_staged(h, kv.first.cs, kv.first.slice_len)) continue;
            std::fill(at, at + kDecClassKernels, -1);
            std::vector<GpeJob> rest;
            for (const GpeJob &g : kv.second) {
                const int id = pat_class[g.pattern];
                if (id >= 0 && linked(id)) add(at, kv.first, id, g);
                else rest.push_back(g);
            }
            kv.second.swap(rest);
        }
        // a call that does not fill the GPU is bound by one stripe's 100-step chain per launch:
        // with more class groups than streams some launches would run after others, so such a
        // call runs on the table-driven kernel in one launch (per call 64 MiB: 3.67 ms as
        // classes against 3.00, r06)
        // (per-call decodes of <= 64 stripes run the classes' one-wave kernels, whose input loads
        // lead by four steps: their chains are short enough to run a few one after another)
        // (small: a call whose class stripes fit one round of per-call workgroups -- <= 2 per CU by
        // LDS -- keeps them; measured slower for 64 MiB per call, kernel 0.596 ms against 0.472)
        size_t ncls = 0, nall = 0, small_wgs = 0;
        for (const DecClassGrp &cg : R.cls) {
            ncls += cg.jobs.size();
            small_wgs += cg.jobs.size() * (size_t)((cg.key.cs / (uint64_t)h.alpha / 4 + 63) / 64);
        }
        for (auto &kv : groups) nall += kv.second.size();
        R.cls_small = small && !R.cls.empty() && small_wgs <= 512;
        R.folded = !R.cls_small && R.cls.size() > (size_t)streams && ncls < 1024 && ncls + nall > kDecSmallStripes;
        if (R.folded) {
            for (DecClassGrp &cg : R.cls) groups[cg.key].insert(groups[cg.key].end(), cg.jobs.begin(), cg.jobs.end());
            R.cls.clear();
        }
    }
    // chunk stripes (TE_RANGE_CHUNK): each on the windowed kernel of its recover class, a launch
    // per class beside the decode classes' (they never join the table-driven launch: only the
    // class kernels clip a recover job's window).  range_chunk_ok admitted the object, so a
    // missing kernel here is an error, not a reason to decode the stripe another way.
    for (const auto &kv : chunk_groups) {
        R.err = TE_ERR_UNSUPPORTED;
        if (!staged || !class_on || !dec_geom_staged(h, kv.first.cs, kv.first.slice_len)) return R;
        std::fill(at, at + kDecClassKernels, -1);
        for (const GpeJob &g : kv.second) {
            const int id = dec_class_win_id(pat_class[g.pattern]);
            if (id < 0 || !linked(id)) return R;
            add(at, kv.first, id, g);
        }
        R.err = TE_OK;
    }
    return R;
}

}  // namespace tec
