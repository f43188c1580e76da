// Window planning of the host pipelines (engine.cpp): copy runs, window cuts and the verify
// workspace's layout.  Host-only and pure: no HIP, no handle -- tests/test_win_plan.py builds this
// header into a stand-alone check (tests/native/win_plan_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace tec {

// Host <-> device copy runs of a window: pieces contiguous on both sides move with one DMA.
struct CopyRun { uint64_t host, dev, len; };

inline void add_run(std::vector<CopyRun> &v, uint64_t host, uint64_t dev, uint64_t len) {
    if (!len) return;
    if (!v.empty() && v.back().host + v.back().len == host && v.back().dev + v.back().len == dev)
        v.back().len += len;
    else
        v.push_back({host, dev, len});
}

// device copies are 16-byte aligned
inline uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

// A batch of objects of bytes[i] each, cut into windows [cuts[w], cuts[w + 1]): at least one object
// per window, then as many as fit window_bytes (0: 128 MiB, the encode pipeline's default).
inline void window_cuts(const std::vector<uint64_t> &bytes, size_t window_bytes, std::vector<size_t> &cuts) {
    if (window_bytes == 0) window_bytes = (size_t)128 << 20;
    cuts.assign(1, 0);
    uint64_t sum = 0;
    for (size_t i = 0; i < bytes.size(); i++) {
        if (i > cuts.back() && sum + bytes[i] > window_bytes) {
            cuts.push_back(i);
            sum = 0;
        }
        sum += bytes[i];
    }
    if (!bytes.empty()) cuts.push_back(bytes.size());
}

// A verify workspace.  Device: expected leaves | digests (peers, then results) | narr mask arrays;
// its page-locked host side: expected leaves | the mask arrays.  Mask array 0 is the peers', 1 the
// rebuilt slices'; a read has dig_o = 0 and narr = 1.
struct VerLayout {
    size_t exp_b, dig_p, dig_o, mask_b, narr;
    size_t dig_off(int which) const { return exp_b + (which ? dig_p : 0); }
    size_t mask_off(int which) const { return exp_b + dig_p + dig_o + (size_t)which * mask_b; }
    size_t total() const { return mask_off(0) + narr * mask_b; }
    size_t h_mask(int which) const { return exp_b + (size_t)which * mask_b; }
    size_t h_total() const { return exp_b + narr * mask_b; }
};

}  // namespace tec
