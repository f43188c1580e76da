// verify.hip -- received slices checked against their leaf commitments on the device: the read
// side of commit.hip.  BlobEncoding::verify_slice (lib/core/src/track/blob.rs:72-79) is
// hash_leaf(data) == leaves[position]; its callers (the gateway's object read, decode.rs:121-139;
// node recover, recover.rs:207-218; repair, repair.rs:339-341; sync, sync.rs:266-289; snapshot,
// snapshot.rs:255) run it on every slice that enters or leaves the codec.
//
// MI355X mapping.  As in commit.hip, SHA-256 is serial within a slice, so the parallelism is the
// number of slices: one lane per item.  A read batch is ragged where a written one is regular --
// some of an object's slices, objects of different lengths -- so a lane takes everything from its
// item: where its bytes are, how long they are, which expected hash they answer to, and which bit
// of which object's mask a match sets.  Each lane has its own block count and leaves the block
// loop at its own end.  The host sorts the items by block count, descending (VerifyItem::index
// is the caller's position, and every output is indexed by it), so the lanes of a wave are alike
// and the waves still hashing at block b0 are a prefix of the grid: a launch covers that prefix
// only.  Launches are short for commit.hip's reason; between them a lane's state is
// parked in its digest slot.
#include "kernels.hpp"
#include "sha256.hpp"

namespace tec {
namespace verify {

#ifndef TEC_VERIFY_PRIO
#define TEC_VERIFY_PRIO 3  // leaf_kernel's wave priority: few waves, each one serial chain
#endif

// Blocks [b0, b1) of items 0 .. live-1, every one of which has more than b0 blocks.
__global__ void __launch_bounds__(64) verify_kernel(VerifyArgs a, uint32_t live, uint64_t b0, uint64_t b1) {
    if constexpr (TEC_VERIFY_PRIO > 0) __builtin_amdgcn_s_setprio(TEC_VERIFY_PRIO);
    const uint32_t gid = blockIdx.x * 64u + threadIdx.x;
    if (gid >= live) return;
    const VerifyItem it = a.items[gid];
    const uint32_t *p = reinterpret_cast<const uint32_t *>(a.data + it.offset);
    const uint64_t L = it.len, M = L + 4u;            // message bytes ("LEAF" || slice)
    const uint64_t T = verify_blocks(L);              // blocks incl. padding and length
    const uint64_t nfull = L >= 60u ? (L - 60u) / 64u + 1u : 0u;  // blocks 0 .. nfull-1 hold data only
    if (b1 > T) b1 = T;
    uint32_t *out = reinterpret_cast<uint32_t *>(a.digests + (uint64_t)it.index * 32u);
    uint32_t st[8];
    if (b0 == 0) {
        sha::init(st);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) st[i] = out[i];
    }
    // leaf_kernel's pipeline: raw words loaded two blocks ahead, byte-swapped when their block starts
    uint32_t w[16], n1[16], n2[16];
    const uint64_t dend = nfull < b1 ? nfull : b1;
    auto ldblk = [&](uint64_t b, uint32_t *dst) {
        if (b == 0) {
            dst[0] = sha::bswap(sha::kLeafWord);
#pragma unroll
            for (int k = 1; k < 16; k++) dst[k] = p[k - 1];
        } else {
            const uint32_t *q = p + b * 16u - 1u;
#pragma unroll
            for (int k = 0; k < 16; k++) dst[k] = q[k];
        }
    };
    if (b0 < dend) ldblk(b0, n1);
    if (b0 + 1 < dend) ldblk(b0 + 1, n2);
    for (uint64_t b = b0; b < dend; b++) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            w[k] = sha::bswap(n1[k]);
            n1[k] = n2[k];
        }
        if (b + 2 < dend) ldblk(b + 2, n2);
        sha::compress(st, w);
    }
    // the lane's own tail: its last data bytes, the 0x80 terminator, zeros and the bit length
    for (uint64_t b = (nfull > b0 ? nfull : b0); b < b1; b++) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint64_t gw = b * 16u + (uint64_t)k, pos = gw * 4u;
            w[k] = gw == 0 ? sha::kLeafWord : (pos < M ? sha::bswap(p[gw - 1u]) : (pos == M ? 0x80000000u : 0u));
        }
        if (b + 1 == T) {
            w[14] = (uint32_t)((M * 8u) >> 32);
            w[15] = (uint32_t)(M * 8u);
        }
        sha::compress(st, w);
    }
    if (b1 < T) {
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = st[i];
        return;
    }
    bool same = true;
    const uint32_t *want = reinterpret_cast<const uint32_t *>(a.expected + (uint64_t)it.expected * 32u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t d = sha::bswap(st[i]);
        out[i] = d;
        if (a.expected) same = same && want[i] == d;
    }
    if (!a.expected) return;
    if (a.ok) a.ok[it.index] = same ? 1u : 0u;
    if (same && a.good_mask) atomicOr(a.good_mask + it.object, it.bit);
}

}  // namespace verify

// h_items: the host copy of a.items (sorted by block count, descending).
hipError_t launch_verify(const VerifyArgs &a, const VerifyItem *h_items, hipStream_t s) {
    if (a.nitems == 0) return hipSuccess;
    if (!a.items || !h_items || !a.digests) return hipErrorInvalidValue;
    const uint64_t T = verify_blocks(h_items[0].len);  // the longest item's
    const uint64_t nl = (T + kVerifyBlocksPerLaunch - 1) / kVerifyBlocksPerLaunch, per = (T + nl - 1) / nl;
    uint32_t live = a.nitems;
    for (uint64_t b0 = 0; b0 < T; b0 += per) {
        while (live && verify_blocks(h_items[live - 1].len) <= b0) live--;
        if (!live) break;
        hipLaunchKernelGGL(verify::verify_kernel, dim3((live + 63u) / 64u), dim3(64), 0, s, a, live, b0, b0 + per);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace tec
