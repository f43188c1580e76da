// root_check.hip -- an object's merkle root from its leaf hashes, checked on the device: the
// compare of verify_track_data (sdk/src/track/read.rs:174-185) after BlobEncoder::encode_with_root
// (sdk/src/codec/encoder.rs:166-193) has re-encoded and hashed the object.  root_from_leaf_hashes
// (lib/crypto/src/merkle/tree.rs:344-350): layer by layer, a missing right sibling is
// EMPTY_ROOTS[level] (tree.rs:430-440).
//
// MI355X mapping.  n <= 64 leaves: one wave per object, lane i holds leaf i as 8 big-endian words
// in registers.  Checking the leaves against BlobEncoding::leaves is one ballot.  Nodes stay in
// place: the node j of level l lives in lane j << l, so a level is one cross-lane exchange (each
// lane fetches the 8 words of lane + 2^l) and one hash_pair -- two SHA-256 blocks, "LEFT" || l ||
// "RIGHT" || r is 73 bytes -- whose result the lanes that are multiples of 2^(l+1) keep; the other
// lanes compute along and are never read again.  Once one node is left (level ceil(log2 n) and
// up) there is no exchange: lane 0 chains against the empty roots.  The empty roots are a kernel
// argument (33 x 8 words the host computes once), read with scalar loads at a wave-uniform level.
// The tree is ~2 log2(n) + 2 (height - log2 n) compressions per wave where tree_kernel's one lane
// per object runs ~2 n + 4 height of them over byte arrays in scratch.
#include <array>
#include "kernels.hpp"
#include "sha256.hpp"

namespace tec {
namespace rootcheck {

constexpr uint32_t kLeftWord = 0x4c454654u;   // "LEFT"
constexpr uint32_t kRighWord = 0x52494748u;   // "RIGH"
constexpr uint32_t kPairBits = 73u * 8u;      // 4 + 32 + 5 + 32 message bytes

// h <- hash_pair(h, r), everything as big-endian message words
__device__ __forceinline__ void pair(uint32_t h[8], const uint32_t r[8]) {
    uint32_t st[8], w[16];
    sha::init(st);
    w[0] = kLeftWord;
#pragma unroll
    for (int i = 0; i < 8; i++) w[1 + i] = h[i];
    w[9] = kRighWord;
    w[10] = 0x54000000u | (r[0] >> 8);  // 'T', then r one byte off the word grid
#pragma unroll
    for (int i = 1; i < 6; i++) w[10 + i] = (r[i - 1] << 24) | (r[i] >> 8);
    sha::compress(st, w);
    w[0] = (r[5] << 24) | (r[6] >> 8);
    w[1] = (r[6] << 24) | (r[7] >> 8);
    w[2] = (r[7] << 24) | 0x00800000u;
#pragma unroll
    for (int i = 3; i < 15; i++) w[i] = 0;
    w[15] = kPairBits;
    sha::compress(st, w);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = st[i];
}

__global__ void __launch_bounds__(kRootCheckWaves * 64) root_check_kernel(RootCheckArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t obj = (uint64_t)blockIdx.x * kRootCheckWaves + (threadIdx.x >> 6);
    if (obj >= a.nobj) return;  // whole waves: no barrier below
    const uint32_t n = a.n;
    const bool mine = lane < n;
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = 0;
    bool bad = false;
    if (mine) {
        const uint32_t *lv = reinterpret_cast<const uint32_t *>(a.leaf + (obj * n + lane) * 32u);
        uint32_t raw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) raw[i] = lv[i];
        if (a.expected_leaf) {
            const uint32_t *want = reinterpret_cast<const uint32_t *>(a.expected_leaf + (obj * n + lane) * 32u);
#pragma unroll
            for (int i = 0; i < 8; i++) bad = bad || want[i] != raw[i];
        }
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = sha::bswap(raw[i]);
    }
    if (a.expected_leaf && a.bad_leaf_mask) {
        const uint64_t m = __ballot(bad);
        if (lane == 0) a.bad_leaf_mask[obj] = m;
    }
    uint32_t c = n;  // nodes of the current level
    for (uint32_t l = 0; l < a.height; l++) {
        uint32_t r[8];
        bool have = false;  // a right sibling among the level's nodes
        if (c > 1) {        // c > 1 only while l < 6: the exchange stays inside the wave
#pragma unroll
            for (int i = 0; i < 8; i++) r[i] = (uint32_t)__shfl_down((int)h[i], 1u << l, 64);
            have = (lane >> l) + 1u < c;
        }
        if (!have) {
#pragma unroll
            for (int i = 0; i < 8; i++) r[i] = a.empty[l][i];
        }
        pair(h, r);
        c = (c + 1u) >> 1;
    }
    if (lane != 0) return;
    const uint32_t *want = reinterpret_cast<const uint32_t *>(a.expected_root + obj * 32u);
    uint32_t *out = a.root ? reinterpret_cast<uint32_t *>(a.root + obj * 32u) : nullptr;
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t d = sha::bswap(h[i]);
        same = same && want[i] == d;
        if (out) out[i] = d;
    }
    a.ok[obj] = same ? 1u : 0u;
}

}  // namespace rootcheck

static void root_check_fill_empty(RootCheckArgs &a) {
    static const auto table = [] {
        std::array<std::array<uint32_t, 8>, kRootCheckLevels> t{};
        uint8_t e[32], e2[32];
        sha::hash_leaf(nullptr, 0, e);
        for (int l = 0; l < kRootCheckLevels; l++) {
            for (int i = 0; i < 8; i++)
                t[l][i] = (uint32_t)e[4 * i] << 24 | (uint32_t)e[4 * i + 1] << 16 | (uint32_t)e[4 * i + 2] << 8 | e[4 * i + 3];
            sha::hash_pair(e, e, e2);
            for (int j = 0; j < 32; j++) e[j] = e2[j];
        }
        return t;
    }();
    for (int l = 0; l < kRootCheckLevels; l++)
        for (int i = 0; i < 8; i++) a.empty[l][i] = table[l][i];
}

hipError_t launch_root_check(RootCheckArgs a, hipStream_t s) {
    if (a.nobj == 0) return hipSuccess;
    if (a.n == 0 || a.n > (uint32_t)kCommitMaxLeaves || a.height >= (uint32_t)kRootCheckLevels || !a.leaf ||
        !a.expected_root || !a.ok)
        return hipErrorInvalidValue;
    const uint64_t grid = (a.nobj + kRootCheckWaves - 1) / kRootCheckWaves;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    root_check_fill_empty(a);
    hipLaunchKernelGGL(rootcheck::root_check_kernel, dim3((uint32_t)grid), dim3(kRootCheckWaves * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace tec
