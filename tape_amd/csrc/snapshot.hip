// snapshot.hip -- the byte-shuffling kernels of the snapshot codec (te_snapshot_*; lib/snapshot/src/
// {encode,decode,chunk}.rs): pack_segment + the OuterCoder's data shards + SnapshotChunkPayload
// headers in one pass on the way in, unpack_segment + concatenation on the way out.  The GF work
// between them is rs16.hip's and the Clay kernels'.
//
// Both copies move bytes between a 16-byte aligned side and a side at an arbitrary byte address
// (the compressed log; `s * segment_bytes + j * symbol_bytes - 4` is no multiple of anything).  The
// unaligned side is read as aligned dwords, five per 16 output bytes, funnel-shifted into place
// (v_alignbyte_b32); the aligned side moves 16 bytes per lane.  No byte loads.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.hpp"

namespace tec {
namespace snapk {

// The 16 bytes at byte address p, from aligned dwords.  [lo, hi) bounds the bytes that may be
// read: a dword is loaded only if it holds one of them (so the loads stay inside the pages of the
// caller's buffer), and bytes outside read as zero.
__device__ __forceinline__ uint4 load16_unaligned(uintptr_t p, uintptr_t lo, uintptr_t hi) {
    const uintptr_t a = p & ~(uintptr_t)3;
    const uint32_t sh = (uint32_t)(p & 3u);
    uint32_t w[5];
    if (a >= lo && a + 20u <= hi) {  // interior: plain loads
#pragma unroll
        for (int i = 0; i < 5; i++) w[i] = *reinterpret_cast<const uint32_t *>(a + 4u * i);
    } else {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uintptr_t wa = a + 4u * i;
            w[i] = 0;
            if (wa + 4u > lo && wa < hi && (i < 4 || sh)) {
                const uint32_t b0 = wa < lo ? (uint32_t)(lo - wa) : 0u;            // 0..3
                const uint32_t b1 = hi - wa < 4u ? (uint32_t)(hi - wa) : 4u;       // 1..4
                const uint32_t m = (b1 == 4u ? ~0u : (1u << (8u * b1)) - 1u) & ~((1u << (8u * b0)) - 1u);
                w[i] = *reinterpret_cast<const uint32_t *>(wa) & m;
            }
        }
    }
    uint4 v;
    v.x = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
    v.y = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
    v.z = __builtin_amdgcn_alignbyte(w[3], w[2], sh);
    v.w = __builtin_amdgcn_alignbyte(w[4], w[3], sh);
    return v;
}

// One thread per 16 bytes of data symbol, then one per payload header.  Unit u of segment s is
// bytes [16 u, 16 u + 16) of the packed segment [u32 LE len | segment bytes | zeros], which is also
// byte r of data shard j (16 u = j * sym + r): the k data shards are the packed segment itself.
__global__ void __launch_bounds__(256) snap_pack_kernel(SnapPackArgs a) {
    const uint64_t units_a = (uint64_t)a.k * a.sym_a / 16u, units_b = (uint64_t)a.k * a.sym_b / 16u;
    const uint64_t units = (uint64_t)(a.segs - 1u) * units_a + units_b;
    const uint64_t seg_slots = (uint64_t)a.n * (a.sym_a + 64u);
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < units) {
        uint64_t s = a.segs - 1u, u = g - s * units_a;
        if (g < s * units_a) { s = g / units_a; u = g - s * units_a; }
        const uint64_t sym = s + 1u < a.segs ? a.sym_a : a.sym_b;
        const uint64_t q = 16u * u, j = q / sym, r = q - j * sym;
        const uint64_t seg_start = s * a.seg_bytes;
        const uint64_t seg_len = seg_start >= a.len ? 0u : (a.len - seg_start < a.seg_bytes ? a.len - seg_start : a.seg_bytes);
        const uintptr_t lo = reinterpret_cast<uintptr_t>(a.src) + seg_start, hi = lo + seg_len;
        uint4 v = load16_unaligned(lo + q - 4u, lo, hi);  // q == 0: the four bytes before lo read as zero
        if (q == 0) v.x = (uint32_t)seg_len;
        *reinterpret_cast<uint4 *>(a.work + 64u + s * seg_slots + j * (sym + 64u) + r) = v;
        return;
    }
    const uint64_t h = g - units;  // payload header: ChunkNumber::pack of the segment index
    if (h >= (uint64_t)a.segs * a.n) return;
    const uint64_t s = h / a.n, p = h - s * a.n;
    const uint64_t sym = s + 1u < a.segs ? a.sym_a : a.sym_b;
    *reinterpret_cast<uint64_t *>(a.work + 56u + s * seg_slots + p * (sym + 64u)) = a.seg0 + s;
}

__global__ void snap_headers_kernel(const uint8_t *__restrict__ work, const uint64_t *__restrict__ off, uint32_t count,
                                    uint64_t *__restrict__ hdr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) hdr[i] = *reinterpret_cast<const uint64_t *>(work + off[i]);
}

// blockIdx.y = segment.  Every workgroup reads all the length prefixes (a snapshot has at most a
// few hundred segments): the sum before its own is its output offset, the total and the checks
// decide whether anything is written at all -- no second host wait.
__global__ void __launch_bounds__(256) snap_unpack_kernel(SnapUnpackArgs a) {
    __shared__ unsigned long long sh_off, sh_total;
    __shared__ uint32_t sh_bad;
    const uint32_t s = blockIdx.y;
    if (threadIdx.x == 0) { sh_off = 0; sh_total = 0; sh_bad = 0; }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.segs; i += blockDim.x) {
        const uint64_t len = *reinterpret_cast<const uint32_t *>(a.packed + (uint64_t)i * a.stride);
        if (4u + len > a.cap[i]) atomicOr(&sh_bad, 1u);  // unpack_segment chunk.rs:82-85
        atomicAdd(&sh_total, (unsigned long long)len);
        if (i < s) atomicAdd(&sh_off, (unsigned long long)len);
    }
    __syncthreads();
    const uint64_t total = sh_total;
    const uint32_t status = sh_bad ? 5u : total > a.out_cap ? 25u : 0u;  // TE_ERR_INVALID_LAYOUT / _BUFFER_TOO_SMALL
    if (s == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        a.result[0] = status;
        a.result[1] = total;
    }
    if (status) return;
    const uint8_t *seg = a.packed + (uint64_t)s * a.stride;
    const uint64_t len = *reinterpret_cast<const uint32_t *>(seg);
    if (len == 0) return;
    const uintptr_t src = reinterpret_cast<uintptr_t>(seg) + 4u;
    const uintptr_t dst = reinterpret_cast<uintptr_t>(a.out) + sh_off, end = dst + len;
    const uintptr_t d0 = dst & ~(uintptr_t)15;
    const uint64_t units = (end - d0 + 15u) / 16u;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (uint64_t)gridDim.x * blockDim.x) {
        const uintptr_t d = d0 + 16u * u;
        // the source of d's 16 bytes; up to 15 bytes before src (the prefix and the slack before
        // it) or past the data (the segment's padding and slack): all readable, never stored
        const uint4 v = load16_unaligned(src + d - dst, 0, ~(uintptr_t)0);
        if (d >= dst && d + 16u <= end) {
            *reinterpret_cast<uint4 *>(d) = v;
        } else {  // a segment's first and last 16 bytes: only its own bytes, its neighbours' are another workgroup's
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t b = 0; b < 16u; b++)
                if (d + b >= dst && d + b < end) *reinterpret_cast<uint8_t *>(d + b) = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
        }
    }
}

}  // namespace snapk

hipError_t launch_snap_pack(const SnapPackArgs &a, hipStream_t s) {
    if (a.segs == 0 || a.k == 0 || a.n < a.k || a.sym_a % 64u || a.sym_b % 64u || !a.sym_a || !a.sym_b ||
        (reinterpret_cast<uintptr_t>(a.work) & 63u))
        return hipErrorInvalidValue;
    const uint64_t threads = (uint64_t)(a.segs - 1u) * a.k * (a.sym_a / 16u) + (uint64_t)a.k * (a.sym_b / 16u) + (uint64_t)a.segs * a.n;
    const uint64_t blocks = (threads + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snapk::snap_pack_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_snap_headers(const uint8_t *work, const uint64_t *off, uint32_t count, uint64_t *hdr, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(snapk::snap_headers_kernel, dim3((count + 255u) / 256u), dim3(256), 0, s, work, off, count, hdr);
    return hipGetLastError();
}

hipError_t launch_snap_unpack(const SnapUnpackArgs &a, hipStream_t s) {
    if (a.segs == 0 || a.segs > 65535u || a.stride % 64u) return hipErrorInvalidValue;
    // workgroups per segment: enough for the largest segment at 4 units per thread, at most 1024
    const uint64_t want = (a.stride / 16u + 1023u) / 1024u;
    const uint32_t gx = (uint32_t)(want < 1u ? 1u : want > 1024u ? 1024u : want);
    hipLaunchKernelGGL(snapk::snap_unpack_kernel, dim3(gx, a.segs), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace tec
