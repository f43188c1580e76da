// recover_multi.hip -- multi-output rebuild for q = 10, t = 2 profiles (n = 20): node recover
// (network/node/src/features/spool/recover.rs:411-442 `reconstruct`) of several lost slices of one
// object from one layered decode.  7..10 peer slices in, any subset of the erased nodes out.
//
// The program is decode_stage.hip's: ClayHost::dec_prog(P, orient, H, steps, -1, out_mask) with
// out_mask = the stripe's lost nodes (data or parity, either column), packed by dec_pack, and the
// step loop below is that kernel's direct-output form (one word per lane, v_perm tables
// scalar-loaded, parked values in lane-private LDS slots or per-tile scratch rows, loads one step
// ahead, no staging rows and no barrier).  What differs is where an output row goes: a flush item
// names its node (x = node | plane << 8), and the job's RmSlots table maps the node to the output
// slot of the slice that holds it in this stripe -- the rotation moves that per stripe, so the
// table is per job, not per pattern.  Row r of node x is stored at
//   out + slot[x] * out_stride + plane * sc        (out_stride = the slice length)
// at the lane's load column; a node without a slot (an output of another pass) is not stored.
// Known nodes are never outputs here (the lost slices are disjoint from the survivors), so the
// known rows' copy path of the decode kernel is gone.
#include "kernels.hpp"
#include "gf_dev.hpp"
#include "dev_io.hpp"

namespace tec {
namespace rmulti {

constexpr int kMaxG = 2;           // waves per workgroup at most (decode_stage.hip: 2 measured best)
constexpr uint32_t kStAux = 2;     // output rows non-temporal, the known rows' own loads too
constexpr uint32_t kOwnAux = 2;

// PFT of the supported profiles (decode_stage.hip): U = 3 C ^ 2 Cp, the inverse has the same form
__device__ __forceinline__ uint32_t pft3(uint32_t a, uint32_t b) { return a ^ xt(a ^ b); }
static_assert(kPft.u_c[0] == 3 && kPft.u_p[0] == 2 && kPft.c_u[0] == 3 && kPft.c_p[0] == 2 &&
              kPft.u_c[1] == 3 && kPft.u_p[1] == 2 && kPft.c_u[1] == 3 && kPft.c_p[1] == 2, "PFT");
static_assert(kPft.t_u[0] == kPft.t_u[1] && kPft.t_p[0] == kPft.t_p[1] && (kPft.t_u[0] ^ kPft.t_p[0]) == 1,
              "type-1 C = t (U ^ Cp) ^ Cp");
static_assert(2 * kRepQ <= (int)sizeof(RmSlots::slot), "a slot per node");

template <int NK, int G>
__global__ void __launch_bounds__(G * 64, 4) recover_multi_kernel(DecArgs a, const RmSlots *__restrict__ slots) {
    constexpr int NE = 2 * kRepQ - NK;  // padded patterns: every other node erased
    constexpr uint32_t RS = G * 256u;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint8_t *const lds8 = reinterpret_cast<uint8_t *>(lds);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t col_local = threadIdx.x * 4u;

    const uint32_t tile = xcd_tile(blockIdx.x, gridDim.x);
    const uint32_t job = tile / a.wgs_per_stripe, seg = tile - job * a.wgs_per_stripe;
    typedef const __attribute__((address_space(4))) GpeJob cJob;
    typedef const __attribute__((address_space(4))) DecProgHdr cHdr;
    typedef const __attribute__((address_space(4))) uint32_t cU32;
    cJob &J = *(cJob *)(uintptr_t)(a.jobs + job);
    cHdr &H = *(cHdr *)(uintptr_t)(a.hdrs + J.pattern);
    const DecStepP *prog = a.steps + ((cU32 *)(uintptr_t)a.step_off)[J.pattern];
    const uint32_t sc = a.sc, wps = a.words_per_stripe;
    // a word whose high half lies past the sub-chunk (sc = 2 mod 4) loads the dword 2 bytes earlier;
    // every value is stored back at its load column and the arithmetic is byte-wise, so the loaded
    // byte order is kept throughout (words past the stripe alias the last: same values, same bytes)
    uint32_t w = seg * G * 64u + threadIdx.x;
    if (w >= wps) w = wps - 1;
    const uint32_t col = w * 4u;
    const uint32_t vcol = col + 4u > sc ? col - 2u : col;
    const uint32_t in_range = (uint32_t)(a.n * a.in_stride);  // host-checked < 2^31
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void *)J.in, 0, (int)in_range, 0x00020000);
    // the object's rebuilt slices from this stripe's chunk of the first one on: out_len ends at the
    // last slot's chunk, so a store past it fails the range check
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void *)J.out, 0, (int)(uint32_t)J.out_len, 0x00020000);
    uint8_t *const scr = a.scratch + (size_t)tile * a.nscratch_max * RS;
    const __amdgpu_buffer_rsrc_t rs_scr = __builtin_amdgcn_make_buffer_rsrc(scr, 0, (int)(a.nscratch_max * RS), 0x00020000);
    constexpr uint32_t kDrop = 0x80000000u;
    // the job's output table: node `lane`'s slot as a byte offset from J.out (kDrop: none)
    const uint32_t slot_l = lane < (uint32_t)(2 * kRepQ) ? slots[job].slot[lane] : kRmNoSlot;
    const uint32_t slot_off = slot_l == kRmNoSlot ? kDrop : slot_l * (uint32_t)a.out_stride;
    // input slice byte offset of internal node i (= shard i, nu = 0) in lane i, rotated
    uint32_t sl_lane = lane + J.rot;
    sl_lane = (sl_lane >= a.n ? sl_lane - a.n : sl_lane) * (uint32_t)a.in_stride;
    uint32_t kbase[NK];  // the known nodes' slices
#pragma unroll
    for (int j = 0; j < NK; j++) kbase[j] = __builtin_amdgcn_readlane(sl_lane, H.knode[j]);
    auto ldraw = [&](uint32_t so) -> uint32_t {
        return __builtin_amdgcn_raw_buffer_load_b32(rs_in, (int)vcol, (int)so, kOwnAux);
    };
    auto ldopt = [&](uint32_t so) -> uint32_t {  // a dropped offset fails the range check: 0
        return __builtin_amdgcn_raw_buffer_load_b32(rs_in, (int)vcol, (int)so, 0);
    };
    // LDS rows: a zero row, a trash row, then the lane-private slots
    constexpr uint32_t zrow = 0u, trow = 1u, srow0 = 2u;
    auto lds_at = [&](uint32_t off) -> uint32_t * { return reinterpret_cast<uint32_t *>(lds8 + off + col_local); };
    *lds_at(zrow * RS) = 0u;  // lane-private: read back only by this lane
    const uint32_t olen = (uint32_t)J.out_len;

    // Step control words in VGPRs (decode_stage.hip): a step's 48 words in lanes 0..47 of one VGPR,
    // loaded two steps ahead; per-word quantities derived in vector code, read with v_readlane
    typedef const __attribute__((address_space(4))) PermTab cPermTab;
    cPermTab(*D)[kGpeMaxKnown] = (cPermTab(*)[kGpeMaxKnown])(uintptr_t)(&a.patterns[J.pattern].D[0][0]);
    const __amdgpu_buffer_rsrc_t rs_prog = __builtin_amdgcn_make_buffer_rsrc((void *)prog, 0, (int)((H.nsteps + 2) * sizeof(DecStepP)), 0x00020000);
    const uint32_t progl = (lane < kDpWords ? lane : 0u) * 4u;
    auto ldw = [&](uint32_t st) -> uint32_t {
        return __builtin_amdgcn_raw_buffer_load_b32(rs_prog, (int)progl, (int)(st * (uint32_t)sizeof(DecStepP)), 0);
    };
    auto W = [](uint32_t v, int i) -> uint32_t { return __builtin_amdgcn_readlane(v, i); };
    const bool kd_l = lane >= kDpKd && lane < kDpKd + NK, ed_l = lane >= kDpEd && lane < kDpEd + NE;
    // input offset of the partner load word x describes (known input partner, type-1 partner)
    auto vec_in = [&](uint32_t x) -> uint32_t {
        const uint32_t k = x >> 28;
        const bool on = (kd_l && k == kKnInput) || (ed_l && k == kErType1);
        uint32_t sl_l = lane + J.rot;  // sl_lane, recomputed (not held across the loop)
        sl_l = (sl_l >= a.n ? sl_l - a.n : sl_l) * (uint32_t)a.in_stride;
        const uint32_t sl = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((x & 0xffu) << 2), (int)sl_l);
        return on ? sl + ((x >> 8) & 0xffu) * sc : kDrop;
    };
    // a consumed location (known partner C, pair partner U): scratch offset or kDrop ...
    auto consumed = [&](uint32_t x, uint32_t ty) {
        const uint32_t k = x >> 28;
        return ((kd_l && k == kKnLoc) || (ed_l && k == kErFinish)) && ((x >> 8) & 3u) == ty;
    };
    auto vec_scr = [&](uint32_t x) -> uint32_t { return consumed(x, kLocScratch) ? (x & 0xffu) * RS : kDrop; };
    // ... and its LDS row (the zero row unless a slot)
    auto vec_slot = [&](uint32_t x) -> uint32_t { return (consumed(x, kLocSlot) ? srow0 + (x & 0xffu) : zrow) * RS; };
    // a produced value's 10-bit location -> LDS row offset (trash row for none / output / scratch)
    auto dst_lds = [&](uint32_t f) -> uint32_t {
        const uint32_t ty = (f >> 8) & 3u, ix = f & 0xffu;
        return (((f & 0x3ffu) != kLoc10None && ty == kLocSlot) ? srow0 + ix : trow) * RS;
    };
    auto dst_scr = [&](uint32_t f) -> uint32_t {
        return ((f & 0x3ffu) != kLoc10None && ((f >> 8) & 3u) == kLocScratch) ? (f & 0xffu) * RS : kDrop;
    };
    // an output destination's flush item (node | plane << 8) through the job's table: the row's
    // byte offset from J.out, or kDrop
    auto vec_out = [&](uint32_t f, uint32_t wd) -> uint32_t {
        const uint32_t ix = f & 0xffu;
        const uint32_t iw = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((kDpOut + (ix >> 1)) << 2), (int)wd);
        const uint32_t it = (iw >> (16u * (ix & 1u))) & 0xffffu;
        const uint32_t so = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((it & 0x1fu) << 2), (int)slot_off);
        const bool st = (f & 0x3ffu) != kLoc10None && ((f >> 8) & 3u) == kLocStage && (it & 0xffu) < 2u * kRepQ;
        return st && so != kDrop ? so + (it >> 8) * sc : kDrop;
    };
    // one rebuilt word (in the lane's load order) to its row at `off` (uniform), at the lane's load
    // column; a row that would cross out_len is written byte by byte (bytes past it fail the range check)
    auto put_out = [&](uint32_t off, uint32_t v) {
        if (off == kDrop) return;
        if (off + sc <= olen) {
            __builtin_amdgcn_raw_buffer_store_b32(v, rs_out, (int)vcol, (int)off, kStAux);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4u; b++)
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v >> (8u * b)), rs_out, (int)(vcol + b), (int)off, 0);
        }
    };

    uint32_t own[NK], part[NK], tkp[NE];
    auto load_known = [&](uint32_t x) {
        const uint32_t zs = (W(x, kDpHdr) & 0xffu) * sc;
        const uint32_t vin = vec_in(x);
#pragma unroll
        for (int j = 0; j < NK; j++) {
            own[j] = ldraw(kbase[j] + zs);
            part[j] = ldopt(W(vin, kDpKd + j));
        }
    };
    auto load_tkp = [&](uint32_t x) {
        const uint32_t vin = vec_in(x);
#pragma unroll
        for (int e = 0; e < NE; e++) tkp[e] = ldopt(W(vin, kDpEd + e));
    };
    // scratch loads of a step, issued after the previous step's scratch stores (lane-private
    // addresses: program order within the lane is the only ordering needed)
    uint32_t ksc[NK], esc[NE];
    auto load_scr = [&](uint32_t x) {
        const uint32_t vs = vec_scr(x);
#pragma unroll
        for (int j = 0; j < NK; j++)
            ksc[j] = __builtin_amdgcn_raw_buffer_load_b32(rs_scr, (int)col_local, (int)W(vs, kDpKd + j), 0);
#pragma unroll
        for (int e = 0; e < NE; e++)
            esc[e] = __builtin_amdgcn_raw_buffer_load_b32(rs_scr, (int)col_local, (int)W(vs, kDpEd + e), 0);
    };

    const uint32_t nsteps = H.nsteps;
    uint32_t w_cur = ldw(0), w_nxt = ldw(1);  // steps nsteps, nsteps + 1 are blank
    load_known(w_cur);
    load_tkp(w_cur);
    load_scr(w_cur);
    for (uint32_t st = 0; st < nsteps; st++) {
        const uint32_t w_nn = ldw(st + 2);
        uint32_t ctkp[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) ctkp[e] = tkp[e];
        // ---- uncouple the known nodes: dropped loads read 0, a non-slot partner reads the zero
        // row, a red node masks the PFT term ----
        const uint32_t vsl = vec_slot(w_cur);
        Sel sel[NK];
#pragma unroll
        for (int j = 0; j < NK; j++) {
            const uint32_t mred = (W(w_cur, kDpKd + j) >> 28) == kKnRed ? 0u : ~0u;
            const uint32_t p = part[j] ^ ksc[j] ^ *lds_at(W(vsl, kDpKd + j));
            sel[j] = Sel(own[j] ^ (xt(own[j] ^ p) & mred));
        }
        // the next step's known-row loads once this step's are consumed (no second register set)
        load_known(w_nxt);
        // pair partners' U (read before this step's writes: a location may be rewritten from its
        // consumer step on)
        uint32_t pu[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) pu[e] = esc[e] ^ *lds_at(W(vsl, kDpEd + e));
        // ---- MDS-solve the erased U's the program needs ----
        uint32_t acc[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            acc[e] = 0;
            if ((W(w_cur, kDpEd + e) >> 28) == kErSkip) continue;
#pragma unroll
            for (int j = 0; j + 1 < NK; j += 2)
                acc[e] = perm_mul2_acc(acc[e], sel[j], D[e][j].t[0], D[e][j].t[1], D[e][j].t[2], D[e][j].t[3], D[e][j].t[4],
                                       sel[j + 1], D[e][j + 1].t[0], D[e][j + 1].t[1], D[e][j + 1].t[2], D[e][j + 1].t[3],
                                       D[e][j + 1].t[4]);
            if (NK & 1)
                acc[e] = perm_mul_acc(acc[e], sel[NK - 1], D[e][NK - 1].t[0], D[e][NK - 1].t[1], D[e][NK - 1].t[2],
                                      D[e][NK - 1].t[3], D[e][NK - 1].t[4]);
        }
        // ---- writes: lane A of an erased word is its park location (ed) / ed0 (eo), B and C the
        // output-only ed1 / epd ----
        const uint32_t fa = ed_l ? (((w_cur >> 28) == kErPark) ? w_cur : kLoc10None) : (kd_l ? kLoc10None : w_cur);
        const uint32_t la = dst_lds(fa), sa = dst_scr(fa);
        const uint32_t oa = vec_out(w_cur, w_cur), ob = vec_out(w_cur >> 10, w_cur), oc = vec_out(w_cur >> 20, w_cur);
        auto put_a = [&](int i, uint32_t v) {
            *lds_at(W(la, i)) = v;
            const uint32_t so = W(sa, i);
            if (so != kDrop) __builtin_amdgcn_raw_buffer_store_b32(v, rs_scr, (int)col_local, (int)so, 0);
        };
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const uint32_t ek = W(w_cur, kDpEd + e) >> 28;
            if (ek == kErRed) {
                put_out(W(oa, kDpEo + e), acc[e]);
            } else if (ek == kErType1) {
                const uint32_t c = mulc(kPft.t_u[0], acc[e] ^ ctkp[e]) ^ ctkp[e];
                put_a(kDpEo + e, c);
                put_out(W(ob, kDpEo + e), c);
            } else if (ek == kErPark) {
                put_a(kDpEd + e, acc[e]);
            } else if (ek == kErFinish) {
                const uint32_t c0 = pft3(acc[e], pu[e]), c1 = pft3(pu[e], acc[e]);
                put_out(W(oa, kDpEo + e), c0);
                put_out(W(oc, kDpEo + e), c1);
            }
        }
        load_tkp(w_nxt);
        load_scr(w_nxt);
        w_cur = w_nxt;
        w_nxt = w_nn;
    }
}

static uint32_t wgs_per_stripe(uint32_t words_per_stripe, uint32_t gmax) {
    const uint32_t groups = (words_per_stripe + 63) / 64, g = recover_multi_g(words_per_stripe, gmax);
    return (groups + g - 1) / g;
}

template <int NK, int G>
static hipError_t launch_g(const DecArgs &a, const RmSlots *slots, uint64_t blocks, hipStream_t s) {
    const size_t lds = (size_t)a.lds_rows * G * 256u;
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void *>(recover_multi_kernel<NK, G>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((recover_multi_kernel<NK, G>), dim3((uint32_t)blocks), dim3(G * 64), lds, s, a, slots);
    return hipGetLastError();
}
template <int NK>
static hipError_t launch_k(const DecArgs &a, const RmSlots *slots, uint32_t g, uint64_t blocks, hipStream_t s) {
    static_assert(kMaxG == 2, "one instance per g");
    return g < 2 ? launch_g<NK, 1>(a, slots, blocks, s) : launch_g<NK, 2>(a, slots, blocks, s);
}

}  // namespace rmulti

uint32_t recover_multi_g(uint32_t words_per_stripe, uint32_t gmax) {
    const uint32_t groups = (words_per_stripe + 63) / 64;
    const uint32_t cap = gmax && gmax < (uint32_t)rmulti::kMaxG ? gmax : (uint32_t)rmulti::kMaxG;
    return groups < cap ? groups : cap;
}

size_t recover_multi_scratch_bytes(const DecArgs &a) {
    const uint32_t g = recover_multi_g(a.words_per_stripe, a.gmax);
    return (size_t)a.njobs * rmulti::wgs_per_stripe(a.words_per_stripe, a.gmax) * (a.nscratch_max ? a.nscratch_max : 1) * g * 256u;
}

hipError_t launch_recover_multi(DecArgs a, const RmSlots *slots, hipStream_t s) {
    if (a.njobs == 0) return hipSuccess;
    if (a.lds_rows < 2 || a.lds_rows > kRmMaxLdsRows || a.sc < 8 || !a.scratch || !slots || a.n != 2u * kRepQ ||
        a.nk < 7 || a.nk > 10 || (uint64_t)a.n * a.in_stride > 0x7fffffffull || (uint64_t)a.n * a.out_stride > 0x7fffffffull)
        return hipErrorInvalidValue;
    const uint32_t g = recover_multi_g(a.words_per_stripe, a.gmax);
    a.wgs_per_stripe = rmulti::wgs_per_stripe(a.words_per_stripe, a.gmax);
    const uint64_t blocks = (uint64_t)a.njobs * a.wgs_per_stripe;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    switch (a.nk) {
        case 7: return rmulti::launch_k<7>(a, slots, g, blocks, s);
        case 8: return rmulti::launch_k<8>(a, slots, g, blocks, s);
        case 9: return rmulti::launch_k<9>(a, slots, g, blocks, s);
        default: return rmulti::launch_k<10>(a, slots, g, blocks, s);
    }
}

}  // namespace tec
