// engine.cpp -- libtapeec.so: the C ABI (include/tape_ec.h) over the gfx950 Clay engines.
//
// Host side of the drop-in for lib/slicer: Slicer striping/padding/rotation/metadata
// (slicer.rs, adaptive.rs, metadata.rs), repair planning (repair.rs), descriptor building and
// launch orchestration.  All GF arithmetic and hashing runs in the HIP kernels (encode_dma.hip,
// encode_stage.hip, decode_stage.hip + the per-pattern kernels of dec_rtc.cpp, repair_fold.hip,
// repair_stage.hip, gpe.hip, commit.hip, rs16.hip); there is no CPU compute fallback -- without a
// device the compute calls fail with TE_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <deque>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <mutex>
#include <vector>
#include <algorithm>
#include <functional>
#include <thread>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include "../../include/tape_ec.h"
#include "kernels.hpp"
#include "sha256.hpp"
#include <array>
#include "clay_host.hpp"
#include "rs16.hpp"
#include "host_hash.hpp"
#include "copy_pool.hpp"
#include "win_plan.hpp"
#include "dec_class.hpp"
#include "dec_plan.hpp"
#include "rec_multi_plan.hpp"

using namespace tec;

namespace {

constexpr size_t kStripeSizes[3] = {100000, 1000000, 10000000};  // adaptive.rs:15-19

thread_local char g_last_error[256] = "";
// TEC_ENCODE_KERNEL=stage selects the previous 1 MB-stripe encode kernel (measurement only)
const bool g_no_dma_encode = [] {
    const char *e = tec_knob("TEC_ENCODE_KERNEL");
    return e && strcmp(e, "stage") == 0;
}();

// Small per-call encodes (te_slicer_encode / te_clay_encode): a call of at most TEC_ENC_SMALL 1 MB
// stripes may run the staged kernel with one wave per workgroup (six workgroups per stripe).
// Measured slower (r05 trace of --mode percall: 438 us per 4 MiB object against 296 us for the
// LDS-DMA kernel -- a lone stripe is bound by the 100-plane chain's latency, not its work per
// step), so it is off (0); measurement only.
// Per-call encodes of at most this many 1 MB stripes run the LDS-DMA kernel split in two launches:
// the seven level-1 plane rows of a stripe on seven workgroups, then the level-2 chain on one --
// a lone stripe is latency-bound by its 100-plane chain (296 us per 4 MiB object).  Measurement
// option TEC_DEBUG_KNOBS=1 TEC_ENC_SPLIT=n (0: never).
const uint32_t g_enc_split = [] {
    const char *e = tec_knob("TEC_ENC_SPLIT");
    return e ? (uint32_t)atoi(e) : 512u;
}();
// Measurement option TEC_DEBUG_KNOBS=1 TEC_ENC_SPLIT_BATCH=1: every call split that way (the seven
// level-1 workgroups of a stripe run side by side on one XCD, so a row one of them reads as its
// own and another as a partner is read twice at about the same time).
const uint32_t g_enc_split_batch = [] {  // 0 off, else the level-1 rows per workgroup (1..7)
    const char *e = tec_knob("TEC_ENC_SPLIT_BATCH");
    const int v = e ? atoi(e) : 0;
    return (uint32_t)(v < 0 ? 0 : v > 7 ? 7 : v);
}();
const uint32_t g_enc_small = [] {
    const char *e = tec_knob("TEC_ENC_SMALL");
    return e ? (uint32_t)atoi(e) : 0u;
}();

// TEC_REPAIR_KERNEL=stage keeps the folded repair kernel off (measurement / cross-check only)
const bool g_no_fold_repair = [] {
    const char *e = tec_knob("TEC_REPAIR_KERNEL");
    return e && strcmp(e, "stage") == 0;
}();

int hip_status(hipError_t e) {
    if (e == hipSuccess) return TE_OK;
    snprintf(g_last_error, sizeof(g_last_error), "%s (%d)", hipGetErrorString(e), (int)e);
    if (e == hipErrorOutOfMemory) return TE_ERR_OUT_OF_MEMORY;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return TE_ERR_NO_DEVICE;
    return TE_ERR_HIP;
}

#define TE_HIP(expr)                              \
    do {                                          \
        hipError_t e_ = (expr);                   \
        if (e_ != hipSuccess) return hip_status(e_); \
    } while (0)

// Wait for the work queued on s so far by sleeping on a blocking-sync event, not spinning in
// hipStreamSynchronize: a caller that waits while the host hashing pool runs must not take one of
// the process's CPUs (the GPU's host share is a 16-CPU quota on the pool this runs on).
int sync_sleep(hipStream_t s) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess)
        return hip_status(hipStreamSynchronize(s));
    hipError_t r = hipEventRecord(e, s);
    if (r == hipSuccess) r = hipEventSynchronize(e);
    (void)hipEventDestroy(e);
    return hip_status(r);
}

int g_device_count = -1;
std::mutex g_dev_mu;

int device_count() {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (g_device_count < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_device_count = n;
    }
    return g_device_count;
}

// Runs the enclosed calls on a handle's device, whatever the calling thread's current device
// is, and restores the thread's device afterwards.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Measurement option (TEC_DEBUG_KNOBS=1 TEC_VMM_BUFS=1): buffers of >= 64 MiB through the virtual
// memory API -- physical memory created at the recommended granularity and mapped into a fresh
// address range -- instead of hipMalloc (to test whether a slowdown follows the page placement of
// re-allocated buffers, DESIGN §4.4's open item).
static bool vmm_bufs() {
    static const bool v = [] {
        const char *s = tec_knob("TEC_VMM_BUFS");
        return s && s[0] == '1';
    }();
    return v;
}

// The last launches that read a shared device resource, one event per stream: each
// call re-records its own stream's event, so a clear / free waits for the readers on EVERY stream
// that used the resource, not only the most recent one.  Bounded: past kMax streams the events are
// drained on the host and their slots reused (a process rarely reads one handle from > 16 streams).
struct ReaderEvents {
    struct E {
        hipStream_t s = nullptr;
        hipEvent_t ev = nullptr;
        bool pending = false;
    };
    static constexpr size_t kMax = 16;
    std::vector<E> v;
    bool any() const {
        for (const E &e : v)
            if (e.pending) return true;
        return false;
    }
    // after the launches on `s` that read the resource
    hipError_t record(hipStream_t s) {
        E *slot = nullptr;
        for (E &e : v)
            if (e.s == s) slot = &e;
        if (!slot) {
            if (v.size() >= kMax) {
                if (hipError_t r = sync(); r != hipSuccess) return r;
                slot = &v[0];
                slot->s = s;
            } else {
                E e;
                e.s = s;
                if (hipError_t r = hipEventCreateWithFlags(&e.ev, hipEventDisableTiming); r != hipSuccess) return r;
                v.push_back(e);
                slot = &v.back();
            }
        }
        hipError_t r = hipEventRecord(slot->ev, s);
        if (r == hipSuccess) slot->pending = true;
        return r;
    }
    // stream `s` waits (on the device) for every reader on the other streams
    hipError_t wait(hipStream_t s) const {
        for (const E &e : v)
            if (e.pending && e.s != s)
                if (hipError_t r = hipStreamWaitEvent(s, e.ev, 0); r != hipSuccess) return r;
        return hipSuccess;
    }
    // the host waits for every reader (before the resource is freed)
    hipError_t sync() {
        for (E &e : v)
            if (e.pending) {
                if (hipError_t r = hipEventSynchronize(e.ev); r != hipSuccess) return r;
                e.pending = false;
            }
        return hipSuccess;
    }
    void destroy() {
        for (E &e : v)
            if (e.ev) (void)hipEventDestroy(e.ev);
        v.clear();
    }
};

// One copy pool per device, so per-call copies of handles on different GPUs do not queue behind
// one another.  Three workers plus the calling thread.
static tec::CopyPool &copy_pool(int device) {
    static std::mutex mu;
    static tec::CopyPool *pools[65] = {};
    const int slot = device < 0 || device >= 64 ? 64 : device;
    std::lock_guard<std::mutex> g(mu);
    if (!pools[slot]) pools[slot] = new tec::CopyPool(std::max(0, std::min(3, hh::default_threads() - 1)));
    return *pools[slot];
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipMemGenericAllocationHandle_t vh{};  // VMM allocation (vmm_bufs), else hipMalloc
    bool vmm = false;
    hipError_t free_() {
        if (!p) return hipSuccess;
        hipError_t e = hipSuccess;
        if (vmm) {
            (void)hipDeviceSynchronize();
            e = hipMemUnmap(p, cap);
            if (e == hipSuccess) e = hipMemRelease(vh);
            if (e == hipSuccess) e = hipMemAddressFree(p, cap);
        } else {
            e = hipFree(p);
        }
        p = nullptr;
        cap = 0;
        vmm = false;
        return e;
    }
    hipError_t alloc_vmm(size_t n) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev;
        size_t g = 0;
        if ((e = hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityRecommended)) != hipSuccess) return e;
        if (g == 0) g = (size_t)2 << 20;
        const size_t sz = (n + g - 1) / g * g;
        void *va = nullptr;
        if ((e = hipMemAddressReserve(&va, sz, g, nullptr, 0)) != hipSuccess) return e;
        hipMemGenericAllocationHandle_t h{};
        if ((e = hipMemCreate(&h, sz, &prop, 0)) != hipSuccess) {
            (void)hipMemAddressFree(va, sz);
            return e;
        }
        if ((e = hipMemMap(va, sz, 0, h, 0)) != hipSuccess) {
            (void)hipMemRelease(h);
            (void)hipMemAddressFree(va, sz);
            return e;
        }
        hipMemAccessDesc ad{};
        ad.location = prop.location;
        ad.flags = hipMemAccessFlagsProtReadWrite;
        if ((e = hipMemSetAccess(va, sz, &ad, 1)) != hipSuccess) {
            (void)hipMemUnmap(va, sz);
            (void)hipMemRelease(h);
            (void)hipMemAddressFree(va, sz);
            return e;
        }
        p = va;
        cap = sz;
        vh = h;
        vmm = true;
        return hipSuccess;
    }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) {
            hipError_t e = free_();
            if (e != hipSuccess) return e;
        }
        if (vmm_bufs() && n >= ((size_t)64 << 20)) return alloc_vmm(n);
        // large buffers in whole 2 MiB units (the device's large-page size)
        size_t want = std::max<size_t>(n, 4096);
        const size_t unit = want >= ((size_t)64 << 20) ? ((size_t)2 << 20) : 4096;
        want = (want + unit - 1) & ~(unit - 1);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    void release() { (void)free_(); }
};

struct HostBuf {  // pinned staging (descriptor uploads, the per-call entry points' host side)
    // hipHostMalloc memory: under unified addressing the host pointer it returns is also the
    // pointer kernels use (hipHostGetDevicePointer gives it back unchanged), which the zero-copy
    // per-call paths rely on when they hand u8() to a kernel.  Memory a caller page-locked itself
    // (hipHostRegister) has no such promise: host_device_ptr asks for its device address.
    void *p = nullptr;
    size_t cap = 0;
    uint8_t *u8() const { return static_cast<uint8_t *>(p); }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n, 4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// A descriptor arena: host image assembled per call, uploaded (only if changed) to a device
// mirror on the caller's stream.  An event guards the pinned staging against reuse while a
// previous upload may still be pending.
struct Arena {
    std::vector<uint8_t> img, last;
    HostBuf stage;
    DevBuf dev;
    DevBuf scratch;  // kernel workspace (encode level-2 parking), ordered like `dev`
    hipEvent_t ev = nullptr;
    bool ev_pending = false;
    hipStream_t last_stream = nullptr;
    hipEvent_t done = nullptr;  // recorded after the launches that read `dev`
    bool done_pending = false;

    size_t put(const void *src, size_t bytes, size_t align = 16) {
        size_t off = (img.size() + align - 1) & ~(align - 1);
        img.resize(off + bytes);
        if (bytes) memcpy(img.data() + off, src, bytes);
        return off;
    }
    int upload(hipStream_t s) {
        if (!ev) TE_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (!done) TE_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        if (img == last && dev.p && dev.cap >= img.size()) return TE_OK;
        // device mirror may still be read by launches on another stream
        if (done_pending && last_stream != s) TE_HIP(hipStreamWaitEvent(s, done, 0));
        if (ev_pending) TE_HIP(hipEventSynchronize(ev));
        ev_pending = false;
        if (img.size() > dev.cap) {
            // old mirror may still be referenced by queued kernels: drain before freeing
            if (done_pending) TE_HIP(hipEventSynchronize(done));
            TE_HIP(dev.ensure(img.size()));
        }
        TE_HIP(stage.ensure(img.size()));
        memcpy(stage.p, img.data(), img.size());
        TE_HIP(hipMemcpyAsync(dev.p, stage.p, img.size(), hipMemcpyHostToDevice, s));
        TE_HIP(hipEventRecord(ev, s));
        ev_pending = true;
        last = img;
        return TE_OK;
    }
    int mark_done(hipStream_t s) {
        TE_HIP(hipEventRecord(done, s));
        done_pending = true;
        last_stream = s;
        return TE_OK;
    }
    template <class T> const T *at(size_t off) const { return reinterpret_cast<const T *>(dev.as<uint8_t>() + off); }
    // workspace of at least `bytes` for launches about to be enqueued on stream s
    int workspace(size_t bytes, hipStream_t s, uint8_t **out) {
        if (bytes > scratch.cap) {
            if (done_pending) TE_HIP(hipEventSynchronize(done));  // queued kernels may still use it
            TE_HIP(scratch.ensure(bytes));
        } else if (done_pending && last_stream != s) {
            TE_HIP(hipStreamWaitEvent(s, done, 0));
        }
        *out = scratch.as<uint8_t>();
        return TE_OK;
    }
    void release() {
        dev.release();
        scratch.release();
        stage.release();
        if (ev) (void)hipEventDestroy(ev);
        if (done) (void)hipEventDestroy(done);
        ev = done = nullptr;
    }
};

// Kernel timing (te_kernel_timing): event pairs around each batch call's kernel launches.
struct KTimeState {
    std::mutex mu;
    bool enabled = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs;
} g_ktime;

struct KTimer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    explicit KTimer(hipStream_t st) : s(st) {
        std::lock_guard<std::mutex> g(g_ktime.mu);
        if (!g_ktime.enabled) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, s) != hipSuccess) {
            a = b = nullptr;
        }
    }
    ~KTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    void stop() {
        if (!a) return;
        std::lock_guard<std::mutex> g(g_ktime.mu);
        if (hipEventRecord(b, s) == hipSuccess) g_ktime.pairs.push_back({a, b});
        a = b = nullptr;
    }
};

void put_u64(uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
uint64_t get_u64(const uint8_t *p) {
    uint64_t v = 0;
    for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

bool valid_stripe(uint64_t s) { return s == kStripeSizes[0] || s == kStripeSizes[1] || s == kStripeSizes[2]; }

// the host read and rebuild pipelines' per-handle window buffers (te_decode_batch_host,
// te_repair_batch_host / te_recover_batch_host, below)
struct WinPipe;
void win_pipe_free(WinPipe *p);

}  // namespace

// ------------------------------------------------------------------------------------------
struct te_clay {
    ClayHost h;
    bool fast_encode = false;
    std::mutex mu;
    int device = 0;                // every allocation and launch of this handle runs on it
    hipStream_t stream = nullptr;  // for the synchronous host-buffer entry points
    Arena enc, dec, rep, rec, ver;
    // the verified read calls' workspace (expected hashes, digests, masks) and its page-locked host
    // side: idle between calls, which wait for their masks before they return
    DevBuf ver_buf;
    HostBuf ver_host;
    DevBuf io_in, io_out;          // staging for host-buffer entry points
    HostBuf hio_in, hio_out;       // their page-locked host side (te_slicer_repair's gather / scatter)
    // te_recover_batch_device workspaces (decoded objects, re-encoded slices); `rec_done` is
    // recorded after the last launch that reads them, on `rec_stream`
    DevBuf rec_blob, rec_slices;
    hipEvent_t rec_done = nullptr;
    bool rec_pending = false;
    hipStream_t rec_stream = nullptr;
    // te_encode_batch_host pipeline: kPipe slots, each with its own stream, descriptor arena
    // and device window buffers, so window w+1's H2D overlaps window w's kernel and D2H.
    static constexpr int kPipe = 3;  // a fourth slot measured slower
    // Compiled decode patterns (layered pattern + staged plane program), by padded erasure mask:
    // building them is host work per distinct pattern (matrix inversion, program, colouring).
    struct DecCache {
        GpePattern P;
        std::vector<uint16_t> planes;  // P's plane list (P.planes_off is set per call)
        bool staged = false;           // a plane program exists for the staged kernel
        DecProgHdr H{};
        std::vector<DecStepP> steps;   // packed program + 2 blank steps
        int orient = 0;                // the program's row orientation (ClayHost::dec_prog)
    };
    // Device-resident store of staged decode patterns (GpePattern, DecProgHdr, program) by
    // cache key: a pattern is uploaded once and serves later calls in place.  Random survivor
    // sets make nearly every stripe a pattern of its own, and re-uploading ~26 KB per stripe per
    // call cost more host time than the kernel takes.  Slots are handed out in order; a full store
    // is emptied after its last reader (`used`) has finished.
    // The store grows by doubling from kMin slots (each slot ~26 KB of device memory: 102 steps
    // of DecStepP plus its GpePattern and header; kCap slots = ~430 MB; te_clay_set_decode_store_cap
    // lowers the cap) once its last reader is done.  New slots are filled with stream-ordered copies from the call's descriptor upload
    // (decode_enqueue), never with a host-blocking copy; a call on another stream waits for the
    // last fill (`written`) before reading.
    struct DecStore {
        // 16,384: a batch of 2,048 x 4 MiB reads with random survivor sets has ~10,000 distinct
        // stripe patterns; at 8,192 every such call overflowed to per-call uploads and recompiles
        static constexpr uint32_t kCap = 16384, kMin = 256;
        uint32_t max_cap = kCap;
        static constexpr uint32_t kSteps = kRepQ * kRepQ + 2;  // 100 planes + 2 blank steps
        DevBuf pats, hdrs, steps, soff;
        uint32_t cap = 0;
        std::unordered_map<uint64_t, uint32_t> slot;
        uint32_t n = 0;
        ReaderEvents readers;             // the last launches that read the store, per stream
        hipEvent_t written = nullptr;
        bool written_pending = false;
        hipStream_t written_stream = nullptr;
        uint64_t clears = 0, grows = 0, arena_calls = 0;  // te_clay_decode_store_stats
    } dstore;
    // per-pattern decode kernels built at run time (dec_rtc.cpp); created on first decode
    DecJit *jit = nullptr;
    int jit_mode = -1;                 // te_clay_set_decode_jit; -1 = the environment's default
    uint64_t jit_min = 0;
    std::unordered_map<uint64_t, DecCache> dec_cache;
    // Compiled repair patterns by (lost shard, helper shards...): the layered pattern with its
    // plane lists, the staged kernel's program, and the folded kernel index (-1: none).  Host work
    // per distinct helper set (matrix inversion, programs) is done once per handle.
    struct RepCache {
        RepPattern P;
        std::vector<uint16_t> pool, pind;
        RepProg prog{};
        bool prog_ok = false;
        int fold = -1;
    };
    struct RepKey {  // (lost shard, helper shard set): rep_pattern depends on the set only
        uint64_t helpers;
        uint32_t lost;
        bool operator==(const RepKey &o) const { return helpers == o.helpers && lost == o.lost; }
    };
    struct RepKeyHash {
        size_t operator()(const RepKey &k) const {
            return (size_t)((k.helpers ^ ((uint64_t)k.lost << 56)) * 0x9E3779B97F4A7C15ull >> 7);
        }
    };
    std::unordered_map<RepKey, RepCache, RepKeyHash> rep_cache;  // node-based: entries stay put
    struct Slot {
        hipStream_t s = nullptr;
        Arena arena;
        DevBuf in, out;
        DevBuf commit;  // te_encode_commit_batch_host: the window's leaf hashes, roots, proofs
    } pipe[kPipe];
    // encode + commit pipeline streams on disjoint CU sets (commit_streams): hashing on a few
    // CUs, slot streams (copies, encodes) on the rest
    hipStream_t cm_ss[2] = {}, cm_hs = nullptr;
    bool cm_tried = false;
    // decode class kernels run side by side (decode_enqueue): side streams forked from and joined
    // back into the call's stream with events, so their work is ordered like the call's
    static constexpr int kClsSide = 7;
    hipStream_t cls_s[kClsSide] = {};
    hipEvent_t cls_fork = nullptr, cls_join[kClsSide] = {};
    // the decode_enqueue launches of the last decode / recover call (te_clay_decode_launch_stats):
    // zeroed when the call starts its device work, summed over its decode_enqueue passes
    te_decode_launch_stats dls{};
    // the last ranged call's stripe outcomes (te_clay_range_launch_stats), zeroed by its entry point
    te_range_launch_stats rgs{};
    // te_clay_set_range_chunk_path: a ranged read's lone erased data chunk on the windowed recover
    // class kernels (off by default), and the last ranged call's share of it
    int range_chunk = 0;
    te_range_chunk_stats rcs{};
    // the same for the encode_enqueue / repair_enqueue launches of the last encode / repair call
    te_encode_launch_stats els{};
    te_repair_launch_stats rls{};
    // te_decode_batch_host / te_decode_verified_batch_host: their window buffers (kept between
    // calls, as the encode pipeline's are) and the last call's te_read_launch_stats
    WinPipe *rpipe = nullptr;
    te_read_launch_stats rds{};
    // te_repair_batch_host / te_recover_batch_host: the same
    WinPipe *rbpipe = nullptr;
    te_rebuild_launch_stats rbs{};
    // te_snapshot_*: the decode's descriptor arena (payload offsets, segment capacities), its
    // page-locked header read-back, the host forms' device buffers (kept between calls) and the last
    // call's te_snapshot_stats
    Arena snap;
    HostBuf snap_host;
    DevBuf snap_in, snap_work, snap_out, snap_commit;
    te_snapshot_stats sns{};
    // the last data-verify call (te_verify_data_batch_device / _host, te_slicer_verify_data)
    te_verify_data_stats vds{};
    // te_recover_multi_batch_device: the sub-masks of a (padded erasure mask, lost nodes) pair
    // (rec_multi_split) and the compiled program of each (rec_multi_key), host work done once per
    // handle; the programs live in `dstore` beside the decode's; the last call's stats
    std::unordered_map<uint64_t, std::vector<uint64_t>> rm_split;
    std::unordered_map<uint64_t, DecCache> rm_cache;
    te_recover_multi_stats rms{};
};

// Drain and free everything a handle holds on its device (on that device).
static void release_device_state(te_clay *c) {
    if (device_count() <= 0) return;
    DeviceGuard dg(c->device);
    if (dg.err != hipSuccess) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->rec_done) (void)hipEventSynchronize(c->rec_done);
    for (auto &sl : c->pipe)
        if (sl.s) (void)hipStreamSynchronize(sl.s);
    for (hipStream_t &cs : c->cls_s)
        if (cs) (void)hipStreamSynchronize(cs), (void)hipStreamDestroy(cs), cs = nullptr;
    if (c->cls_fork) (void)hipEventDestroy(c->cls_fork), c->cls_fork = nullptr;
    for (hipEvent_t &pe : c->cls_join)
        if (pe) (void)hipEventDestroy(pe), pe = nullptr;
    win_pipe_free(c->rpipe);
    c->rpipe = nullptr;
    win_pipe_free(c->rbpipe);
    c->rbpipe = nullptr;
    c->enc.release();
    c->dec.release();
    c->rep.release();
    c->rec.release();
    c->ver.release();
    c->ver_buf.release();
    c->ver_host.release();
    c->io_in.release();
    c->io_out.release();
    c->hio_in.release();
    c->hio_out.release();
    c->rec_blob.release();
    c->rec_slices.release();
    c->snap.release();
    c->snap_host.release();
    for (DevBuf *b : {&c->snap_in, &c->snap_work, &c->snap_out, &c->snap_commit}) b->release();
    for (DevBuf *b : {&c->dstore.pats, &c->dstore.hdrs, &c->dstore.steps, &c->dstore.soff}) b->release();
    c->dstore.slot.clear();
    c->dstore.n = 0;
    c->dstore.readers.destroy();
    if (c->dstore.written) (void)hipEventDestroy(c->dstore.written);
    c->dstore.written = nullptr;
    c->dstore.written_pending = false;
    c->dstore.written_stream = nullptr;
    c->dstore.cap = 0;
    if (c->rec_done) (void)hipEventDestroy(c->rec_done);
    c->rec_done = nullptr;
    dec_jit_free(c->jit);  // joins compiles in flight; every stream is drained above
    c->jit = nullptr;
    c->rec_pending = false;
    if (c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = nullptr;
    for (hipStream_t *ps : {&c->cm_ss[0], &c->cm_ss[1], &c->cm_hs}) {
        if (*ps) (void)hipStreamSynchronize(*ps), (void)hipStreamDestroy(*ps);
        *ps = nullptr;
    }
    c->cm_tried = false;
    for (auto &sl : c->pipe) {
        sl.arena.release();
        sl.in.release();
        sl.out.release();
        sl.commit.release();
        if (sl.s) (void)hipStreamDestroy(sl.s);
        sl.s = nullptr;
    }
}

struct te_repair_plan {
    uint32_t lost = 0, ns = 0, d = 0, beta = 0, n = 0;
    uint64_t cs = 0, sc = 0;
    std::vector<uint32_t> lost_shard;   // [ns]
    std::vector<uint32_t> helper_slice; // [ns*d]
    std::vector<uint32_t> helper_shard; // [ns*d]
    std::vector<uint32_t> sub_chunks;   // [ns*d*beta]
};

namespace tec {
hipError_t ensure_dyn_lds(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> done;  // (device, kernel) -> limit set
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    size_t &cur = done[{dev, fn}];
    if (bytes <= cur) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}
}  // namespace tec

extern "C" {

const char *te_strerror(int s) {
    switch (s) {
        case TE_OK: return "ok";
        case TE_ERR_TOO_MUCH_DATA: return "too much data to encode in a single stripe/coder configuration";
        case TE_ERR_EMPTY_INPUT: return "empty input data";
        case TE_ERR_NOT_ENOUGH_SLICES: return "not enough slices to reconstruct (need at least DATA_SLICES)";
        case TE_ERR_BAD_ENCODING: return "invalid padding in recovered data";
        case TE_ERR_INVALID_LAYOUT: return "invalid layout or inconsistent slices";
        case TE_ERR_NOT_ENOUGH_HELPERS: return "not enough helpers";
        case TE_ERR_INVALID_SLICE: return "invalid slice index";
        case TE_ERR_CLAY: return "clay error";
        case TE_ERR_MISSING_HELPER: return "missing helper data";
        case TE_ERR_MERKLE_TREE_FULL: return "merkle tree full";
        case TE_ERR_MERKLE_INVALID_PROOF: return "invalid merkle proof";
        case TE_ERR_MERKLE_INVALID_INDEX: return "invalid merkle leaf index";
        case TE_ERR_MERKLE_PROOF_LENGTH: return "merkle proof length differs from the tree height";
        case TE_ERR_INVALID_ARG: return "invalid argument";
        case TE_ERR_NO_DEVICE: return "no gfx950 HIP device available (libtapeec has no CPU fallback)";
        case TE_ERR_HIP: return "HIP runtime error";
        case TE_ERR_UNSUPPORTED: return "profile/layout not supported by the GPU engine";
        case TE_ERR_OUT_OF_MEMORY: return "out of device memory";
        case TE_ERR_BUFFER_TOO_SMALL: return "output buffer too small";
    }
    return "unknown status";
}

int te_device_count(void) { return device_count(); }

const char *te_last_error_detail(void) { return g_last_error; }


int te_set_device(int device) {
    if (device < 0 || device >= device_count()) return TE_ERR_NO_DEVICE;
    TE_HIP(hipSetDevice(device));
    return TE_OK;
}

const char *te_version(void) { return "tapeec 0.1.0 (gfx950)"; }

int te_kernel_timing(int enable) {
    std::lock_guard<std::mutex> g(g_ktime.mu);
    g_ktime.enabled = enable != 0;
    return TE_OK;
}

int te_kernel_time_ms(double *total_ms, uint32_t *count) {
    if (!total_ms) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(g_ktime.mu);
    double tot = 0;
    for (auto &p : g_ktime.pairs) {
        TE_HIP(hipEventSynchronize(p.second));
        float ms = 0;
        TE_HIP(hipEventElapsedTime(&ms, p.first, p.second));
        tot += ms;
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    if (count) *count = (uint32_t)g_ktime.pairs.size();
    g_ktime.pairs.clear();
    *total_ms = tot;
    return TE_OK;
}

// ------------------------------------------------------------------------------------------
int te_clay_new(uint32_t n, uint32_t k, uint32_t d, te_clay **out) {
    if (!out) return TE_ERR_INVALID_ARG;
    *out = nullptr;
    if (n > TE_GROUP_SIZE) return TE_ERR_INVALID_ARG;
    te_clay *c = new (std::nothrow) te_clay();
    if (!c) return TE_ERR_OUT_OF_MEMORY;
    const int r = c->h.init((int)n, (int)k, (int)d);
    if (r) {
        delete c;
        return r == -1 ? TE_ERR_INVALID_ARG : TE_ERR_UNSUPPORTED;
    }
    c->fast_encode = encode_rows_supported((int)n, (int)k, (int)d);
    if (device_count() > 0) {  // bound to the creating thread's current device (te_clay_bind_device)
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess) c->device = dev;
    }
    *out = c;
    return TE_OK;
}

int te_clay_bind_device(te_clay *c, int device) {
    if (!c) return TE_ERR_INVALID_ARG;
    if (device < 0 || device >= device_count()) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    if (device == c->device) return TE_OK;
    release_device_state(c);  // buffers and streams live on the old device
    c->device = device;
    return TE_OK;
}

int te_clay_device(const te_clay *c) { return c ? c->device : -1; }

int te_clay_set_decode_jit(te_clay *c, int mode, uint64_t min_stripes) {
    if (!c || mode < 0 || mode > 2) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->jit_mode = mode;
    c->jit_min = min_stripes;
    if (c->jit) dec_jit_set(c->jit, mode, min_stripes);
    return TE_OK;
}

int te_clay_set_decode_store_cap(te_clay *c, uint32_t max_patterns) {
    if (!c || max_patterns < 1 || max_patterns > te_clay::DecStore::kCap) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    te_clay::DecStore &S = c->dstore;
    if (S.cap > max_patterns) {  // shrink: the store is re-allocated at the next decode
        (void)S.readers.sync();
        for (DevBuf *b : {&S.pats, &S.hdrs, &S.steps, &S.soff}) b->release();
        S.cap = 0;
        S.slot.clear();
        S.n = 0;
    }
    S.max_cap = max_patterns;
    return TE_OK;
}

int te_clay_decode_store_stats(te_clay *c, uint32_t *capacity, uint32_t *used, uint64_t *clears, uint64_t *grows,
                               uint64_t *arena_calls) {
    if (!c) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (capacity) *capacity = c->dstore.cap;
    if (used) *used = c->dstore.n;
    if (clears) *clears = c->dstore.clears;
    if (grows) *grows = c->dstore.grows;
    if (arena_calls) *arena_calls = c->dstore.arena_calls;
    return TE_OK;
}

int te_clay_decode_launch_stats(te_clay *c, te_decode_launch_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->dls;
    return TE_OK;
}

int te_clay_encode_launch_stats(te_clay *c, te_encode_launch_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->els;
    return TE_OK;
}

int te_clay_verify_data_launch_stats(te_clay *c, te_verify_data_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->vds;
    return TE_OK;
}

int te_clay_recover_multi_launch_stats(te_clay *c, te_recover_multi_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->rms;
    return TE_OK;
}

int te_clay_repair_launch_stats(te_clay *c, te_repair_launch_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->rls;
    return TE_OK;
}

int te_clay_decode_jit_status(te_clay *c, uint32_t timeout_ms, uint32_t *ready, uint32_t *pending, uint32_t *failed) {
    if (!c) return TE_ERR_INVALID_ARG;
    DecJit *j;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        j = c->jit;
        if (j) dec_jit_hold(j);  // dec_jit_free (te_clay_free / bind_device, under c->mu) waits for it
    }
    uint32_t r = 0, p = 0, f = 0;
    if (j) {
        dec_jit_counts(j, timeout_ms, &r, &p, &f);
        dec_jit_unhold(j);
    }
    if (ready) *ready = r;
    if (pending) *pending = p;
    if (failed) *failed = f;
    return TE_OK;
}

int te_clay_from_params(uint64_t p, te_clay **out) {
    return te_clay_new((uint32_t)(p & 0xFF), (uint32_t)((p >> 8) & 0xFF), (uint32_t)((p >> 16) & 0xFF), out);
}

void te_clay_free(te_clay *c) {
    if (!c) return;
    release_device_state(c);
    delete c;
}

int te_clay_get_info(const te_clay *c, te_clay_info *o) {
    if (!c || !o) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    o->n = h.n; o->k = h.k; o->m = h.m; o->d = h.d;
    o->q = h.q; o->t = h.t; o->nu = h.nu; o->alpha = h.alpha; o->beta = h.beta;
    return TE_OK;
}

size_t te_clay_chunk_size_for(const te_clay *c, size_t len) { return c ? c->h.chunk_size_for(len) : 0; }

size_t te_clay_track_chunk_size(const te_clay *c, size_t stripe, size_t blob_len) {
    return c ? c->h.chunk_size_for(std::min(stripe, blob_len)) : 0;
}

// ------------------------------------------------------------------------------------------
size_t te_pick_stripe_size(size_t blob_len) {
    if (blob_len <= 1000000) return kStripeSizes[0];
    if (blob_len <= 100000000) return kStripeSizes[1];
    return kStripeSizes[2];
}

size_t te_num_stripes(size_t blob_len, size_t stripe) {
    if (blob_len == 0) return 1;
    if (stripe == 0) return 0;
    return (blob_len + stripe - 1) / stripe;
}

uint32_t te_shard_to_slice(int rotated, uint32_t n, uint32_t stripe, uint32_t shard) {
    return shard_to_slice(rotated, n, stripe, shard);
}

uint32_t te_slice_to_shard(int rotated, uint32_t n, uint32_t stripe, uint32_t slice) {
    return slice_to_shard(rotated, n, stripe, slice);
}

void te_slice_metadata_to_bytes(const te_slice_metadata *m, uint8_t out[TE_META_SIZE]) {
    put_u64(out, m->version);
    put_u64(out + 8, m->blob_len);
    put_u64(out + 16, m->stripe_size);
    put_u64(out + 24, m->encoding);
    put_u64(out + 32, m->params);
    put_u64(out + 40, m->chunk_index);
}

int te_slice_metadata_from_slice(const uint8_t *slice, size_t len, te_slice_metadata *out) {
    if (!slice || !out || len < TE_META_SIZE) return TE_ERR_INVALID_LAYOUT;
    const uint8_t *p = slice + len - TE_META_SIZE;
    out->version = get_u64(p);
    out->blob_len = get_u64(p + 8);
    out->stripe_size = get_u64(p + 16);
    out->encoding = get_u64(p + 24);
    out->params = get_u64(p + 32);
    out->chunk_index = get_u64(p + 40);
    if (!valid_stripe(out->stripe_size)) return TE_ERR_INVALID_LAYOUT;
    return TE_OK;
}

int te_slicer_geometry(const te_clay *c, size_t blob_len, te_geometry *g) {
    if (!c || !g) return TE_ERR_INVALID_ARG;
    const size_t S = te_pick_stripe_size(blob_len);
    const size_t ns = te_num_stripes(blob_len, S);
    const size_t eff = blob_len == 0 ? S : std::min(blob_len, S);
    const size_t cs = c->h.chunk_size_for(eff);
    g->stripe_size = S;
    g->num_stripes = ns;
    g->chunk_size = cs;
    g->sub_chunk_size = cs / (size_t)c->h.alpha;
    g->slice_len = ns * cs + TE_META_SIZE;
    return TE_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Encode
// ------------------------------------------------------------------------------------------
namespace {

struct GeomKey {
    uint64_t cs, slice_len;
    bool masked;  // stripe data end not dword aligned -> masked kernel variant
    bool odd;     // stripe data at an odd address: the fast kernels load 4 bytes at 2-aligned
                  // addresses only (an odd-address dword near the data end reads short through
                  // the range check), so such stripes take the generic byte-exact kernel
    bool operator<(const GeomKey &o) const {
        if (cs != o.cs) return cs < o.cs;
        if (slice_len != o.slice_len) return slice_len < o.slice_len;
        if (odd != o.odd) return odd < o.odd;
        return masked < o.masked;
    }
};

int ensure_stream(te_clay *c) {
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    if (!c->stream) TE_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    return TE_OK;
}

// Enqueue the encode of a batch.  raw = ClayCoder::encode semantics (no slicing/rotation/meta,
// slices are the n chunks of one padded input).
// keep(obj, stripe): which stripes to encode and which of their chunks to write -- a mask of
// internal nodes, 0 = skip the stripe (all stripes, all chunks when empty).  With a selector no
// metadata suffix is written (te_recover_batch_device writes its own).  The mask is a store
// filter of the LDS-DMA kernel (it must include the column-0 parity nodes, which that kernel
// reads back); the other kernels write every chunk.
using StripeSel = std::function<uint32_t(size_t, size_t)>;

int encode_enqueue(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_data, const te_object *objs,
                   size_t nobj, uint8_t *d_out, hipStream_t s, bool raw, Arena *arena = nullptr,
                   const StripeSel &keep = StripeSel(), bool per_call = false) {
    const ClayHost &h = c->h;
    const int n = h.n;
    const int rotated = cfg ? cfg->rotated : 0;
    std::map<GeomKey, std::vector<EncJob>> groups;
    std::vector<MetaJob> metas;

    for (size_t i = 0; i < nobj; i++) {
        const te_object &o = objs[i];
        size_t S, ns, cs, slice_len;
        if (raw) {
            if (o.blob_len == 0) return TE_ERR_EMPTY_INPUT;
            cs = h.chunk_size_for(o.blob_len);
            S = cs * h.k;
            ns = 1;
            slice_len = cs;
        } else {
            te_geometry g;
            te_slicer_geometry(c, o.blob_len, &g);
            S = g.stripe_size; ns = g.num_stripes; cs = g.chunk_size; slice_len = g.slice_len;
        }
        if (cs % (size_t)h.alpha || slice_len > 0xffffffffull || cs > 0xffffffffull) return TE_ERR_TOO_MUCH_DATA;
        for (size_t st = 0; st < ns; st++) {
            const uint32_t store = keep ? keep(i, st) : ~0u;
            if (!store) continue;
            EncJob j{};
            j.store_mask = store;
            const uint64_t start = (uint64_t)st * S;
            j.src = d_data + o.data_off + start;
            j.src_len = o.blob_len == 0 ? 0 : std::min<uint64_t>(S, o.blob_len - start);
            j.dst = d_out + o.out_off + st * cs;
            j.rot = rotated ? (uint32_t)((st * TE_ROTATION_STEP) % n) : 0u;
            j.dst_skew = (uint32_t)(st * cs);
            const bool masked = ((reinterpret_cast<uintptr_t>(j.src) & 3u) + j.src_len) % 4 != 0;
            const bool odd = (reinterpret_cast<uintptr_t>(j.src) & 1u) != 0;
            groups[GeomKey{cs, slice_len, masked, odd}].push_back(j);
        }
        if (!raw && !keep) {
            MetaJob m{};
            m.dst = d_out + o.out_off + ns * cs;
            m.slice_len = slice_len;
            m.words[0] = 0;
            m.words[1] = o.blob_len;
            m.words[2] = S;
            m.words[3] = cfg ? cfg->encoding : TE_ENCODING_CLAY;
            m.words[4] = cfg ? cfg->params : TE_CLAY_DEFAULT_PARAMS;
            m.words[5] = o.chunk_index;
            metas.push_back(m);
        }
    }
    // descriptor image
    Arena &A = arena ? *arena : c->enc;
    A.img.clear();
    struct Launch { GeomKey key; size_t off, count; };
    std::vector<Launch> launches;
    for (auto &kv : groups) launches.push_back({kv.first, A.put(kv.second.data(), kv.second.size() * sizeof(EncJob)), kv.second.size()});
    const size_t meta_off = A.put(metas.data(), metas.size() * sizeof(MetaJob));
    // generic-engine pattern (parity erased) for profiles outside the fast path
    size_t pat_off = 0, pool_off = 0;
    GpePattern pat{};
    std::vector<uint16_t> pool;
    std::vector<GpeJob> gjobs;
    std::vector<size_t> gjob_off;
    {
        uint64_t mask = 0;
        for (int i = h.k + h.nu; i < h.qt; i++) mask |= 1ull << i;
        if (!h.gpe_pattern(mask, pat, pool)) return TE_ERR_UNSUPPORTED;
        pat_off = A.put(&pat, sizeof(pat));
        pool_off = A.put(pool.data(), pool.size() * sizeof(uint16_t));
        for (auto &kv : groups) {
            std::vector<GpeJob> gj;
            for (const EncJob &e : kv.second) {
                GpeJob g{};
                g.in = e.src; g.out = e.dst; g.in_len = e.src_len; g.out_len = ~0ull; g.rot = e.rot; g.pattern = 0;
                gj.push_back(g);
            }
            gjob_off.push_back(A.put(gj.data(), gj.size() * sizeof(GpeJob)));
        }
    }
    int r = A.upload(s);
    if (r) return r;
    // one workspace for every fast-path launch of the call (they run in stream order)
    auto fast_path = [&](const Launch &L) {
        return c->fast_encode && !L.key.odd && (uint64_t)n * L.key.slice_len < 0x7fffffffull;
    };
    size_t total_stripes = 0;
    for (const Launch &L : launches) total_stripes += L.count;
    // a small per-call encode (every chunk kept): the staged kernel with one wave per workgroup
    const bool small = per_call && !keep && total_stripes <= g_enc_small;
    auto dma_path = [&](const Launch &L) {
        return fast_path(L) && encode_dma_supported(n, h.k, (uint32_t)(L.key.cs / h.alpha)) && !g_no_dma_encode &&
               !small;
    };
    size_t scratch_bytes = 0;
    for (const Launch &L : launches) {
        if (!fast_path(L) || dma_path(L)) continue;
        const uint32_t wps = ((uint32_t)(L.key.cs / h.alpha) + 3) / 4;
        EncArgs a{};
        a.njobs = (uint32_t)L.count;
        a.groups_per_stripe = (wps + 63) / 64;
        a.groups_per_wg = small ? 1u : 0u;
        scratch_bytes = std::max(scratch_bytes, encode_rows_scratch_bytes(a));
    }
    // the LDS-DMA launches' stripe-queue counters (encode_dma.hip): one dword per launch, after the
    // staged kernel's parking rows in the call's workspace
    const bool split_call = (per_call && total_stripes <= g_enc_split) || g_enc_split_batch;
    uint32_t nqueues = 0;
    for (const Launch &L : launches)
        if (dma_path(L)) nqueues += split_call ? 2u : 1u;
    const size_t queue_off = (scratch_bytes + 255) & ~(size_t)255;
    uint8_t *scratch = nullptr;
    if (scratch_bytes || nqueues) {
        r = A.workspace(queue_off + (size_t)nqueues * 4u, s, &scratch);
        if (r) return r;
    }
    uint32_t *const queues = reinterpret_cast<uint32_t *>(scratch + queue_off);
    uint32_t qi = 0;
    KTimer kt(s);
    // the counters are zero before every launch of the call: the metadata kernel runs first on the
    // stream and clears them; a call without one (raw chunks, a keep filter) clears them with a memset
    if (!metas.empty())
        TE_HIP(launch_meta(A.at<MetaJob>(meta_off), (uint32_t)metas.size(), (uint32_t)n, s, queues, nqueues));
    else if (nqueues)
        TE_HIP(hipMemsetAsync(queues, 0, (size_t)nqueues * 4u, s));
    auto gpe_args = [&](size_t gi, const Launch &L, uint32_t word_base, uint32_t word_end) {
        const uint32_t cs = (uint32_t)L.key.cs, sc = cs / (uint32_t)h.alpha;
        (void)sc;
        GpeArgs a{};
        a.jobs = A.at<GpeJob>(gjob_off[gi]);
        a.patterns = A.at<GpePattern>(pat_off);
        a.plane_pool = A.at<uint16_t>(pool_off);
        a.njobs = (uint32_t)L.count;
        a.word_base = word_base;
        a.word_end = word_end;
        a.groups_per_stripe = (word_end - word_base + kGpeWords - 1) / kGpeWords;
        a.cs = cs; a.sc = cs / (uint32_t)h.alpha; a.q = h.q; a.t = h.t; a.k = h.k; a.nu = h.nu; a.n = n;
        a.alpha = h.alpha;
        a.in_stride = cs; a.out_stride = L.key.slice_len;
        a.in_rotated = 0; a.out_rotated = 1;
        a.out_mask = 0;
        for (int i = 0; i < h.qt; i++)
            if (h.int_to_ext(i) >= 0) a.out_mask |= 1ull << i;
        for (int i = 0; i < 16; i++) a.qpow[i] = h.qpow[i];
        return a;
    };
    size_t gi = 0;
    std::vector<std::pair<bool, EncArgs>> level2;  // split launches' level-2 halves, enqueued last
    te_encode_launch_stats &els = c->els;  // summed: the calling entry point zeroed it
    for (const Launch &L : launches) {
        const uint32_t cs = (uint32_t)L.key.cs, sc = cs / (uint32_t)h.alpha;
        const uint32_t wps = (sc + 3) / 4;   // words incl. a 2-column tail when sc % 4 == 2
        const uint32_t full = sc / 4;        // full 4-column words
        // fast kernel addresses an object's slices with 31-bit buffer offsets
        if (dma_path(L)) {  // the 1 MB-stripe kernel (encode_dma.hip)
            EncArgs a{};
            a.jobs = A.at<EncJob>(L.off);
            a.njobs = (uint32_t)L.count;
            a.cs = cs;
            a.sc = sc;
            a.slice_len = (uint32_t)L.key.slice_len;
            a.n = (uint32_t)n;
            a.queue = queues + qi++;
            if (split_call) {
                // level-1 rows z0 = 0..6: one workgroup each (or g_enc_split_batch rows each)
                const uint32_t per = per_call ? 1u : g_enc_split_batch;
                a.z0_first = 0; a.z0_count = per; a.z0_split = (7 + per - 1) / per; a.z0_limit = 7;
                TE_HIP(launch_encode_dma(L.key.masked, a, s));
                els.dma_level1_launches++;
                a.z0_limit = 0;
                a.z0_first = 7; a.z0_count = 3; a.z0_split = 1;   // level 2 reads their parity back:
                a.queue = queues + qi++;
                level2.push_back({L.key.masked, a});              // after every level-1 launch
            } else {
                TE_HIP(launch_encode_dma(L.key.masked, a, s));
            }
            els.dma_launches++;
            els.dma_stripes += L.count;
        } else if (fast_path(L)) {
            (void)full;
            EncArgs a{};
            a.jobs = A.at<EncJob>(L.off);
            a.njobs = (uint32_t)L.count;
            a.groups_per_stripe = (wps + 63) / 64;
            a.groups_per_wg = small ? 1u : 0u;
            a.words_per_stripe = wps;
            a.cs = cs;
            a.sc = sc;
            a.slice_len = (uint32_t)L.key.slice_len;
            a.n = (uint32_t)n;
            a.scratch = scratch;
            TE_HIP(launch_encode_rows(h.k, L.key.masked, a, s));
            els.stage_launches++;
            els.stage_masked_launches += L.key.masked ? 1u : 0u;
            els.stage_stripes += L.count;
            els.stage_g = encode_stage_g(a);
            els.stage_wgs = encode_stage_wgs(a);
        } else {
            TE_HIP(launch_gpe(gpe_args(gi, L, 0, wps), (uint32_t)pat.nerased, s));
            els.generic_launches++;
            els.generic_stripes += L.count;
        }
        gi++;
    }
    for (const auto &l2 : level2) {
        TE_HIP(launch_encode_dma(l2.first, l2.second, s));
        els.dma_launches++;
        els.dma_level2_launches++;
    }
    kt.stop();
    return A.mark_done(s);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Decode
// ------------------------------------------------------------------------------------------
namespace {

// The chunk path (TE_RANGE_CHUNK) is open to an object where a node recover of its stripes runs a
// class kernel: Clay(20,7,16), the class kernels not switched off (measurement knob), sub-chunks
// of >= 8 bytes and 31-bit slice / share offsets (dec_geom_staged, on the object's own slice
// length).  Host only: te_slicer_range_plan_ex answers from the same rule.
bool range_chunk_ok(const ClayHost &h, uint64_t cs, uint64_t slice_len) {
    if (!dec_class_on() || h.n != kDecClassN || h.k != kDecClassK || h.q != kRepQ || h.t != 2 || h.nu != 0) return false;
    return dec_geom_staged(h, cs, slice_len);
}

// Validate one object like Slicer::decode (slicer.rs:298-331, validate_layout :79-105).
int decode_validate(const te_clay *c, const uint8_t *meta48, uint64_t slice_len, uint32_t avail, DecItem &it) {
    const ClayHost &h = c->h;
    const int na = __builtin_popcount(avail & ((h.n >= 32) ? 0xffffffffu : ((1u << h.n) - 1u)));
    if (na == 0) return TE_ERR_NOT_ENOUGH_SLICES;
    te_slice_metadata m;
    int r = te_slice_metadata_from_slice(meta48, TE_META_SIZE, &m);
    if (r) return r;
    const uint32_t pk = (uint32_t)((m.params >> 8) & 0xFF);  // profile k  slicer.rs:308-311
    if ((uint32_t)na < pk) return TE_ERR_NOT_ENOUGH_SLICES;
    it.blob_len = m.blob_len;
    it.stripe = m.stripe_size;
    it.slice_len = slice_len;
    it.avail = avail;
    if (m.blob_len == 0) { it.ns = 0; it.cs = 0; return TE_OK; }
    it.ns = (m.blob_len + m.stripe_size - 1) / m.stripe_size;
    const uint64_t total = slice_len >= TE_META_SIZE ? slice_len - TE_META_SIZE : 0;
    if (total == 0 || total % it.ns) return TE_ERR_INVALID_LAYOUT;
    it.cs = total / it.ns;
    if (na < h.k) return TE_ERR_NOT_ENOUGH_SLICES;  // ClayCoder::decode clay.rs:107-109
    if (it.cs % (uint64_t)h.alpha) return TE_ERR_BAD_ENCODING;
    // take <= decoded stripe size (slicer.rs:351-357)
    const uint64_t last_take = m.blob_len - (it.ns - 1) * m.stripe_size;
    if (std::max<uint64_t>(it.ns > 1 ? m.stripe_size : 0, last_take) > it.cs * (uint64_t)h.k) return TE_ERR_INVALID_LAYOUT;
    return TE_OK;
}

// Compile one padded erasure pattern (host only, thread-safe: pure ClayHost work).  out_node >= 0:
// the program outputs that internal node's chunk (ClayHost::dec_prog).
bool compile_pattern(const ClayHost &h, uint64_t emask, int out_node, te_clay::DecCache &d) {
    const int n = h.n;
    if (!h.gpe_pattern(emask, d.P, d.planes)) return false;
    d.P.planes_off = 0;
    // node recover of Clay(20,7,16): the lost node first among its column's erased nodes, the
    // order the recover class kernels assume (dec_class.hpp); every program below follows it
    if (out_node >= 0 && dec_class_of(h, d.P) >= 0) dec_class_lost_first(d.P, out_node);
    // staged kernel (decode_stage.hip): compiled per k with every other node erased (padded
    // patterns); of the two row orientations, two workgroups per CU first (2 x 53 x 1536 B <=
    // 160 KB), then fewer scratch rows
    if (decode_stage_k(h.k) && d.P.nknown == (uint32_t)h.k && d.P.nerased == (uint32_t)(n - h.k)) {
        DecProgHdr best{};
        std::vector<DecStep> best_steps;
        bool found = false;
        auto cost = [](const DecProgHdr &x) {
            return (decode_stage_rows(x.nslots, x.max_out) > 53 ? 1u << 20 : 0u) + x.nscratch;
        };
        static const int force = [] {  // TEC_DEC_ORIENT=0/1: one row orientation only (measurement)
            const char *e = tec_knob("TEC_DEC_ORIENT");
            return e ? atoi(e) : -1;
        }();
        for (int orient = 0; orient < 2; orient++) {
            if (force >= 0 && orient != force) continue;
            DecProgHdr H;
            std::vector<DecStep> st;
            if (!h.dec_prog(d.P, orient, H, st, out_node) || !decode_stage_fits(H.nslots, H.max_out)) continue;
            if (!found || cost(H) < cost(best)) { best = H; best_steps.swap(st); found = true; d.orient = orient; }
        }
        bool ok = found;
        for (const DecStep &S : best_steps) {
            d.steps.emplace_back();
            ok = ok && ClayHost::dec_pack(S, d.steps.back());
        }
        d.steps.resize(d.steps.size() + 2);  // blank steps: the kernel reads two steps ahead
        d.staged = ok && d.steps.size() == te_clay::DecStore::kSteps;
        d.H = best;
    }
    return true;
}

// The compiled form of the pattern of `key` (dec_key), built once per handle (caller holds c->mu).
const te_clay::DecCache *dec_pattern(te_clay *c, uint64_t key) {
    auto f = c->dec_cache.find(key);
    if (f != c->dec_cache.end()) return &f->second;
    te_clay::DecCache d;
    if (!compile_pattern(c->h, dec_key_emask(key), dec_key_out_node(key), d)) return nullptr;
    return &c->dec_cache.emplace(key, std::move(d)).first->second;
}

// Compile the patterns of `keys` missing from the cache, on up to 16 host threads (random
// survivor sets bring one new pattern per stripe: ~150 us of host work each).
void dec_precompile(te_clay *c, const std::vector<uint64_t> &keys) {
    std::vector<uint64_t> todo;
    for (uint64_t k : keys)
        if (!c->dec_cache.count(k)) todo.push_back(k);
    if (todo.size() < 8) return;  // dec_pattern compiles the few inline
    std::vector<te_clay::DecCache> out(todo.size());
    std::vector<char> ok(todo.size(), 0);
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nth = std::min<size_t>({16, (size_t)hw, (todo.size() + 7) / 8});
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < todo.size();)
            ok[i] = compile_pattern(c->h, dec_key_emask(todo[i]), dec_key_out_node(todo[i]), out[i]);
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nth; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    for (size_t i = 0; i < todo.size(); i++)
        if (ok[i]) c->dec_cache.emplace(todo[i], std::move(out[i]));
}

// Slots of the device-resident pattern store (te_clay::DecStore) for the staged patterns of one
// call.  The patterns not there yet are appended to U (host images of their store entries) for
// decode_enqueue to upload with the call's descriptors and copy into their slots on the call's
// stream.  false: more distinct patterns than the store holds (the call then uploads its patterns
// through the arena).
struct StoreFill {
    uint32_t n0 = 0;                  // first new slot
    bool wait_used = false;           // new slots overwrite slots earlier launches may still read
    std::vector<GpePattern> pats;
    std::vector<DecProgHdr> hdrs;
    std::vector<DecStepP> steps;
    std::vector<uint32_t> soff;       // slot -> step offset, when the store was (re)allocated
};
bool dec_store_slots(te_clay *c, const std::vector<const te_clay::DecCache *> &cached, const std::vector<uint64_t> &keys,
                     std::vector<uint32_t> &slot_of, StoreFill &U, int &rc) {
    te_clay::DecStore &S = c->dstore;
    constexpr uint32_t kSteps = te_clay::DecStore::kSteps;
    rc = TE_OK;
    const uint32_t cap_max = S.max_cap;
    if (keys.size() > cap_max) {
        S.arena_calls++;
        return false;
    }
    if (!S.written && (rc = hip_status(hipEventCreateWithFlags(&S.written, hipEventDisableTiming)))) return false;
    size_t fresh = 0;
    for (uint64_t k : keys) fresh += S.slot.count(k) == 0;
    if (S.n + fresh > S.cap) {
        // grow (doubling, up to kCap) when the call's patterns do not fit, else empty the full
        // store; either way the old contents go once their last reader is done
        const uint32_t need = (uint32_t)std::min<size_t>(cap_max, std::max<size_t>(keys.size(), (size_t)S.n + fresh));
        if (S.cap < cap_max && need > S.cap) {
            uint32_t cap = std::min(te_clay::DecStore::kMin, cap_max);
            while (cap < need) cap *= 2;
            cap = std::min(cap, cap_max);
            // the buffers are freed: every launch that read them must be done (rare: <= 6 times)
            if ((rc = hip_status(S.readers.sync()))) return false;
            S.pats.release();
            S.hdrs.release();
            S.steps.release();
            S.soff.release();
            if ((rc = hip_status(S.pats.ensure((size_t)cap * sizeof(GpePattern))))) return false;
            if ((rc = hip_status(S.hdrs.ensure((size_t)cap * sizeof(DecProgHdr))))) return false;
            if ((rc = hip_status(S.steps.ensure((size_t)cap * kSteps * sizeof(DecStepP))))) return false;
            if ((rc = hip_status(S.soff.ensure((size_t)cap * sizeof(uint32_t))))) return false;
            S.cap = cap;
            U.soff.resize(cap);
            for (uint32_t i = 0; i < cap; i++) U.soff[i] = i * kSteps;
            S.grows++;
        } else {
            U.wait_used = S.readers.any();  // the fill waits (on the device) for the last reader on every stream
            S.clears++;
        }
        S.slot.clear();
        S.n = 0;
    }
    slot_of.assign(keys.size(), 0);
    U.n0 = S.n;
    for (size_t i = 0; i < keys.size(); i++) {
        auto f = S.slot.find(keys[i]);
        if (f != S.slot.end()) {
            slot_of[i] = f->second;
            continue;
        }
        const uint32_t sl = S.n++;
        S.slot.emplace(keys[i], sl);
        slot_of[i] = sl;
        U.pats.push_back(cached[i]->P);
        U.hdrs.push_back(cached[i]->H);
        U.steps.insert(U.steps.end(), cached[i]->steps.begin(), cached[i]->steps.end());
    }
    return true;
}

// One arena's gather launch (if any job), then its metadata launch (if any)
int gather_meta_enqueue(Arena &A, hipStream_t s, const std::vector<CopyJob> &copies, const std::vector<MetaJob> &metas) {
    A.img.clear();
    const size_t off = A.put(copies.data(), copies.size() * sizeof(CopyJob));
    const size_t moff = A.put(metas.data(), metas.size() * sizeof(MetaJob));
    const int r = A.upload(s);
    if (r) return r;
    KTimer kt(s);
    if (!copies.empty()) TE_HIP(launch_gather(A.at<CopyJob>(off), (uint32_t)copies.size(), s));
    if (!metas.empty()) TE_HIP(launch_meta(A.at<MetaJob>(moff), (uint32_t)metas.size(), 1u, s));
    kt.stop();
    return A.mark_done(s);
}
// A pattern with a per-pattern kernel built (dec_rtc.cpp): its jobs leave their group for a launch of their own
struct DecFixed { DecGroupKey key; const DecJitKernel *k; std::vector<GpeJob> jobs; size_t off = 0; };

// What the steps of one decode_enqueue call share
struct DecCall {
    te_clay *c; hipStream_t s; int rotated;
    DecPlan plan;
    std::vector<const te_clay::DecCache *> cached;  // by pattern id (plan.keys)
    bool staged = true;  // every pattern compiles to a plane program (decode_stage.hip, the class kernels)
    uint32_t lds_rows = 0, nscr_max = 0, max_er = 0;
    std::vector<DecFixed> fixed;
    DecRoute route;
    // staged patterns live in the device store (uploaded once per handle), the jobs name slots;
    // otherwise (generic kernel, or more patterns than the store holds) they go in the arena
    bool in_store = false;
    StoreFill fill;
    std::vector<std::pair<DecGroupKey, size_t>> offs;  // the table groups left non-empty: their jobs in the arena
    size_t pat_off = 0, pool_off = 0, hdr_off = 0, step_off = 0, soff_off = 0, copy_off = 0;
    size_t fp_off = 0, fh_off = 0, fs_off = 0, fo_off = 0;  // new store entries
    bool small_dec = false;  // one wave per workgroup
    uint32_t class_g = 2;
    int class_streams = 1;  // streams the class groups run on, side by side
    uint8_t *scratch = nullptr, *cls_scratch = nullptr;

    bool staged_group(const DecGroupKey &k) const { return staged && dec_geom_staged(c->h, k.cs, k.slice_len); }
    uint32_t sc(const DecGroupKey &k) const { return (uint32_t)(k.cs / (uint64_t)c->h.alpha); }
    const GpePattern *pats() const { return in_store ? c->dstore.pats.as<GpePattern>() : c->dec.at<GpePattern>(pat_off); }
};
// Step 2: every key's compiled pattern
int dec_resolve(DecCall &D) {
    dec_precompile(D.c, D.plan.keys);
    for (uint64_t key : D.plan.keys) {
        const te_clay::DecCache *dc = dec_pattern(D.c, key);
        if (!dc) return TE_ERR_BAD_ENCODING;
        D.cached.push_back(dc);
        D.max_er = std::max(D.max_er, dc->P.nerased);
    }
    for (const te_clay::DecCache *dc : D.cached) {
        if (!(D.staged = dc->staged)) break;
        D.lds_rows = std::max(D.lds_rows, decode_stage_rows(dc->H.nslots, dc->H.max_out));
        D.nscr_max = std::max(D.nscr_max, dc->H.nscratch);
    }
    D.lds_rows = std::max(D.lds_rows, 1u);
    return TE_OK;
}
// Step 3: patterns with a per-pattern kernel built (dec_rtc.cpp) leave their group for a launch of
// their own; every staged stripe counts toward building its pattern's kernel.
// (pattern kernels write data chunks whole: recover's outputs are other nodes, and a ranged
// call's jobs carry a window the pattern kernels do not clip)
void dec_pick_jit(DecCall &D) {
    te_clay *c = D.c;
    if (!D.staged || D.plan.fused || D.plan.ranged_call) return;
    constexpr uint64_t kJitMinStripes = 512;  // two workgroups per CU
    // a caller that lowered the build threshold (te_clay_set_decode_jit, tests) lowers the floor too
    const uint64_t jit_floor = c->jit_mode >= 0 ? std::min<uint64_t>(kJitMinStripes, c->jit_min) : kJitMinStripes;
    if (!c->jit) {
        c->jit = dec_jit_new(c->device);
        if (c->jit_mode >= 0) dec_jit_set(c->jit, c->jit_mode, c->jit_min);
    }
    const size_t np = D.cached.size();
    for (auto &kv : D.plan.groups) {
        if (!D.staged_group(kv.first)) continue;
        const DecJitGeom geo = dec_jit_geom(D.sc(kv.first));
        std::vector<uint64_t> cnt(np, 0);
        for (const GpeJob &g : kv.second) cnt[g.pattern]++;
        std::vector<int> fx(np, -1);
        for (size_t p = 0; p < np; p++) {
            // a pattern kernel gets a launch of its own: only worth it for a group that fills
            // the GPU; smaller groups stay in the shared table-driven launch (recover's
            // windows hold ~64 stripes per pattern: 80 small launches per step ran 29.3 ms
            // against 14.5 for the shared one).  Such groups do not count toward building a
            // kernel either: it could never be launched for them.
            if (cnt[p] < std::max<uint64_t>(1, jit_floor)) continue;
            // a survivor set with a class kernel runs it: after the load fusions the class
            // kernels time at or below the hipRTC pattern kernels (4.26 vs 4.36-4.39 ms, worst
            // case, same box) with no 25 s compile; a caller that asked for the pattern kernels
            // (te_clay_set_decode_jit) still gets them
            if (c->jit_mode < 0 && dec_class_on() && dec_class_of(c->h, D.cached[p]->P) >= 0) continue;
            const DecJitKernel *k = dec_jit_get(c->jit, c->h, D.cached[p]->P, D.cached[p]->orient, (int)geo.G, (int)geo.wb, cnt[p]);
            if (!k) continue;
            fx[p] = (int)D.fixed.size();
            D.fixed.push_back(DecFixed{kv.first, k, {}});
        }
        std::vector<GpeJob> rest;
        for (const GpeJob &g : kv.second) {
            if (fx[g.pattern] >= 0) D.fixed[fx[g.pattern]].jobs.push_back(g);
            else rest.push_back(g);
        }
        kv.second.swap(rest);
    }
}
// Step 4: the class kernels' share (dec_route, dec_plan.hpp), with this process's knobs
int dec_route_call(DecCall &D) {
    // measurement option TEC_DEC_CLASS_SMALL=1 (off by default)
    static const bool small_dec_cls = [] { const char *e = tec_knob("TEC_DEC_CLASS_SMALL"); return e && e[0] == '1'; }();
    static const int class_streams = [] {
        const char *e = tec_knob("TEC_DEC_CLASS_STREAMS");
        const int v = e ? atoi(e) : 4;  // the process's hardware queues (GPU_MAX_HW_QUEUES default)
        return std::max(1, std::min(v, 1 + te_clay::kClsSide));
    }();
    D.class_streams = class_streams;
    std::vector<int> pat_class(D.cached.size());
    for (size_t p = 0; p < D.cached.size(); p++)  // (an output node >= 0: node recover's, a chunk stripe's)
        pat_class[p] = dec_class_of(D.c->h, D.cached[p]->P, dec_key_out_node(D.plan.keys[p]));
    D.route = dec_route(D.c->h, D.staged, pat_class, [](int id) { return dec_class_info(id, nullptr, nullptr); },
                        D.plan.groups, D.plan.chunk_groups, dec_class_on(), class_streams, small_dec_cls);
    return D.route.err;
}
// Step 5: the patterns' store slots, and the call's descriptors in the arena's host image
int dec_image(DecCall &D) {
    te_clay *c = D.c;
    DecGroups &groups = D.plan.groups;
    std::vector<uint32_t> slot_of;
    bool every_group_staged = D.staged;  // the generic kernel reads per-call patterns (plane lists)
    for (auto &kv : groups) every_group_staged = every_group_staged && (kv.second.empty() || D.staged_group(kv.first));
    if (every_group_staged) {
        int rs = TE_OK;
        D.in_store = dec_store_slots(c, D.cached, D.plan.keys, slot_of, D.fill, rs);
        if (rs) return rs;
        if (D.in_store) {
            for (auto &kv : groups)
                for (GpeJob &g : kv.second) g.pattern = slot_of[g.pattern];
            for (DecClassGrp &cg : D.route.cls)
                for (GpeJob &g : cg.jobs) g.pattern = slot_of[g.pattern];
        }
    }
    std::vector<GpePattern> pats;  // the per-call copies (not in the store): patterns and plane lists, programs
    std::vector<uint16_t> pool;
    std::vector<DecProgHdr> dhdrs; std::vector<DecStepP> dsteps; std::vector<uint32_t> dstep_off;
    const bool progs = D.staged && !D.in_store;
    if (!D.in_store)
        for (const te_clay::DecCache *dc : D.cached) {
            if (progs) {
                dhdrs.push_back(dc->H);
                dstep_off.push_back((uint32_t)dsteps.size());
                dsteps.insert(dsteps.end(), dc->steps.begin(), dc->steps.end());
            }
            pats.push_back(dc->P);
            pats.back().planes_off = (uint32_t)pool.size();
            pool.insert(pool.end(), dc->planes.begin(), dc->planes.end());
        }
    Arena &A = c->dec;
    A.img.clear();
    D.pat_off = D.in_store ? 0 : A.put(pats.data(), pats.size() * sizeof(GpePattern));
    D.pool_off = A.put(pool.data(), pool.size() * sizeof(uint16_t));
    if (progs) {
        D.hdr_off = A.put(dhdrs.data(), dhdrs.size() * sizeof(DecProgHdr));
        D.step_off = A.put(dsteps.data(), dsteps.size() * sizeof(DecStepP), 64);
        D.soff_off = A.put(dstep_off.data(), dstep_off.size() * sizeof(uint32_t));
    }
    for (auto &kv : groups)
        if (!kv.second.empty()) D.offs.push_back({kv.first, A.put(kv.second.data(), kv.second.size() * sizeof(GpeJob))});
    for (DecFixed &f : D.fixed) f.off = A.put(f.jobs.data(), f.jobs.size() * sizeof(GpeJob));
    for (DecClassGrp &cg : D.route.cls) cg.off = A.put(cg.jobs.data(), cg.jobs.size() * sizeof(GpeJob));
    D.copy_off = A.put(D.plan.copies.data(), D.plan.copies.size() * sizeof(CopyJob));
    // new store entries ride in the same upload, then move to their slots on this stream
    const StoreFill &fill = D.fill;
    if (D.in_store && !fill.pats.empty()) {
        D.fp_off = A.put(fill.pats.data(), fill.pats.size() * sizeof(GpePattern));
        D.fh_off = A.put(fill.hdrs.data(), fill.hdrs.size() * sizeof(DecProgHdr));
        D.fs_off = A.put(fill.steps.data(), fill.steps.size() * sizeof(DecStepP), 64);
    }
    if (D.in_store && !fill.soff.empty()) D.fo_off = A.put(fill.soff.data(), fill.soff.size() * sizeof(uint32_t));
    return TE_OK;
}
// Step 6: the descriptors go up; new store entries move to their slots on the call's stream
int dec_upload(DecCall &D) {
    Arena &A = D.c->dec;
    hipStream_t s = D.s;
    int r = A.upload(s);
    if (r || !D.in_store) return r;
    te_clay::DecStore &S = D.c->dstore;
    const StoreFill &fill = D.fill;
    if (fill.wait_used) TE_HIP(S.readers.wait(s));
    // entries another stream filled and nobody on this stream has waited for yet
    if (S.written_pending && S.written_stream != s) TE_HIP(hipStreamWaitEvent(s, S.written, 0));
    if (!fill.pats.empty()) {
        const size_t np = fill.pats.size();
        TE_HIP(hipMemcpyAsync(S.pats.as<GpePattern>() + fill.n0, A.at<GpePattern>(D.fp_off), np * sizeof(GpePattern),
                              hipMemcpyDeviceToDevice, s));
        TE_HIP(hipMemcpyAsync(S.hdrs.as<DecProgHdr>() + fill.n0, A.at<DecProgHdr>(D.fh_off), np * sizeof(DecProgHdr),
                              hipMemcpyDeviceToDevice, s));
        TE_HIP(hipMemcpyAsync(S.steps.as<DecStepP>() + (size_t)fill.n0 * te_clay::DecStore::kSteps,
                              A.at<DecStepP>(D.fs_off), fill.steps.size() * sizeof(DecStepP), hipMemcpyDeviceToDevice, s));
    }
    if (!fill.soff.empty())
        TE_HIP(hipMemcpyAsync(S.soff.p, A.at<uint32_t>(D.fo_off), fill.soff.size() * sizeof(uint32_t),
                              hipMemcpyDeviceToDevice, s));
    if (!fill.pats.empty() || !fill.soff.empty()) {
        TE_HIP(hipEventRecord(S.written, s));
        S.written_pending = true;
        S.written_stream = s;
    }
    return TE_OK;
}
DecArgs dec_table_args(const DecCall &D, const std::pair<DecGroupKey, size_t> &o) {
    const te_clay *c = D.c;
    const Arena &A = c->dec;
    const te_clay::DecStore &S = c->dstore;
    DecArgs a{};
    a.jobs = A.at<GpeJob>(o.second);
    a.patterns = D.pats();
    a.hdrs = D.in_store ? S.hdrs.as<DecProgHdr>() : A.at<DecProgHdr>(D.hdr_off);
    a.steps = D.in_store ? S.steps.as<DecStepP>() : A.at<DecStepP>(D.step_off);
    a.step_off = D.in_store ? S.soff.as<uint32_t>() : A.at<uint32_t>(D.soff_off);
    a.njobs = (uint32_t)D.plan.groups.at(o.first).size();
    a.sc = D.sc(o.first);
    a.words_per_stripe = (a.sc + 3) / 4;
    a.cs = (uint32_t)o.first.cs; a.n = (uint32_t)c->h.n; a.nk = (uint32_t)c->h.k;
    a.lds_rows = D.lds_rows;
    a.nscratch_max = D.nscr_max;
    a.in_stride = o.first.slice_len;
    a.out_stride = o.first.cs;
    a.gmax = D.small_dec ? 1u : 0u;
    return a;
}
dfix_args dec_fixed_args(const DecCall &D, const DecFixed &f) {
    dfix_args a{};
    a.jobs = reinterpret_cast<const dfix::Job *>(D.c->dec.at<GpeJob>(f.off));
    a.scratch = D.scratch;
    a.in_stride = f.key.slice_len;
    a.out_stride = f.key.cs;
    a.njobs = (uint32_t)f.jobs.size();
    a.sc = D.sc(f.key);
    const DecJitGeom geo = dec_jit_geom(a.sc);  // the geometry the kernel was built for
    a.wps = geo.wps;
    a.wgs_per_stripe = geo.wgs;
    a.n = (uint32_t)D.c->h.n;
    a.nscratch = f.k->nscratch;
    return a;
}
// Step 7: the call's workspace -- the table and pattern launches share one range (they run in
// stream order), each class launch has its own after it (they may run side by side)
int dec_scratch(DecCall &D) {
    // a small call (a per-call decode: a few stripes on a 256-CU chip) runs one wave per
    // workgroup, so each stripe's 100-step chain is split over more workgroups with less work per
    // step.  Measurement option TEC_DEBUG_KNOBS=1 TEC_DEC_SMALL=n: the stripe bound (0: never).
    static const size_t dec_small_max = [] {
        const char *e = tec_knob("TEC_DEC_SMALL");
        return e ? (size_t)atoi(e) : kDecSmallStripes;
    }();
    static const uint32_t class_g_big = [] {  // measurement option TEC_DEC_CLASS_G (1 or 2)
        const char *e = tec_knob("TEC_DEC_CLASS_G");
        return e && atoi(e) == 1 ? 1u : 2u;
    }();
    size_t call_stripes = 0;
    for (auto &o : D.offs) call_stripes += D.plan.groups.at(o.first).size();
    for (const DecClassGrp &cg : D.route.cls) call_stripes += cg.jobs.size();
    D.small_dec = call_stripes <= dec_small_max;
    D.class_g = D.small_dec || D.route.cls_small ? 1u : class_g_big;
    size_t scratch_bytes = 0;
    for (auto &o : D.offs)
        if (D.staged_group(o.first)) scratch_bytes = std::max(scratch_bytes, decode_stage_scratch_bytes(dec_table_args(D, o)));
    for (const DecFixed &f : D.fixed) {
        const dfix_args a = dec_fixed_args(D, f);
        const DecJitGeom geo = dec_jit_geom(a.sc);
        const size_t b = (size_t)a.njobs * a.wgs_per_stripe * std::max(a.nscratch, 1u) * geo.G * 64u * geo.wb;
        scratch_bytes = std::max(scratch_bytes, b);
    }
    size_t cls_bytes = 0;
    for (const DecClassGrp &cg : D.route.cls)
        cls_bytes += dec_class_scratch_bytes(cg.id, (uint32_t)cg.jobs.size(), D.sc(cg.key), D.class_g);
    const size_t cls_off = (scratch_bytes + 255) & ~(size_t)255;
    if (cls_bytes) scratch_bytes = cls_off + cls_bytes;
    if (!scratch_bytes) return TE_OK;
    const int r = D.c->dec.workspace(scratch_bytes, D.s, &D.scratch);
    if (!r) D.cls_scratch = D.scratch + cls_off;
    return r;
}
// The class groups side by side on up to 1 + kClsSide streams, largest first, each with its own
// scratch range: one class's launch has a 100-step chain as its floor whatever its size, so
// groups one after another leave the GPU idle at every tail
int dec_launch_classes(DecCall &D) {
    te_clay *c = D.c;
    hipStream_t s = D.s;
    te_decode_launch_stats &dls = c->dls;
    const std::vector<DecClassGrp> &cls = D.route.cls;
    const int ns = std::min<int>(D.class_streams, (int)cls.size());
    std::vector<size_t> order(cls.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return cls[x].jobs.size() > cls[y].jobs.size(); });
    hipStream_t ss[1 + te_clay::kClsSide] = {s};
    if (ns > 1) {
        if (!c->cls_fork) TE_HIP(hipEventCreateWithFlags(&c->cls_fork, hipEventDisableTiming));
        TE_HIP(hipEventRecord(c->cls_fork, s));
        for (int i = 1; i < ns; i++) {
            if (!c->cls_s[i - 1]) TE_HIP(hipStreamCreateWithFlags(&c->cls_s[i - 1], hipStreamNonBlocking));
            if (!c->cls_join[i - 1]) TE_HIP(hipEventCreateWithFlags(&c->cls_join[i - 1], hipEventDisableTiming));
            TE_HIP(hipStreamWaitEvent(c->cls_s[i - 1], c->cls_fork, 0));
            ss[i] = c->cls_s[i - 1];
        }
    }
    size_t scr_at = 0;
    for (size_t k = 0; k < order.size(); k++) {
        const DecClassGrp &cg = cls[order[k]];
        const uint32_t sc = D.sc(cg.key);
        TE_HIP(launch_dec_class(cg.id, c->dec.at<GpeJob>(cg.off), D.pats(), (uint32_t)cg.jobs.size(), sc, cg.key.slice_len,
                                cg.key.cs, (uint32_t)c->h.n, D.cls_scratch + scr_at, D.class_g, ss[k % (size_t)ns]));
        scr_at += dec_class_scratch_bytes(cg.id, (uint32_t)cg.jobs.size(), sc, D.class_g);
        dls.class_launches[dec_class_base_id(cg.id)]++;  // a windowed kernel under its class
        dls.class_stripes += cg.jobs.size();
    }
    dls.class_g = D.class_g;
    dls.class_streams = std::max(dls.class_streams, (uint32_t)ns);
    for (int i = 1; i < ns; i++) {
        TE_HIP(hipEventRecord(c->cls_join[i - 1], ss[i]));
        TE_HIP(hipStreamWaitEvent(s, c->cls_join[i - 1], 0));
    }
    return TE_OK;
}
// Step 8: gather, pattern kernels, class kernels, then each table group on the staged or the generic kernel
int dec_launch(DecCall &D) {
    te_clay *c = D.c;
    const ClayHost &h = c->h;
    hipStream_t s = D.s;
    Arena &A = c->dec;
    te_decode_launch_stats &dls = c->dls;  // summed: the calling entry point zeroed it
    KTimer kt(s);
    if (!D.plan.copies.empty()) TE_HIP(launch_gather(A.at<CopyJob>(D.copy_off), (uint32_t)D.plan.copies.size(), s));
    for (const DecFixed &f : D.fixed) {
        const dfix_args a = dec_fixed_args(D, f);
        TE_HIP(launch_dec_fixed(*f.k, a, dec_jit_geom(a.sc).G, s));
        dls.jit_launches++;
        dls.jit_stripes += f.jobs.size();
    }
    if (!D.route.cls.empty())
        if (int r = dec_launch_classes(D)) return r;
    for (auto &o : D.offs) {
        if (D.staged_group(o.first)) {
            DecArgs a = dec_table_args(D, o);
            a.scratch = D.scratch;
            TE_HIP(launch_decode_stage(a, s));
            dls.table_launches++;
            dls.table_stripes += a.njobs;
            continue;
        }
        const uint32_t sc = D.sc(o.first);
        const uint32_t wps = sc >= 4 ? (sc + 3) / 4 : 1;
        GpeArgs a{};
        a.jobs = A.at<GpeJob>(o.second);
        a.patterns = A.at<GpePattern>(D.pat_off);
        a.plane_pool = A.at<uint16_t>(D.pool_off);
        a.njobs = (uint32_t)D.plan.groups.at(o.first).size();
        a.word_base = 0;
        a.word_end = wps;
        a.groups_per_stripe = (wps + kGpeWords - 1) / kGpeWords;
        a.cs = (uint32_t)o.first.cs; a.sc = sc; a.q = h.q; a.t = h.t; a.k = h.k; a.nu = h.nu; a.n = h.n; a.alpha = h.alpha;
        a.in_stride = o.first.slice_len;
        a.out_stride = o.first.cs;
        a.in_rotated = D.rotated ? 1u : 0u;
        a.out_rotated = 0;
        a.out_mask = (h.k >= 64) ? ~0ull : ((1ull << h.k) - 1ull);
        for (int i = 0; i < 16; i++) a.qpow[i] = h.qpow[i];
        TE_HIP(launch_gpe(a, D.max_er, s));
        dls.generic_launches++;
        dls.generic_stripes += a.njobs;
    }
    kt.stop();
    if (D.in_store) TE_HIP(c->dstore.readers.record(s));  // a later call that empties the store waits for these launches
    return A.mark_done(s);
}
// Items with lost >= 0 (node recover) need the staged kernel: TE_ERR_UNSUPPORTED, before anything
// is enqueued, when a pattern has no plane program (the caller then decodes and re-encodes).
int decode_enqueue(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const DecItem *items,
                   size_t nitems, uint8_t *d_out, hipStream_t s, bool raw) {
    static_assert(TE_DECODE_CLASSES == kDecClasses, "te_decode_launch_stats counts every class");
    // compiled programs kept on the host: <= ~430 MB (26 KB per pattern, as many as the device
    // store's cap; 77,520 masks exist for k = 7, x 20 outputs for node recover)
    if (c->dec_cache.size() > std::max<size_t>(c->dstore.max_cap, nitems)) c->dec_cache.clear();
    DecCall D{c, s, (cfg && !raw) ? cfg->rotated : 0};
    D.plan = dec_plan(c->h, D.rotated, raw, items, nitems, d_slices, d_out);
    const DecPlan &P = D.plan;
    c->rgs.stripes_touched += P.touched; c->rgs.stripes_copied += P.copied; c->rgs.stripes_decoded += P.decoded;
    c->rgs.gather_jobs += P.copies.size();
    c->rcs.stripes_rebuilt += P.rebuilt; c->rcs.gather_jobs += P.chunk_gather; c->rcs.bytes_stored += P.bytes_stored;
    if (P.groups.empty() && P.chunk_groups.empty())  // nothing to decode: a ranged call of copy stripes only (or of nothing)
        return P.copies.empty() ? (int)TE_OK : gather_meta_enqueue(c->dec, s, P.copies, {});
    int r = dec_resolve(D);
    if (r) return r;
    if (P.fused)
        for (auto &kv : P.groups)
            if (!D.staged_group(kv.first)) return TE_ERR_UNSUPPORTED;
    dec_pick_jit(D);
    if ((r = dec_route_call(D)) || (r = dec_image(D)) || (r = dec_upload(D)) || (r = dec_scratch(D))) return r;
    return dec_launch(D);
}

// ------------------------------------------------------------------------------------------
// Repair
// ------------------------------------------------------------------------------------------
struct RepItem {
    const te_repair_plan *plan;
    const uint64_t *helper_off;  // [n] offsets into d_helpers by slice id (UINT64_MAX = absent)
    uint64_t out_off;
    const uint8_t *meta;         // 48 bytes or null (raw)
};

int repair_enqueue(te_clay *c, const uint8_t *d_helpers, const RepItem *items, size_t nitems, uint8_t *d_out,
                   hipStream_t s) {
    const ClayHost &h = c->h;
    using RepKey = te_clay::RepKey;
    std::unordered_map<RepKey, uint32_t, te_clay::RepKeyHash> pat_index;  // -> pattern id of this call
    std::vector<RepPattern> pats;
    std::vector<const te_clay::RepCache *> cached;  // entries stay put: the map is trimmed only here
    if (c->rep_cache.size() > 4096) c->rep_cache.clear();
    std::vector<uint16_t> pool, pind;
    // jobs by (chunk size, folded kernel or not), in first-seen order; usually one chunk size
    struct Group { uint64_t cs; std::vector<RepJob> jobs[2]; };
    std::vector<Group> groups;
    std::vector<MetaJob> metas;
    uint32_t max_er = 0;
    uint64_t run[64];
    RepKey last_key{~0ull, ~0u};
    uint32_t last_pid = 0;
    for (size_t i = 0; i < nitems; i++) {
        const te_repair_plan *p = items[i].plan;
        if (p->n > 64) return TE_ERR_INVALID_ARG;
        std::fill(run, run + p->n, 0ull);
        Group *grp = nullptr;
        for (Group &g : groups)
            if (g.cs == p->cs) grp = &g;
        if (!grp) {
            groups.push_back(Group{p->cs, {}});
            grp = &groups.back();
            grp->jobs[0].reserve(nitems * p->ns);
        }
        const uint32_t sc = (uint32_t)(p->cs / (uint64_t)h.alpha);
        for (uint32_t st = 0; st < p->ns; st++) {
            const uint32_t *hsh = p->helper_shard.data() + (size_t)st * p->d;
            RepKey key{0, p->lost_shard[st]};
            for (uint32_t j = 0; j < p->d; j++) key.helpers |= 1ull << hsh[j];
            uint32_t pid;
            auto f = key == last_key ? pat_index.end() : pat_index.find(key);
            if (key == last_key) {
                pid = last_pid;
            } else if (f == pat_index.end()) {
                auto cf = c->rep_cache.find(key);
                if (cf == c->rep_cache.end()) {
                    te_clay::RepCache rc;
                    const std::vector<int> hs(hsh, hsh + p->d);
                    if (!h.rep_pattern((int)p->lost_shard[st], hs, rc.P, rc.pool, rc.pind)) return TE_ERR_CLAY;
                    if (h.nu == 0 && h.n == 2 * h.q && !g_no_fold_repair)
                        rc.fold = repair_fold_column(h.q, h.t, h.k, rc.P.beta, 8, rc.P.lost, rc.P.erased_mask,
                                                     rc.P.aloof_mask);
                    rc.prog_ok = repair_stage_supported(h.q, rc.P.beta, 8, rc.P.nerased, rc.P.nknown, rc.P.aloof_mask) &&
                                 h.rep_prog(rc.P, rc.pool.data(), rc.pind.data(), rc.prog);
                    cf = c->rep_cache.emplace(key, std::move(rc)).first;
                }
                const te_clay::RepCache &rc = cf->second;
                pid = (uint32_t)pats.size();
                pats.push_back(rc.P);
                pats.back().planes_off = (uint32_t)pool.size();
                pool.insert(pool.end(), rc.pool.begin(), rc.pool.end());
                pind.insert(pind.end(), rc.pind.begin(), rc.pind.end());
                cached.push_back(&rc);
                pat_index[key] = pid;
                max_er = std::max(max_er, rc.P.nerased);
            } else {
                pid = f->second;
            }
            last_key = key;
            last_pid = pid;
            RepJob j{};
            const uint8_t *any = nullptr;
            for (uint32_t hj = 0; hj < p->d; hj++) {
                const uint32_t sl = p->helper_slice[st * p->d + hj];
                const uint64_t off = items[i].helper_off[sl];
                if (off == ~0ull) return TE_ERR_MISSING_HELPER;
                any = j.helper[h.ext_to_int((int)hsh[hj])] = d_helpers + off + run[sl];
                run[sl] += (uint64_t)p->beta * p->sc;
            }
            j.out = d_out + items[i].out_off + (uint64_t)st * p->cs;
            j.pattern = pid;
            // stripes whose pattern is one of the folded kernel's helper sets of Clay(20,7,16) (all
            // 19 others available, or one of the other column's first 7 down) go to that kernel,
            // the rest to the staged / generic kernel
            const int fc = sc >= 8 ? cached[pid]->fold : -1;
            if (fc >= 0) {  // the folded kernel loads every node unconditionally (repair_fold.hip)
                j.aux = pats[pid].lost % (uint32_t)h.q | (uint32_t)fc << 8;
                for (int nd = 0; nd < h.qt; nd++)
                    if (!j.helper[nd]) j.helper[nd] = any;
            }
            grp->jobs[fc >= 0 ? 0 : 1].push_back(j);
        }
        if (items[i].meta) {
            MetaJob m{};
            m.dst = d_out + items[i].out_off + (uint64_t)p->ns * p->cs;
            m.slice_len = 0;
            for (int w = 0; w < 6; w++) m.words[w] = get_u64(items[i].meta + 8 * w);
            metas.push_back(m);
        }
    }
    // staged kernel when every pattern outside the folded kernel has a plane program
    std::vector<RepProg> progs(pats.size());
    bool staged = true;
    for (size_t i = 0; i < pats.size(); i++) {
        progs[i] = cached[i]->prog;
        if (cached[i]->fold < 0) staged = staged && cached[i]->prog_ok;
    }
    Arena &A = c->rep;
    A.img.clear();
    const size_t pat_off = A.put(pats.data(), pats.size() * sizeof(RepPattern));
    const size_t prog_off = staged ? A.put(progs.data(), progs.size() * sizeof(RepProg)) : 0;
    const size_t pool_off = A.put(pool.data(), pool.size() * sizeof(uint16_t));
    const size_t pind_off = A.put(pind.data(), pind.size() * sizeof(uint16_t));
    const size_t meta_off = A.put(metas.data(), metas.size() * sizeof(MetaJob));
    // one launch per chunk size for the folded kernel (every helper set), one for the others
    struct Launch { uint64_t cs; int fold; size_t off, njobs; };
    std::vector<Launch> offs;
    for (Group &g : groups)
        for (int f = 0; f < 2; f++)
            if (!g.jobs[f].empty())
                offs.push_back({g.cs, f == 0 ? 0 : -1, A.put(g.jobs[f].data(), g.jobs[f].size() * sizeof(RepJob)),
                                g.jobs[f].size()});
    int r = A.upload(s);
    if (r) return r;
    KTimer kt(s);
    if (!metas.empty()) TE_HIP(launch_meta(A.at<MetaJob>(meta_off), (uint32_t)metas.size(), 1u, s));
    for (auto &o : offs) {
        const uint64_t cs = o.cs;
        const uint32_t sc = (uint32_t)(cs / (uint64_t)h.alpha);
        const uint32_t wps = sc >= 4 ? (sc + 3) / 4 : 1;
        RepArgs a{};
        a.jobs = A.at<RepJob>(o.off);
        a.patterns = A.at<RepPattern>(pat_off);
        a.plane_pool = A.at<uint16_t>(pool_off);
        a.plane_ind = A.at<uint16_t>(pind_off);
        a.njobs = (uint32_t)o.njobs;
        a.words_per_stripe = wps;
        a.groups_per_stripe = (wps + kGpeWords - 1) / kGpeWords;
        a.cs = (uint32_t)cs; a.sc = sc; a.q = h.q; a.t = h.t; a.alpha = h.alpha;
        for (int i = 0; i < 16; i++) a.qpow[i] = h.qpow[i];
        te_repair_launch_stats &rls = c->rls;  // summed: the calling entry point zeroed it
        if (o.fold >= 0) {
            TE_HIP(launch_repair_fold(a, s));
            rls.fold_launches++;
            rls.fold_stripes += o.njobs;
            rls.fold_g = repair_fold_g(wps);
            rls.fold_wgs = repair_wgs(wps, rls.fold_g);
        } else if (staged && sc >= 8) {  // staged kernel: coalesced loads, whole-row stores
            a.progs = A.at<RepProg>(prog_off);
            TE_HIP(launch_repair_stage(a, s));
            rls.stage_launches++;
            rls.stage_stripes += o.njobs;
            rls.stage_g = repair_stage_g(wps);
            rls.stage_wgs = repair_wgs(wps, rls.stage_g);
        } else {
            TE_HIP(launch_repair(a, max_er, s));
            rls.generic_launches++;
            rls.generic_stripes += o.njobs;
        }
    }
    kt.stop();
    return A.mark_done(s);
}

// ClayCoder::plan_repair maps every minimum_to_repair failure to RepairError::Clay(e.to_string())
// (repair.rs:59-62); the detail text goes to te_last_error_detail().
int clay_plan_error(int r, int lost_shard, size_t navail, int d) {
    if (r == -1)
        snprintf(g_last_error, sizeof(g_last_error), "minimum_to_repair: need %d helpers, %zu available (lost shard %d)",
                 d, navail, lost_shard);
    else
        snprintf(g_last_error, sizeof(g_last_error),
                 "minimum_to_repair: a column-mate of lost shard %d is not available", lost_shard);
    return TE_ERR_CLAY;
}

int build_plan(const te_clay *c, int rotated, uint32_t lost, const uint32_t *avail, size_t navail, uint64_t ns,
               uint64_t cs, te_repair_plan **out) {
    const ClayHost &h = c->h;
    if (lost >= (uint32_t)h.n) return TE_ERR_INVALID_SLICE;
    if (cs % (uint64_t)h.alpha) return TE_ERR_INVALID_LAYOUT;
    te_repair_plan *p = new (std::nothrow) te_repair_plan();
    if (!p) return TE_ERR_OUT_OF_MEMORY;
    p->lost = lost; p->ns = (uint32_t)ns; p->d = (uint32_t)h.d; p->beta = (uint32_t)h.beta; p->n = (uint32_t)h.n;
    p->cs = cs; p->sc = cs / (uint64_t)h.alpha;
    for (uint64_t st = 0; st < ns; st++) {
        const int ls = (int)te_slice_to_shard(rotated, (uint32_t)h.n, (uint32_t)st, lost);
        std::vector<int> av;
        for (size_t i = 0; i < navail; i++) {
            if (avail[i] >= (uint32_t)h.n) { delete p; return TE_ERR_INVALID_SLICE; }
            av.push_back((int)te_slice_to_shard(rotated, (uint32_t)h.n, (uint32_t)st, avail[i]));
        }
        std::vector<int> hs;
        const int r = h.min_to_repair(ls, av, hs);
        if (r) { delete p; return clay_plan_error(r, ls, navail, h.d); }
        const std::vector<int> planes = h.repair_planes(ls);
        p->lost_shard.push_back((uint32_t)ls);
        for (int sh : hs) {
            p->helper_shard.push_back((uint32_t)sh);
            p->helper_slice.push_back(te_shard_to_slice(rotated, (uint32_t)h.n, (uint32_t)st, (uint32_t)sh));
            for (int z : planes) p->sub_chunks.push_back((uint32_t)z);
        }
    }
    *out = p;
    return TE_OK;
}

}  // namespace

// Host -> host encode pipeline (te_encode_batch_host), optionally with the slice commitments of
// BlobEncoder::encode_with_proofs (sdk/src/codec/encoder.rs:220-260): per object the n leaf hashes,
// the root and n proofs, computed on the device from the window's slices before they leave HBM.
struct CommitOut {
    uint8_t *leaf, *root, *proof;  // host: nobj * n * 32, nobj * 32, nobj * n * height * 32 (or null)
    uint32_t height;
};

// Device layout of objects [a, b) placed from offsets (din, dout) of a slot's buffers: the encode
// descriptors (`local`, offsets relative to the buffers) and the H2D / D2H copy runs.
static void window_layout(const te_object *objs, const std::vector<uint64_t> &out_bytes, size_t a, size_t b,
                          uint64_t din, uint64_t dout, std::vector<te_object> &local, std::vector<CopyRun> &hin,
                          std::vector<CopyRun> &hout) {
    local.clear();
    hin.clear();
    hout.clear();
    for (size_t o = a; o < b; o++) {
        local.push_back(te_object{din, objs[o].blob_len, dout, objs[o].chunk_index});
        add_run(hin, objs[o].data_off, din, objs[o].blob_len);
        add_run(hout, objs[o].out_off, dout, out_bytes[o]);
        din += align16(objs[o].blob_len);  // device copies 16-byte aligned
        dout += out_bytes[o];
    }
}

static int copy_runs(const std::vector<CopyRun> &runs, uint8_t *dev, const uint8_t *host, hipMemcpyKind kind,
                     hipStream_t s) {
    for (const CopyRun &r : runs) {
        const bool h2d = kind == hipMemcpyHostToDevice;
        void *dst = h2d ? (void *)(dev + r.dev) : (void *)(host + r.host);
        const void *src = h2d ? (const void *)(host + r.host) : (const void *)(dev + r.dev);
        TE_HIP(hipMemcpyAsync(dst, src, r.len, kind, s));
    }
    return TE_OK;
}

static int encode_host_impl(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data, const te_object *objs,
                            size_t nobj, uint8_t *h_out, size_t window_bytes) {
    if (!c || !cfg || (!objs && nobj) || (nobj && (!h_data || !h_out))) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    // default window 128 MiB (1024 x 4 MiB pinned: 14.1 GiB/s against 12.6 at 1 GiB -- smaller
    // windows overlap the H2D, kernels and D2H more finely; 64 MiB varied 11.1-14.3, below that the
    // per-window launches cost more; a fourth slot measured slower)
    if (window_bytes == 0) window_bytes = (size_t)128 << 20;
    const uint32_t n = (uint32_t)c->h.n;
    std::vector<uint64_t> out_bytes(nobj);
    for (size_t i = 0; i < nobj; i++) {
        te_geometry g;
        te_slicer_geometry(c, objs[i].blob_len, &g);
        out_bytes[i] = (uint64_t)n * g.slice_len;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    c->els = te_encode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    // three slot streams: the handle's two pipe streams and its own stream -- the same three the
    // commit pipeline uses (commit_streams), so with the caller's stream a process holds four
    // streams for its four hardware queues (GPU_MAX_HW_QUEUES) whichever host paths it runs
    if (int r0 = ensure_stream(c)) return r0;
    for (int k = 0; k < 2; k++)
        if (!c->pipe[k].s) TE_HIP(hipStreamCreateWithFlags(&c->pipe[k].s, hipStreamNonBlocking));
    auto slot_stream = [&](size_t k) { return k < 2 ? c->pipe[k].s : c->stream; };
    int rc = TE_OK;
    size_t i = 0, w = 0;
    std::vector<te_object> local;
    std::vector<CopyRun> hin, hout;
    while (i < nobj && rc == TE_OK) {
        // window [i, j): at least one object, in + out bytes within window_bytes
        size_t j = i;
        uint64_t in_sz = 0, out_sz = 0;
        while (j < nobj && (j == i || in_sz + out_sz + objs[j].blob_len + out_bytes[j] <= window_bytes)) {
            in_sz += align16(objs[j].blob_len);  // device copies 16-byte aligned
            out_sz += out_bytes[j];
            j++;
        }
        te_clay::Slot &sl = c->pipe[w % te_clay::kPipe];
        const hipStream_t ss = slot_stream(w % te_clay::kPipe);
        if ((rc = hip_status(sl.in.ensure(in_sz + 16))) || (rc = hip_status(sl.out.ensure(out_sz)))) break;
        window_layout(objs, out_bytes, i, j, 0, 0, local, hin, hout);
        if ((rc = copy_runs(hin, sl.in.as<uint8_t>(), h_data, hipMemcpyHostToDevice, ss))) break;
        rc = encode_enqueue(c, cfg, sl.in.as<uint8_t>(), local.data(), local.size(), sl.out.as<uint8_t>(), ss,
                            false, &sl.arena);
        if (rc) break;
        if ((rc = copy_runs(hout, sl.out.as<uint8_t>(), h_out, hipMemcpyDeviceToHost, ss))) break;
        i = j;
        w++;
    }
    for (size_t k = 0; k < te_clay::kPipe; k++) {
        const int r2 = hip_status(hipStreamSynchronize(slot_stream(k)));
        if (rc == TE_OK) rc = r2;
    }
    return rc;
}

// te_encode_commit_batch_host / te_stream_submit: encode + commitments, host -> host.  The leaf
// kernel's time per launch is one slice stream's SHA-256 (~27-30 ms for a 715 KB slice, DESIGN
// §4.4) whatever the number of objects, so hashing must not sit between a window's encode and its
// D2H copy (hashing each window on its slot stream: 9.6-10.5 GiB/s).  Objects go through the
// device in GROUPS of at most `group_bytes` (input + output); a group's slices stay in one of three
// resident group buffers until hashed.  Each group is encoded in copy windows of <= 128 MiB that
// rotate over two slot streams (H2D of the window into the slot's input buffer, encode into the
// group buffer, D2H of its slices: copies stay in stream order behind kernels and overlap across
// slots).  The hash stream hashes a whole group at once (one leaf/tree launch per run of equal
// slice lengths, then the D2H of leaf hashes, roots and proofs) after every slot stream has passed
// the group's last window.  A group buffer is refilled once its hashing is done.  Every ordering
// is a GPU-side event wait, so the host enqueues a group without blocking: consecutive calls on a
// CommitPipe (te_stream_submit's windows) overlap one window's encode with the previous one's
// hashing and copies.

// One device's pipeline state.  The one-shot entry point points it at the handle's slot streams,
// buffers and arenas (c->pipe, c->stream); a stream writer owns its own (te_stream_writer).
struct CommitPipe {
    static constexpr int R = te_clay::kPipe;  // resident group buffers
    // copy windows rotate over two slot streams: with the hashing stream and the caller's stream
    // that is four streams for four hardware queues (three slots: 9.5 against 12.0 GiB/s on one
    // box, 1024 x 4 MiB, in a process that had used its current stream, as bench.py has)
    static constexpr int S = 2;
    hipStream_t ss[S] = {}, hs = nullptr;
    DevBuf *in[S] = {};
    Arena *arena[S] = {};
    DevBuf *gout[R] = {}, *gcom[R] = {};
    // per slot stream "encoded its latest window" and "copied it out", per group buffer "hashed"
    // (which implies copied out); a stream wait binds to the record current when enqueued
    hipEvent_t ev_enc[S] = {}, ev_slot[S] = {}, ev_hashed[R] = {};
    bool slot_used[S] = {}, hashed_pending[R] = {};
    bool grow_ok = false;  // buffers may grow (after draining their users); else pre-sized
    size_t w = 0, groups = 0;

    int make_events() {
        for (hipEvent_t *e : {ev_enc, ev_slot})
            for (int k = 0; k < S; k++)
                if (!e[k]) TE_HIP(hipEventCreateWithFlags(&e[k], hipEventDisableTiming));
        for (int r = 0; r < R; r++)
            if (!ev_hashed[r]) TE_HIP(hipEventCreateWithFlags(&ev_hashed[r], hipEventDisableTiming));
        return TE_OK;
    }
    void destroy_events() {
        for (hipEvent_t *e : {ev_enc, ev_slot})
            for (int k = 0; k < S; k++)
                if (e[k]) (void)hipEventDestroy(e[k]), e[k] = nullptr;
        for (int r = 0; r < R; r++)
            if (ev_hashed[r]) (void)hipEventDestroy(ev_hashed[r]), ev_hashed[r] = nullptr;
    }
};

// One call's (or one submitted window's) objects and their commitment outputs.
struct CommitBatch {
    const uint8_t *h_data = nullptr;
    const te_object *objs = nullptr;
    size_t nobj = 0;
    uint8_t *h_out = nullptr;
    CommitOut co{};
    uint32_t n = 0;
    std::vector<uint64_t> out_bytes, slice_len;
    uint64_t leaf_b = 0, proof_b = 0;
    uint64_t in_bytes(size_t o) const { return align16(objs[o].blob_len); }  // device copies 16-byte aligned
};

static int commit_prepare(const te_clay *c, CommitBatch &B) {
    B.n = (uint32_t)c->h.n;
    B.out_bytes.assign(B.nobj, 0);
    B.slice_len.assign(B.nobj, 0);
    for (size_t i = 0; i < B.nobj; i++) {
        te_geometry g;
        te_slicer_geometry(c, B.objs[i].blob_len, &g);
        B.slice_len[i] = g.slice_len;
        B.out_bytes[i] = (uint64_t)B.n * g.slice_len;
        if (g.slice_len % 4) return TE_ERR_INVALID_ARG;  // the leaf kernel reads dwords
        // encode_enqueue's per-object check, made before a window touches a shared group
        if (g.chunk_size % (size_t)c->h.alpha || g.slice_len > 0xffffffffull || g.chunk_size > 0xffffffffull)
            return TE_ERR_TOO_MUCH_DATA;
    }
    B.leaf_b = (uint64_t)B.n * TE_HASH_SIZE;
    B.proof_b = B.co.proof ? B.leaf_b * B.co.height : 0;
    return TE_OK;
}

// Groups [gcut[x], gcut[x+1]) of about equal size (a small last group would be hashed after the
// previous one), and each group's copy windows.
struct CommitPlan {
    std::vector<size_t> gcut{0};
    std::vector<std::vector<size_t>> wcut;  // per group: window boundaries, first = group start
    uint64_t max_win_in = 16, max_group_out = 0, max_group_obj = 0;
};
static void commit_plan(const CommitBatch &B, uint64_t group_bytes, uint64_t copy_bytes, CommitPlan &P) {
    uint64_t total = 0;
    for (size_t o = 0; o < B.nobj; o++) total += B.objs[o].blob_len + B.out_bytes[o];
    const uint64_t target = total / std::max<uint64_t>(1, (total + group_bytes - 1) / group_bytes);
    for (size_t i = 0; i < B.nobj;) {
        size_t j = i;
        uint64_t gsz = 0, gout = 0;
        while (j < B.nobj && (j == i || (gsz < target && gsz + B.objs[j].blob_len + B.out_bytes[j] <= group_bytes))) {
            gsz += B.objs[j].blob_len + B.out_bytes[j];
            gout += B.out_bytes[j];
            j++;
        }
        std::vector<size_t> wc{i};
        for (size_t a = i; a < j;) {
            size_t b = a;
            uint64_t win = 0, win_in = 0;
            while (b < j && (b == a || win + B.objs[b].blob_len + B.out_bytes[b] <= copy_bytes)) {
                win += B.objs[b].blob_len + B.out_bytes[b];
                win_in += B.in_bytes(b);
                b++;
            }
            P.max_win_in = std::max(P.max_win_in, win_in + 16);
            wc.push_back(b);
            a = b;
        }
        P.wcut.push_back(std::move(wc));
        P.max_group_out = std::max(P.max_group_out, gout);
        P.max_group_obj = std::max<uint64_t>(P.max_group_obj, j - i);
        P.gcut.push_back(j);
        i = j;
    }
}

// One object's slices copied out in row pieces (host-hashed groups, pinned host output): piece p
// is bytes [beg[p], beg[p+1]) of every slice, landed once ev[p] has completed.  The host hashing
// tasks follow the pieces as they land instead of waiting for the whole window's D2H.
//
// The piece events come from a per-device pool and are waited for by polling (hipEventQuery with
// short sleeps), not by blocking-sync waits: with one blocking-sync event created, waited for by
// interrupt and destroyed per piece (ten per 64 MiB chunk), the SDK-shape stream slowed to
// 7.1 GiB/s (chunk latency 33.6 ms, against 15-16 ms in a fresh process) once the process had run
// the earlier copy-inclusive legs -- and ran 11.6 GiB/s in that same state with no pieces
// (r05, gpurun_out/r5h).  Polling costs a worker a few microseconds per check and no interrupt.
class EventPool {
  public:
    static EventPool &get(int device) {
        static std::mutex mu;
        static std::map<int, EventPool *> pools;
        std::lock_guard<std::mutex> g(mu);
        EventPool *&p = pools[device];
        if (!p) p = new EventPool();  // never destroyed (events outlive static destructors' order)
        return *p;
    }
    hipError_t acquire(hipEvent_t &e) {
        {
            std::lock_guard<std::mutex> g(m_);
            if (!free_.empty()) {
                e = free_.back();
                free_.pop_back();
                return hipSuccess;
            }
        }
        return hipEventCreateWithFlags(&e, hipEventDisableTiming);
    }
    void release(hipEvent_t e) {
        std::lock_guard<std::mutex> g(m_);
        if (free_.size() < 4096) free_.push_back(e);
        else (void)hipEventDestroy(e);
    }

  private:
    std::mutex m_;
    std::vector<hipEvent_t> free_;
};

// Wait for an event by polling: a short spin, then sleeps of 20 us (hashing workers waiting for
// the next row piece of their slices).
static hipError_t event_wait_poll(hipEvent_t e) {
    for (int i = 0;; i++) {
        const hipError_t r = hipEventQuery(e);
        if (r != hipErrorNotReady) return r;
        if (i < 16) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

struct PieceEvents {
    int device = 0;
    std::vector<hipEvent_t> ev;
    std::vector<uint64_t> beg;
    ~PieceEvents() {
        EventPool &pool = EventPool::get(device);
        for (hipEvent_t e : ev) pool.release(e);
    }
};

// Row pieces of kPiece bytes per slice (measurement option TEC_DEBUG_KNOBS=1 TEC_D2H_PIECE=bytes,
// 0 = one copy per window as before; TEC_D2H_ROWS=1 copies each piece slice by slice instead of
// one 2-D copy).  Objects whose slices are shorter than two pieces are copied whole.
static uint64_t d2h_piece_bytes() {
    static const uint64_t v = [] {
        const char *s = tec_knob("TEC_D2H_PIECE");
        return s ? (uint64_t)strtoull(s, nullptr, 10) : (uint64_t)1 << 20;
    }();
    return v;
}
static bool d2h_rows() {
    static const bool v = [] {
        const char *s = tec_knob("TEC_D2H_ROWS");
        return s && s[0] == '1';
    }();
    return v;
}

// Page-locked (te_host_alloc / te_host_register / hipHostMalloc): row-piece copies of pageable
// memory would each go through the driver's staging.
static bool host_pinned(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
// The address a kernel may use for page-locked host memory `p` (hipPointerAttribute_t's
// devicePointer: HIP promises no other, and a registered range need not map at its host address),
// or null when `p` is pageable or has no device mapping.
static uint8_t *host_device_ptr(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? static_cast<uint8_t *>(a.devicePointer) : nullptr;
}

// Copy object o's n slices (slice_len bytes each, at dev / host) out in row pieces on stream s.
static int copy_out_pieces(uint8_t *host, const uint8_t *dev, uint64_t slice_len, uint32_t n, int device,
                           hipStream_t s, std::shared_ptr<PieceEvents> &out) {
    const uint64_t piece = d2h_piece_bytes();
    auto pe = std::make_shared<PieceEvents>();
    pe->device = device;
    for (uint64_t off = 0; off < slice_len;) {
        const uint64_t w = std::min(piece, slice_len - off);
        if (d2h_rows()) {
            for (uint32_t i = 0; i < n; i++)
                TE_HIP(hipMemcpyAsync(host + i * slice_len + off, dev + i * slice_len + off, w, hipMemcpyDeviceToHost, s));
        } else {
            TE_HIP(hipMemcpy2DAsync(host + off, slice_len, dev + off, slice_len, w, n, hipMemcpyDeviceToHost, s));
        }
        hipEvent_t e = nullptr;
        TE_HIP(EventPool::get(device).acquire(e));
        pe->ev.push_back(e);
        pe->beg.push_back(off);
        TE_HIP(hipEventRecord(e, s));
        off += w;
    }
    pe->beg.push_back(slice_len);
    out = std::move(pe);
    return TE_OK;
}

// A group's commitment outputs on the device: leaf hashes of row q at q * leaf_b, roots after
// `rows_cap` rows of leaves, proofs after the roots (rows = objects, in group order).
struct GroupSeg {
    CommitOut co;            // the host outputs of the segment's window
    size_t obj0 = 0;         // first object of the segment in its window (host output index)
    uint64_t row0 = 0, cnt = 0, gout_off = 0;
    std::vector<uint64_t> slice_len, out_bytes;
    const uint8_t *h_out = nullptr;  // the window's host slices (host-hashed groups read them)
    std::vector<uint64_t> h_off;     // per object: its slices at h_out + h_off
    std::vector<std::shared_ptr<PieceEvents>> pieces;  // per object: row pieces, or null (copied whole)
};
struct OpenGroup {
    bool open = false;
    size_t r = 0;                 // group buffer
    uint64_t out_off = 0, rows = 0, rows_cap = 0, bytes = 0;
    bool slots_used[CommitPipe::S] = {};
    std::vector<GroupSeg> segs;
};

// Open a group in the next group buffer: its previous group must be hashed (and copied out)
// before the slot streams write into it.  need_out / need_rows: what the first segment needs
// (a buffer grows only after the work queued on it has drained).
static int group_open(CommitPipe &P, OpenGroup &G, uint64_t need_out, uint64_t need_rows, uint64_t row_b) {
    constexpr int S = CommitPipe::S;
    const size_t r = P.groups % CommitPipe::R;
    if (P.gout[r]->cap < need_out || P.gcom[r]->cap < need_rows * row_b) {
        if (!P.grow_ok) return TE_ERR_INVALID_ARG;
        if (P.hashed_pending[r]) TE_HIP(hipEventSynchronize(P.ev_hashed[r]));
        TE_HIP(P.gout[r]->ensure(need_out));
        TE_HIP(P.gcom[r]->ensure(need_rows * row_b));
    }
    if (P.hashed_pending[r])
        for (int k = 0; k < S; k++) TE_HIP(hipStreamWaitEvent(P.ss[k], P.ev_hashed[r], 0));
    G.open = true;
    G.r = r;
    G.out_off = G.rows = G.bytes = 0;
    G.rows_cap = row_b ? P.gcom[r]->cap / row_b : 0;
    for (int k = 0; k < S; k++) G.slots_used[k] = false;
    G.segs.clear();
    return TE_OK;
}

// Encode group x of plan L into the open group (after its earlier segments): H2D, encode and D2H
// of the slices per copy window, rotating over the slot streams.  `last`: the caller's final group
// -- its encodes run ahead of the copies (one D2H per two encodes on a slot, the rest after the
// group's last encode), so its hashing, the only exposed one, starts about halfway through the
// group's copies.  `pieces` (a host-hashed group with pinned output): each large object's slices
// are copied out in row pieces with an event per piece (copy_out_pieces).  `slices_out` false (the
// data-verify pipeline): the slices stay in the group buffer, no D2H at all.
static int group_add(te_clay *c, const te_slicer_cfg *cfg, CommitPipe &P, OpenGroup &G, const CommitBatch &B,
                     const CommitPlan &L, size_t x, bool last, bool pieces = false, bool slices_out = true) {
    if (last || !slices_out) pieces = false;
    constexpr int S = CommitPipe::S;
    const size_t i = L.gcut[x], j = L.gcut[x + 1];
    const std::vector<size_t> &wc = L.wcut[x];
    uint64_t win_in_max = 16;
    for (size_t y = 0; y + 1 < wc.size(); y++) {
        uint64_t win_in = 16;
        for (size_t o = wc[y]; o < wc[y + 1]; o++) win_in += B.in_bytes(o);
        win_in_max = std::max(win_in_max, win_in);
    }
    for (int k = 0; k < S; k++)
        if (P.in[k]->cap < win_in_max) {
            if (!P.grow_ok) return TE_ERR_INVALID_ARG;
            TE_HIP(hipStreamSynchronize(P.ss[k]));
            TE_HIP(P.in[k]->ensure(win_in_max));
        }
    GroupSeg seg;
    seg.co = B.co;
    seg.obj0 = i;
    seg.row0 = G.rows;
    seg.cnt = j - i;
    seg.gout_off = G.out_off;
    uint8_t *gout = P.gout[G.r]->as<uint8_t>();
    std::deque<std::vector<CopyRun>> pend[S];
    int encs[S] = {};
    uint64_t dout = G.out_off;
    std::vector<te_object> local;
    std::vector<CopyRun> hin, hout;
    int rc = TE_OK;
    for (size_t y = 0; y + 1 < wc.size() && !rc; y++) {
        const size_t a = wc[y], b = wc[y + 1];
        const int k = (int)(P.w % S);
        window_layout(B.objs, B.out_bytes, a, b, 0, dout, local, hin, hout);
        if ((rc = copy_runs(hin, P.in[k]->as<uint8_t>(), B.h_data, hipMemcpyHostToDevice, P.ss[k]))) break;
        if ((rc = encode_enqueue(c, cfg, P.in[k]->as<uint8_t>(), local.data(), local.size(), gout, P.ss[k], false,
                                 P.arena[k])))
            break;
        if ((rc = hip_status(hipEventRecord(P.ev_enc[k], P.ss[k])))) break;
        if (pieces) {
            const uint64_t pb = d2h_piece_bytes();
            uint64_t od = dout;
            for (size_t o = a; o < b && !rc; o++) {
                std::shared_ptr<PieceEvents> pe;
                if (pb && B.slice_len[o] >= 2 * pb)
                    rc = copy_out_pieces(B.h_out + B.objs[o].out_off, gout + od, B.slice_len[o], B.n, c->device, P.ss[k], pe);
                else
                    rc = hip_status(hipMemcpyAsync(B.h_out + B.objs[o].out_off, gout + od, B.out_bytes[o],
                                                   hipMemcpyDeviceToHost, P.ss[k]));
                seg.pieces.push_back(std::move(pe));
                od += B.out_bytes[o];
            }
        } else if (slices_out) {
            pend[k].push_back(hout);
        }
        if (rc) break;
        if (slices_out && !pieces && (!last || ++encs[k] % 2 == 0)) {
            if ((rc = copy_runs(pend[k].front(), gout, B.h_out, hipMemcpyDeviceToHost, P.ss[k]))) break;
            pend[k].pop_front();
        }
        P.slot_used[k] = true;
        G.slots_used[k] = true;
        for (size_t o = a; o < b; o++) dout += B.out_bytes[o];
        P.w++;
    }
    for (int k = 0; k < S && !rc; k++) {
        for (; !pend[k].empty() && !rc; pend[k].pop_front())
            rc = copy_runs(pend[k].front(), gout, B.h_out, hipMemcpyDeviceToHost, P.ss[k]);
        if (!rc && G.slots_used[k]) rc = hip_status(hipEventRecord(P.ev_slot[k], P.ss[k]));
    }
    if (rc) return rc;
    seg.h_out = B.h_out;
    for (size_t o = i; o < j; o++) {
        seg.slice_len.push_back(B.slice_len[o]);
        seg.out_bytes.push_back(B.out_bytes[o]);
        seg.h_off.push_back(B.objs[o].out_off);
        G.bytes += B.objs[o].blob_len + B.out_bytes[o];
    }
    G.out_off = dout;
    G.rows += seg.cnt;
    G.segs.push_back(std::move(seg));
    return TE_OK;
}

// Hash the open group: once every slot stream has encoded its last window (the last windows' D2H
// overlaps the hashing: 11.9 -> 12.4-12.6 GiB/s, one box), one leaf/tree launch per run of equal
// slice lengths across all its segments, then the D2H of each segment's leaf hashes, roots and
// proofs into its window's host buffers.
// root_from_leaf_hashes::<height> and create_proof_from_leaf_hashes::<height> of n leaves
// (lib/crypto/src/merkle/tree.rs:344-358, 397-455) from one set of layers: odd layers padded with
// EMPTY_ROOTS[level], proof i = the sibling at each level.
static int host_tree(const uint8_t *leaf, uint32_t n, uint32_t height, uint8_t *root, uint8_t *proof) {
    if (height == 0 || height > TE_MAX_MERKLE_TREE_HEIGHT || n == 0) return TE_ERR_INVALID_ARG;
    std::vector<std::array<uint8_t, 32>> cur(n), next;
    for (uint32_t i = 0; i < n; i++) memcpy(cur[i].data(), leaf + (size_t)i * 32, 32);
    std::array<uint8_t, 32> empty;
    sha::empty_root(0, empty.data());
    for (uint32_t l = 0; l < height; l++) {
        if (cur.size() % 2) cur.push_back(empty);
        if (proof)
            for (uint32_t i = 0; i < n; i++)
                memcpy(proof + ((size_t)i * height + l) * 32, cur[(i >> l) ^ 1].data(), 32);
        next.resize(cur.size() / 2);
        for (size_t j = 0; j < next.size(); j++) sha::hash_pair(cur[2 * j].data(), cur[2 * j + 1].data(), next[j].data());
        cur.swap(next);
        std::array<uint8_t, 32> e2;
        sha::hash_pair(empty.data(), empty.data(), e2.data());
        empty = e2;
    }
    memcpy(root, cur[0].data(), 32);
    return TE_OK;
}

// Host-hashed close (host_hash.hpp):the group's slices are hashed from the host output buffers
// once their D2H copies have landed -- one pool task per te_host_hash_lanes slices of an object
// (interleaved, hh::hash_leaves), the object's root and proofs by whichever of its tasks finishes
// last.  The group buffer is free as soon as the copies are
// done.  Returns the job the window tickets wait for.
static int group_close_host(CommitPipe &P, OpenGroup &G, uint32_t n, uint32_t height, int device,
                            std::shared_ptr<hh::Job> &job) {
    constexpr int S = CommitPipe::S;
    if (!G.open) return TE_OK;
    G.open = false;
    for (int k = 0; k < S; k++)
        if (G.slots_used[k]) TE_HIP(hipStreamWaitEvent(P.hs, P.ev_slot[k], 0));
    TE_HIP(hipEventRecord(P.ev_hashed[G.r], P.hs));
    P.hashed_pending[G.r] = true;
    P.groups++;
    hipEvent_t landed = nullptr;
    TE_HIP(hipEventCreateWithFlags(&landed, hipEventDisableTiming | hipEventBlockingSync));
    if (hipError_t e = hipEventRecord(landed, P.hs); e != hipSuccess) {
        (void)hipEventDestroy(landed);
        return hip_status(e);
    }
    job = std::make_shared<hh::Job>();
    // objects copied out in row pieces hash piece by piece as the pieces land (their tasks go to
    // the workers at once and wait on the piece events); the rest once the group's copies are done
    std::vector<std::function<void()>> tasks, streamed;
    const uint32_t lanes = (uint32_t)hh::Pool::get().lanes();
    for (const GroupSeg &sg : G.segs) {
        for (size_t q = 0; q < sg.cnt; q++) {
            const uint8_t *slices = sg.h_out + sg.h_off[q];
            const uint64_t slen = sg.slice_len[q];
            uint8_t *leaf = sg.co.leaf + (sg.obj0 + q) * (uint64_t)n * TE_HASH_SIZE;
            uint8_t *root = sg.co.root + (sg.obj0 + q) * TE_HASH_SIZE;
            uint8_t *proof = sg.co.proof ? sg.co.proof + (sg.obj0 + q) * (uint64_t)n * height * TE_HASH_SIZE : nullptr;
            auto left = std::make_shared<std::atomic<uint32_t>>(n);
            std::shared_ptr<PieceEvents> pe = q < sg.pieces.size() ? sg.pieces[q] : nullptr;
            // one task per `lanes` slices of the object (LeafLanes interleaves them)
            for (uint32_t i0 = 0; i0 < n; i0 += lanes)
                (pe ? streamed : tasks).push_back([=, j = job.get()] {
                    const uint32_t L = std::min(lanes, n - i0);
                    const uint8_t *src[hh::kMaxLanes];
                    uint8_t *dst[hh::kMaxLanes];
                    for (uint32_t l = 0; l < L; l++) {
                        src[l] = slices + (uint64_t)(i0 + l) * slen;
                        dst[l] = leaf + (uint64_t)(i0 + l) * TE_HASH_SIZE;
                    }
                    int rc = TE_OK;
                    hh::LeafLanes h((int)L);
                    if (!pe) {
                        h.update(src, slen);
                    } else {
                        (void)hipSetDevice(pe->device);
                        const uint8_t *at[hh::kMaxLanes];
                        for (size_t p = 0; p < pe->ev.size() && !rc; p++) {
                            rc = hip_status(event_wait_poll(pe->ev[p]));
                            for (uint32_t l = 0; l < L; l++) at[l] = src[l] + pe->beg[p];
                            if (!rc) h.update(at, pe->beg[p + 1] - pe->beg[p]);
                        }
                    }
                    h.final(dst);
                    if (left->fetch_sub(L) == L && !rc) rc = host_tree(leaf, n, height, root, proof);
                    j->done(rc);
                });
        }
    }
    job->add((int64_t)(tasks.size() + streamed.size()));
    G.segs.clear();
    if (!streamed.empty()) hh::Pool::get().submit_after(nullptr, device, std::move(streamed));
    if (tasks.empty()) {
        (void)hipEventDestroy(landed);
        return TE_OK;
    }
    hh::Pool::get().submit_after(landed, device, std::move(tasks));
    return TE_OK;
}

static int group_close(CommitPipe &P, OpenGroup &G, uint32_t n, uint32_t height, uint64_t leaf_b, uint64_t proof_b) {
    constexpr int S = CommitPipe::S;
    if (!G.open) return TE_OK;
    G.open = false;
    for (int k = 0; k < S; k++)
        if (G.slots_used[k]) TE_HIP(hipStreamWaitEvent(P.hs, P.ev_enc[k], 0));
    uint8_t *gout = P.gout[G.r]->as<uint8_t>(), *dc = P.gcom[G.r]->as<uint8_t>();
    const uint64_t root_at = G.rows_cap * leaf_b, proof_at = root_at + G.rows_cap * TE_HASH_SIZE;
    // flatten the rows: (slice length, out bytes, slice offset) in group order
    struct Row { uint64_t slen, obytes, off; };
    std::vector<Row> rows;
    rows.reserve(G.rows);
    for (const GroupSeg &sg : G.segs) {
        uint64_t off = sg.gout_off;
        for (size_t q = 0; q < sg.cnt; q++) {
            rows.push_back({sg.slice_len[q], sg.out_bytes[q], off});
            off += sg.out_bytes[q];
        }
    }
    for (size_t o = 0; o < rows.size();) {
        size_t e = o + 1;
        while (e < rows.size() && rows[e].slen == rows[o].slen) e++;
        CommitArgs ca{};
        ca.slices = gout + rows[o].off;
        ca.obj_stride = rows[o].obytes;
        ca.slice_len = rows[o].slen;
        ca.n = n;
        ca.nobj = (uint32_t)(e - o);
        ca.height = height;
        ca.leaf = dc + o * leaf_b;
        ca.root = dc + root_at + o * TE_HASH_SIZE;
        ca.proof = proof_b ? dc + proof_at + o * proof_b : nullptr;
        TE_HIP(launch_commit(ca, P.hs));
        o = e;
    }
    for (const GroupSeg &sg : G.segs) {
        const struct { uint8_t *h; uint64_t d, len; } back[3] = {
            {sg.co.leaf + sg.obj0 * leaf_b, sg.row0 * leaf_b, sg.cnt * leaf_b},
            {sg.co.root + sg.obj0 * TE_HASH_SIZE, root_at + sg.row0 * TE_HASH_SIZE, sg.cnt * TE_HASH_SIZE},
            {sg.co.proof ? sg.co.proof + sg.obj0 * proof_b : nullptr, proof_at + sg.row0 * proof_b, sg.cnt * proof_b}};
        for (const auto &bk : back)
            if (bk.h && bk.len) TE_HIP(hipMemcpyAsync(bk.h, dc + bk.d, bk.len, hipMemcpyDeviceToHost, P.hs));
    }
    for (int k = 0; k < S; k++)
        if (G.slots_used[k]) TE_HIP(hipStreamWaitEvent(P.hs, P.ev_slot[k], 0));
    TE_HIP(hipEventRecord(P.ev_hashed[G.r], P.hs));
    P.hashed_pending[G.r] = true;
    P.groups++;
    G.segs.clear();
    return TE_OK;
}

// te_verify_data_batch_host's side of a call: the expected commitments and the results, all in one
// page-locked staging block (a copy to or from the caller's pageable arrays would make the host
// wait for the hashing stream once per group) that the call fills before its first group and
// empties after its last.
struct VerifyData {
    const uint8_t *exp_root = nullptr, *exp_leaf = nullptr;  // nobj * 32, nobj * n * 32 (or null)
    uint8_t *root = nullptr;                                 // nobj * 32
    uint64_t *mask = nullptr;                                // nobj (or null: not asked for)
    uint32_t *ok = nullptr;                                  // nobj
    te_verify_data_stats *st = nullptr;
};
// A verify group's rows in its commitment buffer: leaf hashes, expected leaves, expected roots,
// observed roots, masks, verdicts -- each an array over the buffer's rows_cap rows.
static uint64_t verify_row_bytes(uint64_t leaf_b) { return 2 * leaf_b + 2 * TE_HASH_SIZE + 8 + 4; }

// group_close for the data-verify pipeline: the leaf launches per run of equal slice lengths, no
// tree and no proofs, then one root-check launch over the group's rows and the D2H of its results
// -- the group's only copy back.
static int group_close_verify(CommitPipe &P, OpenGroup &G, uint32_t n, uint32_t height, uint64_t leaf_b,
                              const VerifyData &vd) {
    constexpr int S = CommitPipe::S;
    if (!G.open) return TE_OK;
    G.open = false;
    uint8_t *gout = P.gout[G.r]->as<uint8_t>(), *dc = P.gcom[G.r]->as<uint8_t>();
    const uint64_t cap = G.rows_cap;
    const uint64_t xleaf_at = cap * leaf_b, xroot_at = 2 * cap * leaf_b, root_at = xroot_at + cap * TE_HASH_SIZE,
                   mask_at = root_at + cap * TE_HASH_SIZE, ok_at = mask_at + cap * 8;
    // the expected commitments go up while the slot streams still encode
    for (const GroupSeg &sg : G.segs) {
        TE_HIP(hipMemcpyAsync(dc + xroot_at + sg.row0 * TE_HASH_SIZE, vd.exp_root + sg.obj0 * TE_HASH_SIZE,
                              sg.cnt * TE_HASH_SIZE, hipMemcpyHostToDevice, P.hs));
        vd.st->h2d_expected_bytes += sg.cnt * TE_HASH_SIZE;
        if (vd.exp_leaf) {
            TE_HIP(hipMemcpyAsync(dc + xleaf_at + sg.row0 * leaf_b, vd.exp_leaf + sg.obj0 * leaf_b, sg.cnt * leaf_b,
                                  hipMemcpyHostToDevice, P.hs));
            vd.st->h2d_expected_bytes += sg.cnt * leaf_b;
        }
    }
    for (int k = 0; k < S; k++)
        if (G.slots_used[k]) TE_HIP(hipStreamWaitEvent(P.hs, P.ev_enc[k], 0));
    uint64_t o = 0;
    for (const GroupSeg &sg : G.segs) {
        uint64_t off = sg.gout_off;
        for (size_t q = 0; q < sg.cnt;) {
            size_t e = q + 1;
            uint64_t run = sg.out_bytes[q];
            while (e < sg.cnt && sg.slice_len[e] == sg.slice_len[q]) run += sg.out_bytes[e++];
            CommitArgs ca{};
            ca.slices = gout + off;
            ca.obj_stride = sg.out_bytes[q];
            ca.slice_len = sg.slice_len[q];
            ca.n = n;
            ca.nobj = (uint32_t)(e - q);
            ca.height = height;
            ca.leaf = dc + o * leaf_b;
            TE_HIP(launch_commit(ca, P.hs));
            vd.st->leaf_launches += commit_leaf_launches(ca.slice_len);
            o += e - q;
            off += run;
            q = e;
        }
    }
    RootCheckArgs ra{};
    ra.leaf = dc;
    ra.expected_root = dc + xroot_at;
    ra.expected_leaf = vd.exp_leaf ? dc + xleaf_at : nullptr;
    ra.root = dc + root_at;
    ra.ok = reinterpret_cast<uint32_t *>(dc + ok_at);
    ra.bad_leaf_mask = vd.exp_leaf && vd.mask ? reinterpret_cast<uint64_t *>(dc + mask_at) : nullptr;
    ra.nobj = G.rows;
    ra.n = n;
    ra.height = height;
    TE_HIP(launch_root_check(ra, P.hs));
    vd.st->root_check_launches++;
    for (const GroupSeg &sg : G.segs) {
        const struct { void *h; uint64_t d, len; } back[3] = {
            {vd.root ? vd.root + sg.obj0 * TE_HASH_SIZE : nullptr, root_at + sg.row0 * TE_HASH_SIZE, sg.cnt * TE_HASH_SIZE},
            {vd.ok + sg.obj0, ok_at + sg.row0 * 4, sg.cnt * 4},
            {ra.bad_leaf_mask ? vd.mask + sg.obj0 : nullptr, mask_at + sg.row0 * 8, sg.cnt * 8}};
        for (const auto &bk : back)
            if (bk.h && bk.len) {
                TE_HIP(hipMemcpyAsync(bk.h, dc + bk.d, bk.len, hipMemcpyDeviceToHost, P.hs));
                vd.st->d2h_bytes += bk.len;
            }
    }
    for (int k = 0; k < S; k++)
        if (G.slots_used[k]) TE_HIP(hipStreamWaitEvent(P.hs, P.ev_slot[k], 0));
    TE_HIP(hipEventRecord(P.ev_hashed[G.r], P.hs));
    P.hashed_pending[G.r] = true;
    P.groups++;
    G.segs.clear();
    return TE_OK;
}

// Who hashes a group (te_set_commit_hashing / te_stream_writer_set_hashing, TE_HASH_*).  A leaf
// launch hashes one slice per lane at ~24 MB/s per lane (715,048 B in ~29.5 ms)
// whatever the number of slices up to ~64k of them; the host pool hashes at its measured
// per-thread rate (SHA extensions: 1-2 GB/s) times its threads.
// The device wins for very many short slices (tens of thousands of small objects' slices per
// group); with the contended device rate (below) the host pool takes the 4 MiB objects' groups too
// (r05: host 12.4-12.9 GiB/s against device 7.5-12.2 for 1024 x 4 MiB, every group size and
// window size measured) and the SDK's 64 MiB chunks (~9.7 MB slices: ~0.4 s per leaf launch).
std::atomic<int> g_commit_hashing{TE_HASH_AUTO};
bool host_hash_wins(int mode, uint64_t streams, uint64_t max_slice, uint64_t slice_bytes) {
    if (mode == TE_HASH_HOST) return true;
    if (mode == TE_HASH_DEVICE) return false;
    // a leaf lane hashes its slice at ~24 MB/s alone, but a group's hashing runs beside the next
    // groups' encodes and copies, which cut that to ~8 MB/s (r05 group traces: 90-128 ms per
    // 715 KB-slice group against 29 ms alone; with 24 MB/s here the 4 GiB groups went to the device
    // and the one-shot call ran 7.5 GiB/s against 12.4 host-hashed)
    const double dev_s = (double)max_slice / 8e6 * std::max(1.0, (double)streams / 65536.0);
    const hh::Pool &pool = hh::Pool::get();
    const double host_s = (double)slice_bytes / (pool.thread_rate() * pool.threads());
    return host_s < dev_s;
}

// The bytes a group of plan L needs in a group buffer, and its commitment rows.
static void group_need(const CommitBatch &B, const CommitPlan &L, size_t x, uint64_t &out, uint64_t &rows) {
    out = 0;
    for (size_t o = L.gcut[x]; o < L.gcut[x + 1]; o++) out += B.out_bytes[o];
    rows = L.gcut[x + 1] - L.gcut[x];
}

// The streams of the encode + commit pipeline (handle locked, its device current): two slot
// streams and the hashing stream -- the handle's pipe streams and its own stream.
// Measurement option (TEC_DEBUG_KNOBS=1 TEC_COMMIT_HASH_CUS=n): hash on n CUs of their own and
// copy / encode on the rest (hipExtStreamCreateWithCUMask), so no leaf wave shares a SIMD with an
// encode wave.  Not the default: it measured within the run-to-run spread (scripts/sw_probe.py,
// DESIGN §4.4), and CU-masked streams are blocking streams (they synchronise with the null stream).
static int commit_streams(te_clay *c, hipStream_t ss[2], hipStream_t &hs) {
    int hash_cus = 0;
    if (const char *e = tec_knob("TEC_COMMIT_HASH_CUS")) hash_cus = atoi(e);
    if (hash_cus > 0 && !c->cm_tried) {
        c->cm_tried = true;
        hipDeviceProp_t prop{};
        int ncu = 0;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess) ncu = prop.multiProcessorCount;
        if (ncu > 2 * hash_cus) {
            const uint32_t words = (uint32_t)(ncu + 31) / 32;
            std::vector<uint32_t> hm(words, 0), sm(words, 0);
            for (int i = 0; i < ncu; i++) (i < hash_cus ? hm : sm)[i / 32] |= 1u << (i % 32);
            bool ok = hipExtStreamCreateWithCUMask(&c->cm_hs, words, hm.data()) == hipSuccess;
            for (int k = 0; k < 2 && ok; k++) ok = hipExtStreamCreateWithCUMask(&c->cm_ss[k], words, sm.data()) == hipSuccess;
            if (!ok)
                for (hipStream_t *ps : {&c->cm_ss[0], &c->cm_ss[1], &c->cm_hs}) {
                    if (*ps) (void)hipStreamDestroy(*ps);
                    *ps = nullptr;
                }
            (void)hipGetLastError();
        }
    }
    if (hash_cus > 0 && c->cm_hs) {
        ss[0] = c->cm_ss[0];
        ss[1] = c->cm_ss[1];
        hs = c->cm_hs;
        return TE_OK;
    }
    for (int k = 0; k < 2; k++)
        if (!c->pipe[k].s) TE_HIP(hipStreamCreateWithFlags(&c->pipe[k].s, hipStreamNonBlocking));
    if (!c->stream) TE_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    ss[0] = c->pipe[0].s;
    ss[1] = c->pipe[1].s;
    hs = c->stream;
    return TE_OK;
}

static int encode_commit_host_impl(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data,
                                   const te_object *objs, size_t nobj, uint8_t *h_out, size_t group_bytes,
                                   const CommitOut &co, const VerifyData *vd = nullptr) {
    // vd set: the data-verify form -- the same plan, streams and buffers; no h_out, the slices stay
    // in the group buffers, every group hashed on the device and closed by group_close_verify
    if (!c || !cfg || (!objs && nobj) || (nobj && (!h_data || (!h_out && !vd)))) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    if (group_bytes == 0) group_bytes = (size_t)4 << 30;
    const uint64_t copy_bytes = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)128 << 20, group_bytes / 8));
    CommitBatch B;
    B.h_data = h_data;
    B.objs = objs;
    B.nobj = nobj;
    B.h_out = h_out;
    B.co = co;
    int rc = commit_prepare(c, B);
    if (rc) return rc;
    CommitPlan L;
    commit_plan(B, group_bytes, copy_bytes, L);
    const uint64_t row_b = vd ? verify_row_bytes(B.leaf_b) : B.leaf_b + TE_HASH_SIZE + B.proof_b;
    const uint64_t commit_cap = L.max_group_obj * row_b;

    // (a verify call holds the handle's lock already: it stages its commitments under it)
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    if (!vd) lk.lock();
    c->els = te_encode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    // three streams: two slot streams and the hashing stream (a fifth stream beside the caller's
    // shared a hardware queue with a slot stream in bench.py: 9.5 against 12.1 GiB/s)
    CommitPipe P;
    static_assert(CommitPipe::S == 2, "commit_streams makes two slot streams");
    if ((rc = commit_streams(c, P.ss, P.hs))) return rc;
    for (int k = 0; k < CommitPipe::S; k++) {
        P.in[k] = &c->pipe[k].in;
        P.arena[k] = &c->pipe[k].arena;
    }
    for (int r = 0; r < CommitPipe::R; r++) {
        P.gout[r] = &c->pipe[r].out;
        P.gcom[r] = &c->pipe[r].commit;
    }
    // every buffer sized up front (the pipeline never reallocates under queued work)
    const size_t ngroups = L.gcut.size() - 1, nring = std::min<size_t>(CommitPipe::R, ngroups);
    for (int k = 0; k < CommitPipe::S && nobj; k++) TE_HIP(P.in[k]->ensure(L.max_win_in));
    for (size_t r = 0; r < nring; r++) {
        TE_HIP(P.gout[r]->ensure(L.max_group_out));
        TE_HIP(P.gcom[r]->ensure(commit_cap));
    }
    rc = P.make_events();
    const bool pinned_out = !vd && host_pinned(h_out);
    if (vd) {
        vd->st->objects = nobj;
        vd->st->groups = L.gcut.size() - 1;
        for (const auto &wc : L.wcut) vd->st->windows += wc.size() - 1;
        for (size_t o = 0; o < nobj; o++) vd->st->h2d_bytes += objs[o].blob_len;
    }
    OpenGroup G;
    std::vector<std::shared_ptr<hh::Job>> jobs;
    for (size_t x = 0; x < ngroups && rc == TE_OK; x++) {
        uint64_t need_out, need_rows;
        group_need(B, L, x, need_out, need_rows);
        uint64_t max_slice = 0;
        for (size_t o = L.gcut[x]; o < L.gcut[x + 1]; o++) max_slice = std::max<uint64_t>(max_slice, B.slice_len[o]);
        const bool host = !vd && host_hash_wins(g_commit_hashing.load(), need_rows * B.n, max_slice, need_out);
        static const bool trace = tec_knob("TEC_COMMIT_TRACE") != nullptr;  // measurement: the choice per group
        if (trace)
            fprintf(stderr, "[tapeec] commit group %zu/%zu: %llu objects, %llu slice bytes, %s hashing (pool %.2f GB/s x %d)\n",
                    x + 1, ngroups, (unsigned long long)need_rows, (unsigned long long)need_out, host ? "host" : "device",
                    hh::Pool::get().thread_rate() / 1e9, hh::Pool::get().threads());
        const auto t0 = std::chrono::steady_clock::now();
        rc = group_open(P, G, need_out, need_rows, row_b);
        const auto t1 = std::chrono::steady_clock::now();
        if (!rc) rc = group_add(c, cfg, P, G, B, L, x, x + 1 == ngroups && !host, host && pinned_out, !vd);
        const auto t2 = std::chrono::steady_clock::now();
        if (!rc && vd) {
            rc = group_close_verify(P, G, B.n, B.co.height, B.leaf_b, *vd);
        } else if (!rc && host) {
            jobs.emplace_back();
            rc = group_close_host(P, G, B.n, B.co.height, c->device, jobs.back());
        } else if (!rc) {
            rc = group_close(P, G, B.n, B.co.height, B.leaf_b, B.proof_b);
        }
        if (trace) {  // host time enqueueing the group (a long one is a host wait inside)
            const auto t3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "[tapeec]   host ms: open %.2f add %.2f close %.2f\n", ms(t0, t1), ms(t1, t2), ms(t2, t3));
        }
    }
    for (int k = 0; k < CommitPipe::S; k++) {
        const int r2 = sync_sleep(P.ss[k]);
        if (rc == TE_OK) rc = r2;
    }
    const int r2 = sync_sleep(P.hs);
    if (rc == TE_OK) rc = r2;
    for (auto &j : jobs) {  // host-hashed groups: their tasks read the output buffers
        const int r3 = j ? j->wait() : TE_OK;
        if (rc == TE_OK) rc = r3;
    }
    P.destroy_events();
    return rc;
}

// ------------------------------------------------------------------------------------------
// te_stream_writer: the ordered, asynchronous window submission of the SDK's stream writer
// (sdk/src/stream/write.rs:332-362: up to min(cores, 4) chunk encodes in flight, handed on in
// order through FuturesOrdered), over one or more device-bound handles.  Window t goes to handle
// (t - 1) mod ncoders and is enqueued there without blocking; each handle's CommitPipe persists
// across windows, so window t+1's encode overlaps window t's hashing and copies.  te_stream_wait
// completes windows in submission order.
// ------------------------------------------------------------------------------------------
struct te_stream_writer {
    struct Dev {
        te_clay *c = nullptr;
        int device = 0;
        CommitPipe P;
        hipStream_t ss[CommitPipe::S] = {}, hs = nullptr;
        DevBuf in[CommitPipe::S], gout[CommitPipe::R], gcom[CommitPipe::R];
        Arena arena[CommitPipe::S];
        // windows share a hashing group until it holds group_bytes / 2 (a leaf launch costs one
        // slice's SHA-256 whatever its size: one launch per window capped small windows at
        // 7.3-7.5 GiB/s); tickets whose last group is still open complete when it closes
        OpenGroup G;
        bool G_host = false;        // the open group is hashed on the host (host_hash.hpp)
        std::vector<uint64_t> pend;
    };
    struct Ticket {
        int dev = -1;
        hipEvent_t done = nullptr;  // its groups' device work (hashing or the copies host hashing reads)
        std::vector<std::shared_ptr<hh::Job>> jobs;  // host-hashed groups holding its objects
        int rc = TE_OK;
        bool pending = false;  // its last group is the device's open group
    };
    std::vector<std::unique_ptr<Dev>> devs;
    te_slicer_cfg cfg{};
    uint32_t height = 0;
    bool proofs = true;
    uint64_t group_bytes = 0;
    int hashing = TE_HASH_AUTO;
    std::mutex mu;
    std::mutex wait_mu;  // te_stream_wait calls complete tickets one caller at a time
    uint64_t next = 1;                   // next ticket
    std::map<uint64_t, Ticket> tickets;  // submitted, not yet waited
};

namespace {
uint64_t writer_row_bytes(const te_stream_writer &w, const te_stream_writer::Dev &d, uint64_t &leaf_b, uint64_t &proof_b) {
    leaf_b = (uint64_t)d.c->h.n * TE_HASH_SIZE;
    proof_b = leaf_b * w.height;  // proofs always computed (a window may ask for them)
    return leaf_b + TE_HASH_SIZE + proof_b;
}
// Hash the device's open group and complete the tickets waiting on it.  Called with w.mu held.
int writer_close(te_stream_writer &w, te_stream_writer::Dev &d) {
    int rc = TE_OK;
    std::shared_ptr<hh::Job> job;
    if (d.G.open) {
        uint64_t leaf_b, proof_b;
        (void)writer_row_bytes(w, d, leaf_b, proof_b);
        std::lock_guard<std::mutex> lk(d.c->mu);
        DeviceGuard dg(d.device);
        rc = hip_status(dg.err);
        if (!rc && d.G_host)
            rc = group_close_host(d.P, d.G, (uint32_t)d.c->h.n, w.height, d.device, job);
        else if (!rc)
            rc = group_close(d.P, d.G, (uint32_t)d.c->h.n, w.height, leaf_b, proof_b);
        d.G.open = false;
    }
    for (uint64_t t : d.pend) {
        auto it = w.tickets.find(t);
        if (it == w.tickets.end()) continue;
        te_stream_writer::Ticket &T = it->second;
        T.pending = false;
        if (!rc) {
            // after the group's hashing and copies (a ticket spanning several groups re-records)
            DeviceGuard dg(d.device);
            // blocking: te_stream_wait sleeps in hipEventSynchronize instead of spinning a core the
            // host hashing pool could use (the GPU's host share is 16 CPUs of time on the pool)
            if (!T.done) rc = hip_status(hipEventCreateWithFlags(&T.done, hipEventDisableTiming | hipEventBlockingSync));
            if (!rc) rc = hip_status(hipEventRecord(T.done, d.hs));
        }
        if (job) T.jobs.push_back(job);
        if (rc && !T.rc) T.rc = rc;
    }
    d.pend.clear();
    return rc;
}
int writer_drain(te_stream_writer::Dev &d) {
    DeviceGuard dg(d.device);
    TE_HIP(dg.err);
    int rc = TE_OK;
    for (int k = 0; k < CommitPipe::S; k++)
        if (d.ss[k]) {
            const int r = sync_sleep(d.ss[k]);
            if (!rc) rc = r;
        }
    if (d.hs) {
        const int r = sync_sleep(d.hs);
        if (!rc) rc = r;
    }
    return rc;
}
void writer_release(te_stream_writer::Dev &d) {
    DeviceGuard dg(d.device);
    (void)writer_drain(d);
    for (auto &b : d.in) b.release();
    for (auto &b : d.gout) b.release();
    for (auto &b : d.gcom) b.release();
    for (auto &a : d.arena) a.release();
    d.P.destroy_events();  // the streams are the handle's (released with it)
}
}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI: compute entry points
// ------------------------------------------------------------------------------------------
extern "C" {

int te_encode_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_data, const te_object *objs,
                           size_t nobj, uint8_t *d_out, void *stream) {
    if (!c || !cfg || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->els = te_encode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return encode_enqueue(c, cfg, d_data, objs, nobj, d_out, (hipStream_t)stream, false);
}

int te_encode_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data, const te_object *objs,
                         size_t nobj, uint8_t *h_out, size_t window_bytes) {
    return encode_host_impl(c, cfg, h_data, objs, nobj, h_out, window_bytes);
}

int te_encode_commit_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data, const te_object *objs,
                                size_t nobj, uint8_t *h_out, uint32_t height, uint8_t *h_leaf_hashes,
                                uint8_t *h_roots, uint8_t *h_proofs, size_t window_bytes) {
    if (!c || !h_leaf_hashes || !h_roots || height == 0 || height > TE_MAX_MERKLE_TREE_HEIGHT)
        return TE_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)c->h.n;
    if (n > TE_COMMIT_MAX_LEAVES) return TE_ERR_INVALID_ARG;
    if (height < 64 && (uint64_t)n > (1ull << height)) return TE_ERR_MERKLE_TREE_FULL;
    const CommitOut co{h_leaf_hashes, h_roots, h_proofs, height};
    return encode_commit_host_impl(c, cfg, h_data, objs, nobj, h_out, window_bytes, co);
}
int te_stream_writer_new(te_clay *const *coders, size_t ncoders, const te_slicer_cfg *cfg, uint32_t height,
                         size_t group_bytes, te_stream_writer **out) {
    if (!out) return TE_ERR_INVALID_ARG;
    *out = nullptr;
    if (!coders || ncoders == 0 || !cfg || height == 0 || height > TE_MAX_MERKLE_TREE_HEIGHT) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    for (size_t i = 0; i < ncoders; i++) {
        if (!coders[i]) return TE_ERR_INVALID_ARG;
        const uint32_t n = (uint32_t)coders[i]->h.n;
        if (n > TE_COMMIT_MAX_LEAVES) return TE_ERR_INVALID_ARG;
        if (height < 64 && (uint64_t)n > (1ull << height)) return TE_ERR_MERKLE_TREE_FULL;
    }
    auto *w = new (std::nothrow) te_stream_writer();
    if (!w) return TE_ERR_OUT_OF_MEMORY;
    w->cfg = *cfg;
    w->height = height;
    w->group_bytes = group_bytes ? group_bytes : ((size_t)8 << 30);  // see te_stream_writer_new's header note
    w->hashing = g_commit_hashing.load();
    int rc = TE_OK;
    for (size_t i = 0; i < ncoders && !rc; i++) {
        auto d = std::make_unique<te_stream_writer::Dev>();
        d->c = coders[i];
        d->device = coders[i]->device;
        DeviceGuard dg(d->device);
        if ((rc = hip_status(dg.err))) break;
        {
            // the handle's own slot and hashing streams (created if missing): the process has four
            // hardware queues, and streams of their own would put the writer's slot and hashing
            // streams on shared queues behind other streams' work (te_encode_commit_batch_host's
            // note); calls on the handle serialise with the writer's windows on them
            te_clay *c = coders[i];
            std::lock_guard<std::mutex> lk(c->mu);
            rc = commit_streams(c, d->ss, d->hs);
        }
        CommitPipe &P = d->P;
        P.hs = d->hs;
        for (int k = 0; k < CommitPipe::S; k++) {
            P.ss[k] = d->ss[k];
            P.in[k] = &d->in[k];
            P.arena[k] = &d->arena[k];
        }
        for (int r = 0; r < CommitPipe::R; r++) {
            P.gout[r] = &d->gout[r];
            P.gcom[r] = &d->gcom[r];
        }
        P.grow_ok = true;  // buffers grow on demand, after the work queued on them has drained
        if (!rc) rc = P.make_events();
        w->devs.push_back(std::move(d));
    }
    if (rc) {
        te_stream_writer_free(w);
        return rc;
    }
    *out = w;
    return TE_OK;
}

int te_stream_submit(te_stream_writer *w, const uint8_t *h_data, const te_object *objs, size_t nobj, uint8_t *h_out,
                     uint8_t *h_leaf_hashes, uint8_t *h_roots, uint8_t *h_proofs, uint64_t *ticket) {
    if (!w || !ticket || (!objs && nobj) || (nobj && (!h_data || !h_out || !h_leaf_hashes || !h_roots)))
        return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(w->mu);
    const uint64_t t = w->next++;
    *ticket = t;
    te_stream_writer::Ticket &T = w->tickets[t];
    T.dev = (int)((t - 1) % w->devs.size());
    te_stream_writer::Dev &d = *w->devs[(size_t)T.dev];
    te_clay *c = d.c;
    CommitBatch B;
    B.h_data = h_data;
    B.objs = objs;
    B.nobj = nobj;
    B.h_out = h_out;
    B.co = CommitOut{h_leaf_hashes, h_roots, h_proofs, w->height};
    // every per-object check happens here, before the window touches the device's open group
    int rc = commit_prepare(c, B);
    if (!rc) {  // the window's group_add passes below sum into it
        std::lock_guard<std::mutex> lk(c->mu);
        c->els = te_encode_launch_stats{};
    }
    auto pend_t = [&] {
        if (d.pend.empty() || d.pend.back() != t) d.pend.push_back(t);
        T.pending = true;
    };
    if (!rc && nobj == 0) {  // completes after everything queued before it
        pend_t();
        rc = writer_close(*w, d);
    } else if (!rc) {
        CommitPlan L;
        const uint64_t copy_bytes = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)128 << 20, w->group_bytes / 8));
        commit_plan(B, w->group_bytes, copy_bytes, L);
        uint64_t leaf_b, proof_b;
        const uint64_t row_b = writer_row_bytes(*w, d, leaf_b, proof_b);
        B.leaf_b = leaf_b;
        B.proof_b = proof_b;
        // host or device hashing, per window (host_hash_wins): the SDK's 64 MiB chunks hash on the
        // host, each window a group of its own closed at once; batches of small objects share
        // device groups
        uint64_t max_slice = 0, slice_bytes = 0;
        for (size_t o = 0; o < nobj; o++) {
            max_slice = std::max<uint64_t>(max_slice, B.slice_len[o]);
            slice_bytes += B.out_bytes[o];
        }
        const bool host = host_hash_wins(w->hashing, (uint64_t)nobj * B.n, max_slice, slice_bytes);
        const bool pinned_out = host && host_pinned(h_out);
        if (d.G.open && d.G_host != host) rc = writer_close(*w, d);
        const uint64_t close_at = std::max<uint64_t>(1, w->group_bytes / 2);
        for (size_t x = 0; x + 1 < L.gcut.size() && !rc; x++) {
            uint64_t need_out, need_rows, gbytes = 0;
            group_need(B, L, x, need_out, need_rows);
            for (size_t o = L.gcut[x]; o < L.gcut[x + 1]; o++) gbytes += B.objs[o].blob_len + B.out_bytes[o];
            OpenGroup &G = d.G;
            if (G.open && (G.out_off + need_out > d.P.gout[G.r]->cap || G.rows + need_rows > G.rows_cap ||
                           G.bytes + gbytes > w->group_bytes))
                rc = writer_close(*w, d);  // earlier windows' tickets complete with it
            if (rc) break;
            pend_t();
            {
                std::lock_guard<std::mutex> lk(c->mu);
                DeviceGuard dg(d.device);
                rc = c->device != d.device ? TE_ERR_INVALID_ARG : hip_status(dg.err);  // handle re-bound under the writer
                if (!rc && !G.open) {
                    // a group buffer holds a full group's slices (group_bytes of objects + slices,
                    // ~3/4 of it slices for Clay(20, 7)) and its commitment rows; a host-hashed
                    // group holds one window
                    const uint64_t want_out = host ? need_out : std::max<uint64_t>(need_out, w->group_bytes - w->group_bytes / 4);
                    const uint64_t want_rows = host ? need_rows : std::max<uint64_t>(need_rows, 4096);
                    rc = group_open(d.P, G, want_out, want_rows, row_b);
                    d.G_host = host;
                }
                // on failure the group keeps its earlier segments (group_add adds one only on
                // success): the earlier windows still complete below
                if (!rc) rc = group_add(c, &w->cfg, d.P, G, B, L, x, false, host && pinned_out);
            }
            if (!rc && (host || G.bytes >= close_at)) rc = writer_close(*w, d);  // pending windows complete with it
        }
    }
    if (rc) {
        // only this window fails: the earlier windows of the open group are hashed and complete
        // normally; then the device is drained, since work already enqueued for this window may
        // still read or write its host buffers
        d.pend.erase(std::remove(d.pend.begin(), d.pend.end(), t), d.pend.end());
        T.pending = false;
        (void)writer_close(*w, d);
        (void)writer_drain(d);
        for (auto &j : T.jobs) (void)j->wait();
        T.jobs.clear();
        if (T.done) (void)hipEventDestroy(T.done);
        T.done = nullptr;
    }
    T.rc = rc;
    return rc;
}

int te_stream_wait(te_stream_writer *w, uint64_t ticket) {
    if (!w || ticket == 0) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> wg(w->wait_mu);
    int first = TE_OK;
    for (;;) {
        te_stream_writer::Ticket T;
        {
            std::lock_guard<std::mutex> g(w->mu);
            if (ticket >= w->next) return TE_ERR_INVALID_ARG;  // never submitted
            if (w->tickets.empty() || w->tickets.begin()->first > ticket) return first;
            if (w->tickets.begin()->second.pending) {  // its group is still open: hash it now
                te_stream_writer::Dev &d = *w->devs[(size_t)w->tickets.begin()->second.dev];
                const int r = writer_close(*w, d);
                if (r) (void)writer_drain(d);
            }
            // claimed: only this caller (wait_mu) completes it
            T = std::move(w->tickets.begin()->second);
            w->tickets.erase(w->tickets.begin());
        }
        int rc = T.rc;
        if (T.done) {
            DeviceGuard dg(w->devs[(size_t)T.dev]->device);
            const int r = hip_status(hipEventSynchronize(T.done));
            if (!rc) rc = r;
            (void)hipEventDestroy(T.done);
        }
        for (auto &j : T.jobs) {
            const int r = j->wait();
            if (!rc) rc = r;
        }
        if (!first) first = rc;
    }
}

int te_stream_writer_set_hashing(te_stream_writer *w, int mode) {
    if (!w || mode < TE_HASH_AUTO || mode > TE_HASH_HOST) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(w->mu);
    w->hashing = mode;
    return TE_OK;
}

int te_set_commit_hashing(int mode) {
    if (mode < TE_HASH_AUTO || mode > TE_HASH_HOST) return TE_ERR_INVALID_ARG;
    g_commit_hashing.store(mode);
    return TE_OK;
}

int te_set_host_hash_threads(int threads) {
    if (threads < 0) return TE_ERR_INVALID_ARG;
    return hh::Pool::get().set_threads(threads);
}

int te_host_hash_threads(void) { return hh::Pool::get().threads(); }

int te_host_sha_extensions(void) { return hh::have_sha_ext() ? 1 : 0; }

double te_host_hash_rate(void) { return hh::Pool::get().thread_rate(); }

int te_host_hash_lanes(void) { return hh::Pool::get().lanes(); }

int te_host_alloc(size_t bytes, void **out) {
    if (!out) return TE_ERR_INVALID_ARG;
    *out = nullptr;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    if (bytes == 0) bytes = 1;
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? TE_ERR_OUT_OF_MEMORY : hip_status(e);
    *out = p;
    return TE_OK;
}

void te_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int te_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    TE_HIP(hipHostRegister(p, bytes, hipHostRegisterPortable));
    return TE_OK;
}

int te_host_unregister(void *p) {
    if (!p) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    TE_HIP(hipHostUnregister(p));
    return TE_OK;
}

void te_stream_writer_free(te_stream_writer *w) {
    if (!w) return;
    if (w->next > 1) (void)te_stream_wait(w, w->next - 1);
    for (auto &d : w->devs) writer_release(*d);
    delete w;
}

int te_balance_object_ranges(const te_object *objs, size_t nobj, size_t nparts, size_t *cuts) {
    if (!cuts || nparts == 0 || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    // contiguous ranges of about equal input bytes (+1 per object, so empty blobs count too):
    // cut p is the first object index after which the running byte count reaches p/nparts of the total
    uint64_t total = 0;
    for (size_t i = 0; i < nobj; i++) total += objs[i].blob_len + 1;
    for (size_t p = 0; p <= nparts; p++) cuts[p] = nobj;
    cuts[0] = 0;
    unsigned __int128 acc = 0;
    size_t part = 1;
    for (size_t i = 0; i < nobj && part < nparts; i++) {
        acc += objs[i].blob_len + 1;
        while (part < nparts && acc * nparts >= (unsigned __int128)total * part) cuts[part++] = i + 1;
    }
    return TE_OK;
}

int te_encode_batch_host_multi(te_clay *const *coders, size_t ncoders, const te_slicer_cfg *cfg, const uint8_t *h_data,
                               const te_object *objs, size_t nobj, uint8_t *h_out, size_t window_bytes) {
    if (!coders || ncoders == 0 || !cfg || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    for (size_t i = 0; i < ncoders; i++)
        if (!coders[i]) return TE_ERR_INVALID_ARG;
    if (ncoders == 1 || nobj <= 1) return te_encode_batch_host(coders[0], cfg, h_data, objs, nobj, h_out, window_bytes);
    std::vector<size_t> cut(ncoders + 1);
    (void)te_balance_object_ranges(objs, nobj, ncoders, cut.data());
    std::vector<int> rc(ncoders, TE_OK);
    std::vector<std::string> why(ncoders);  // each worker's te_last_error_detail (thread-local)
    std::vector<std::thread> th;
    for (size_t p = 0; p < ncoders; p++) {
        if (cut[p + 1] <= cut[p]) continue;
        th.emplace_back([&, p] {
            rc[p] = te_encode_batch_host(coders[p], cfg, h_data, objs + cut[p], cut[p + 1] - cut[p], h_out, window_bytes);
            if (rc[p]) why[p] = g_last_error;
        });
    }
    for (auto &t : th) t.join();
    for (size_t p = 0; p < ncoders; p++)
        if (rc[p]) {  // the first failing handle's status and detail, on the calling thread
            snprintf(g_last_error, sizeof(g_last_error), "%s", why[p].c_str());
            return rc[p];
        }
    return TE_OK;
}

int te_decode_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const te_decode_object *objs,
                           const uint8_t *h_meta, size_t nobj, uint8_t *d_out, void *stream) {
    if (!c || !cfg || (!objs && nobj) || (!h_meta && nobj)) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::vector<DecItem> items(nobj);
    for (size_t i = 0; i < nobj; i++) {
        int r = decode_validate(c, h_meta + i * TE_META_SIZE, objs[i].slice_len, objs[i].avail_mask, items[i]);
        if (r) return r;
        items[i].in_base = objs[i].slices_off;
        items[i].out_off = objs[i].out_off;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return decode_enqueue(c, cfg, d_slices, items.data(), items.size(), d_out, (hipStream_t)stream, false);
}

int te_slicer_range_plan_ex(const te_clay *c, const te_slicer_cfg *cfg, uint64_t blob_len, uint32_t avail_mask,
                            uint64_t start, uint64_t len, int chunk_path, uint64_t *first_stripe, uint64_t *nstripes,
                            uint32_t *classes, uint64_t *lo, uint64_t *hi, uint32_t *shards) {
    if (!c || !cfg || !first_stripe || !nstripes) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    if (!range_valid(blob_len, start, len)) return TE_ERR_INVALID_ARG;
    const uint32_t avail = avail_mask & (h.n >= 32 ? 0xffffffffu : (1u << h.n) - 1u);
    if (__builtin_popcount(avail) < h.k) return TE_ERR_NOT_ENOUGH_SLICES;
    te_geometry g;
    int r = te_slicer_geometry(c, (size_t)blob_len, &g);
    if (r) return r;
    uint64_t sb, se;
    range_stripes(g.stripe_size, start, len, sb, se);
    *first_stripe = sb;
    *nstripes = se - sb;
    const bool chunk_ok = chunk_path && range_chunk_ok(h, g.chunk_size, g.slice_len);
    for (uint64_t st = sb; st < se; st++) {
        const RangeWin w = range_window(h.n, cfg->rotated, avail, blob_len, g.stripe_size, g.chunk_size, st, start, len);
        const bool chunk = chunk_ok && w.miss == 1;
        if (classes) classes[st - sb] = chunk ? TE_RANGE_CHUNK : w.copy ? TE_RANGE_COPY : TE_RANGE_DECODE;
        if (lo) lo[st - sb] = w.lo;
        if (hi) hi[st - sb] = w.hi;
        if (shards) shards[st - sb] = chunk ? w.miss_x : UINT32_MAX;
    }
    return TE_OK;
}

int te_slicer_range_plan(const te_clay *c, const te_slicer_cfg *cfg, uint64_t blob_len, uint32_t avail_mask,
                         uint64_t start, uint64_t len, uint64_t *first_stripe, uint64_t *nstripes, uint32_t *classes,
                         uint64_t *lo, uint64_t *hi) {
    return te_slicer_range_plan_ex(c, cfg, blob_len, avail_mask, start, len, 0, first_stripe, nstripes, classes, lo, hi, nullptr);
}

int te_clay_set_range_chunk_path(te_clay *c, int on) {
    if (!c || (on != 0 && on != 1)) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->range_chunk = on;
    return TE_OK;
}

int te_clay_range_chunk_path(const te_clay *c) { return c ? c->range_chunk : 0; }

int te_clay_range_chunk_launch_stats(te_clay *c, te_range_chunk_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->rcs;
    return TE_OK;
}

int te_clay_range_launch_stats(te_clay *c, te_range_launch_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->rgs;
    return TE_OK;
}

int te_decode_range_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                 const te_decode_range_object *objs, const uint8_t *h_meta, size_t nobj, uint8_t *d_out,
                                 void *stream) {
    if (!c || !cfg || (!objs && nobj) || (!h_meta && nobj)) return TE_ERR_INVALID_ARG;
    std::vector<DecItem> items(nobj);
    for (size_t i = 0; i < nobj; i++) {
        int r = decode_validate(c, h_meta + i * TE_META_SIZE, objs[i].slice_len, objs[i].avail_mask, items[i]);
        if (r) return r;
        if (!range_valid(items[i].blob_len, objs[i].start, objs[i].len)) return TE_ERR_INVALID_ARG;
        items[i].in_base = objs[i].slices_off;
        items[i].out_off = objs[i].out_off;
        items[i].ranged = true;
        items[i].w_start = objs[i].start;
        items[i].w_len = objs[i].len;
    }
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    c->rgs = te_range_launch_stats{};
    c->rcs = te_range_chunk_stats{};
    if (c->range_chunk)
        for (size_t i = 0; i < nobj; i++) items[i].chunk = range_chunk_ok(c->h, items[i].cs, objs[i].slice_len);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return decode_enqueue(c, cfg, d_slices, items.data(), items.size(), d_out, (hipStream_t)stream, false);
}

int te_repair_batch_device(te_clay *c, const uint8_t *d_helpers, const te_repair_object *objs, size_t nobj,
                           uint8_t *d_out, void *stream) {
    if (!c || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::vector<RepItem> items(nobj);
    for (size_t i = 0; i < nobj; i++) {
        if (!objs[i].plan) return TE_ERR_INVALID_ARG;
        if (objs[i].plan->n != (uint32_t)c->h.n || objs[i].plan->d != (uint32_t)c->h.d) return TE_ERR_INVALID_ARG;
        items[i] = RepItem{objs[i].plan, objs[i].helper_off, objs[i].out_off, objs[i].metadata};
    }
    std::lock_guard<std::mutex> lk(c->mu);
    c->rls = te_repair_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return repair_enqueue(c, d_helpers, items.data(), items.size(), d_out, (hipStream_t)stream);
}

int te_slicer_encode(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *data, size_t len, uint8_t *slices,
                     size_t cap) {
    if (!c || !cfg || (!data && len) || !slices) return TE_ERR_INVALID_ARG;
    te_geometry g;
    te_slicer_geometry(c, len, &g);
    const size_t total = (size_t)c->h.n * g.slice_len;
    if (cap < total) return TE_ERR_BUFFER_TOO_SMALL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->els = te_encode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    TE_HIP(c->io_in.ensure(len + 16));
    TE_HIP(c->io_out.ensure(total));
    if (len) TE_HIP(hipMemcpyAsync(c->io_in.p, data, len, hipMemcpyHostToDevice, c->stream));
    te_object o{0, len, 0, cfg->chunk_index};
    r = encode_enqueue(c, cfg, c->io_in.as<uint8_t>(), &o, 1, c->io_out.as<uint8_t>(), c->stream, false, nullptr,
                       StripeSel(), true);
    if (r) return r;
    // (copying the level-1 rows out while level 2 runs, as 2-D copies on a second stream, measured
    // slower: 0.62 against 0.50 ms pageable, 0.505 against 0.485 pinned, r05)
    TE_HIP(hipMemcpyAsync(slices, c->io_out.p, total, hipMemcpyDeviceToHost, c->stream));
    TE_HIP(hipStreamSynchronize(c->stream));
    return TE_OK;
}

int te_clay_encode(te_clay *c, const uint8_t *data, size_t len, uint8_t *chunks, size_t cap, size_t *chunk_size) {
    if (!c || (!data && len) || !chunks) return TE_ERR_INVALID_ARG;
    if (len == 0) return TE_ERR_EMPTY_INPUT;  // clay.rs:100-102
    const size_t cs = c->h.chunk_size_for(len);
    const size_t total = (size_t)c->h.n * cs;
    if (chunk_size) *chunk_size = cs;
    if (cap < total) return TE_ERR_BUFFER_TOO_SMALL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->els = te_encode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    TE_HIP(c->io_in.ensure(len + 16));
    TE_HIP(c->io_out.ensure(total));
    TE_HIP(hipMemcpyAsync(c->io_in.p, data, len, hipMemcpyHostToDevice, c->stream));
    te_object o{0, len, 0, 0};
    te_slicer_cfg cfg{0, TE_ENCODING_CLAY, TE_CLAY_DEFAULT_PARAMS, 0};
    r = encode_enqueue(c, &cfg, c->io_in.as<uint8_t>(), &o, 1, c->io_out.as<uint8_t>(), c->stream, true, nullptr,
                       StripeSel(), true);
    if (r) return r;
    TE_HIP(hipMemcpyAsync(chunks, c->io_out.p, total, hipMemcpyDeviceToHost, c->stream));
    TE_HIP(hipStreamSynchronize(c->stream));
    return TE_OK;
}

}  // extern "C"
// The given slices (n pointers, null = absent) to c->io_in at i * len, on c->stream.  Page-locked
// ones, and long ones, are copied directly; only the short pageable ones are first gathered into
// the handle's pinned staging by the device's copy pool (one pageable slice used to
// send every slice, pinned ones included, through the gather): each pageable H2D goes through the
// driver's staging at ~57 us of fixed cost (te_slicer_decode, 7 x 715 KB: 1.11 -> 0.81 ms per
// 4 MiB call, against 0.70 with pinned slices, r05).  Long ones go to the driver, whose pageable
// path outruns the 4-thread memcpy there (7 x 11.4 MB, 64 MiB object: 3.03 ms direct, 4.2-4.5
// gathered).
constexpr size_t kGatherMaxSlice = 2u << 20;
static int upload_slices(te_clay *c, const uint8_t *const *slices, size_t len, size_t out_bytes) {
    const int n = c->h.n;
    TE_HIP(c->io_in.ensure((size_t)n * len));
    TE_HIP(c->io_out.ensure(out_bytes));  // (both buffers before the first copy is queued)
    const uint8_t *src[64];
    int gather = 0;
    for (int i = 0; i < n; i++) {
        src[i] = slices[i];
        if (slices[i] && len <= kGatherMaxSlice && !host_pinned(slices[i])) gather++;
    }
    if (gather) {
        TE_HIP(c->hio_in.ensure((size_t)gather * len));
        std::vector<tec::CopyPool::Seg> segs;
        for (int i = 0, g = 0; i < n; i++)
            if (slices[i] && len <= kGatherMaxSlice && !host_pinned(slices[i])) {
                src[i] = c->hio_in.u8() + (size_t)g++ * len;
                segs.push_back({const_cast<uint8_t *>(src[i]), slices[i], len});
            }
        copy_pool(c->device).run(segs);
    }
    for (int i = 0; i < n; i++)
        if (slices[i])
            TE_HIP(hipMemcpyAsync(c->io_in.as<uint8_t>() + (size_t)i * len, src[i], len, hipMemcpyHostToDevice,
                                  c->stream));
    return TE_OK;
}
// The present ones of n slice pointers (null = absent) as a mask; *first: the lowest, or -1
static uint32_t slices_avail(const uint8_t *const *slices, int n, int *first = nullptr) {
    uint32_t avail = 0;
    for (int i = 0; i < n; i++)
        if (slices[i]) avail |= 1u << i;
    if (first) *first = avail ? __builtin_ctz(avail) : -1;
    return avail;
}
// Measurement option TEC_DEBUG_KNOBS=1 TEC_DECODE_ZC=0: the per-call decodes' device copies instead
static bool decode_zc() {
    static const bool zc = [] { const char *e = tec_knob("TEC_DECODE_ZC"); return !(e && e[0] == '0'); }();
    return zc;
}
// A per-call decode (<= 64 stripes, the one-wave class kernels) reads its slices from page-locked
// host staging and writes the object to page-locked memory over PCIe, with no H2D / D2H copy around
// a 0.3 ms kernel whose loader wave issues its loads four steps ahead.  slices: gathered into the
// staging at i * len by the copy pool (the repair call's scheme); null: the caller staged them.  A
// page-locked `out` is written at its device address; otherwise the `bytes` of output are staged.
static int percall_decode_pinned(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t len,
                                 const DecItem &it, uint8_t *out, size_t bytes, bool raw) {
    if (slices) {
        TE_HIP(c->hio_in.ensure((size_t)c->h.n * len));
        std::vector<tec::CopyPool::Seg> segs;
        for (int i = 0; i < c->h.n; i++)
            if (slices[i]) segs.push_back({c->hio_in.u8() + (size_t)i * len, slices[i], len});
        copy_pool(c->device).run(segs);
    }
    uint8_t *const d_out = host_device_ptr(out);
    if (!d_out) TE_HIP(c->hio_out.ensure(bytes));
    const int r = decode_enqueue(c, cfg, c->hio_in.u8(), &it, 1, d_out ? d_out : c->hio_out.u8(), c->stream, raw);
    if (r) return r;
    TE_HIP(hipStreamSynchronize(c->stream));
    if (!d_out) copy_pool(c->device).run({{out, c->hio_out.p, bytes}});
    c->dls.direct_out = d_out ? 1u : 0u;
    return TE_OK;
}
// ... or through device copies: the slices are in c->io_in, `bytes` of output come back from c->io_out
static int percall_decode_device(te_clay *c, const te_slicer_cfg *cfg, const DecItem &it, uint8_t *out, size_t bytes, bool raw) {
    TE_HIP(c->io_out.ensure(bytes));
    const int r = decode_enqueue(c, cfg, c->io_in.as<uint8_t>(), &it, 1, c->io_out.as<uint8_t>(), c->stream, raw);
    if (r) return r;
    TE_HIP(hipMemcpyAsync(out, c->io_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    TE_HIP(hipStreamSynchronize(c->stream));
    return TE_OK;
}

// ------------------------------------------------------------------------------------------
// Node recover (network/node/src/features/spool/recover.rs:411-442 `reconstruct`): rebuild the lost
// slices of an object from >= k peer slices.  One lost slice (te_recover_object) is a lost mask of
// one bit (te_recover_multi_object): every entry point validates its objects into RecItem and
// routes them by rec_multi_plan.hpp's rec_route -- the class path, the multi-output kernel
// (recover_multi.hip) or the generic path (decode, re-encode, keep the lost slices).
// ------------------------------------------------------------------------------------------
namespace {
struct RecItem {
    DecItem it;        // validated like Slicer::decode; in_base set
    uint32_t lost;     // the lost slices
    uint64_t out_off;  // the j-th of them at d_out + out_off + j * it.slice_len
    uint64_t cs, ns, stripe;  // the slices' chunk size, stripes (an empty blob: one zero chunk) and stripe size
    uint64_t chunk_index, meta_w[6];
};

// A single-slice entry point's object as the one form: its lost index is a one-bit mask.  These
// entry points ask only lost < n (an empty mask here, rec_validate's TE_ERR_INVALID_SLICE): not
// that the lost slice is absent, as the multi forms do.
te_recover_multi_object rec_single(const te_clay *c, const te_recover_object &o) {
    return te_recover_multi_object{o.slices_off, o.slice_len, o.avail_mask, o.lost < (uint32_t)c->h.n ? 1u << o.lost : 0u,
                                   o.out_off};
}

// One object's checks, host only: the mask by its entry point's rule (single = rec_single's, else
// rec_multi_check), then Slicer::decode's, then the slice length
int rec_validate(const te_clay *c, const te_recover_multi_object &o, const uint8_t *meta48, bool single, RecItem &m) {
    int r = single ? (o.lost_mask ? TE_OK : TE_ERR_INVALID_SLICE) : rec_multi_check(c->h.n, c->h.k, o.avail_mask, o.lost_mask);
    if (r || (r = decode_validate(c, meta48, o.slice_len, o.avail_mask, m.it))) return r;
    te_slice_metadata md;
    te_slice_metadata_from_slice(meta48, TE_META_SIZE, &md);
    te_geometry g;
    te_slicer_geometry(c, m.it.blob_len, &g);
    if (g.slice_len != o.slice_len) return TE_ERR_INVALID_LAYOUT;
    m.it.in_base = o.slices_off;
    m.lost = o.lost_mask;
    m.out_off = o.out_off;
    m.cs = g.chunk_size;
    m.ns = g.num_stripes;
    m.stripe = g.stripe_size;
    m.chunk_index = md.chunk_index;
    for (int w = 0; w < 6; w++) m.meta_w[w] = get_u64(meta48 + 8 * w);
    return TE_OK;
}

// The metadata suffix of m's j-th rebuilt slice
MetaJob rec_meta(const RecItem &m, uint8_t *d_out, uint64_t j) {
    MetaJob mj{};
    mj.dst = d_out + m.out_off + j * m.it.slice_len + m.ns * m.cs;
    for (int k = 0; k < 6; k++) mj.words[k] = m.meta_w[k];
    return mj;
}

// The recover workspaces (rec_blob, rec_slices, the gather arena) are ordered against a previous
// call on another stream by `rec_done`: later calls (any stream) order against everything this
// one enqueued on s
int rec_mark_done(te_clay *c, hipStream_t s) {
    if (!c->rec_done) TE_HIP(hipEventCreateWithFlags(&c->rec_done, hipEventDisableTiming));
    const int r = hip_status(hipEventRecord(c->rec_done, s));
    c->rec_pending = true;
    c->rec_stream = s;
    return r;
}

// The sub-masks of a stripe's (padded erasure mask, lost nodes) and their programs, compiled once
// per handle (caller holds c->mu).  Empty: no program (the caller takes the generic path).
// The host work of one pair, pure ClayHost work (thread-safe): the split and each part's program.
struct RecMultiPair {
    bool ok = false;  // false: no pattern, or a part without a staged program
    std::vector<uint64_t> subs;
    std::vector<te_clay::DecCache> progs;  // one per sub-mask
};
void rec_multi_pair(const ClayHost &h, uint64_t emask, uint64_t lostn, RecMultiPair &R) {
    te_clay::DecCache base;
    if (!h.gpe_pattern(emask, base.P, base.planes)) return;
    base.P.planes_off = 0;
    std::vector<RecMultiProg> progs;
    R.subs = rec_multi_split(h, base.P, lostn, &progs);
    for (size_t i = 0; i < R.subs.size(); i++) {
        te_clay::DecCache d = base;
        d.staged = progs[i].steps.size() == te_clay::DecStore::kSteps;
        if (!d.staged) return;
        d.H = progs[i].H;
        d.steps = std::move(progs[i].steps);
        d.orient = progs[i].orient;
        R.progs.push_back(std::move(d));
    }
    R.ok = true;
}
// ... and its place in the handle's caches (caller holds c->mu)
const std::vector<uint64_t> *rec_multi_commit(te_clay *c, uint64_t emask, uint64_t lostn, RecMultiPair &R) {
    // a pair without programs is remembered as an empty split, which the caller reads as "take the
    // generic path": it is not compiled again by a later call
    if (!R.ok) return &c->rm_split.emplace(rec_multi_key(emask, lostn), std::vector<uint64_t>{}).first->second;
    for (size_t i = 0; i < R.subs.size(); i++) {
        const uint64_t k = rec_multi_key(emask, R.subs[i]);
        if (!c->rm_cache.count(k)) c->rm_cache.emplace(k, std::move(R.progs[i]));
    }
    return &c->rm_split.emplace(rec_multi_key(emask, lostn), std::move(R.subs)).first->second;
}
const std::vector<uint64_t> *rec_multi_subs(te_clay *c, uint64_t emask, uint64_t lostn) {
    auto f = c->rm_split.find(rec_multi_key(emask, lostn));
    if (f != c->rm_split.end()) return &f->second;
    RecMultiPair R;
    rec_multi_pair(c->h, emask, lostn, R);
    return rec_multi_commit(c, emask, lostn, R);
}

// The (padded erasure mask, lost nodes) pairs of a call that the handle has not seen, compiled
// before the call enqueues, on up to 16 host threads as dec_precompile's patterns are (a first-time
// pair is about a millisecond of host work: the split tries a program per part and orientation).
// rec_multi_subs then finds every pair of the call in the cache.  Caller holds c->mu.
void rec_multi_precompile(te_clay *c, int rotated, const std::vector<const RecItem *> &items) {
    const ClayHost &h = c->h;
    std::vector<std::pair<uint64_t, uint64_t>> todo;
    std::unordered_set<uint64_t> seen;
    for (const RecItem *p : items)
        for (uint64_t st = 0; st < p->it.ns; st++) {
            const uint64_t emask = stripe_emask(h, rotated, p->it.avail, st);
            const uint64_t lostn = rec_multi_lost_nodes(h, rotated, p->lost, st);
            const uint64_t key = rec_multi_key(emask, lostn);
            if (!c->rm_split.count(key) && seen.insert(key).second) todo.push_back({emask, lostn});
        }
    if (todo.size() < 2) return;  // rec_multi_subs compiles the one inline
    std::vector<RecMultiPair> out(todo.size());
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nth = std::min<size_t>({16, (size_t)hw, todo.size()});
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < todo.size();) rec_multi_pair(h, todo[i].first, todo[i].second, out[i]);
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nth; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    for (size_t i = 0; i < todo.size(); i++) (void)rec_multi_commit(c, todo[i].first, todo[i].second, out[i]);
}

// The objects on the multi-output kernel: a job per (stripe, sub-mask), all of one chunk size and
// slice length in one launch -- a split stripe's passes are jobs of the same launch, reading the
// same resident slices.  The programs go through the decode's device store and descriptor arena
// (dec_image / dec_upload).  TE_ERR_UNSUPPORTED, before anything is enqueued: a stripe without a
// program.  Caller holds c->mu, the handle's device current.
int recover_multi_enqueue(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const std::vector<const RecItem *> &items,
                          uint8_t *d_out, hipStream_t s, te_recover_multi_stats &st_out) {
    const ClayHost &h = c->h;
    if (c->rm_cache.size() > c->dstore.max_cap) {
        c->rm_cache.clear();
        c->rm_split.clear();
    }
    rec_multi_precompile(c, cfg->rotated, items);
    DecCall D{c, s, cfg->rotated};
    std::unordered_map<uint64_t, uint32_t> pat_index;
    std::map<DecGroupKey, std::vector<RmSlots>> tabs;
    te_recover_multi_stats add{};
    for (const RecItem *p : items) {
        const RecItem &m = *p;
        const DecItem &it = m.it;
        const uint64_t nlost = (uint64_t)__builtin_popcount(m.lost);
        const DecGroupKey gk{it.cs, it.slice_len};
        for (uint64_t st = 0; st < it.ns; st++) {
            const uint64_t emask = stripe_emask(h, D.rotated, it.avail, st);
            const uint64_t lostn = rec_multi_lost_nodes(h, D.rotated, m.lost, st);
            const std::vector<uint64_t> *subs = rec_multi_subs(c, emask, lostn);
            if (!subs || subs->empty()) return TE_ERR_UNSUPPORTED;
            for (uint64_t sub : *subs) {
                const uint64_t key = rec_multi_key(emask, sub);
                const auto f = pat_index.emplace(key, (uint32_t)D.plan.keys.size());
                if (f.second) {
                    D.plan.keys.push_back(key);
                    D.cached.push_back(&c->rm_cache.at(key));
                }
                GpeJob g{};
                g.in = d_slices + it.in_base + st * it.cs;
                g.in_len = ~0ull;
                g.out = d_out + m.out_off + st * it.cs;  // slot j's chunk of this stripe at + j * slice_len
                g.out_len = (nlost - 1) * it.slice_len + it.cs;
                g.rot = D.rotated ? (uint32_t)((st * TE_ROTATION_STEP) % (uint64_t)h.n) : 0u;
                g.pattern = f.first->second;
                D.plan.groups[gk].push_back(g);
                tabs[gk].push_back(rec_multi_slots(h, D.rotated, m.lost, sub, st));
                add.jobs++;
                add.out_rows += (uint64_t)__builtin_popcountll(sub) * (uint64_t)h.alpha;
            }
            add.stripes++;
            add.split_stripes += subs->size() > 1;
            add.passes = std::max(add.passes, (uint32_t)subs->size());
        }
    }
    if (D.plan.groups.empty()) return TE_OK;
    for (const te_clay::DecCache *dc : D.cached) {
        D.lds_rows = std::max(D.lds_rows, recover_multi_rows(dc->H.nslots));
        D.nscr_max = std::max(D.nscr_max, dc->H.nscratch);
        D.max_er = std::max(D.max_er, dc->P.nerased);
    }
    D.small_dec = add.jobs <= kDecSmallStripes;  // a per-call rebuild: one wave per workgroup
    int r = dec_image(D);
    if (r) return r;
    Arena &A = c->dec;
    std::vector<size_t> tab_off;
    for (auto &o : D.offs) tab_off.push_back(A.put(tabs.at(o.first).data(), tabs.at(o.first).size() * sizeof(RmSlots)));
    if ((r = dec_upload(D))) return r;
    size_t scratch_bytes = 0;
    for (auto &o : D.offs) scratch_bytes = std::max(scratch_bytes, recover_multi_scratch_bytes(dec_table_args(D, o)));
    if ((r = A.workspace(scratch_bytes, s, &D.scratch))) return r;
    KTimer kt(s);
    for (size_t i = 0; i < D.offs.size(); i++) {
        DecArgs a = dec_table_args(D, D.offs[i]);
        a.scratch = D.scratch;
        a.out_stride = D.offs[i].first.slice_len;  // between output slots
        TE_HIP(launch_recover_multi(a, A.at<RmSlots>(tab_off[i]), s));
        add.multi_launches++;
    }
    kt.stop();
    if (D.in_store) TE_HIP(c->dstore.readers.record(s));
    if ((r = A.mark_done(s))) return r;
    st_out.multi_launches += add.multi_launches;
    st_out.passes = std::max(st_out.passes, add.passes);
    st_out.jobs += add.jobs;
    st_out.out_rows += add.out_rows;
    st_out.stripes += add.stripes;
    st_out.split_stripes += add.split_stripes;
    return TE_OK;
}

// The generic path, for any lost mask: decode into the object, re-encode, keep the lost slices.
// Per stripe a lost slice holds one shard (rotation): a data shard is a piece of the decoded object
// (zero-padded like Slicer::encode's stripe, slicer.rs:276-283), so only the stripes with a parity
// shard among the lost ones are re-encoded, writing those shards' chunks alone.  Objects go through
// the device workspaces in windows (bounded memory).  Caller holds c->mu.
int recover_generic(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const std::vector<const RecItem *> &items,
                    uint8_t *d_out, hipStream_t s) {
    const ClayHost &h = c->h;
    const uint32_t n = (uint32_t)h.n;
    const int rotated = cfg->rotated;
    // windows: <= kWinBlob decoded bytes and <= kWinSlices re-encoded slice bytes
    uint64_t kWinBlob = 1ull << 30, kWinSlices = 3ull << 30;
    if (const char *e = tec_knob("TEC_RECOVER_WINDOW_BYTES")) {  // tests: force several windows
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v) kWinBlob = kWinSlices = v;
    }
    struct Win { size_t b, e; uint64_t blob, slices; };
    std::vector<Win> wins;
    uint64_t max_blob = 16, max_slices = 16;
    for (size_t i = 0; i < items.size();) {
        Win w{i, i, 0, 0};
        while (w.e < items.size()) {
            const uint64_t bb = align16(items[w.e]->it.blob_len), sb = (uint64_t)n * items[w.e]->it.slice_len;
            if (w.e > w.b && (w.blob + bb > kWinBlob || w.slices + sb > kWinSlices)) break;
            w.blob += bb;
            w.slices += sb;
            w.e++;
        }
        max_blob = std::max(max_blob, w.blob + 16);
        max_slices = std::max(max_slices, w.slices + 16);
        wins.push_back(w);
        i = w.e;
    }
    if (max_blob > c->rec_blob.cap || max_slices > c->rec_slices.cap) {
        if (c->rec_pending) TE_HIP(hipEventSynchronize(c->rec_done));  // queued work may still use them
    } else if (c->rec_pending && c->rec_stream != s) {
        TE_HIP(hipStreamWaitEvent(s, c->rec_done, 0));
    }
    TE_HIP(c->rec_blob.ensure(max_blob));
    TE_HIP(c->rec_slices.ensure(max_slices));
    uint8_t *const blob = c->rec_blob.as<uint8_t>(), *const slices = c->rec_slices.as<uint8_t>();
    // the keep filter of object m's stripe st: its parity shards among the lost slices, plus the
    // column-0 parity chunks the LDS-DMA kernel reads back internally; 0 = all data, not encoded
    const uint32_t col0_parity = ((1u << h.q) - 1u) & ~((1u << h.k) - 1u);
    auto keep = [&](const RecItem &m, uint64_t st) {
        uint32_t par = 0;
        rec_each_lost(m.lost, [&](uint32_t sl, uint64_t) {
            const uint32_t sh = slice_to_shard(rotated, n, (uint32_t)st, sl);
            if (sh >= (uint32_t)h.k) par |= 1u << sh;
        });
        return par ? col0_parity | par : 0u;
    };
    std::vector<DecItem> dit;
    std::vector<te_object> wenc;
    std::vector<CopyJob> jobs;
    std::vector<MetaJob> metas;
    int r = TE_OK;
    for (const Win &w : wins) {
        dit.clear();
        wenc.clear();
        uint64_t bo = 0, so = 0;
        bool any_parity = false;
        for (size_t i = w.b; i < w.e; i++) {
            const RecItem &m = *items[i];
            dit.push_back(m.it);
            dit.back().out_off = bo;
            wenc.push_back(te_object{bo, m.it.blob_len, so, m.chunk_index});
            bo += align16(m.it.blob_len);
            so += (uint64_t)n * m.it.slice_len;
            for (uint64_t st = 0; st < m.ns && !any_parity; st++) any_parity = keep(m, st) != 0;
        }
        if ((r = decode_enqueue(c, cfg, d_slices, dit.data(), dit.size(), blob, s, false))) break;
        if (any_parity && (r = encode_enqueue(c, cfg, blob, wenc.data(), wenc.size(), slices, s, false, nullptr,
                                              [&](size_t o, size_t st) { return keep(*items[w.b + o], st); })))
            break;
        // assemble the lost slices: per stripe the lost shard's chunk, then the suffix
        jobs.clear();
        metas.clear();
        for (size_t i = w.b; i < w.e; i++) {
            const RecItem &m = *items[i];
            const te_object &e = wenc[i - w.b];
            const uint64_t cs = m.cs, slen = m.it.slice_len, len = m.it.blob_len;
            rec_each_lost(m.lost, [&](uint32_t sl, uint64_t j) {
                uint8_t *dst = d_out + m.out_off + j * slen;
                for (uint64_t st = 0; st < m.ns; st++) {
                    const uint32_t sh = slice_to_shard(rotated, n, (uint32_t)st, sl);
                    if (sh >= (uint32_t)h.k) {
                        jobs.push_back(CopyJob{slices + e.out_off + (uint64_t)sl * slen + st * cs, dst + st * cs, cs, cs});
                    } else {
                        // data shard sh of stripe st: object bytes [st*S + sh*cs, ...) clipped to the
                        // stripe and the object, zero beyond
                        const uint64_t start = st * m.stripe + (uint64_t)sh * cs;
                        const uint64_t end = std::min<uint64_t>(len, (st + 1) * m.stripe);
                        const uint64_t valid = start < end ? std::min<uint64_t>(cs, end - start) : 0;
                        jobs.push_back(CopyJob{blob + e.data_off + std::min(start, len), dst + st * cs, cs, valid});
                    }
                }
                metas.push_back(rec_meta(m, d_out, j));
            });
        }
        if ((r = gather_meta_enqueue(c->rec, s, jobs, metas))) break;
    }
    const int r2 = rec_mark_done(c, s);
    return r ? r : r2;
}

// Every recover call's device work: handle locked, its device current, the items validated.  The
// items go by route (rec_route), each non-empty part in turn -- the class path, the multi-output
// kernel, the generic path, which also takes the items of a part that answers TE_ERR_UNSUPPORTED
// before it enqueues anything -- so one small object does not send a whole batch to the windowed
// decode + re-encode.  The call's figures are added to `st`.
int recover_enqueue(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const std::vector<RecItem> &items,
                    uint8_t *d_out, hipStream_t s, te_recover_multi_stats &st) {
    const ClayHost &h = c->h;
    std::vector<const RecItem *> part[3];
    for (auto &p : part) p.reserve(items.size());
    for (const RecItem &m : items)
        part[rec_route(h, (uint32_t)__builtin_popcount(m.lost), m.it.ns, m.it.cs, m.it.slice_len)].push_back(&m);
    std::vector<const RecItem *> &cls = part[kRecClass], &multi = part[kRecKernel], &generic = part[kRecGeneric];
    // a part's metadata suffixes (and an empty blob's zero chunk), after its kernels
    auto finish = [&](const std::vector<CopyJob> &zeros, const std::vector<MetaJob> &metas) {
        if (c->rec_pending && c->rec_stream != s) TE_HIP(hipStreamWaitEvent(s, c->rec_done, 0));
        const int r = gather_meta_enqueue(c->rec, s, zeros, metas), r2 = rec_mark_done(c, s);
        return r ? r : r2;
    };
    if (!cls.empty()) {
        // One staged decode whose program outputs only the lost node's chunk of every stripe,
        // straight into the lost slice -- k slices read, 1 written, no decoded object and no
        // re-encode (a lost parity node's C is produced by the same layered decode)
        std::vector<DecItem> fi;
        std::vector<CopyJob> zeros;
        std::vector<MetaJob> metas;
        fi.reserve(cls.size());
        metas.reserve(cls.size());
        for (const RecItem *m : cls)
            rec_each_lost(m->lost, [&](uint32_t sl, uint64_t j) {
                fi.push_back(m->it);
                fi.back().lost = (int32_t)sl;
                fi.back().out_off = m->out_off + j * m->it.slice_len;
                if (m->it.ns == 0) zeros.push_back(CopyJob{d_out, d_out + fi.back().out_off, m->cs * m->ns, 0});
                metas.push_back(rec_meta(*m, d_out, j));
            });
        int r = decode_enqueue(c, cfg, d_slices, fi.data(), fi.size(), d_out, s, false);
        if (r == TE_ERR_UNSUPPORTED) {
            generic.insert(generic.begin(), cls.begin(), cls.end());
            cls.clear();
        } else if (r || (r = finish(zeros, metas))) {
            return r;
        }
    }
    if (!multi.empty()) {
        std::vector<MetaJob> metas;
        for (const RecItem *m : multi)
            rec_each_lost(m->lost, [&](uint32_t, uint64_t j) { metas.push_back(rec_meta(*m, d_out, j)); });
        int r = recover_multi_enqueue(c, cfg, d_slices, multi, d_out, s, st);
        if (r == TE_ERR_UNSUPPORTED) {
            generic.insert(generic.end(), multi.begin(), multi.end());
            multi.clear();
        } else if (r || (r = finish({}, metas))) {
            return r;
        }
    }
    st.single_objects += cls.size();
    st.multi_objects += multi.size();
    st.generic_objects += generic.size();
    return generic.empty() ? (int)TE_OK : recover_generic(c, cfg, d_slices, generic, d_out, s);
}

// The device forms after their argument checks: the one lock of the call, its launch stats reset
int recover_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const std::vector<RecItem> &items,
                   uint8_t *d_out, void *stream) {
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    c->els = te_encode_launch_stats{};  // the keep-filter re-encode of the parity-lost stripes
    c->rms = te_recover_multi_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return recover_enqueue(c, cfg, d_slices, items, d_out, (hipStream_t)stream, c->rms);
}

}  // namespace
extern "C" {

// The argument rule of the single-slice forms (rec_single); nothing is validated without a device
int te_recover_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                            const te_recover_object *objs, const uint8_t *h_meta, size_t nobj, uint8_t *d_out,
                            void *stream) {
    if (!c || !cfg || (!objs && nobj) || (!h_meta && nobj)) return TE_ERR_INVALID_ARG;
    if (nobj == 0) return TE_OK;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::vector<RecItem> items(nobj);
    for (size_t i = 0; i < nobj; i++)
        if (int r = rec_validate(c, rec_single(c, objs[i]), h_meta + i * TE_META_SIZE, true, items[i])) return r;
    return recover_device(c, cfg, d_slices, items, d_out, stream);
}

int te_recover_multi_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                  const te_recover_multi_object *objs, const uint8_t *h_meta, size_t nobj, uint8_t *d_out,
                                  void *stream) {
    if (!c || !cfg || (!objs && nobj) || (!h_meta && nobj)) return TE_ERR_INVALID_ARG;
    std::vector<RecItem> items(nobj);
    for (size_t i = 0; i < nobj; i++)
        if (int r = rec_validate(c, objs[i], h_meta + i * TE_META_SIZE, false, items[i])) return r;
    if (nobj == 0) return TE_OK;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    return recover_device(c, cfg, d_slices, items, d_out, stream);
}

// Per call: the present slices go up once (upload_slices, the decode's staging), every lost slice
// comes back from the one device buffer
int te_slicer_recover_multi(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t slice_len,
                            uint32_t lost_mask, uint8_t *const *out) {
    if (!c || !cfg || !slices || !out) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    int first;
    const uint32_t avail = slices_avail(slices, h.n, &first);
    int r = rec_multi_check(h.n, h.k, avail, lost_mask);
    if (r) return r;
    const size_t nlost = (size_t)__builtin_popcount(lost_mask);
    for (size_t j = 0; j < nlost; j++)
        if (!out[j]) return TE_ERR_INVALID_ARG;
    if (first < 0) return TE_ERR_NOT_ENOUGH_SLICES;
    if (slice_len < TE_META_SIZE) return TE_ERR_INVALID_LAYOUT;
    const uint8_t *meta = slices[first] + slice_len - TE_META_SIZE;
    const te_recover_multi_object o{0, slice_len, avail, lost_mask, 0};
    std::vector<RecItem> m(1);
    if ((r = rec_validate(c, o, meta, false, m[0]))) return r;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    if ((r = ensure_stream(c))) return r;
    if ((r = upload_slices(c, slices, slice_len, nlost * slice_len))) return r;
    c->dls = te_decode_launch_stats{};
    c->els = te_encode_launch_stats{};
    c->rms = te_recover_multi_stats{};
    if ((r = recover_enqueue(c, cfg, c->io_in.as<uint8_t>(), m, c->io_out.as<uint8_t>(), c->stream, c->rms))) return r;
    for (size_t j = 0; j < nlost; j++)
        TE_HIP(hipMemcpyAsync(out[j], c->io_out.as<uint8_t>() + j * slice_len, slice_len, hipMemcpyDeviceToHost, c->stream));
    TE_HIP(hipStreamSynchronize(c->stream));
    return TE_OK;
}

int te_clay_decode(te_clay *c, const uint8_t *const *chunks, size_t cs, uint8_t *out, size_t cap) {
    if (!c || !chunks || !out) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    const uint32_t avail = slices_avail(chunks, h.n);
    if (__builtin_popcount(avail) < h.k) return TE_ERR_NOT_ENOUGH_SLICES;  // clay.rs:107-109
    if (cs == 0 || cs % (size_t)h.alpha) return TE_ERR_BAD_ENCODING;
    if (cap < (size_t)h.k * cs) return TE_ERR_BUFFER_TOO_SMALL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    DecItem it{};
    it.in_base = 0; it.slice_len = cs; it.blob_len = (uint64_t)h.k * cs; it.stripe = it.blob_len; it.ns = 1; it.cs = cs;
    it.out_off = 0; it.avail = avail;
    // one stripe: the zero-copy per-call path of te_slicer_decode (staging read and written over PCIe)
    if (decode_zc()) return percall_decode_pinned(c, nullptr, chunks, cs, it, out, (size_t)h.k * cs, true);
    if ((r = upload_slices(c, chunks, cs, (size_t)h.k * cs))) return r;
    return percall_decode_device(c, nullptr, it, out, (size_t)h.k * cs, true);
}

int te_slicer_decode(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t slice_len,
                     uint8_t *out, size_t cap, size_t *out_len) {
    if (!c || !cfg || !slices) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    int first;
    const uint32_t avail = slices_avail(slices, h.n, &first);
    if (first < 0) return TE_ERR_NOT_ENOUGH_SLICES;
    if (slice_len < TE_META_SIZE) return TE_ERR_INVALID_LAYOUT;
    DecItem it{};
    int r = decode_validate(c, slices[first] + slice_len - TE_META_SIZE, slice_len, avail, it);
    if (r) return r;
    if (out_len) *out_len = it.blob_len;
    if (it.blob_len == 0) return TE_OK;
    if (!out || cap < it.blob_len) return TE_ERR_BUFFER_TOO_SMALL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    r = ensure_stream(c);
    if (r) return r;
    it.in_base = 0;
    it.out_off = 0;
    if (decode_zc() && it.ns <= kDecSmallStripes) return percall_decode_pinned(c, cfg, slices, slice_len, it, out, it.blob_len, false);
    if ((r = upload_slices(c, slices, slice_len, it.blob_len))) return r;
    return percall_decode_device(c, cfg, it, out, it.blob_len, false);
}

int te_slicer_decode_range(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t slice_len,
                           uint64_t start, uint64_t len, uint8_t *out, size_t cap, size_t *out_len) {
    if (!c || !cfg || !slices) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    const int n = h.n;
    int first;
    const uint32_t avail = slices_avail(slices, n, &first);
    if (first < 0) return TE_ERR_NOT_ENOUGH_SLICES;
    if (slice_len < TE_META_SIZE) return TE_ERR_INVALID_LAYOUT;
    DecItem it{};
    int r = decode_validate(c, slices[first] + slice_len - TE_META_SIZE, slice_len, avail, it);
    if (r) return r;
    if (!range_valid(it.blob_len, start, len)) return TE_ERR_INVALID_ARG;
    if (out_len) *out_len = (size_t)len;
    if (len && (!out || cap < len)) return TE_ERR_BUFFER_TOO_SMALL;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    c->rgs = te_range_launch_stats{};
    c->rcs = te_range_chunk_stats{};
    if (len == 0) return TE_OK;
    it.chunk = c->range_chunk && range_chunk_ok(h, it.cs, slice_len);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    r = ensure_stream(c);
    if (r) return r;
    // The staging holds, per slice, only the touched stripes' chunks: slice i's bytes
    // [sb cs, se cs) at i * T.  Of those, a decode stripe stages the chunks of the k slices its
    // (padded) pattern reads, a copy stripe the present data-chunk bytes inside the window, a
    // chunk stripe both: its recover job's k chunks and the other present pieces of the window.
    uint64_t sb, se;
    range_stripes(it.stripe, start, len, sb, se);
    const uint64_t T = (se - sb) * it.cs;
    const int rotated = cfg->rotated;
    struct Piece { uint64_t at; const uint8_t *src; uint64_t len; };  // staging offset <- slice bytes
    std::vector<Piece> pieces;
    auto stage = [&](uint32_t sl, uint64_t from, uint64_t bytes) {  // slice bytes [from, from + bytes)
        const uint64_t at = sl * T + (from - sb * it.cs);
        if (!pieces.empty() && pieces.back().at + pieces.back().len == at && pieces.back().src + pieces.back().len == slices[sl] + from)
            pieces.back().len += bytes;  // the next stripe's chunk of the same slice
        else
            pieces.push_back({at, slices[sl] + from, bytes});
        c->rgs.bytes_staged += bytes;
    };
    const std::vector<RangeWin> wins = range_windows(n, rotated, avail, it.blob_len, it.stripe, it.cs, start, len);
    std::vector<uint64_t> emasks(wins.size(), 0);  // the decode and chunk stripes' padded erasure sets
    for (size_t i = 0; i < wins.size(); i++)
        if (!wins[i].copy) emasks[i] = stripe_emask(h, rotated, avail, sb + i);
    for (int sl = 0; sl < n; sl++) {  // slice-major, so a slice's consecutive chunks merge into one piece
        if (!slices[sl]) continue;
        for (uint64_t st = sb; st < se; st++) {
            const uint32_t sh = te_slice_to_shard(rotated, (uint32_t)n, (uint32_t)st, (uint32_t)sl);
            const RangeWin &w = wins[st - sb];
            const bool read = !w.copy && !((emasks[st - sb] >> h.ext_to_int((int)sh)) & 1ull);  // one of the pattern's k
            if (read) {
                stage((uint32_t)sl, st * it.cs, it.cs);
            } else if (w.copy || range_is_chunk(it, w)) {
                const uint64_t a = std::max(w.lo, sh * it.cs), b = std::min(w.hi, (sh + 1) * it.cs);
                if ((int)sh < h.k && a < b) stage((uint32_t)sl, st * it.cs + (a - sh * it.cs), b - a);
            }
        }
    }
    it.in_base = 0;
    it.in_skew = sb * it.cs;
    it.slice_len = T;  // the stride between the staged slices
    it.out_off = 0;
    it.ranged = true;
    it.w_start = start;
    it.w_len = len;
    const size_t total = (size_t)n * T;
    TE_HIP(c->hio_in.ensure(total));
    std::vector<tec::CopyPool::Seg> segs;
    for (const Piece &p : pieces) segs.push_back({c->hio_in.u8() + p.at, p.src, (size_t)p.len});
    copy_pool(c->device).run(segs);
    // few stripes: the kernels read the page-locked staging and write a page-locked `out` over
    // PCIe, as te_slicer_decode does; more: the staged pieces go to device memory first
    if (se - sb <= kDecSmallStripes) return percall_decode_pinned(c, cfg, nullptr, 0, it, out, (size_t)len, false);
    TE_HIP(c->io_in.ensure(total));
    TE_HIP(c->io_out.ensure(len));
    for (const Piece &p : pieces)
        TE_HIP(hipMemcpyAsync(c->io_in.as<uint8_t>() + p.at, c->hio_in.u8() + p.at, p.len, hipMemcpyHostToDevice, c->stream));
    return percall_decode_device(c, cfg, it, out, (size_t)len, false);
}

// ------------------------------------------------------------------------------------------
// Repair planning (host only)
// ------------------------------------------------------------------------------------------
int te_clay_plan_repair(const te_clay *c, uint32_t lost, const uint32_t *available, size_t navail,
                        uint32_t *helpers_out, uint32_t *sub_chunks_out) {
    if (!c || (!available && navail)) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    if (lost >= (uint32_t)h.n) return TE_ERR_INVALID_SLICE;
    std::vector<int> av(available, available + navail), hs;
    const int r = h.min_to_repair((int)lost, av, hs);
    if (r) return clay_plan_error(r, (int)lost, navail, h.d);
    if (helpers_out)
        for (size_t i = 0; i < hs.size(); i++) helpers_out[i] = (uint32_t)hs[i];
    if (sub_chunks_out) {
        const std::vector<int> pl = h.repair_planes((int)lost);
        for (size_t i = 0; i < pl.size(); i++) sub_chunks_out[i] = (uint32_t)pl[i];
    }
    return TE_OK;
}

int te_repair_plan_from_params(const te_clay *c, int rotated, uint32_t lost, const uint32_t *avail, size_t navail,
                               uint64_t blob_len, uint64_t stripe, te_repair_plan **out) {
    if (!c || !out || (!avail && navail) || stripe == 0) return TE_ERR_INVALID_ARG;
    *out = nullptr;
    const uint64_t ns = blob_len == 0 ? 1 : (blob_len + stripe - 1) / stripe;
    const uint64_t cs = c->h.chunk_size_for(std::min(stripe, blob_len));  // track_chunk_size
    return build_plan(c, rotated, lost, avail, navail, ns, cs, out);
}

int te_repair_plan_from_slice(const te_clay *c, int rotated, uint32_t lost, const uint32_t *avail, size_t navail,
                              const uint8_t *ref, size_t ref_len, te_repair_plan **out) {
    if (!c || !out || !ref) return TE_ERR_INVALID_ARG;
    *out = nullptr;
    te_slice_metadata m;
    if (te_slice_metadata_from_slice(ref, ref_len, &m)) return TE_ERR_INVALID_LAYOUT;
    const uint64_t ns = m.blob_len == 0 ? 1 : (m.blob_len + m.stripe_size - 1) / m.stripe_size;
    const uint64_t total = ref_len >= TE_META_SIZE ? ref_len - TE_META_SIZE : 0;
    if (total == 0 || total % ns) return TE_ERR_INVALID_LAYOUT;
    return build_plan(c, rotated, lost, avail, navail, ns, total / ns, out);
}

void te_repair_plan_free(te_repair_plan *p) { delete p; }

int te_repair_plan_get_info(const te_repair_plan *p, te_repair_plan_info *o) {
    if (!p || !o) return TE_ERR_INVALID_ARG;
    o->lost = p->lost; o->num_stripes = p->ns; o->d = p->d; o->beta = p->beta;
    o->chunk_size = p->cs; o->sub_chunk_size = p->sc;
    return TE_OK;
}

int te_repair_plan_stripe(const te_repair_plan *p, uint32_t st, uint32_t *lost_shard, uint32_t *helper_slices,
                          uint32_t *helper_shards, uint32_t *sub_chunks) {
    if (!p || st >= p->ns) return TE_ERR_INVALID_ARG;
    if (lost_shard) *lost_shard = p->lost_shard[st];
    for (uint32_t j = 0; j < p->d; j++) {
        if (helper_slices) helper_slices[j] = p->helper_slice[st * p->d + j];
        if (helper_shards) helper_shards[j] = p->helper_shard[st * p->d + j];
        if (sub_chunks)
            for (uint32_t b = 0; b < p->beta; b++) sub_chunks[j * p->beta + b] = p->sub_chunks[(st * p->d + j) * p->beta + b];
    }
    return TE_OK;
}

size_t te_extract_repair_data_size(const te_repair_plan *p, uint32_t helper) {
    if (!p) return 0;
    size_t total = 0;
    for (uint32_t st = 0; st < p->ns; st++)
        for (uint32_t j = 0; j < p->d; j++)
            if (p->helper_slice[st * p->d + j] == helper) total += (size_t)p->beta * p->sc;
    return total;
}

int te_extract_repair_data(const te_repair_plan *p, const uint8_t *slice, size_t slice_len, uint32_t helper,
                           uint8_t *out, size_t cap, size_t *out_len) {
    if (!p || !slice) return TE_ERR_INVALID_ARG;
    const size_t need = te_extract_repair_data_size(p, helper);
    if (out_len) *out_len = need;
    if (cap < need || (!out && need)) return TE_ERR_BUFFER_TOO_SMALL;
    size_t w = 0;
    for (uint32_t st = 0; st < p->ns; st++) {
        const uint64_t co = (uint64_t)st * p->cs;
        for (uint32_t j = 0; j < p->d; j++) {
            if (p->helper_slice[st * p->d + j] != helper) continue;
            if (co + p->cs > slice_len) return TE_ERR_INVALID_LAYOUT;  // "slice too short for chunk"
            for (uint32_t b = 0; b < p->beta; b++) {
                const uint64_t z = p->sub_chunks[(st * p->d + j) * p->beta + b];
                if ((z + 1) * p->sc > p->cs) return TE_ERR_INVALID_LAYOUT;  // "sub-chunk out of bounds"
                memcpy(out + w, slice + co + z * p->sc, p->sc);
                w += p->sc;
            }
        }
    }
    return TE_OK;
}

int te_repair_plan_helper_request(const te_repair_plan *p, uint32_t helper, uint32_t *stripes, uint32_t *sub_chunks,
                                  size_t cap_stripes, size_t *count) {
    if (!p || !count) return TE_ERR_INVALID_ARG;
    size_t k = 0;
    for (uint32_t st = 0; st < p->ns; st++)
        for (uint32_t j = 0; j < p->d; j++) {
            if (p->helper_slice[st * p->d + j] != helper) continue;
            if (k < cap_stripes && stripes && sub_chunks) {
                stripes[k] = st;
                memcpy(sub_chunks + k * p->beta, &p->sub_chunks[(st * p->d + j) * p->beta], p->beta * sizeof(uint32_t));
            }
            k++;
        }
    *count = k;
    return k <= cap_stripes || (!stripes && !sub_chunks) ? TE_OK : TE_ERR_BUFFER_TOO_SMALL;
}

int te_serve_repair_request(te_clay *c, const uint8_t *slice, size_t slice_len, const uint32_t *stripes,
                            const uint32_t *nsub, const uint32_t *sub_chunks, size_t nstripes, uint8_t *out, size_t cap,
                            size_t *out_len) {
    if (!c || !slice || (nstripes && (!stripes || !nsub))) return TE_ERR_INVALID_ARG;
    auto fail = [](const char *why) {
        snprintf(g_last_error, sizeof(g_last_error), "%s", why);
        return TE_ERR_INVALID_LAYOUT;
    };
    te_slice_metadata m;
    if (slice_len < TE_META_SIZE) return fail("slice too short for metadata");
    if (te_slice_metadata_from_slice(slice, slice_len, &m) != TE_OK) return fail("parse slice metadata failed");
    if (m.blob_len && !m.stripe_size) return fail("parse slice metadata failed: zero stripe size");
    const uint64_t ns = m.blob_len == 0 ? 1 : (m.blob_len + m.stripe_size - 1) / m.stripe_size;
    const uint64_t total = slice_len - TE_META_SIZE;
    if (total == 0 || total % ns) return fail("slice layout is inconsistent");
    const uint64_t cs = total / ns, alpha = (uint64_t)c->h.alpha;
    if (cs % alpha) return fail("chunk size is not divisible by alpha");
    const uint64_t sc = cs / alpha;
    uint64_t need = 0;
    size_t at = 0;
    for (size_t i = 0; i < nstripes; i++) {
        const uint64_t c0 = (uint64_t)stripes[i] * cs;
        if (c0 + cs > total + TE_META_SIZE) return fail("slice too short for requested stripe");
        for (uint32_t b = 0; b < nsub[i]; b++, at++)
            if (!sub_chunks || ((uint64_t)sub_chunks[at] + 1) * sc > cs) return fail("sub-chunk out of bounds");
        need += (uint64_t)nsub[i] * sc;
    }
    if (out_len) *out_len = (size_t)need;
    if (cap < need || (!out && need)) return TE_ERR_BUFFER_TOO_SMALL;
    uint64_t w = 0;
    at = 0;
    for (size_t i = 0; i < nstripes; i++)
        for (uint32_t b = 0; b < nsub[i]; b++, at++) {
            memcpy(out + w, slice + (uint64_t)stripes[i] * cs + (uint64_t)sub_chunks[at] * sc, sc);
            w += sc;
        }
    return TE_OK;
}

int te_slicer_repair(te_clay *c, const te_repair_plan *p, const uint8_t *const *helper_data, const size_t *helper_lens,
                     const uint8_t metadata[TE_META_SIZE], uint8_t *out, size_t cap) {
    if (!c || !p || !helper_data || !helper_lens || !metadata || !out) return TE_ERR_INVALID_ARG;
    if (p->n != (uint32_t)c->h.n || p->d != (uint32_t)c->h.d) return TE_ERR_INVALID_ARG;
    const size_t out_bytes = (size_t)p->ns * p->cs + TE_META_SIZE;
    if (cap < out_bytes) return TE_ERR_BUFFER_TOO_SMALL;
    // per-helper byte need (Slicer::repair walks a running offset per helper: repair.rs:340-354)
    std::vector<uint64_t> need(p->n, 0), off(p->n, ~0ull);
    for (uint32_t st = 0; st < p->ns; st++)
        for (uint32_t j = 0; j < p->d; j++) need[p->helper_slice[st * p->d + j]] += (uint64_t)p->beta * p->sc;
    uint64_t total = 0;
    for (uint32_t sl = 0; sl < p->n; sl++) {
        if (!need[sl]) continue;
        if (!helper_data[sl] || helper_lens[sl] < need[sl]) return TE_ERR_MISSING_HELPER;
        off[sl] = total;
        total += align16(need[sl]);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    c->rls = te_repair_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    TE_HIP(c->io_in.ensure(total + 16));
    TE_HIP(c->io_out.ensure(out_bytes));
    // the d helpers' buffers gathered into page-locked staging (parallel memcpy), one H2D; the
    // repaired slice back through staging: per call two DMA copies, not d + 1 driver-staged ones
    TE_HIP(c->hio_in.ensure(total + 16));
    TE_HIP(c->hio_out.ensure(out_bytes));
    std::vector<tec::CopyPool::Seg> segs;
    for (uint32_t sl = 0; sl < p->n; sl++)
        if (need[sl]) segs.push_back({c->hio_in.u8() + off[sl], helper_data[sl], need[sl]});
    copy_pool(c->device).run(segs);
    // the kernels read the helpers from and write the slice to the pinned staging directly, over
    // PCIe, with no H2D / D2H copy: 0.131 -> 0.103 ms per 4 MiB call, 0.85 -> 0.73 ms at 64 MiB
    // (r05, scripts/gpu_percall_zc.sh; the repair kernels only read their inputs and write their
    // output once).  Measurement option TEC_DEBUG_KNOBS=1 TEC_REPAIR_ZC=0: the copies instead.
    static const bool zc = [] { const char *e = tec_knob("TEC_REPAIR_ZC"); return !(e && e[0] == '0'); }();
    RepItem it{p, off.data(), 0, metadata};
    if (zc) {
        r = repair_enqueue(c, c->hio_in.u8(), &it, 1, c->hio_out.u8(), c->stream);
        if (r) return r;
    } else {
        TE_HIP(hipMemcpyAsync(c->io_in.p, c->hio_in.p, total, hipMemcpyHostToDevice, c->stream));
        r = repair_enqueue(c, c->io_in.as<uint8_t>(), &it, 1, c->io_out.as<uint8_t>(), c->stream);
        if (r) return r;
        TE_HIP(hipMemcpyAsync(c->hio_out.p, c->io_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    TE_HIP(hipStreamSynchronize(c->stream));  // (an event spin-wait measured no better: 0.146 vs 0.132-0.139 ms, r05)
    // (pipelining the gather with the H2D in four pieces and the scatter with the D2H in two
    // halves measured slower: 0.17 against 0.134-0.143 ms per 4 MiB call, r05)
    copy_pool(c->device).run({{out, c->hio_out.p, out_bytes}});
    return TE_OK;
}

int te_clay_repair(te_clay *c, uint32_t lost, const uint32_t *helpers, const uint8_t *const *helper_data,
                   size_t nhelpers, size_t chunk_size, uint8_t *out) {
    if (!c || !helpers || !helper_data || !out) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    if (lost >= (uint32_t)h.n) return TE_ERR_INVALID_SLICE;
    if (nhelpers != (size_t)h.d) {  // clay_codes::ClayCode::repair rejects it -> RepairError::Clay (repair.rs:85-87)
        snprintf(g_last_error, sizeof(g_last_error), "repair: need exactly d=%d helpers, got %zu", h.d, nhelpers);
        return TE_ERR_CLAY;
    }
    if (chunk_size == 0 || chunk_size % (size_t)h.alpha) return TE_ERR_INVALID_LAYOUT;
    // one-stripe, identity-mapped plan with the caller's helper set
    te_repair_plan p;
    p.lost = lost; p.ns = 1; p.d = (uint32_t)h.d; p.beta = (uint32_t)h.beta; p.n = (uint32_t)h.n;
    p.cs = chunk_size; p.sc = chunk_size / (size_t)h.alpha;
    p.lost_shard.push_back(lost);
    const std::vector<int> planes = h.repair_planes((int)lost);
    std::vector<const uint8_t *> by_slice(h.n, nullptr);
    std::vector<size_t> lens(h.n, 0);
    std::vector<int> hs;
    for (size_t j = 0; j < nhelpers; j++) {
        if (helpers[j] >= (uint32_t)h.n || helpers[j] == lost) return TE_ERR_INVALID_SLICE;
        hs.push_back((int)helpers[j]);
    }
    std::sort(hs.begin(), hs.end());
    for (size_t j = 0; j < nhelpers; j++) {
        by_slice[helpers[j]] = helper_data[j];
        lens[helpers[j]] = (size_t)h.beta * p.sc;
    }
    for (int sh : hs) {
        p.helper_shard.push_back((uint32_t)sh);
        p.helper_slice.push_back((uint32_t)sh);
        for (int z : planes) p.sub_chunks.push_back((uint32_t)z);
    }
    std::vector<uint8_t> tmp(chunk_size + TE_META_SIZE);
    uint8_t meta[TE_META_SIZE] = {0};
    int r = te_slicer_repair(c, &p, by_slice.data(), lens.data(), meta, tmp.data(), tmp.size());
    if (r) return r;
    memcpy(out, tmp.data(), chunk_size);
    return TE_OK;
}


// ---- slice commitments (lib/crypto/src/merkle/tree.rs) ----
int te_hash_leaf(const uint8_t *data, size_t len, uint8_t out[TE_HASH_SIZE]) {
    if ((!data && len) || !out) return TE_ERR_INVALID_ARG;
    hh::hash_leaf(data, len, out);
    return TE_OK;
}

int te_hash_leaves(const uint8_t *data, size_t len, size_t count, uint32_t lanes, uint8_t *out) {
    if ((!data && len && count) || (!out && count) || lanes > (uint32_t)hh::kMaxLanes) return TE_ERR_INVALID_ARG;
    if (lanes == 0) lanes = (uint32_t)hh::Pool::get().lanes();
    const uint8_t *src[hh::kMaxLanes];
    uint8_t *dst[hh::kMaxLanes];
    for (size_t i0 = 0; i0 < count; i0 += lanes) {
        const int L = (int)std::min<size_t>(lanes, count - i0);
        for (int l = 0; l < L; l++) {
            src[l] = data + (i0 + l) * len;
            dst[l] = out + (i0 + l) * TE_HASH_SIZE;
        }
        hh::hash_leaves(L, src, len, dst);
    }
    return TE_OK;
}

int te_hash_pair(const uint8_t left[TE_HASH_SIZE], const uint8_t right[TE_HASH_SIZE], uint8_t out[TE_HASH_SIZE]) {
    if (!left || !right || !out) return TE_ERR_INVALID_ARG;
    sha::hash_pair(left, right, out);
    return TE_OK;
}

int te_empty_subtree_root(uint32_t height, uint8_t out[TE_HASH_SIZE]) {
    if (height >= TE_MAX_MERKLE_TREE_HEIGHT || !out) return TE_ERR_INVALID_ARG;
    sha::empty_root(height, out);
    return TE_OK;
}

// MerkleTree::<N>::new() + add_leaf_hash per leaf (tree.rs:86-153, 344-350)
int te_merkle_root_from_leaf_hashes(const uint8_t *hashes, size_t count, uint32_t height, uint8_t out[TE_HASH_SIZE]) {
    if (height == 0 || height > TE_MAX_MERKLE_TREE_HEIGHT || (!hashes && count) || !out) return TE_ERR_INVALID_ARG;
    if (height < 64 && (uint64_t)count > (1ull << height)) return TE_ERR_MERKLE_TREE_FULL;
    std::vector<std::array<uint8_t, 32>> empty(height), filled(height);
    for (uint32_t l = 0; l < height; l++) {
        sha::empty_root(l, empty[l].data());
        filled[l] = empty[l];
    }
    std::array<uint8_t, 32> root = empty[height - 1];
    for (size_t index = 0; index < count; index++) {
        std::array<uint8_t, 32> cur, t;
        memcpy(cur.data(), hashes + index * 32, 32);
        uint64_t idx = index;
        for (uint32_t l = 0; l < height; l++) {
            if ((idx & 1) == 0) {
                filled[l] = cur;
                sha::hash_pair(cur.data(), empty[l].data(), t.data());
            } else {
                sha::hash_pair(filled[l].data(), cur.data(), t.data());
            }
            cur = t;
            idx >>= 1;
        }
        root = cur;
    }
    memcpy(out, root.data(), 32);
    return TE_OK;
}

// create_merkle_proof_hashes (tree.rs:397-455)
int te_merkle_proof_from_leaf_hashes(const uint8_t *hashes, size_t count, size_t index, uint32_t height,
                                     uint8_t *proof_out) {
    if (!proof_out) return TE_ERR_INVALID_ARG;
    if (!hashes || count == 0 || index >= count || height > TE_MAX_MERKLE_TREE_HEIGHT ||
        (height < 64 && (uint64_t)count > (1ull << height)))
        return TE_ERR_MERKLE_INVALID_PROOF;
    std::vector<std::array<uint8_t, 32>> cur(count);
    for (size_t i = 0; i < count; i++) memcpy(cur[i].data(), hashes + i * 32, 32);
    std::array<uint8_t, 32> empty;
    sha::empty_root(0, empty.data());
    size_t ci = index;
    for (uint32_t l = 0; l < height; l++) {
        if (cur.size() % 2) cur.push_back(empty);
        memcpy(proof_out + (size_t)l * 32, cur[ci ^ 1].data(), 32);
        std::vector<std::array<uint8_t, 32>> next(cur.size() / 2);
        for (size_t j = 0; j < next.size(); j++) sha::hash_pair(cur[2 * j].data(), cur[2 * j + 1].data(), next[j].data());
        cur.swap(next);
        std::array<uint8_t, 32> e2;
        sha::hash_pair(empty.data(), empty.data(), e2.data());
        empty = e2;
        ci >>= 1;
    }
    return TE_OK;
}

// verify_proof (tree.rs:462-481), leaf already hashed
int te_merkle_verify_leaf_hash(const uint8_t leaf_hash[TE_HASH_SIZE], const uint8_t root[TE_HASH_SIZE],
                               const uint8_t *proof, size_t proof_len, uint64_t index, uint32_t height) {
    if (!leaf_hash || !root || (!proof && proof_len)) return TE_ERR_INVALID_ARG;
    if (proof_len != height) return 0;
    uint8_t node[32], t[32];
    memcpy(node, leaf_hash, 32);
    uint64_t idx = index;
    for (size_t i = 0; i < proof_len; i++) {
        if ((idx & 1) == 0) sha::hash_pair(node, proof + i * 32, t);
        else sha::hash_pair(proof + i * 32, node, t);
        memcpy(node, t, 32);
        idx >>= 1;
    }
    return memcmp(node, root, 32) == 0 ? 1 : 0;
}

int te_commit_batch_device(const uint8_t *d_slices, uint64_t obj_stride, uint64_t slice_len, uint32_t n,
                           size_t nobj, uint32_t height, uint8_t *d_leaf_hashes, uint8_t *d_roots,
                           uint8_t *d_proofs, void *stream) {
    if (nobj == 0) return TE_OK;
    // the leaf kernel reads every slice as dwords: its base, its length and the object stride are 4-aligned
    if (!d_slices || !d_leaf_hashes || n == 0 || n > TE_COMMIT_MAX_LEAVES || slice_len % 4 || obj_stride % 4 ||
        (reinterpret_cast<uintptr_t>(d_slices) & 3u) || nobj > 0xffffffffull / n || ((d_roots || d_proofs) && (height == 0 || height > TE_MAX_MERKLE_TREE_HEIGHT)) ||
        (d_proofs && !d_roots))
        return TE_ERR_INVALID_ARG;
    if ((d_roots || d_proofs) && height < 64 && (uint64_t)n > (1ull << height)) return TE_ERR_MERKLE_TREE_FULL;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    CommitArgs a{};
    a.slices = d_slices;
    a.obj_stride = obj_stride;
    a.slice_len = slice_len;
    a.n = n;
    a.nobj = (uint32_t)nobj;
    a.height = height;
    a.leaf = d_leaf_hashes;
    a.root = d_roots;
    a.proof = d_proofs;
    hipStream_t s = (hipStream_t)stream;
    KTimer kt(s);
    TE_HIP(launch_commit(a, s));
    kt.stop();
    return TE_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Data verify (root_check.hip): verify_track_data's coded branch (sdk/src/track/read.rs:174-185)
// -- BlobEncoder::encode_with_root (sdk/src/codec/encoder.rs:166-193) and the compare with
// blob.commitment -- with the slices kept in HBM
// ------------------------------------------------------------------------------------------
namespace {

// the tree arguments every data-verify entry point shares, checked before any device call
int verify_data_tree_args(const te_clay *c, uint32_t height) {
    if (height == 0 || height > TE_MAX_MERKLE_TREE_HEIGHT) return TE_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)c->h.n;
    if (n > TE_COMMIT_MAX_LEAVES) return TE_ERR_INVALID_ARG;
    if ((uint64_t)n > (1ull << height)) return TE_ERR_MERKLE_TREE_FULL;
    return TE_OK;
}

// The device batch's work buffer: the objects' slices back to back (each n * slice_len, a multiple
// of 4), padded to 32 bytes, then nobj * n leaf hashes.
struct VerifyWork {
    std::vector<te_object> local;       // the encode's descriptors: out_off = the slices' place
    std::vector<uint64_t> slice_len;
    uint64_t leaf_at = 0, bytes = 0;
};
int verify_work_layout(const te_clay *c, const te_object *objs, size_t nobj, VerifyWork &W) {
    const uint64_t n = (uint64_t)c->h.n;
    W.local.resize(nobj);
    W.slice_len.resize(nobj);
    uint64_t at = 0;
    for (size_t o = 0; o < nobj; o++) {
        te_geometry g;
        te_slicer_geometry(c, objs[o].blob_len, &g);
        if (g.slice_len % 4) return TE_ERR_INVALID_ARG;  // the leaf kernel reads dwords
        W.local[o] = te_object{objs[o].data_off, objs[o].blob_len, at, objs[o].chunk_index};
        W.slice_len[o] = g.slice_len;
        at += n * g.slice_len;
    }
    W.leaf_at = (at + 31) & ~(uint64_t)31;
    W.bytes = W.leaf_at + (uint64_t)nobj * n * TE_HASH_SIZE;
    return TE_OK;
}

// Encode into d_work, hash each run of equal slice lengths, root-check every object: all enqueued
// on s (handle locked, its device current).
int verify_data_enqueue(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_data, const VerifyWork &W,
                        uint32_t height, const uint8_t *d_expected_roots, const uint8_t *d_expected_leaves,
                        uint8_t *d_work, uint8_t *d_roots, uint32_t *d_ok, uint64_t *d_bad_leaf_mask, hipStream_t s,
                        bool per_call) {
    const size_t nobj = W.local.size();
    const uint32_t n = (uint32_t)c->h.n;
    const uint64_t leaf_b = (uint64_t)n * TE_HASH_SIZE;
    int r = encode_enqueue(c, cfg, d_data, W.local.data(), nobj, d_work, s, false, nullptr, StripeSel(), per_call);
    if (r) return r;
    KTimer kt(s);
    for (size_t o = 0; o < nobj;) {
        size_t e = o + 1;
        while (e < nobj && W.slice_len[e] == W.slice_len[o]) e++;
        CommitArgs ca{};
        ca.slices = d_work + W.local[o].out_off;
        ca.obj_stride = (uint64_t)n * W.slice_len[o];
        ca.slice_len = W.slice_len[o];
        ca.n = n;
        ca.nobj = (uint32_t)(e - o);
        ca.height = height;
        ca.leaf = d_work + W.leaf_at + o * leaf_b;
        TE_HIP(launch_commit(ca, s));
        c->vds.groups++;
        c->vds.leaf_launches += commit_leaf_launches(ca.slice_len);
        o = e;
    }
    RootCheckArgs ra{};
    ra.leaf = d_work + W.leaf_at;
    ra.expected_root = d_expected_roots;
    ra.expected_leaf = d_expected_leaves;
    ra.root = d_roots;
    ra.ok = d_ok;
    ra.bad_leaf_mask = d_bad_leaf_mask;
    ra.nobj = nobj;
    ra.n = n;
    ra.height = height;
    TE_HIP(launch_root_check(ra, s));
    kt.stop();
    c->vds.objects = nobj;
    c->vds.windows = 1;
    c->vds.root_check_launches = 1;
    return TE_OK;
}

}  // namespace

extern "C" {

int te_roots_check_device(const uint8_t *d_leaf_hashes, uint32_t n, size_t nobj, uint32_t height,
                          const uint8_t *d_expected_roots, const uint8_t *d_expected_leaves, uint8_t *d_roots,
                          uint32_t *d_ok, uint64_t *d_bad_leaf_mask, void *stream) {
    auto odd = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (n == 0 || n > TE_COMMIT_MAX_LEAVES || height > TE_MAX_MERKLE_TREE_HEIGHT || (uint64_t)n > (1ull << height) ||
        !d_leaf_hashes || !d_expected_roots || !d_ok || nobj > 0xffffffffull / n || odd(d_leaf_hashes) ||
        odd(d_expected_roots) || odd(d_expected_leaves) || odd(d_roots) || odd(d_ok) ||
        (reinterpret_cast<uintptr_t>(d_bad_leaf_mask) & 7u))
        return TE_ERR_INVALID_ARG;
    if (nobj == 0) return TE_OK;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    RootCheckArgs a{};
    a.leaf = d_leaf_hashes;
    a.expected_root = d_expected_roots;
    a.expected_leaf = d_expected_leaves;
    a.root = d_roots;
    a.ok = d_ok;
    a.bad_leaf_mask = d_bad_leaf_mask;
    a.nobj = nobj;
    a.n = n;
    a.height = height;
    hipStream_t s = (hipStream_t)stream;
    KTimer kt(s);
    TE_HIP(launch_root_check(a, s));
    kt.stop();
    return TE_OK;
}

size_t te_verify_data_work_bytes(const te_clay *c, const te_object *objs, size_t nobj) {
    if (!c || (!objs && nobj)) return 0;
    VerifyWork W;
    if (verify_work_layout(c, objs, nobj, W)) return 0;
    return (size_t)W.bytes;
}

int te_verify_data_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_data, const te_object *objs,
                                size_t nobj, uint32_t height, const uint8_t *d_expected_roots,
                                const uint8_t *d_expected_leaves, uint8_t *d_work, size_t work_bytes, uint8_t *d_roots,
                                uint32_t *d_ok, uint64_t *d_bad_leaf_mask, void *stream) {
    if (!c || !cfg || (!objs && nobj) || (nobj && (!d_data || !d_expected_roots || !d_work || !d_ok)))
        return TE_ERR_INVALID_ARG;
    if (int r = verify_data_tree_args(c, height)) return r;
    if ((reinterpret_cast<uintptr_t>(d_work) & 15u) || nobj > 0xffffffffull / (size_t)c->h.n) return TE_ERR_INVALID_ARG;
    VerifyWork W;
    if (int r = verify_work_layout(c, objs, nobj, W)) return r;
    if (work_bytes < W.bytes) return TE_ERR_BUFFER_TOO_SMALL;
    if (nobj == 0) return TE_OK;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->els = te_encode_launch_stats{};
    c->vds = te_verify_data_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return verify_data_enqueue(c, cfg, d_data, W, height, d_expected_roots, d_expected_leaves, d_work, d_roots, d_ok,
                               d_bad_leaf_mask, (hipStream_t)stream, false);
}

int te_verify_data_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data, const te_object *objs,
                              size_t nobj, uint32_t height, const uint8_t *h_expected_roots,
                              const uint8_t *h_expected_leaves, uint8_t *h_roots, uint32_t *h_ok,
                              uint64_t *h_bad_leaf_mask, size_t window_bytes) {
    if (!c || !cfg || (!objs && nobj) || (nobj && (!h_data || !h_expected_roots || !h_ok))) return TE_ERR_INVALID_ARG;
    if (int r = verify_data_tree_args(c, height)) return r;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    const uint64_t leaf_b = (uint64_t)c->h.n * TE_HASH_SIZE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->vds = te_verify_data_stats{};
    if (nobj == 0) return TE_OK;
    // the page-locked staging block: expected roots, expected leaves | roots, masks, verdicts
    const uint64_t xleaf_at = nobj * TE_HASH_SIZE, root_at = xleaf_at + (h_expected_leaves ? nobj * leaf_b : 0),
                   mask_at = root_at + nobj * TE_HASH_SIZE, ok_at = mask_at + nobj * 8, total = ok_at + nobj * 4;
    {
        DeviceGuard dg(c->device);
        TE_HIP(dg.err);
        TE_HIP(c->ver_host.ensure(total));
    }
    uint8_t *st = c->ver_host.u8();
    memcpy(st, h_expected_roots, nobj * TE_HASH_SIZE);
    if (h_expected_leaves) memcpy(st + xleaf_at, h_expected_leaves, nobj * leaf_b);
    VerifyData vd;
    vd.exp_root = st;
    vd.exp_leaf = h_expected_leaves ? st + xleaf_at : nullptr;
    vd.root = h_roots ? st + root_at : nullptr;
    vd.mask = h_bad_leaf_mask ? reinterpret_cast<uint64_t *>(st + mask_at) : nullptr;
    vd.ok = reinterpret_cast<uint32_t *>(st + ok_at);
    vd.st = &c->vds;
    const CommitOut co{nullptr, nullptr, nullptr, height};
    // default group 8 GiB: a group costs one slice's SHA-256 chain (~30 ms at 4 MiB objects) whatever
    // it holds and nothing is copied out meanwhile, so fewer groups are faster -- 1024 x 4 MiB: 532 ms
    // at 1 GiB (18 groups), 166 at 4 GiB (5), 137 at 8 GiB (3), 115 in one group;
    // 8 GiB keeps the three resident group buffers at 6.3 GB each
    if (window_bytes == 0) window_bytes = (size_t)8 << 30;
    const int rc = encode_commit_host_impl(c, cfg, h_data, objs, nobj, nullptr, window_bytes, co, &vd);
    if (rc) return rc;
    if (h_roots) memcpy(h_roots, st + root_at, nobj * TE_HASH_SIZE);
    if (h_bad_leaf_mask && h_expected_leaves) memcpy(h_bad_leaf_mask, st + mask_at, nobj * 8);
    memcpy(h_ok, st + ok_at, nobj * 4);
    return TE_OK;
}

int te_slicer_verify_data(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *data, size_t len, uint32_t height,
                          const uint8_t expected_root[TE_HASH_SIZE], uint8_t observed_root[TE_HASH_SIZE], int *ok) {
    if (!c || !cfg || (!data && len) || !expected_root || !ok) return TE_ERR_INVALID_ARG;
    if (int r = verify_data_tree_args(c, height)) return r;
    const te_object obj{0, len, 0, cfg->chunk_index};
    VerifyWork W;
    if (int r = verify_work_layout(c, &obj, 1, W)) return r;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->els = te_encode_launch_stats{};
    c->vds = te_verify_data_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    // the handle's staging: the object in io_in, the work buffer in io_out with the expected root,
    // the observed root and the verdict behind it; their host side in ver_host
    const uint64_t xroot_at = (W.bytes + 31) & ~(uint64_t)31, root_at = xroot_at + TE_HASH_SIZE, ok_at = root_at + TE_HASH_SIZE;
    TE_HIP(c->io_in.ensure(len + 16));
    TE_HIP(c->io_out.ensure(ok_at + 4));
    TE_HIP(c->ver_host.ensure(2 * TE_HASH_SIZE + 4));
    uint8_t *hst = c->ver_host.u8(), *dw = c->io_out.as<uint8_t>();
    memcpy(hst, expected_root, TE_HASH_SIZE);
    if (len) TE_HIP(hipMemcpyAsync(c->io_in.p, data, len, hipMemcpyHostToDevice, c->stream));
    TE_HIP(hipMemcpyAsync(dw + xroot_at, hst, TE_HASH_SIZE, hipMemcpyHostToDevice, c->stream));
    r = verify_data_enqueue(c, cfg, c->io_in.as<uint8_t>(), W, height, dw + xroot_at, nullptr, dw, dw + root_at,
                            reinterpret_cast<uint32_t *>(dw + ok_at), nullptr, c->stream, true);
    if (r) return r;
    TE_HIP(hipMemcpyAsync(hst + TE_HASH_SIZE, dw + root_at, TE_HASH_SIZE + 4, hipMemcpyDeviceToHost, c->stream));
    TE_HIP(hipStreamSynchronize(c->stream));
    c->vds.h2d_bytes = len;
    c->vds.h2d_expected_bytes = TE_HASH_SIZE;
    c->vds.d2h_bytes = TE_HASH_SIZE + 4;
    if (observed_root) memcpy(observed_root, hst + TE_HASH_SIZE, TE_HASH_SIZE);
    uint32_t v;
    memcpy(&v, hst + 2 * TE_HASH_SIZE, 4);
    *ok = v ? 1 : 0;
    return TE_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Verified reads (verify.hip): BlobEncoding::verify_slice (lib/core/src/track/blob.rs:72-79) and
// its call sites -- the gateway's object read (network/gateway/src/http/handlers/object/
// decode.rs:121-139), node recover (recover.rs:207-218) and repair (repair.rs:339-341)
// ------------------------------------------------------------------------------------------
namespace {

// The kernel's walk order: by block count, descending, equal counts in the caller's order.
void verify_order(const te_verify_item *items, size_t nitems, std::vector<uint32_t> &order) {
    order.resize(nitems);
    for (size_t i = 0; i < nitems; i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return verify_blocks(items[x].len) > verify_blocks(items[y].len);
    });
}

int verify_check_items(const te_verify_item *items, size_t nitems) {
    if (nitems > 0xffffffffull || (!items && nitems)) return TE_ERR_INVALID_ARG;
    for (size_t i = 0; i < nitems; i++)
        if (items[i].len % 4u || items[i].offset % 4u) return TE_ERR_INVALID_ARG;
    return TE_OK;
}

// Handle locked, its device current: the sorted item list through the handle's descriptor arena,
// then the launches.
int verify_enqueue(te_clay *c, const uint8_t *d_data, const te_verify_item *items, size_t nitems,
                   const uint8_t *d_expected, uint8_t *d_digests, uint32_t *d_ok, uint32_t *d_good_mask,
                   hipStream_t s) {
    if (nitems == 0) return TE_OK;
    std::vector<uint32_t> order;
    verify_order(items, nitems, order);
    std::vector<VerifyItem> v(nitems);
    for (size_t j = 0; j < nitems; j++) {
        const te_verify_item &t = items[order[j]];
        v[j] = VerifyItem{t.offset, t.len, t.expected, t.object, t.bit, order[j]};
    }
    Arena &A = c->ver;
    A.img.clear();
    const size_t off = A.put(v.data(), v.size() * sizeof(VerifyItem));
    int r = A.upload(s);
    if (r) return r;
    VerifyArgs a{};
    a.data = d_data;
    a.items = A.at<VerifyItem>(off);
    a.nitems = (uint32_t)nitems;
    a.expected = d_expected;
    a.digests = d_digests;
    a.ok = d_ok;
    a.good_mask = d_good_mask;
    KTimer kt(s);
    TE_HIP(launch_verify(a, v.data(), s));
    kt.stop();
    return A.mark_done(s);
}

// Device hashing in a verify workspace (the handle's or a window slot's) of layout L: the expected
// leaves on the device and every mask array zeroed ...
int ver_begin(DevBuf &ver, HostBuf &verh, const VerLayout &L, const uint8_t *h_leaves, hipStream_t s) {
    TE_HIP(ver.ensure(L.total()));
    TE_HIP(verh.ensure(L.h_total()));
    memcpy(verh.p, h_leaves, L.exp_b);
    TE_HIP(hipMemcpyAsync(ver.p, verh.p, L.exp_b, hipMemcpyHostToDevice, s));
    TE_HIP(hipMemsetAsync(ver.as<uint8_t>() + L.mask_off(0), 0, L.narr * L.mask_b, s));
    return TE_OK;
}

// ... then `items` of d_data hashed into mask array `which` (0: peers, 1: rebuilt slices) and that
// array's D2H copy to the workspace's host side.
int ver_masks(te_clay *c, DevBuf &ver, HostBuf &verh, const uint8_t *d_data, const std::vector<te_verify_item> &items,
              const VerLayout &L, int which, hipStream_t s) {
    uint8_t *const d = ver.as<uint8_t>();
    uint32_t *const d_mask = reinterpret_cast<uint32_t *>(d + L.mask_off(which));
    if (int r = verify_enqueue(c, d_data, items.data(), items.size(), d, d + L.dig_off(which), nullptr, d_mask, s)) return r;
    TE_HIP(hipMemcpyAsync(verh.u8() + L.h_mask(which), d_mask, L.mask_b, hipMemcpyDeviceToHost, s));
    return TE_OK;
}

// Handle locked, its device current.  Verify `items` (their `expected` index h_expected's nexp
// hashes, their `object` one of nmask masks) in the handle's workspace and WAIT for the masks:
// h_good[o] = the bits of object o's matching items.
int verify_wait(te_clay *c, const uint8_t *d_data, const std::vector<te_verify_item> &items, const uint8_t *h_expected,
                size_t nexp, size_t nmask, uint32_t *h_good, hipStream_t s) {
    for (size_t o = 0; o < nmask; o++) h_good[o] = 0;
    if (items.empty()) return TE_OK;
    const VerLayout L{nexp * TE_HASH_SIZE, items.size() * TE_HASH_SIZE, 0, nmask * sizeof(uint32_t), 1};
    int r = ver_begin(c->ver_buf, c->ver_host, L, h_expected, s);
    if (!r) r = ver_masks(c, c->ver_buf, c->ver_host, d_data, items, L, 0, s);
    if (!r) r = sync_sleep(s);
    if (r) return r;
    memcpy(h_good, c->ver_host.u8() + L.h_mask(0), L.mask_b);
    return TE_OK;
}

inline uint32_t slice_bits(const te_clay *c) { return c->h.n >= 32 ? 0xffffffffu : (1u << c->h.n) - 1u; }

// One verify item per present slice of an object whose slices lie slice_len apart.
void verify_push_slices(std::vector<te_verify_item> &vi, size_t obj, uint32_t n, uint64_t slices_off, uint64_t slice_len,
                        uint32_t avail) {
    for (uint32_t b = 0; b < n; b++)
        if ((avail >> b) & 1u)
            vi.push_back(te_verify_item{slices_off + (uint64_t)b * slice_len, slice_len, (uint32_t)(obj * n + b),
                                        (uint32_t)obj, 1u << b, 0});
}

// One object's survivor set once its slices are hashed: ok = the present slices (`avail`) that
// matched (`good`), the others into *rej; an object that passed on its present slices (`pre`, the
// caller's validation before anything was enqueued) is validated again on ok, and that is its
// *status.  Returns the status; with TE_OK, `it` is the object's decode item and ok what it reads.
int resolve_survivors(const te_clay *c, uint32_t avail, uint64_t slice_len, const uint8_t *meta, int pre, uint32_t good,
                      uint32_t *rej, int *status, uint32_t &ok, DecItem &it) {
    ok = avail & good;
    if (rej) *rej = avail & ~ok;
    int st = pre;
    if (!st) st = decode_validate(c, meta, slice_len, ok, it);
    if (status) *status = st;
    if (st) ok = 0;
    return st;
}

}  // namespace

extern "C" {

int te_verify_slice(const uint8_t *leaves, uint32_t n, uint32_t position, const uint8_t *data, size_t len) {
    if (!leaves || (!data && len) || position >= n) return 0;
    uint8_t d[TE_HASH_SIZE];
    hh::hash_leaf(data, len, d);
    return memcmp(d, leaves + (size_t)position * TE_HASH_SIZE, TE_HASH_SIZE) == 0 ? 1 : 0;
}

int te_verify_order(const te_verify_item *items, size_t nitems, uint32_t *order) {
    if ((!items || !order) && nitems) return TE_ERR_INVALID_ARG;
    if (nitems > 0xffffffffull) return TE_ERR_INVALID_ARG;
    std::vector<uint32_t> o;
    verify_order(items, nitems, o);
    if (nitems) memcpy(order, o.data(), nitems * sizeof(uint32_t));
    return TE_OK;
}

int te_verify_leaves_device(te_clay *c, const uint8_t *d_data, const te_verify_item *items, size_t nitems,
                            const uint8_t *d_expected, uint8_t *d_digests, uint32_t *d_ok, uint32_t *d_good_mask,
                            void *stream) {
    if (!c) return TE_ERR_INVALID_ARG;
    if (nitems == 0) return TE_OK;
    if (!d_digests) return TE_ERR_INVALID_ARG;
    int r = verify_check_items(items, nitems);
    if (r) return r;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return verify_enqueue(c, d_data, items, nitems, d_expected, d_digests, d_ok, d_good_mask, (hipStream_t)stream);
}

}  // extern "C"
namespace {
// te_decode_verified_batch_device's work after its argument checks: handle locked, its device
// current (te_snapshot_decode_device runs it under its own lock).
int decode_verified_locked(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const te_decode_object *objs,
                           const uint8_t *h_meta, const uint8_t *h_leaves, size_t nobj, uint8_t *d_out,
                           uint32_t *h_rejected_mask, int *h_status, hipStream_t s) {
    const uint32_t n = (uint32_t)c->h.n, all = slice_bits(c);
    std::vector<DecItem> items(nobj);
    std::vector<te_verify_item> vi;
    for (size_t i = 0; i < nobj; i++) {
        // an object with too few slices to begin with is that object's outcome, not the call's
        // (the device entry points validate on the caller's unmasked avail_mask, the host pipelines
        // on avail_mask & all)
        const int r = decode_validate(c, h_meta + i * TE_META_SIZE, objs[i].slice_len, objs[i].avail_mask, items[i]);
        if (r && r != TE_ERR_NOT_ENOUGH_SLICES) return r;
        h_status[i] = r;
        verify_push_slices(vi, i, n, objs[i].slices_off, objs[i].slice_len, objs[i].avail_mask & all);
    }
    std::vector<uint32_t> good(nobj);
    int r = verify_wait(c, d_slices, vi, h_leaves, nobj * n, nobj, good.data(), s);
    if (r) return r;
    std::vector<DecItem> run;
    for (size_t i = 0; i < nobj; i++) {
        uint32_t ok;
        DecItem it{};
        if (resolve_survivors(c, objs[i].avail_mask & all, objs[i].slice_len, h_meta + i * TE_META_SIZE, h_status[i], good[i],
                              h_rejected_mask ? h_rejected_mask + i : nullptr, h_status + i, ok, it))
            continue;
        it.in_base = objs[i].slices_off;
        it.out_off = objs[i].out_off;
        run.push_back(it);
    }
    c->dls = te_decode_launch_stats{};
    if (run.empty()) return TE_OK;
    return decode_enqueue(c, cfg, d_slices, run.data(), run.size(), d_out, s, false);
}
}  // namespace
extern "C" {

int te_decode_verified_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                    const te_decode_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                    size_t nobj, uint8_t *d_out, uint32_t *h_rejected_mask, int *h_status,
                                    void *stream) {
    if (!c || !cfg || ((!objs || !h_meta || !h_leaves || !h_status) && nobj)) return TE_ERR_INVALID_ARG;
    if (nobj > 0xffffffffull / (uint32_t)c->h.n) return TE_ERR_INVALID_ARG;
    for (size_t i = 0; i < nobj; i++)
        if (objs[i].slice_len % 4u || objs[i].slices_off % 4u) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return decode_verified_locked(c, cfg, d_slices, objs, h_meta, h_leaves, nobj, d_out, h_rejected_mask, h_status,
                                  (hipStream_t)stream);
}

}  // extern "C"
namespace {
// The verified recover forms' work after their own argument checks (`pre`: each object's outcome
// on its present slices, `items` filled where that is TE_OK): the peers verified, the objects with
// k verified peers rebuilt from those -- lost_mask stays what the caller asked for -- and one
// launch over every rebuilt slice of every object; h_ok_mask[i] = the rebuilt slices that match.
int recover_verified(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices, const te_recover_multi_object *objs,
                     std::vector<RecItem> &items, const std::vector<int> &pre, const uint8_t *h_meta, const uint8_t *h_leaves,
                     uint8_t *d_out, uint32_t *h_rejected_mask, uint32_t *h_ok_mask, int *h_status, hipStream_t s) {
    const size_t nobj = items.size();
    const uint32_t n = (uint32_t)c->h.n, all = slice_bits(c);
    std::vector<te_verify_item> vi;
    for (size_t i = 0; i < nobj; i++) {
        h_ok_mask[i] = 0;
        verify_push_slices(vi, i, n, objs[i].slices_off, objs[i].slice_len, objs[i].avail_mask & all);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    c->els = te_encode_launch_stats{};
    c->rms = te_recover_multi_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    std::vector<uint32_t> good(nobj);
    int r = verify_wait(c, d_slices, vi, h_leaves, nobj * n, nobj, good.data(), s);
    if (r) return r;
    std::vector<RecItem> run;
    std::vector<size_t> run_of;
    for (size_t i = 0; i < nobj; i++) {
        uint32_t ok;
        if (resolve_survivors(c, objs[i].avail_mask & all, objs[i].slice_len, h_meta + i * TE_META_SIZE, pre[i], good[i],
                              h_rejected_mask ? h_rejected_mask + i : nullptr, h_status + i, ok, items[i].it))
            continue;
        items[i].it.in_base = objs[i].slices_off;
        run.push_back(items[i]);
        run_of.push_back(i);
    }
    if (run.empty()) return TE_OK;
    if ((r = recover_enqueue(c, cfg, d_slices, run, d_out, s, c->rms))) return r;
    vi.clear();
    for (size_t i : run_of)
        rec_each_lost(objs[i].lost_mask, [&](uint32_t sl, uint64_t j) {
            vi.push_back(te_verify_item{objs[i].out_off + j * objs[i].slice_len, objs[i].slice_len, (uint32_t)(i * n + sl),
                                        (uint32_t)i, 1u << sl, 0});
        });
    if ((r = verify_wait(c, d_out, vi, h_leaves, nobj * n, nobj, good.data(), s))) return r;
    for (size_t i : run_of) h_ok_mask[i] = good[i] & objs[i].lost_mask;
    return TE_OK;
}
}  // namespace
extern "C" {

// The single form: its own argument rule (rec_single), and nothing validated without a device;
// h_ok[i] is bit `lost` of the mask, as 0 or 1
int te_recover_verified_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                     const te_recover_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                     size_t nobj, uint8_t *d_out, uint32_t *h_rejected_mask, uint32_t *h_ok,
                                     int *h_status, void *stream) {
    if (!c || !cfg || ((!objs || !h_meta || !h_leaves || !h_status || !h_ok) && nobj)) return TE_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)c->h.n;
    if (nobj > 0xffffffffull / n) return TE_ERR_INVALID_ARG;
    for (size_t i = 0; i < nobj; i++) {
        if (objs[i].slice_len % 4u || objs[i].slices_off % 4u || objs[i].out_off % 4u) return TE_ERR_INVALID_ARG;
        if (objs[i].lost >= n) return TE_ERR_INVALID_SLICE;
    }
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::vector<te_recover_multi_object> mo(nobj);
    std::vector<RecItem> items(nobj);
    std::vector<int> pre(nobj, TE_OK);
    for (size_t i = 0; i < nobj; i++) {
        mo[i] = rec_single(c, objs[i]);
        // on the caller's unmasked avail_mask, as te_decode_verified_batch_device
        const int r = rec_validate(c, mo[i], h_meta + i * TE_META_SIZE, true, items[i]);
        if (r && r != TE_ERR_NOT_ENOUGH_SLICES) return r;
        h_status[i] = pre[i] = r;
        h_ok[i] = 0;
    }
    const int r = recover_verified(c, cfg, d_slices, mo.data(), items, pre, h_meta, h_leaves, d_out, h_rejected_mask, h_ok,
                                   h_status, (hipStream_t)stream);
    for (size_t i = 0; i < nobj; i++) h_ok[i] = (h_ok[i] >> objs[i].lost) & 1u;
    return r;
}

// The multi form: every argument check comes before the call looks for a device.
int te_recover_multi_verified_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                           const te_recover_multi_object *objs, const uint8_t *h_meta,
                                           const uint8_t *h_leaves, size_t nobj, uint8_t *d_out,
                                           uint32_t *h_rejected_mask, uint32_t *h_ok_mask, int *h_status, void *stream) {
    if (!c || !cfg || ((!objs || !h_meta || !h_leaves || !h_status || !h_ok_mask) && nobj)) return TE_ERR_INVALID_ARG;
    if (nobj > 0xffffffffull / (uint32_t)c->h.n) return TE_ERR_INVALID_ARG;
    std::vector<RecItem> items(nobj);
    std::vector<int> pre(nobj, TE_OK);
    for (size_t i = 0; i < nobj; i++) {
        if (objs[i].slice_len % 4u || objs[i].slices_off % 4u || objs[i].out_off % 4u) return TE_ERR_INVALID_ARG;
        const int r = rec_validate(c, objs[i], h_meta + i * TE_META_SIZE, false, items[i]);
        if (r && r != TE_ERR_NOT_ENOUGH_SLICES) return r;
        pre[i] = r;
    }
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    return recover_verified(c, cfg, d_slices, objs, items, pre, h_meta, h_leaves, d_out, h_rejected_mask, h_ok_mask, h_status,
                            (hipStream_t)stream);
}

int te_repair_verified_batch_device(te_clay *c, const uint8_t *d_helpers, const te_repair_object *objs,
                                    const uint8_t *h_leaves, size_t nobj, uint8_t *d_out, uint32_t *h_ok,
                                    void *stream) {
    if (!c || ((!objs || !h_leaves || !h_ok) && nobj)) return TE_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)c->h.n;
    if (nobj > 0xffffffffull / n) return TE_ERR_INVALID_ARG;
    std::vector<te_verify_item> vi;
    for (size_t i = 0; i < nobj; i++) {
        const te_repair_plan *p = objs[i].plan;
        if (!p || p->n != n || p->lost >= n) return TE_ERR_INVALID_ARG;
        const uint64_t len = (uint64_t)p->ns * p->cs + TE_META_SIZE;
        if (len % 4u || objs[i].out_off % 4u) return TE_ERR_INVALID_ARG;
        vi.push_back(te_verify_item{objs[i].out_off, len, (uint32_t)(i * n + p->lost), (uint32_t)i, 1u, 0});
    }
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    int r = te_repair_batch_device(c, d_helpers, objs, nobj, d_out, stream);
    if (r) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    std::vector<uint32_t> good(nobj);
    if ((r = verify_wait(c, d_out, vi, h_leaves, nobj * n, nobj, good.data(), (hipStream_t)stream))) return r;
    for (size_t i = 0; i < nobj; i++) h_ok[i] = good[i] & 1u;
    return TE_OK;
}

int te_slicer_decode_verified(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t slice_len,
                              const uint8_t *leaves, uint8_t *out, size_t cap, size_t *out_len,
                              uint32_t *rejected_mask) {
    if (!c || !cfg || !slices || !leaves) return TE_ERR_INVALID_ARG;
    const ClayHost &h = c->h;
    const int n = h.n;
    uint32_t good = 0;
    const uint32_t avail = slices_avail(slices, n);
    if (!avail) return TE_ERR_NOT_ENOUGH_SLICES;
    if (slice_len < TE_META_SIZE) return TE_ERR_INVALID_LAYOUT;
    // one call's 7..20 slices: a host core with the SHA extensions hashes a slice about as fast as
    // it crosses PCIe, a device lane at ~24 MB/s, so TE_HASH_AUTO is the host
    const bool device = g_commit_hashing.load() == TE_HASH_DEVICE && slice_len % 4u == 0;
    auto finish = [&](uint32_t ok) {
        if (rejected_mask) *rejected_mask = avail & ~ok;
        return __builtin_popcount(ok) < h.k ? (int)TE_ERR_NOT_ENOUGH_SLICES : (int)TE_OK;
    };
    if (!device) {
        // te_hash_leaves' interleaved lanes over the present slices, on the calling thread
        const int lanes = hh::Pool::get().lanes();
        uint8_t dig[64][TE_HASH_SIZE];
        int idx[64], m = 0;
        for (int i = 0; i < n; i++)
            if (slices[i]) idx[m++] = i;
        for (int j0 = 0; j0 < m; j0 += lanes) {
            const int L = std::min(lanes, m - j0);
            const uint8_t *src[hh::kMaxLanes];
            uint8_t *dst[hh::kMaxLanes];
            for (int l = 0; l < L; l++) {
                src[l] = slices[idx[j0 + l]];
                dst[l] = dig[j0 + l];
            }
            hh::hash_leaves(L, src, slice_len, dst);
        }
        for (int j = 0; j < m; j++)
            if (memcmp(dig[j], leaves + (size_t)idx[j] * TE_HASH_SIZE, TE_HASH_SIZE) == 0) good |= 1u << idx[j];
        int r = finish(good);
        if (r) return r;
        const uint8_t *kept[64];
        for (int i = 0; i < n; i++) kept[i] = ((good >> i) & 1u) ? slices[i] : nullptr;
        return te_slicer_decode(c, cfg, kept, slice_len, out, cap, out_len);
    }
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    // the slices go up once: the kernel hashes them in the staging the decode then reads
    if ((r = upload_slices(c, slices, slice_len, 0))) return r;
    std::vector<te_verify_item> vi;
    verify_push_slices(vi, 0, (uint32_t)n, 0, slice_len, avail);
    if ((r = verify_wait(c, c->io_in.as<uint8_t>(), vi, leaves, (size_t)n, 1, &good, c->stream))) return r;
    if ((r = finish(good))) return r;
    const int first = __builtin_ctz(good);  // the layout comes from a verified slice
    DecItem it{};
    if ((r = decode_validate(c, slices[first] + slice_len - TE_META_SIZE, slice_len, good, it))) return r;
    if (out_len) *out_len = it.blob_len;
    if (it.blob_len == 0) return TE_OK;
    if (!out || cap < it.blob_len) return TE_ERR_BUFFER_TOO_SMALL;
    it.in_base = 0;
    it.out_off = 0;
    return percall_decode_device(c, cfg, it, out, it.blob_len, false);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Host read pipeline (te_decode_batch_host, te_decode_verified_batch_host, te_stream_reader_*):
// the decode, class, table and leaf-verify kernels behind a host boundary.  A batch is cut into
// windows (read_cuts); window w runs on slot w mod 3 -- the handle's three streams, as the encode
// pipeline's -- in two stages:
//   A  pick who hashes; host hashing: the pool hashes the present slices where they lie and the
//      survivor sets are final; enqueue the H2D copies of the slices that go up (each to its slot
//      i * slice_len of the object's device range: the layout the decode kernels read, so no
//      repacking kernel); device hashing: enqueue the leaves, the verify kernel and the D2H copy
//      of the masks, and record the slot's event;
//   B  device hashing: wait for that event -- the window's one host wait -- and pick the survivor
//      sets from the masks; enqueue the decode of the objects that have k verified slices and the
//      D2H copies of their blob_len bytes.
// The driver runs A(w+1) before B(w): B(w)'s wait is spent with the next window's upload queued
// behind this window's, and the copy engines, the kernels and the host pool overlap across slots.
// The rebuild pipeline (below) runs on the same pieces, each written once: window_cuts, add_run,
// align16 and VerLayout (win_plan.hpp), the slots (WinPipe), the pool's hashing (hash_items_host),
// the verify workspace (ver_begin, ver_masks), an object's survivor set (resolve_survivors) and
// stage A of a window of peer slices (peer_stage_a: a read's and a recover's).
// ------------------------------------------------------------------------------------------
namespace {

// A pipeline's window slots.  The handle's read pipeline, its rebuild pipeline and every stream
// reader hold an instance of their own (what persists between calls is each one's).
struct WinPipe {
    static constexpr int R = te_clay::kPipe;
    struct Slot {
        DevBuf in, out;     // the window's slices / fragments and its decoded objects / rebuilt slices
        DevBuf ver;         // device hashing: the verify workspace (VerLayout)
        HostBuf verh;       // its page-locked host side
        HostBuf hin, hout;  // rebuild: page-locked staging of pageable caller buffers
        hipEvent_t peers = nullptr;  // after the peer masks' D2H copy
        hipEvent_t done = nullptr;   // rebuild: after the window's last D2H copy
    } slot[R];
};

void win_pipe_free(WinPipe *p) {  // its streams drained, its device current
    if (!p) return;
    for (auto &sl : p->slot) {
        for (DevBuf *b : {&sl.in, &sl.out, &sl.ver}) b->release();
        for (HostBuf *b : {&sl.verh, &sl.hin, &sl.hout}) b->release();
        if (sl.peers) (void)hipEventDestroy(sl.peers);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    delete p;
}

// One window: nobj objects of the caller's arrays (already offset to the window's first object).
struct ReadWin {
    te_slicer_cfg cfg{};
    const uint8_t *h_slices = nullptr;
    uint8_t *h_out = nullptr;
    const te_decode_object *objs = nullptr;
    const uint8_t *h_meta = nullptr, *h_leaves = nullptr;  // h_leaves null: unverified
    size_t nobj = 0;
    uint32_t *h_rej = nullptr;
    int *h_status = nullptr;
    const int *pre = nullptr;  // verified: each object's outcome on its present slices (read_validate)
    int mode = TE_HASH_AUTO;
    // measurement option TEC_DEBUG_KNOBS=1 TEC_READ_COPY_ONLY=1 (scripts/read_pipeline_bench.py): the
    // window's copies with no hashing and no kernels -- the ceiling of the pipeline on a box
    bool copy_only = false;
    // stage A -> stage B
    bool device_hash = false, resolved = false;
    std::vector<uint64_t> in_base;  // object o's slice 0 in the slot's input buffer
    std::vector<uint32_t> good;     // verified present slices (unverified: the present slices)
    std::vector<DecItem> run;       // the objects that decode; out_off = their place in the slot's output
    std::vector<CopyRun> hout;
    uint64_t out_sz = 0;
    VerLayout vl{};                 // device hashing: the slot's verify workspace
};

// Every object checked like Slicer::decode on its present slices (nothing is enqueued before this
// has passed).  Unverified: the first failure is the call's.  Verified: too few slices is that
// object's outcome (status[i]), anything else the call's.
int read_validate(const te_clay *c, const te_decode_object *objs, const uint8_t *h_meta, size_t nobj, bool verified,
                  int *status) {
    const uint32_t all = slice_bits(c);
    for (size_t i = 0; i < nobj; i++) {
        DecItem it{};
        const int r = decode_validate(c, h_meta + i * TE_META_SIZE, objs[i].slice_len, objs[i].avail_mask & all, it);
        if (r && !(verified && r == TE_ERR_NOT_ENOUGH_SLICES)) return r;
        if (status) status[i] = r;
    }
    return TE_OK;
}

// te_decode_window_plan: an object counts its present slices and its decoded bytes.
int read_cuts(const te_clay *c, const te_decode_object *objs, const uint8_t *h_meta, size_t nobj, size_t window_bytes,
              std::vector<size_t> &cuts) {
    const uint32_t all = slice_bits(c);
    std::vector<uint64_t> bytes(nobj);
    for (size_t i = 0; i < nobj; i++) {
        te_slice_metadata m;
        if (int r = te_slice_metadata_from_slice(h_meta + i * TE_META_SIZE, TE_META_SIZE, &m)) return r;
        bytes[i] = (uint64_t)__builtin_popcount(objs[i].avail_mask & all) * objs[i].slice_len + m.blob_len;
    }
    window_cuts(bytes, window_bytes, cuts);
    return TE_OK;
}

// A window plan out through the C ABI (te_*_window_plan).
int cuts_out(const std::vector<size_t> &v, size_t *cuts, size_t cap, size_t *nwindows) {
    *nwindows = v.size() - 1;
    if (!cuts) return TE_OK;
    if (cap < v.size()) return TE_ERR_BUFFER_TOO_SMALL;
    memcpy(cuts, v.data(), v.size() * sizeof(size_t));
    return TE_OK;
}

hipStream_t read_slot_stream(te_clay *c, int k) { return k < 2 ? c->pipe[k].s : c->stream; }

int read_streams(te_clay *c) {  // handle locked, its device current
    if (int r = ensure_stream(c)) return r;
    for (int k = 0; k < 2; k++)
        if (!c->pipe[k].s) TE_HIP(hipStreamCreateWithFlags(&c->pipe[k].s, hipStreamNonBlocking));
    return TE_OK;
}

struct HashItem { const uint8_t *p; uint64_t len; const uint8_t *expect; };

// hash_leaf of the items on the host pool against their expected hashes; waits for the pool.
void hash_items_host(const std::vector<HashItem> &items, int device, std::vector<uint8_t> &okv) {
    okv.assign(items.size(), 0);
    if (items.empty()) return;
    hh::Pool &pool = hh::Pool::get();
    // interleaved lanes raise one thread's rate, but a window of a few long slices (a 64 MiB
    // track: 7..20 slices of ~9.6 MB) needs every thread first
    const int lanes = (int)std::max<size_t>(1, std::min<size_t>((size_t)pool.lanes(), items.size() / (size_t)std::max(1, pool.threads())));
    auto ok = std::make_shared<std::vector<uint8_t>>(items.size(), 0);
    auto job = std::make_shared<hh::Job>();
    std::vector<std::function<void()>> tasks;
    for (size_t j0 = 0; j0 < items.size();) {
        size_t j1 = j0 + 1;  // a task's lanes hash messages of one length
        while (j1 < items.size() && j1 - j0 < (size_t)lanes && items[j1].len == items[j0].len) j1++;
        std::vector<HashItem> part(items.begin() + (ptrdiff_t)j0, items.begin() + (ptrdiff_t)j1);
        tasks.push_back([part, j0, ok, job] {
            const int L = (int)part.size();
            uint8_t dig[hh::kMaxLanes][TE_HASH_SIZE];
            const uint8_t *src[hh::kMaxLanes];
            uint8_t *dst[hh::kMaxLanes];
            for (int l = 0; l < L; l++) {
                src[l] = part[(size_t)l].p;
                dst[l] = dig[l];
            }
            hh::hash_leaves(L, src, part[0].len, dst);
            for (int l = 0; l < L; l++) (*ok)[j0 + (size_t)l] = memcmp(dig[l], part[(size_t)l].expect, TE_HASH_SIZE) == 0;
            job->done();
        });
        j0 = j1;
    }
    job->add((int64_t)tasks.size());
    pool.submit_after(nullptr, device, std::move(tasks));
    (void)job->wait();
    okv = *ok;
}

// The survivor sets are known: masks and statuses out, the objects that decode and their place in
// the slot's output buffer.
void read_resolve(const te_clay *c, ReadWin &W) {
    const uint32_t all = slice_bits(c);
    W.run.clear();
    W.hout.clear();
    W.out_sz = 0;
    for (size_t o = 0; o < W.nobj; o++) {
        DecItem it{};
        // h_rej is written only when leaves were given; W.good becomes what the decode reads from
        const int st = resolve_survivors(c, W.objs[o].avail_mask & all, W.objs[o].slice_len, W.h_meta + o * TE_META_SIZE,
                                         W.pre ? W.pre[o] : TE_OK, W.good[o], W.h_leaves && W.h_rej ? W.h_rej + o : nullptr,
                                         W.h_status ? W.h_status + o : nullptr, W.good[o], it);
        if (st) continue;
        it.in_base = W.in_base[o];
        it.out_off = W.out_sz;
        W.run.push_back(it);
        add_run(W.hout, W.objs[o].out_off, W.out_sz, it.blob_len);
        W.out_sz += align16(it.blob_len);
    }
    W.resolved = true;
}

// Stage A of a peer window -- a read's or a recover's -- on a slot and its stream (handle locked,
// its device current).  `objs` are te_decode_object or te_recover_object, by the fields they share
// (slices_off, slice_len, avail_mask), their slices in h_in.  The caller gives what differs:
// `dword`, its own conditions for device hashing besides slice_len % 4; `results`, that the window
// goes on to verify that many rebuilt slices in the same workspace (0: none); the stats and their upload
// counter; `resolve`, run once W.good holds the final survivor sets; `upload`, the H2D copy runs.
template <class Win, class Obj, class Stats, class Resolve, class Upload>
int peer_stage_a(te_clay *c, WinPipe::Slot &sl, hipStream_t s, Win &W, const Obj *objs, const uint8_t *h_in, bool dword,
                 size_t results, Stats &st, uint64_t Stats::*uploaded, Resolve resolve, Upload upload) {
    const uint32_t n = (uint32_t)c->h.n, all = slice_bits(c);
    st.windows++;
    st.objects += W.nobj;
    W.in_base.resize(W.nobj);
    W.good.assign(W.nobj, 0);
    uint64_t in_sz = 0, max_slice = 0, slice_bytes = 0, nslices = 0;
    for (size_t o = 0; o < W.nobj; o++) {
        W.in_base[o] = in_sz;
        in_sz += align16((uint64_t)n * objs[o].slice_len);
        const uint64_t np = (uint64_t)__builtin_popcount(objs[o].avail_mask & all);
        nslices += np;
        slice_bytes += np * objs[o].slice_len;
        if (np) max_slice = std::max<uint64_t>(max_slice, objs[o].slice_len);
        dword = dword && objs[o].slice_len % 4u == 0;
    }
    const bool verified = W.h_leaves && !W.copy_only;
    W.device_hash = verified && nslices && dword && !host_hash_wins(W.mode, nslices, max_slice, slice_bytes);
    if (verified && !W.device_hash) {  // the pool hashes the present slices where they lie
        std::vector<HashItem> items;
        std::vector<std::pair<uint32_t, uint32_t>> who;
        for (size_t o = 0; o < W.nobj; o++)
            for (uint32_t b = 0; b < n; b++)
                if (((objs[o].avail_mask & all) >> b) & 1u) {
                    items.push_back({h_in + objs[o].slices_off + (uint64_t)b * objs[o].slice_len, objs[o].slice_len,
                                     W.h_leaves + (o * n + b) * TE_HASH_SIZE});
                    who.push_back({(uint32_t)o, b});
                }
        std::vector<uint8_t> ok;
        hash_items_host(items, c->device, ok);
        for (size_t j = 0; j < items.size(); j++)
            if (ok[j]) W.good[who[j].first] |= 1u << who[j].second;
        st.slices_hashed_host += items.size();
    } else {  // unverified: the present slices; device hashing: every present slice goes up
        for (size_t o = 0; o < W.nobj; o++) W.good[o] = objs[o].avail_mask & all;
    }
    if (!W.device_hash) resolve();
    TE_HIP(sl.in.ensure(in_sz + 16));
    std::vector<CopyRun> hin;
    std::vector<te_verify_item> vi;
    for (size_t o = 0; o < W.nobj; o++) {
        const uint64_t len = objs[o].slice_len;
        for (uint32_t b = 0; b < n; b++) {
            if (!((W.good[o] >> b) & 1u) || !len) continue;
            add_run(hin, objs[o].slices_off + (uint64_t)b * len, W.in_base[o] + (uint64_t)b * len, len);
            (st.*uploaded)++;
            st.bytes_h2d += len;
        }
        if (W.device_hash) verify_push_slices(vi, o, n, W.in_base[o], len, W.good[o]);
    }
    if (int r = upload(hin)) return r;
    if (!W.device_hash) return TE_OK;
    // verify_wait's launches without its wait, in the slot's own workspace
    W.vl = VerLayout{W.nobj * n * TE_HASH_SIZE, vi.size() * TE_HASH_SIZE, results * TE_HASH_SIZE,
                     W.nobj * sizeof(uint32_t), results ? 2u : 1u};
    if (int r = ver_begin(sl.ver, sl.verh, W.vl, W.h_leaves, s)) return r;
    if (int r = ver_masks(c, sl.ver, sl.verh, sl.in.as<uint8_t>(), vi, W.vl, 0, s)) return r;
    if (!sl.peers) TE_HIP(hipEventCreateWithFlags(&sl.peers, hipEventDisableTiming | hipEventBlockingSync));
    TE_HIP(hipEventRecord(sl.peers, s));
    st.slices_hashed_device += vi.size();
    return TE_OK;
}

// Stage A of a read window on slot k: the slices go up from the caller's buffer as they lie.
int read_stage_a(te_clay *c, WinPipe &P, int k, ReadWin &W) {
    WinPipe::Slot &sl = P.slot[k];
    const hipStream_t s = read_slot_stream(c, k);
    return peer_stage_a(
        c, sl, s, W, W.objs, W.h_slices, true, 0, c->rds, &te_read_launch_stats::slices_uploaded,
        [&] { read_resolve(c, W); },
        [&](const std::vector<CopyRun> &hin) { return copy_runs(hin, sl.in.as<uint8_t>(), W.h_slices, hipMemcpyHostToDevice, s); });
}

// The one host wait of a device-hashed window (its device current; the handle need not be locked).
int read_wait_masks(WinPipe &P, int k, const ReadWin &W) {
    if (!W.device_hash || W.resolved) return TE_OK;
    TE_HIP(hipEventSynchronize(P.slot[k].peers));
    return TE_OK;
}

// Stage B (handle locked, its device current, read_wait_masks passed).
int read_stage_b(te_clay *c, WinPipe &P, int k, ReadWin &W) {
    WinPipe::Slot &sl = P.slot[k];
    const hipStream_t s = read_slot_stream(c, k);
    te_read_launch_stats &st = c->rds;
    if (!W.resolved) {
        memcpy(W.good.data(), sl.verh.u8() + W.vl.h_mask(0), W.vl.mask_b);
        st.host_waits++;
        read_resolve(c, W);
    }
    if (W.run.empty()) return TE_OK;
    TE_HIP(sl.out.ensure(W.out_sz + 16));
    if (!W.copy_only)
        if (int r = decode_enqueue(c, &W.cfg, sl.in.as<uint8_t>(), W.run.data(), W.run.size(), sl.out.as<uint8_t>(), s, false))
            return r;
    for (const CopyRun &r : W.hout) st.bytes_d2h += r.len;
    return copy_runs(W.hout, sl.out.as<uint8_t>(), W.h_out, hipMemcpyDeviceToHost, s);
}

int read_drain(te_clay *c) {  // its device current
    int rc = TE_OK;
    for (int k = 0; k < WinPipe::R; k++)
        if (hipStream_t s = read_slot_stream(c, k)) {
            const int r = sync_sleep(s);
            if (!rc) rc = r;
        }
    return rc;
}

int decode_host_impl(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices, const te_decode_object *objs,
                     const uint8_t *h_meta, const uint8_t *h_leaves, bool verified, size_t nobj, uint8_t *h_out,
                     uint32_t *h_rej, int *h_status, size_t window_bytes) {
    if (!c || !cfg || ((!objs || !h_meta || !h_slices || !h_out) && nobj)) return TE_ERR_INVALID_ARG;
    if (verified && ((!h_leaves || !h_status) && nobj)) return TE_ERR_INVALID_ARG;
    if (nobj > 0xffffffffull / (uint32_t)c->h.n) return TE_ERR_INVALID_ARG;
    std::vector<int> pre(nobj, TE_OK);
    if (int r = read_validate(c, objs, h_meta, nobj, verified, pre.data())) return r;
    std::vector<size_t> cuts;
    if (int r = read_cuts(c, objs, h_meta, nobj, window_bytes, cuts)) return r;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    c->rds = te_read_launch_stats{};
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    if (int r = read_streams(c)) return r;
    if (!c->rpipe) c->rpipe = new WinPipe();
    WinPipe &P = *c->rpipe;
    const size_t nw = cuts.size() - 1;
    const size_t n = (size_t)c->h.n;
    const char *co = tec_knob("TEC_READ_COPY_ONLY");  // read per call: a benchmark switches it between legs
    const bool copy_only = co && co[0] == '1';
    std::vector<ReadWin> wins(nw);
    for (size_t w = 0; w < nw; w++) {
        ReadWin &W = wins[w];
        const size_t a = cuts[w];
        W.cfg = *cfg;
        W.h_slices = h_slices;
        W.h_out = h_out;
        W.objs = objs + a;
        W.h_meta = h_meta + a * TE_META_SIZE;
        W.h_leaves = verified ? h_leaves + a * n * TE_HASH_SIZE : nullptr;
        W.nobj = cuts[w + 1] - a;
        W.h_rej = h_rej ? h_rej + a : nullptr;
        W.h_status = h_status ? h_status + a : nullptr;
        W.pre = verified ? pre.data() + a : nullptr;
        W.mode = g_commit_hashing.load();
        W.copy_only = copy_only;
    }
    // A(w + 1) before B(w): window w's host wait is spent with the next upload already queued
    int rc = TE_OK;
    for (size_t w = 0; w <= nw && !rc; w++) {
        if (w < nw) rc = read_stage_a(c, P, (int)(w % WinPipe::R), wins[w]);
        if (w > 0 && !rc) {
            const int k = (int)((w - 1) % WinPipe::R);
            if (!(rc = read_wait_masks(P, k, wins[w - 1]))) rc = read_stage_b(c, P, k, wins[w - 1]);
        }
    }
    const int r2 = read_drain(c);
    return rc ? rc : r2;
}

}  // namespace

// Ordered, asynchronous reads: one host thread per handle runs the handle's windows through the
// same two stages, A of the next window before B of the last, whenever a next window is queued.
struct te_stream_reader {
    struct Job {
        uint64_t ticket = 0;
        ReadWin W;
        std::vector<te_decode_object> objs;
        std::vector<uint8_t> meta, leaves;
        std::vector<int> pre;
        int slot = 0, rc = TE_OK;
        bool done = false;           // its work is enqueued (or it failed)
        hipEvent_t ev = nullptr;     // after its last D2H copy
    };
    struct Dev {
        te_clay *c = nullptr;
        int device = 0;
        WinPipe *P = nullptr;
        std::thread th;
        std::deque<std::shared_ptr<Job>> q;
        uint64_t nwin = 0;
    };
    std::vector<std::unique_ptr<Dev>> devs;
    te_slicer_cfg cfg{};
    int hashing = TE_HASH_AUTO;
    std::mutex mu;       // queues, tickets, done flags
    std::condition_variable cv_work, cv_done;
    std::mutex wait_mu;  // te_stream_read_wait calls complete tickets one caller at a time
    bool quit = false;
    uint64_t next = 1;
    std::map<uint64_t, std::shared_ptr<Job>> tickets;  // submitted, not yet waited
};

namespace {

void reader_worker(te_stream_reader *r, te_stream_reader::Dev *d) {
    using Job = te_stream_reader::Job;
    te_clay *c = d->c;
    std::shared_ptr<Job> staged;  // stage A done, stage B to do
    auto finish = [&](const std::shared_ptr<Job> &j, int rc) {
        if (rc) {
            // only this window fails; work already enqueued for it may still touch its buffers
            DeviceGuard dg(d->device);
            (void)read_drain(c);
        }
        std::lock_guard<std::mutex> g(r->mu);
        j->rc = rc;
        j->done = true;
        r->cv_done.notify_all();
    };
    for (;;) {
        std::shared_ptr<Job> nxt;
        {
            std::unique_lock<std::mutex> g(r->mu);
            if (!staged) r->cv_work.wait(g, [&] { return r->quit || !d->q.empty(); });
            if (!d->q.empty()) {
                nxt = d->q.front();
                d->q.pop_front();
            } else if (!staged) {
                return;
            }
        }
        int rca = TE_OK;
        if (nxt) {
            std::lock_guard<std::mutex> lk(c->mu);
            DeviceGuard dg(d->device);
            rca = c->device != d->device ? (int)TE_ERR_INVALID_ARG : hip_status(dg.err);  // handle re-bound under the reader
            if (!rca) rca = read_stage_a(c, *d->P, nxt->slot, nxt->W);
        }
        if (staged) {
            DeviceGuard dg(d->device);
            int rc = hip_status(dg.err);
            if (!rc) rc = read_wait_masks(*d->P, staged->slot, staged->W);  // the handle stays free meanwhile
            if (!rc) {
                std::lock_guard<std::mutex> lk(c->mu);
                rc = read_stage_b(c, *d->P, staged->slot, staged->W);
                if (!rc) rc = hip_status(hipEventCreateWithFlags(&staged->ev, hipEventDisableTiming | hipEventBlockingSync));
                if (!rc) rc = hip_status(hipEventRecord(staged->ev, read_slot_stream(c, staged->slot)));
            }
            finish(staged, rc);
            staged.reset();
        }
        if (nxt) {
            if (rca) finish(nxt, rca);
            else staged = nxt;
        }
    }
}

}  // namespace

extern "C" {

int te_decode_window_plan(const te_clay *c, const te_decode_object *objs, const uint8_t *h_meta, size_t nobj,
                          size_t window_bytes, size_t *cuts, size_t cap, size_t *nwindows) {
    if (!c || !nwindows || ((!objs || !h_meta) && nobj)) return TE_ERR_INVALID_ARG;
    *nwindows = 0;
    std::vector<size_t> v;
    if (int r = read_cuts(c, objs, h_meta, nobj, window_bytes, v)) return r;
    return cuts_out(v, cuts, cap, nwindows);
}

int te_decode_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices, const te_decode_object *objs,
                         const uint8_t *h_meta, size_t nobj, uint8_t *h_out, size_t window_bytes) {
    return decode_host_impl(c, cfg, h_slices, objs, h_meta, nullptr, false, nobj, h_out, nullptr, nullptr, window_bytes);
}

int te_decode_verified_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices,
                                  const te_decode_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                  size_t nobj, uint8_t *h_out, uint32_t *h_rejected_mask, int *h_status,
                                  size_t window_bytes) {
    return decode_host_impl(c, cfg, h_slices, objs, h_meta, h_leaves, true, nobj, h_out, h_rejected_mask, h_status,
                            window_bytes);
}

int te_clay_read_launch_stats(te_clay *c, te_read_launch_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->rds;
    return TE_OK;
}

int te_stream_reader_new(te_clay *const *coders, size_t ncoders, const te_slicer_cfg *cfg, te_stream_reader **out) {
    if (!out) return TE_ERR_INVALID_ARG;
    *out = nullptr;
    if (!coders || ncoders == 0 || !cfg) return TE_ERR_INVALID_ARG;
    for (size_t i = 0; i < ncoders; i++)
        if (!coders[i]) return TE_ERR_INVALID_ARG;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    auto *r = new (std::nothrow) te_stream_reader();
    if (!r) return TE_ERR_OUT_OF_MEMORY;
    r->cfg = *cfg;
    r->hashing = g_commit_hashing.load();
    int rc = TE_OK;
    for (size_t i = 0; i < ncoders && !rc; i++) {
        auto d = std::make_unique<te_stream_reader::Dev>();
        d->c = coders[i];
        d->device = coders[i]->device;
        d->P = new WinPipe();
        {
            std::lock_guard<std::mutex> lk(d->c->mu);
            DeviceGuard dg(d->device);
            if (!(rc = hip_status(dg.err))) rc = read_streams(d->c);
            d->c->rds = te_read_launch_stats{};
        }
        r->devs.push_back(std::move(d));
    }
    if (!rc)
        for (auto &d : r->devs) d->th = std::thread(reader_worker, r, d.get());
    if (rc) {
        te_stream_reader_free(r);
        return rc;
    }
    *out = r;
    return TE_OK;
}

int te_stream_read_submit(te_stream_reader *r, const uint8_t *h_slices, const te_decode_object *objs,
                          const uint8_t *h_meta, const uint8_t *h_leaves, size_t nobj, uint8_t *h_out,
                          uint32_t *h_rejected_mask, int *h_status, uint64_t *ticket) {
    if (!r || !ticket) return TE_ERR_INVALID_ARG;
    *ticket = 0;
    if ((!objs || !h_meta || !h_slices || !h_out) && nobj) return TE_ERR_INVALID_ARG;
    if (h_leaves && !h_status && nobj) return TE_ERR_INVALID_ARG;
    const te_clay *c0 = r->devs[0]->c;
    const size_t n = (size_t)c0->h.n;
    if (nobj > 0xffffffffull / n) return TE_ERR_INVALID_ARG;
    auto j = std::make_shared<te_stream_reader::Job>();
    j->pre.assign(nobj, TE_OK);
    if (int rc = read_validate(c0, objs, h_meta, nobj, h_leaves != nullptr, j->pre.data())) return rc;
    if (nobj) {
        j->objs.assign(objs, objs + nobj);
        j->meta.assign(h_meta, h_meta + nobj * TE_META_SIZE);
        if (h_leaves) j->leaves.assign(h_leaves, h_leaves + nobj * n * TE_HASH_SIZE);
    }
    ReadWin &W = j->W;
    W.cfg = r->cfg;
    W.h_slices = h_slices;
    W.h_out = h_out;
    W.objs = j->objs.data();
    W.h_meta = j->meta.data();
    W.h_leaves = h_leaves ? j->leaves.data() : nullptr;
    W.nobj = nobj;
    W.h_rej = h_rejected_mask;
    W.h_status = h_status;
    W.pre = h_leaves ? j->pre.data() : nullptr;
    W.mode = r->hashing;
    std::lock_guard<std::mutex> g(r->mu);
    const uint64_t t = r->next++;
    te_stream_reader::Dev &d = *r->devs[(size_t)((t - 1) % r->devs.size())];
    j->ticket = t;
    j->slot = (int)(d.nwin++ % WinPipe::R);
    r->tickets[t] = j;
    d.q.push_back(j);
    r->cv_work.notify_all();
    *ticket = t;
    return TE_OK;
}

int te_stream_read_wait(te_stream_reader *r, uint64_t ticket) {
    if (!r || ticket == 0) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> wg(r->wait_mu);
    int first = TE_OK;
    for (;;) {
        std::shared_ptr<te_stream_reader::Job> j;
        int dev = 0;
        {
            std::unique_lock<std::mutex> g(r->mu);
            if (ticket >= r->next) return TE_ERR_INVALID_ARG;  // never submitted
            if (r->tickets.empty() || r->tickets.begin()->first > ticket) return first;
            j = r->tickets.begin()->second;
            r->cv_done.wait(g, [&] { return j->done; });
            r->tickets.erase(r->tickets.begin());
            dev = r->devs[(size_t)((j->ticket - 1) % r->devs.size())]->device;
        }
        int rc = j->rc;
        if (j->ev) {
            DeviceGuard dg(dev);
            const int r2 = hip_status(hipEventSynchronize(j->ev));
            if (!rc) rc = r2;
            (void)hipEventDestroy(j->ev);
            j->ev = nullptr;
        }
        if (!first) first = rc;
    }
}

void te_stream_reader_free(te_stream_reader *r) {
    if (!r) return;
    if (r->next > 1) (void)te_stream_read_wait(r, r->next - 1);
    {
        std::lock_guard<std::mutex> g(r->mu);
        r->quit = true;
    }
    r->cv_work.notify_all();
    for (auto &d : r->devs)
        if (d->th.joinable()) d->th.join();
    for (auto &d : r->devs) {
        std::lock_guard<std::mutex> lk(d->c->mu);
        DeviceGuard dg(d->device);
        (void)read_drain(d->c);
        win_pipe_free(d->P);
        d->P = nullptr;
    }
    delete r;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Host rebuild pipeline (te_repair_batch_host, te_recover_batch_host): the node's repair loop
// (network/node/src/features/spool/repair.rs:94-226) and its escalation (recover.rs:77-244) behind
// a host boundary, on the read pipeline's plan and its pieces (listed above it): windows
// (window_cuts), window w on slot w mod 3 of the handle's three streams (a WinPipe of its own), a
// recover window's stage A the read's peer_stage_a with rebuild_upload for the copies; three stages:
//   A  pick who hashes; recover with host hashing: the pool hashes the peer slices where they lie
//      and the survivor sets are final; enqueue the H2D copies (repair: the plan's fragments,
//      packed; recover: each slice to its slot of the object's n * slice_len range); recover with
//      device hashing: the leaves, the verify kernel, the masks' D2H copy and the slot's event;
//   B  recover with device hashing: wait for that event and pick the survivor sets; enqueue the
//      repair / recover kernels, device hashing of the rebuilt slices, the D2H copies, and record
//      the slot's `done` event;
//   C  wait for `done`; scatter a pageable output out of its staging, hash the rebuilt slices on the
//      pool (host hashing) or read their masks, and fill h_ok.
// The driver runs A(w+1), B(w), C(w-1): every wait is spent with later windows' work queued.
// ------------------------------------------------------------------------------------------
namespace {

// The bytes of helper `sl`'s fragment under plan p (te_extract_repair_data_size for every slice).
void plan_needs(const te_repair_plan *p, uint64_t *need) {
    std::fill(need, need + p->n, 0ull);
    for (uint32_t st = 0; st < p->ns; st++)
        for (uint32_t j = 0; j < p->d; j++) need[p->helper_slice[st * p->d + j]] += (uint64_t)p->beta * p->sc;
}

inline uint64_t plan_out_bytes(const te_repair_plan *p) { return (uint64_t)p->ns * p->cs + TE_META_SIZE; }

int repair_object_bytes(const te_clay *c, const te_repair_object *objs, size_t nobj, std::vector<uint64_t> &bytes) {
    bytes.resize(nobj);
    uint64_t need[64];
    for (size_t i = 0; i < nobj; i++) {
        const te_repair_plan *p = objs[i].plan;
        if (!p || p->n != (uint32_t)c->h.n || p->n > 64) return TE_ERR_INVALID_ARG;
        plan_needs(p, need);
        bytes[i] = plan_out_bytes(p);
        for (uint32_t sl = 0; sl < p->n; sl++) bytes[i] += need[sl];
    }
    return TE_OK;
}

// One window: nobj objects of the caller's arrays (already offset to the window's first object).
struct RebuildWin {
    const te_repair_object *rep = nullptr;        // repair window
    const te_recover_multi_object *rm = nullptr;  // recover window: L rebuilt slices per object, packed
    RecItem *items = nullptr;                     // ... its objects as validated on their present slices
    bool ok_flag = false;  // h_ok is 0 or 1 (a repair window, the single-slice recover form), not a mask of slices
    te_slicer_cfg cfg{};
    const uint8_t *h_in = nullptr, *h_meta = nullptr, *h_leaves = nullptr;  // h_leaves null: unverified
    uint8_t *h_out = nullptr;
    size_t nobj = 0;
    uint32_t *h_rej = nullptr, *h_ok = nullptr;
    int *h_status = nullptr;
    const int *pre = nullptr;  // verified recover: each object's outcome on its present slices
    int mode = TE_HASH_AUTO;
    bool pinned_in = false, pinned_out = false;
    // measurement option TEC_DEBUG_KNOBS=1 TEC_REBUILD_COPY_ONLY=1 (scripts/rebuild_bench.py): the
    // window's copies with no hashing and no kernels -- the ceiling of the pipeline on a box
    bool copy_only = false;
    // stage A -> B -> C
    bool device_hash = false, resolved = false;
    std::vector<uint64_t> in_base;               // recover: object o's slice 0 in the slot's input
    std::vector<uint64_t> frag_off;              // repair: object o's helper_off[] on the device, o * n + slice
    std::vector<uint32_t> good;                  // recover: the slices that go up / rebuild from
    std::vector<size_t> run;                     // the objects that rebuild
    std::vector<uint64_t> out_dev, out_len, out_host;  // per object: its rebuilt slice on the device / host
    std::vector<uint32_t> lost;                  // repair: the lost slice; recover: the lost mask
    std::vector<uint32_t> avail;                 // recover: the caller's avail_mask and slice_len
    std::vector<uint64_t> slen;
    std::vector<CopyRun> hout;
    uint64_t out_sz = 0;
    VerLayout vl{};  // device hashing: the slot's verify workspace
};

// The window's H2D copies: pinned memory directly, pageable memory gathered by the copy pool into
// the slot's page-locked staging first (one DMA per run instead of one driver-staged copy).
int rebuild_upload(te_clay *c, WinPipe::Slot &sl, const RebuildWin &W, const std::vector<CopyRun> &runs, hipStream_t s) {
    uint8_t *const d_in = sl.in.as<uint8_t>();
    if (W.pinned_in) return copy_runs(runs, d_in, W.h_in, hipMemcpyHostToDevice, s);
    uint64_t total = 0;
    for (const CopyRun &r : runs) total += align16(r.len);
    if (!total) return TE_OK;
    TE_HIP(sl.hin.ensure(total));
    std::vector<tec::CopyPool::Seg> segs;
    std::vector<CopyRun> staged;  // host = offset in the staging
    uint64_t at = 0;
    for (const CopyRun &r : runs) {
        segs.push_back({sl.hin.u8() + at, W.h_in + r.host, (size_t)r.len});
        add_run(staged, at, r.dev, r.len);
        at += align16(r.len);
    }
    copy_pool(c->device).run(segs);
    return copy_runs(staged, d_in, sl.hin.u8(), hipMemcpyHostToDevice, s);
}

// Recover: the survivor sets are known: masks and statuses out, the objects that rebuild and
// their place in the slot's output buffer.
void recover_resolve(const te_clay *c, RebuildWin &W) {
    const uint32_t all = slice_bits(c);
    W.run.clear();
    W.hout.clear();
    W.out_sz = 0;
    for (size_t o = 0; o < W.nobj; o++) {
        // h_rej is written only when leaves were given; the object's item is now that of its survivors
        const int st = resolve_survivors(c, W.avail[o] & all, W.slen[o], W.h_meta + o * TE_META_SIZE,
                                         W.pre ? W.pre[o] : TE_OK, W.good[o], W.h_leaves && W.h_rej ? W.h_rej + o : nullptr,
                                         W.h_status ? W.h_status + o : nullptr, W.good[o], W.items[o].it);
        if (W.h_leaves && W.h_ok) W.h_ok[o] = 0;  // unverified: h_ok is not the call's to write
        if (st) continue;
        W.run.push_back(o);
        W.out_dev[o] = W.out_sz;
        add_run(W.hout, W.out_host[o], W.out_sz, W.out_len[o]);
        W.out_sz += align16(W.out_len[o]);
    }
    W.resolved = true;
}

// Stage A of a recover window on slot k: peer_stage_a with a rebuilt slice per object to verify
// afterwards, and rebuild_upload for the slices.
int recover_stage_a(te_clay *c, WinPipe &P, int k, RebuildWin &W) {
    WinPipe::Slot &sl = P.slot[k];
    const hipStream_t s = read_slot_stream(c, k);
    W.out_dev.assign(W.nobj, 0);
    W.out_len.resize(W.nobj);
    W.out_host.resize(W.nobj);
    W.lost.resize(W.nobj);
    W.avail.resize(W.nobj);
    W.slen.resize(W.nobj);
    bool dword = true;  // the recover kernels' and the rebuilt slice's verify item's alignment
    size_t results = 0;
    for (size_t o = 0; o < W.nobj; o++) {
        const te_recover_multi_object &ob = W.rm[o];
        const uint64_t nlost = (uint64_t)__builtin_popcount(ob.lost_mask);
        W.out_len[o] = nlost * ob.slice_len;
        W.out_host[o] = ob.out_off;
        W.lost[o] = ob.lost_mask;
        W.avail[o] = ob.avail_mask;
        W.slen[o] = ob.slice_len;
        results += nlost;
        dword = dword && ob.slices_off % 4u == 0 && ob.out_off % 4u == 0;
    }
    return peer_stage_a(c, sl, s, W, W.rm, W.h_in, dword, results, c->rbs, &te_rebuild_launch_stats::pieces_uploaded,
                        [&] { recover_resolve(c, W); },
                        [&](const std::vector<CopyRun> &hin) { return rebuild_upload(c, sl, W, hin, s); });
}

// Stage A of a repair window: the plan's fragments, packed (each 16-byte aligned, as
// te_slicer_repair places them); the repair kernels address them through helper_off.
int repair_stage_a(te_clay *c, WinPipe &P, int k, RebuildWin &W) {
    const uint32_t n = (uint32_t)c->h.n;
    WinPipe::Slot &sl = P.slot[k];
    const hipStream_t s = read_slot_stream(c, k);
    te_rebuild_launch_stats &st = c->rbs;
    st.windows++;
    st.objects += W.nobj;
    W.frag_off.assign(W.nobj * n, ~0ull);
    W.out_dev.resize(W.nobj);
    W.out_len.resize(W.nobj);
    W.out_host.resize(W.nobj);
    W.lost.resize(W.nobj);
    W.run.resize(W.nobj);
    W.hout.clear();
    std::vector<CopyRun> hin;
    uint64_t in_sz = 0, need[64], max_len = 0, sum_len = 0;
    bool dword = true;
    W.out_sz = 0;
    for (size_t o = 0; o < W.nobj; o++) {
        const te_repair_plan *p = W.rep[o].plan;
        plan_needs(p, need);
        for (uint32_t b = 0; b < n; b++) {
            if (!need[b]) continue;
            W.frag_off[o * n + b] = in_sz;
            add_run(hin, W.rep[o].helper_off[b], in_sz, need[b]);
            in_sz += align16(need[b]);
            st.pieces_uploaded++;
            st.bytes_h2d += need[b];
        }
        W.run[o] = o;
        W.lost[o] = p->lost;
        W.out_len[o] = plan_out_bytes(p);
        W.out_host[o] = W.rep[o].out_off;
        W.out_dev[o] = W.out_sz;
        add_run(W.hout, W.out_host[o], W.out_sz, W.out_len[o]);
        W.out_sz += align16(W.out_len[o]);
        max_len = std::max(max_len, W.out_len[o]);
        sum_len += W.out_len[o];
        dword = dword && W.out_len[o] % 4u == 0 && W.out_host[o] % 4u == 0;
    }
    W.device_hash = W.h_leaves && !W.copy_only && W.nobj && dword && !host_hash_wins(W.mode, W.nobj, max_len, sum_len);
    W.resolved = true;
    TE_HIP(sl.in.ensure(in_sz + 16));
    if (int r = rebuild_upload(c, sl, W, hin, s)) return r;
    if (!W.device_hash) return TE_OK;
    W.vl = VerLayout{W.nobj * n * TE_HASH_SIZE, 0, W.nobj * TE_HASH_SIZE, W.nobj * sizeof(uint32_t), 2};  // no peers
    return ver_begin(sl.ver, sl.verh, W.vl, W.h_leaves, s);
}

// One call of f(slice, offset, length, bit) per rebuilt slice of the window's object o: the slice's
// place in the object's output and the value its match adds to h_ok.  A repair window rebuilds
// one slice per object (W.lost the slice, h_ok 0 or 1), a recover window its lost mask's, packed.
template <class F>
void rebuilt_slices(const RebuildWin &W, size_t o, F f) {
    if (W.rep) return f(W.lost[o], 0, W.out_len[o], 1u);
    rec_each_lost(W.lost[o], [&](uint32_t b, uint64_t j) { f(b, j * W.slen[o], W.slen[o], 1u << b); });
}

// Stage B (handle locked, its device current): the kernels, the rebuilt slices' hashes, the D2H copies.
int rebuild_stage_b(te_clay *c, WinPipe &P, int k, RebuildWin &W) {
    const uint32_t n = (uint32_t)c->h.n;
    WinPipe::Slot &sl = P.slot[k];
    const hipStream_t s = read_slot_stream(c, k);
    te_rebuild_launch_stats &st = c->rbs;
    if (!W.resolved) {  // recover, device hashing: the window's wait for its peers' masks
        TE_HIP(hipEventSynchronize(sl.peers));
        st.host_waits++;
        memcpy(W.good.data(), sl.verh.u8() + W.vl.h_mask(0), W.vl.mask_b);
        recover_resolve(c, W);
    }
    if (!sl.done) TE_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming | hipEventBlockingSync));
    if (!W.run.empty()) {
        TE_HIP(sl.out.ensure(W.out_sz + 16));
        uint8_t *const d_in = sl.in.as<uint8_t>(), *const d_out = sl.out.as<uint8_t>();
        if (W.copy_only) {
        } else if (W.rep) {
            std::vector<RepItem> items(W.nobj);
            for (size_t o = 0; o < W.nobj; o++)
                items[o] = RepItem{W.rep[o].plan, W.frag_off.data() + o * n, W.out_dev[o], W.rep[o].metadata};
            if (int r = repair_enqueue(c, d_in, items.data(), items.size(), d_out, s)) return r;
        } else {  // the device form's routing (rec_route), on the window's survivors; the figures sum over the windows
            std::vector<RecItem> run;
            run.reserve(W.run.size());
            for (size_t o : W.run) {
                run.push_back(W.items[o]);
                run.back().it.in_base = W.in_base[o];
                run.back().out_off = W.out_dev[o];
            }
            if (int r = recover_enqueue(c, &W.cfg, d_in, run, d_out, s, c->rms)) return r;
        }
        if (W.device_hash) {
            std::vector<te_verify_item> vi;  // the mask of object o gets the bit of each rebuilt slice that matches
            for (size_t o : W.run)
                rebuilt_slices(W, o, [&](uint32_t b, uint64_t off, uint64_t len, uint32_t bit) {
                    vi.push_back(te_verify_item{W.out_dev[o] + off, len, (uint32_t)(o * n + b), (uint32_t)o, bit, 0});
                });
            if (int r = ver_masks(c, sl.ver, sl.verh, d_out, vi, W.vl, 1, s)) return r;
            st.slices_hashed_device += vi.size();
        }
        for (const CopyRun &r : W.hout) st.bytes_d2h += r.len;
        if (W.pinned_out) {
            if (int r = copy_runs(W.hout, d_out, W.h_out, hipMemcpyDeviceToHost, s)) return r;
        } else {  // the device image as it is, into the slot's staging
            TE_HIP(sl.hout.ensure(W.out_sz));
            TE_HIP(hipMemcpyAsync(sl.hout.p, d_out, W.out_sz, hipMemcpyDeviceToHost, s));
        }
    }
    TE_HIP(hipEventRecord(sl.done, s));
    return TE_OK;
}

// Stage C (its device current): the window's results are on the host.
int rebuild_stage_c(te_clay *c, WinPipe &P, int k, RebuildWin &W, bool last) {
    WinPipe::Slot &sl = P.slot[k];
    te_rebuild_launch_stats &st = c->rbs;
    TE_HIP(hipEventSynchronize(sl.done));
    if (W.run.empty()) return TE_OK;
    const bool verified = W.h_leaves && !W.copy_only;
    if (!last && (verified || !W.pinned_out)) st.host_waits++;
    if (!W.pinned_out) {
        std::vector<tec::CopyPool::Seg> segs;
        for (const CopyRun &r : W.hout) segs.push_back({W.h_out + r.host, sl.hout.u8() + r.dev, (size_t)r.len});
        copy_pool(c->device).run(segs);
    }
    if (!verified) return TE_OK;
    if (W.device_hash) {
        const uint32_t *m = reinterpret_cast<const uint32_t *>(sl.verh.u8() + W.vl.h_mask(1));
        for (size_t o : W.run) {
            const uint32_t ok = m[o] & (W.rep ? 1u : W.lost[o]);
            W.h_ok[o] = W.ok_flag ? ok != 0 : ok;
        }
        return TE_OK;
    }
    const size_t n = (size_t)c->h.n;
    std::vector<HashItem> items;
    std::vector<std::pair<size_t, uint32_t>> who;  // the item's object and the value its match adds to h_ok
    for (size_t o : W.run)
        rebuilt_slices(W, o, [&](uint32_t b, uint64_t off, uint64_t len, uint32_t bit) {
            items.push_back({W.h_out + W.out_host[o] + off, len, W.h_leaves + (o * n + b) * TE_HASH_SIZE});
            who.push_back({o, bit});
        });
    std::vector<uint8_t> ok;
    hash_items_host(items, c->device, ok);
    for (size_t o : W.run) W.h_ok[o] = 0;  // a repair window's h_ok is first written here: whatever the caller left goes
    for (size_t j = 0; j < items.size(); j++)
        if (ok[j]) W.h_ok[who[j].first] |= W.ok_flag ? 1u : who[j].second;
    st.slices_hashed_host += items.size();
    return TE_OK;
}

// The driver: handle locked, its device current, the windows filled in.
int rebuild_run(te_clay *c, std::vector<RebuildWin> &wins) {
    if (int r = read_streams(c)) return r;
    if (!c->rbpipe) c->rbpipe = new WinPipe();
    WinPipe &P = *c->rbpipe;
    const size_t nw = wins.size();
    int rc = TE_OK;
    for (size_t w = 0; w < nw + 2 && !rc; w++) {
        if (w < nw) rc = wins[w].rep ? repair_stage_a(c, P, (int)(w % WinPipe::R), wins[w])
                                     : recover_stage_a(c, P, (int)(w % WinPipe::R), wins[w]);
        if (!rc && w >= 1 && w - 1 < nw) rc = rebuild_stage_b(c, P, (int)((w - 1) % WinPipe::R), wins[w - 1]);
        if (!rc && w >= 2) rc = rebuild_stage_c(c, P, (int)((w - 2) % WinPipe::R), wins[w - 2], w - 2 == nw - 1);
    }
    // also after a failure: copies from and to the caller's buffers may still be queued
    const int r2 = read_drain(c);
    for (auto &sl : P.slot)  // as the snapshot host calls: large window buffers are not kept
        for (DevBuf *b : {&sl.in, &sl.out})
            if (b->cap > ((size_t)256 << 20)) b->release();
    return rc ? rc : r2;
}

bool rebuild_copy_only() {  // read per call: a benchmark switches it between legs
    const char *co = tec_knob("TEC_REBUILD_COPY_ONLY");
    return co && co[0] == '1';
}

// te_recover_batch_host (single: rec_single's objects and argument rule) and
// te_recover_multi_batch_host: every argument check, then the windows
int recover_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices, const te_recover_multi_object *objs,
                 const uint8_t *h_meta, const uint8_t *h_leaves, size_t nobj, uint8_t *h_out, uint32_t *h_rejected_mask,
                 uint32_t *h_ok_mask, int *h_status, size_t window_bytes, bool single) {
    if (!c || !cfg || ((!objs || !h_meta || !h_slices || !h_out) && nobj)) return TE_ERR_INVALID_ARG;
    const bool verified = h_leaves != nullptr;
    if (verified && (!h_status || !h_ok_mask) && nobj) return TE_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)c->h.n;
    if (nobj > 0xffffffffull / n) return TE_ERR_INVALID_ARG;
    std::vector<RecItem> items(nobj);
    std::vector<int> pre(nobj, TE_OK);
    std::vector<uint64_t> bytes(nobj);
    for (size_t i = 0; i < nobj; i++) {
        const int r = rec_validate(c, objs[i], h_meta + i * TE_META_SIZE, single, items[i]);
        if (r && !(verified && r == TE_ERR_NOT_ENOUGH_SLICES)) return r;
        pre[i] = r;
        bytes[i] = rec_multi_object_bytes(c->h.n, objs[i].avail_mask, objs[i].lost_mask, objs[i].slice_len);
    }
    std::vector<size_t> cuts;
    window_cuts(bytes, window_bytes, cuts);
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dls = te_decode_launch_stats{};
    c->els = te_encode_launch_stats{};
    c->rbs = te_rebuild_launch_stats{};
    c->rms = te_recover_multi_stats{};
    if (nobj == 0) return TE_OK;
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    // h_slices is of one kind (header): asked of the first present slice, absent slots may be unmapped
    bool pin_in = true;
    for (size_t i = 0; i < nobj; i++)
        if (const uint32_t m = objs[i].avail_mask & slice_bits(c)) {
            pin_in = host_pinned(h_slices + objs[i].slices_off + (uint64_t)__builtin_ctz(m) * objs[i].slice_len);
            break;
        }
    const bool pin_out = host_pinned(h_out), copy_only = rebuild_copy_only();
    std::vector<RebuildWin> wins(cuts.size() - 1);
    for (size_t w = 0; w < wins.size(); w++) {
        RebuildWin &W = wins[w];
        const size_t a = cuts[w];
        W.rm = objs + a;
        W.items = items.data() + a;
        W.ok_flag = single;
        W.cfg = *cfg;
        W.h_in = h_slices;
        W.h_out = h_out;
        W.h_meta = h_meta + a * TE_META_SIZE;
        W.h_leaves = verified ? h_leaves + a * n * TE_HASH_SIZE : nullptr;
        W.nobj = cuts[w + 1] - a;
        W.h_rej = h_rejected_mask ? h_rejected_mask + a : nullptr;
        W.h_ok = h_ok_mask ? h_ok_mask + a : nullptr;
        W.h_status = h_status ? h_status + a : nullptr;
        W.pre = pre.data() + a;
        W.mode = g_commit_hashing.load();
        W.pinned_in = pin_in;
        W.pinned_out = pin_out;
        W.copy_only = copy_only;
    }
    return rebuild_run(c, wins);
}

}  // namespace

extern "C" {

int te_repair_window_plan(const te_clay *c, const te_repair_object *objs, size_t nobj, size_t window_bytes,
                          size_t *cuts, size_t cap, size_t *nwindows) {
    if (!c || !nwindows || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    *nwindows = 0;
    std::vector<uint64_t> bytes;
    if (int r = repair_object_bytes(c, objs, nobj, bytes)) return r;
    std::vector<size_t> v;
    window_cuts(bytes, window_bytes, v);
    return cuts_out(v, cuts, cap, nwindows);
}

int te_recover_window_plan(const te_clay *c, const te_recover_object *objs, size_t nobj, size_t window_bytes,
                           size_t *cuts, size_t cap, size_t *nwindows) {
    if (!c || !nwindows || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    *nwindows = 0;
    std::vector<uint64_t> bytes(nobj);  // rec_multi_object_bytes of one lost slice, whatever `lost` says
    for (size_t i = 0; i < nobj; i++)
        bytes[i] = ((uint64_t)__builtin_popcount(objs[i].avail_mask & slice_bits(c)) + 1u) * objs[i].slice_len;
    std::vector<size_t> v;
    window_cuts(bytes, window_bytes, v);
    return cuts_out(v, cuts, cap, nwindows);
}

int te_repair_batch_host(te_clay *c, const uint8_t *h_helpers, const te_repair_object *objs, const uint8_t *h_leaves,
                         size_t nobj, uint8_t *h_out, uint32_t *h_ok, size_t window_bytes) {
    if (!c || ((!objs || !h_helpers || !h_out) && nobj) || (h_leaves && !h_ok && nobj)) return TE_ERR_INVALID_ARG;
    const uint32_t n = (uint32_t)c->h.n;
    if (nobj > 0xffffffffull / n) return TE_ERR_INVALID_ARG;
    uint64_t need[64];
    for (size_t i = 0; i < nobj; i++) {
        const te_repair_plan *p = objs[i].plan;
        if (!p || p->n != n || p->d != (uint32_t)c->h.d || p->n > 64 || p->lost >= n) return TE_ERR_INVALID_ARG;
        plan_needs(p, need);
        for (uint32_t sl = 0; sl < n; sl++)
            if (need[sl] && objs[i].helper_off[sl] == ~0ull) return TE_ERR_MISSING_HELPER;
    }
    std::vector<uint64_t> bytes;
    if (int r = repair_object_bytes(c, objs, nobj, bytes)) return r;
    std::vector<size_t> cuts;
    window_cuts(bytes, window_bytes, cuts);
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    c->rls = te_repair_launch_stats{};
    c->rbs = te_rebuild_launch_stats{};
    if (nobj == 0) return TE_OK;
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    const bool pin_in = host_pinned(h_helpers), pin_out = host_pinned(h_out), copy_only = rebuild_copy_only();
    std::vector<RebuildWin> wins(cuts.size() - 1);
    for (size_t w = 0; w < wins.size(); w++) {
        RebuildWin &W = wins[w];
        const size_t a = cuts[w];
        W.rep = objs + a;
        W.ok_flag = true;
        W.h_in = h_helpers;
        W.h_out = h_out;
        W.h_leaves = h_leaves ? h_leaves + a * n * TE_HASH_SIZE : nullptr;
        W.nobj = cuts[w + 1] - a;
        W.h_ok = h_ok ? h_ok + a : nullptr;
        W.mode = g_commit_hashing.load();
        W.pinned_in = pin_in;
        W.pinned_out = pin_out;
        W.copy_only = copy_only;
    }
    return rebuild_run(c, wins);
}

// The single form converts its objects at its boundary; its one lost slice makes h_ok 0 or 1 (ok_flag)
int te_recover_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices, const te_recover_object *objs,
                          const uint8_t *h_meta, const uint8_t *h_leaves, size_t nobj, uint8_t *h_out,
                          uint32_t *h_rejected_mask, uint32_t *h_ok, int *h_status, size_t window_bytes) {
    std::vector<te_recover_multi_object> mo;
    if (c && objs && nobj <= 0xffffffffull / (uint32_t)c->h.n) {  // (a larger count is recover_host's TE_ERR_INVALID_ARG)
        mo.reserve(nobj);
        for (size_t i = 0; i < nobj; i++) mo.push_back(rec_single(c, objs[i]));
    }
    return recover_host(c, cfg, h_slices, objs ? mo.data() : nullptr, h_meta, h_leaves, nobj, h_out, h_rejected_mask, h_ok,
                        h_status, window_bytes, true);
}

int te_recover_multi_window_plan(const te_clay *c, const te_recover_multi_object *objs, size_t nobj, size_t window_bytes,
                                 size_t *cuts, size_t cap, size_t *nwindows) {
    if (!c || !nwindows || (!objs && nobj)) return TE_ERR_INVALID_ARG;
    *nwindows = 0;
    std::vector<uint64_t> bytes(nobj);
    for (size_t i = 0; i < nobj; i++)
        bytes[i] = rec_multi_object_bytes(c->h.n, objs[i].avail_mask, objs[i].lost_mask, objs[i].slice_len);
    std::vector<size_t> v;
    window_cuts(bytes, window_bytes, v);
    return cuts_out(v, cuts, cap, nwindows);
}

int te_recover_multi_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices,
                                const te_recover_multi_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                size_t nobj, uint8_t *h_out, uint32_t *h_rejected_mask, uint32_t *h_ok_mask, int *h_status,
                                size_t window_bytes) {
    return recover_host(c, cfg, h_slices, objs, h_meta, h_leaves, nobj, h_out, h_rejected_mask, h_ok_mask, h_status,
                        window_bytes, false);
}

int te_clay_rebuild_launch_stats(te_clay *c, te_rebuild_launch_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->rbs;
    return TE_OK;
}

}  // extern "C"

extern "C" {

// ------------------------------------------------------------------------------------------
// OuterCoder: GF(2^16) Leopard RS (lib/slicer/src/outer.rs:19-197)
// ------------------------------------------------------------------------------------------
size_t te_outer_chunk_bytes(uint32_t k, size_t len) {  // outer.rs:74-80
    if (k == 0) return 0;
    if (len == 0) return 64;
    const size_t raw = (len + k - 1) / k;
    return (raw + 63) / 64 * 64;
}

}  // extern "C"
namespace {
// shard j of a segment at + j * stride (te_outer_encode_device: stride = chunk_bytes; the snapshot
// encode: its payload slots); wait = false leaves the launch enqueued
int outer_encode_matrix(uint32_t k, uint32_t m, const uint8_t *d_in, uint64_t chunk_bytes, uint64_t stride,
                        uint32_t segments, uint64_t seg_in, uint8_t *d_out, uint64_t seg_out, hipStream_t s, bool wait);
// te_outer_launch_stats: the outermost te_outer_* call on this thread zeroes the stats once its
// arguments are checked (te_outer_encode calls te_outer_encode_device); the launchers
// (rs16.hip) and outer_lut add to them
thread_local int g_outer_depth = 0;
struct OuterCall {
    OuterCall() { if (g_outer_depth++ == 0) rs16_launch_stats() = te_outer_launch_stats{}; }
    ~OuterCall() { g_outer_depth--; }
    OuterCall(const OuterCall &) = delete;
    OuterCall &operator=(const OuterCall &) = delete;
};
// te_outer_encode_device with the shards of a segment `stride` bytes apart, in and out (the kernels
// address 16-bit units through in_stride / out_stride; nothing in them assumes stride ==
// chunk_bytes).  *waited (or NULL): whether the call waited for the stream -- always with
// wait = true; with wait = false only the transform path does, whose host tables must outlive
// their copy.
int outer_encode_strided(uint32_t k, uint32_t m, const uint8_t *d_in, uint64_t chunk_bytes, uint64_t stride,
                         uint32_t segments, uint64_t seg_in, uint8_t *d_out, uint64_t seg_out, void *stream, bool wait,
                         bool *waited) {
    if (waited) *waited = true;
    if (k == 0 || m == 0 || !d_in || !d_out || chunk_bytes == 0 || chunk_bytes % 64 || chunk_bytes / 2 > 0xffffffffull)
        return TE_ERR_INVALID_ARG;
    if (rs16::use_high_rate(k, m) < 0) return TE_ERR_UNSUPPORTED;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    const OuterCall call;
    // the encode as a matrix product (rs16_matrix_kernel) when its lookup image fits the LDS budget:
    // OuterCoder(17, 50) 17 x 33; the transforms below otherwise
    if (rs16_mat_supported(k, m) && !tec_knob("TEC_RS16_NO_MATRIX"))
    {
        if (waited) *waited = wait;
        return outer_encode_matrix(k, m, d_in, chunk_bytes, stride, segments, seg_in, d_out, seg_out, (hipStream_t)stream,
                                   wait);
    }
    const rs16::Tables &T = rs16::tables();
    const uint32_t c = rs16::chunk(k, m), span = rs16::skew_span(k, m), wl = rs16::work_len(k, m);
    if ((size_t)span * 128 + (size_t)wl * 256 > 160 * 1024 || span > rs16::kModulus) return TE_ERR_UNSUPPORTED;
    // nibble tables of every skew multiplier the transforms touch (zeros for the basis' zero)
    std::vector<uint16_t> lut((size_t)span * 64, 0);
    for (uint32_t sx = 0; sx < span; sx++) {
        const uint16_t lm = T.skew[sx];
        if (lm == rs16::kModulus) continue;
        for (int q = 0; q < 4; q++)
            for (uint32_t nb = 0; nb < 16; nb++) lut[(size_t)sx * 64 + q * 16 + nb] = T.mul((uint16_t)(nb << (4 * q)), lm);
    }
    hipStream_t s = (hipStream_t)stream;
    uint16_t *d_lut = nullptr;
    TE_HIP(hipMallocAsync((void **)&d_lut, lut.size() * sizeof(uint16_t), s));
    int r = hip_status(hipMemcpyAsync(d_lut, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    if (r == TE_OK) {
        Rs16EncArgs a{};
        a.in = d_in;
        a.out = d_out;
        a.in_stride = a.out_stride = stride;
        a.seg_in = seg_in;
        a.seg_out = seg_out;
        a.lut = d_lut;
        a.k = k; a.m = m; a.c = c; a.high = (uint32_t)rs16::use_high_rate(k, m);
        a.work_len = wl; a.span = span; a.elems = (uint32_t)(chunk_bytes / 2);
        a.one_chunk = !a.high && c <= 32 && wl > c;
        KTimer kt(s);
        r = hip_status(launch_rs16_encode(a, segments, s));
        kt.stop();
    }
    const int r2 = hip_status(hipFreeAsync(d_lut, s));
    if (r == TE_OK) r = hip_status(hipStreamSynchronize(s));  // the host table must outlive the copy
    return r ? r : r2;
}
}  // namespace
extern "C" {

int te_outer_encode_device(uint32_t k, uint32_t m, const uint8_t *d_in, uint64_t chunk_bytes, uint32_t segments,
                           uint64_t seg_in, uint8_t *d_out, uint64_t seg_out, void *stream) {
    return outer_encode_strided(k, m, d_in, chunk_bytes, chunk_bytes, segments, seg_in, d_out, seg_out, stream, true,
                                nullptr);
}

int te_outer_encode(uint32_t k, uint32_t n, const uint8_t *data, size_t len, uint8_t *out, size_t cap,
                    size_t *chunk_bytes_out) {
    if (k == 0 || k > n || (!data && len)) return TE_ERR_INVALID_ARG;
    const size_t cb = te_outer_chunk_bytes(k, len);
    if (chunk_bytes_out) *chunk_bytes_out = cb;
    if (cb > TE_OUTER_MAX_CHUNK_BYTES) return TE_ERR_TOO_MUCH_DATA;  // outer.rs:82-84
    if (!out || cap < (size_t)n * cb) return TE_ERR_BUFFER_TOO_SMALL;
    if (len) memcpy(out, data, len);
    memset(out + len, 0, (size_t)k * cb - len);
    const uint32_t m = n - k;
    if (m == 0) return TE_OK;
    if (rs16::use_high_rate(k, m) < 0) return TE_ERR_UNSUPPORTED;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    const OuterCall call;
    uint8_t *d = nullptr;
    TE_HIP(hipMalloc((void **)&d, (size_t)n * cb));
    int r = hip_status(hipMemcpy(d, out, (size_t)k * cb, hipMemcpyHostToDevice));
    if (r == TE_OK) r = te_outer_encode_device(k, m, d, cb, 1, 0, d + (size_t)k * cb, 0, nullptr);
    if (r == TE_OK) r = hip_status(hipMemcpy(out + (size_t)k * cb, d + (size_t)k * cb, (size_t)m * cb, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return r;
}

}  // extern "C"

// OuterCoder decode tables on the device, cached per (device, k, m, received set, missing set):
// a snapshot read repeats its erasure pattern for every segment, and deriving the decoding matrix
// (k unit-vector encodes and a k x 2k inversion over GF(2^16)), its nmiss x k nibble tables and
// their upload cost ~0.2 ms of host time per call (r04: 3.5 ms of the 6.8 ms step for 16
// segments).  At most kOuterLutCache patterns; the least recently used is freed once the last
// launch that read it (an event) has finished.
namespace {
constexpr size_t kOuterLutCache = 64;
struct OuterLut {
    uint16_t *d = nullptr;
    bool mat = false;      // rs16::mat_image for rs16_matrix_kernel (else per-coefficient nibble tables)
    ReaderEvents readers;  // the last launches that read the table, per stream
    uint64_t tick = 0;
};
std::mutex g_outer_mu;
std::map<std::vector<uint32_t>, OuterLut> g_outer_luts;
uint64_t g_outer_tick = 0;

int outer_lut(uint32_t k, uint32_t m, const std::vector<uint32_t> &recv, const std::vector<uint32_t> &miss, int dev,
              OuterLut *&out) {
    std::vector<uint32_t> key{(uint32_t)dev, k, m};
    key.insert(key.end(), recv.begin(), recv.end());
    key.push_back(0xffffffffu);
    key.insert(key.end(), miss.begin(), miss.end());
    auto it = g_outer_luts.find(key);
    if (it != g_outer_luts.end()) {
        it->second.tick = ++g_outer_tick;
        out = &it->second;
        return TE_OK;
    }
    rs16_launch_stats().lut_misses++;
    const uint32_t nm = (uint32_t)miss.size();
    const bool enc = nm == 1 && miss[0] == 0xfffffffeu;  // the encode matrix (outer_enc_lut)
    const uint32_t rows = enc ? m : nm;
    std::vector<uint16_t> D;
    if (enc) rs16::encode_matrix(k, m, D);
    else if (!rs16::decode_matrix(k, m, recv, D)) return TE_ERR_INVALID_LAYOUT;
    const bool mat = rs16_mat_supported(k, rows);
    if (enc && !mat) return TE_ERR_UNSUPPORTED;
    std::vector<uint16_t> lut;
    if (mat) {  // the missing rows of D, as the matrix kernel's lookup image
        std::vector<uint16_t> Dm((size_t)rows * k);
        for (uint32_t i = 0; i < rows; i++)
            memcpy(&Dm[(size_t)i * k], &D[(size_t)(enc ? i : miss[i]) * k], k * sizeof(uint16_t));
        lut = rs16::mat_image(k, rows, Dm.data(), rs16_mat_tailv(rows), rs16_mat_tail_bytes(rows));
    } else {
        const rs16::Tables &T = rs16::tables();
        lut.assign((size_t)nm * k * 64, 0);
        for (uint32_t i = 0; i < nm; i++)
            for (uint32_t r = 0; r < k; r++) {
                const uint16_t coef = D[(size_t)miss[i] * k + r];
                if (!coef) continue;
                for (int q = 0; q < 4; q++)
                    for (uint32_t nb = 0; nb < 16; nb++)
                        lut[((size_t)i * k + r) * 64 + q * 16 + nb] = T.gmul((uint16_t)(nb << (4 * q)), coef);
            }
    }
    if (g_outer_luts.size() >= kOuterLutCache) {
        auto lru = g_outer_luts.begin();
        for (auto j = g_outer_luts.begin(); j != g_outer_luts.end(); ++j)
            if (j->second.tick < lru->second.tick) lru = j;
        DeviceGuard dg(lru->first[0]);
        (void)lru->second.readers.sync();  // every stream's last reader, then free
        lru->second.readers.destroy();
        (void)hipFree(lru->second.d);
        g_outer_luts.erase(lru);
        rs16_launch_stats().lut_evictions++;
    }
    OuterLut L;
    TE_HIP(hipMalloc((void **)&L.d, lut.size() * sizeof(uint16_t)));
    if (hipError_t e = hipMemcpy(L.d, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(L.d);
        return hip_status(e);
    }
    L.mat = mat;
    L.tick = ++g_outer_tick;
    out = &(g_outer_luts[key] = L);
    return TE_OK;
}

// The encode matrix's image, cached like a decode pattern's (key: received = none, missing = the
// marker 0xfffffffe); the launch waits for its stream (te_outer_encode_device's contract).
int outer_encode_matrix(uint32_t k, uint32_t m, const uint8_t *d_in, uint64_t chunk_bytes, uint64_t stride,
                        uint32_t segments, uint64_t seg_in, uint8_t *d_out, uint64_t seg_out, hipStream_t s, bool wait) {
    int dev = 0;
    TE_HIP(hipGetDevice(&dev));
    int r = TE_OK;
    {
        std::lock_guard<std::mutex> lk(g_outer_mu);
        OuterLut *L = nullptr;
        if ((r = outer_lut(k, m, {}, {0xfffffffeu}, dev, L))) return r;
        Rs16MatArgs a{};
        a.in = d_in;
        a.out = d_out;
        a.in_stride = a.out_stride = stride;
        a.seg_in = seg_in;
        a.seg_out = seg_out;
        a.tab = L->d;
        a.k = k; a.rows = m; a.elems = (uint32_t)(chunk_bytes / 2); a.segments = segments; a.ptrs = 0;
        KTimer kt(s);
        r = hip_status(launch_rs16_matrix(a, s));
        kt.stop();
        if (r == TE_OK) r = hip_status(L->readers.record(s));
    }
    if (r == TE_OK && wait) r = hip_status(hipStreamSynchronize(s));
    return r;
}

// Restore a group's missing chunks: `cnt` segments whose shard pointers are laid out as
// Rs16DecArgs::ptr (per segment k received, then nm outputs), through the matrix kernel when the
// pattern's table is a matrix image.
int outer_restore(const OuterLut *L, uint32_t k, uint32_t nm, const uint8_t *const *ptr, uint32_t cnt,
                  uint64_t chunk_bytes, hipStream_t s) {
    if (L->mat) {
        Rs16MatArgs a{};
        memcpy(a.ptr, ptr, (size_t)cnt * (k + nm) * sizeof(ptr[0]));
        a.tab = L->d;
        a.k = k; a.rows = nm; a.elems = (uint32_t)(chunk_bytes / 2); a.segments = cnt; a.ptrs = 1;
        KTimer kt(s);
        const int r = hip_status(launch_rs16_matrix(a, s));
        kt.stop();
        return r;
    }
    Rs16DecArgs a{};
    memcpy(a.ptr, ptr, (size_t)cnt * (k + nm) * sizeof(ptr[0]));
    a.lut = L->d;
    a.k = k; a.nmiss = nm; a.elems = (uint32_t)(chunk_bytes / 2);
    KTimer kt(s);
    const int r = hip_status(launch_rs16_decode(a, cnt, s));
    kt.stop();
    return r;
}
}  // namespace

extern "C" {

int te_outer_decode(uint32_t k, uint32_t n, const uint8_t *const *chunks, size_t chunk_bytes, uint8_t *out, size_t cap) {
    if (k == 0 || k > n || !chunks || !out) return TE_ERR_INVALID_ARG;
    std::vector<uint32_t> have;
    for (uint32_t i = 0; i < n; i++)
        if (chunks[i]) have.push_back(i);
    if (have.size() < k) return TE_ERR_NOT_ENOUGH_SLICES;   // outer.rs:127-129
    if (cap < (size_t)k * chunk_bytes) return TE_ERR_BUFFER_TOO_SMALL;
    const uint32_t m = n - k;
    std::vector<uint32_t> miss;
    for (uint32_t i = 0; i < k; i++) {
        if (chunks[i]) memcpy(out + (size_t)i * chunk_bytes, chunks[i], chunk_bytes);
        else miss.push_back(i);
    }
    if (miss.empty()) return TE_OK;
    if (m == 0) return TE_ERR_INVALID_LAYOUT;                 // outer.rs:143-152
    if (chunk_bytes == 0 || chunk_bytes % 64) return TE_ERR_INVALID_LAYOUT;  // the decoder's shard-size check
    if (rs16::use_high_rate(k, m) < 0 || k > kRs16MaxK) return TE_ERR_UNSUPPORTED;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    const OuterCall call;
    std::vector<uint32_t> recv(have.begin(), have.begin() + k);  // any k shards determine the originals
    const uint32_t nm = (uint32_t)miss.size();
    int dev = 0;
    TE_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_outer_mu);
    OuterLut *L = nullptr;
    int r = outer_lut(k, m, recv, miss, dev, L);
    if (r) return r;
    // device image: received shards, then restored shards
    const size_t sh = (size_t)k * chunk_bytes, rs = (size_t)nm * chunk_bytes;
    uint8_t *d = nullptr;
    TE_HIP(hipMalloc((void **)&d, sh + rs));
    std::vector<const uint8_t *> ptr(k + nm);
    for (uint32_t j = 0; j < k && r == TE_OK; j++) {
        ptr[j] = d + (size_t)j * chunk_bytes;
        r = hip_status(hipMemcpy(d + (size_t)j * chunk_bytes, chunks[recv[j]], chunk_bytes, hipMemcpyHostToDevice));
    }
    for (uint32_t i = 0; i < nm; i++) ptr[k + i] = d + sh + (size_t)i * chunk_bytes;
    if (r == TE_OK) {
        r = outer_restore(L, k, nm, ptr.data(), 1, chunk_bytes, nullptr);
        if (r == TE_OK) r = hip_status(L->readers.record(nullptr));
    }
    for (uint32_t i = 0; i < nm && r == TE_OK; i++)
        r = hip_status(hipMemcpy(out + (size_t)miss[i] * chunk_bytes, d + sh + (size_t)i * chunk_bytes, chunk_bytes,
                                 hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return r;
}

}  // extern "C"

namespace {
// OuterCoder decode of `segments` segments on the device (outer.rs:126-197 per segment): segment g's
// chunk i at d_chunks[g * n + i] (NULL = missing), its k data chunks to d_out + g * seg_out.
// Received data chunks are copied; segments are grouped by erasure pattern, and each group's
// missing chunks are restored from its first k received chunks in launches of as many segments
// as fit the kernel's pointer arguments.  Enqueued on the stream, nothing uploaded but a new
// pattern's tables (cached): a snapshot read's segments queue back to back (r04: a host wait per
// segment cost 0.19 ms per 0.2 ms kernel).
int outer_decode_segs(uint32_t k, uint32_t n, const uint8_t *const *d_chunks, uint32_t segments, uint64_t chunk_bytes,
                      uint8_t *d_out, uint64_t seg_out, hipStream_t s) {
    if (k == 0 || k > n || !d_chunks || !d_out || segments == 0) return TE_ERR_INVALID_ARG;
    const uint32_t m = n - k;
    if (chunk_bytes == 0 || chunk_bytes % 64 || chunk_bytes / 2 > 0xffffffffull) return TE_ERR_INVALID_LAYOUT;
    if (segments > 1 && seg_out < (uint64_t)k * chunk_bytes) return TE_ERR_INVALID_ARG;  // segment outputs would overlap
    // validate every segment before anything is enqueued
    std::map<std::vector<uint32_t>, std::vector<uint32_t>> groups;  // recv | miss -> segments
    for (uint32_t g = 0; g < segments; g++) {
        const uint8_t *const *ch = d_chunks + (size_t)g * n;
        std::vector<uint32_t> have, miss;
        for (uint32_t i = 0; i < n; i++)
            if (ch[i]) have.push_back(i);
        if (have.size() < k) return TE_ERR_NOT_ENOUGH_SLICES;   // outer.rs:127-129
        for (uint32_t i = 0; i < k; i++)
            if (!ch[i]) miss.push_back(i);
        if (miss.empty()) continue;
        if (m == 0) return TE_ERR_INVALID_LAYOUT;  // outer.rs:143-152
        if (rs16::use_high_rate(k, m) < 0 || k > kRs16MaxK || k + miss.size() > kRs16DecPtrs) return TE_ERR_UNSUPPORTED;
        std::vector<uint32_t> key(have.begin(), have.begin() + k);  // any k shards determine the originals
        key.push_back(0xffffffffu);
        key.insert(key.end(), miss.begin(), miss.end());
        groups[key].push_back(g);
    }
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    const OuterCall call;
    int r = TE_OK;
    for (uint32_t g = 0; g < segments && r == TE_OK; g++)
        for (uint32_t i = 0; i < k && r == TE_OK; i++)
            if (const uint8_t *c = d_chunks[(size_t)g * n + i])
                r = hip_status(hipMemcpyAsync(d_out + g * seg_out + (size_t)i * chunk_bytes, c, chunk_bytes,
                                              hipMemcpyDeviceToDevice, s));
    if (r != TE_OK || groups.empty()) return r;
    int dev = 0;
    TE_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_outer_mu);
    for (const auto &gr : groups) {
        const auto sep = std::find(gr.first.begin(), gr.first.end(), 0xffffffffu);
        const std::vector<uint32_t> recv(gr.first.begin(), sep), miss(sep + 1, gr.first.end());
        const uint32_t nm = (uint32_t)miss.size(), per = k + nm, fit = kRs16DecPtrs / per;
        OuterLut *L = nullptr;
        if ((r = outer_lut(k, m, recv, miss, dev, L))) return r;
        for (size_t g0 = 0; g0 < gr.second.size(); g0 += fit) {
            const uint32_t cnt = (uint32_t)std::min<size_t>(fit, gr.second.size() - g0);
            const uint8_t *ptr[kRs16DecPtrs];
            for (uint32_t q = 0; q < cnt; q++) {
                const uint32_t g = gr.second[g0 + q];
                for (uint32_t j = 0; j < k; j++) ptr[q * per + j] = d_chunks[(size_t)g * n + recv[j]];
                for (uint32_t i = 0; i < nm; i++) ptr[q * per + k + i] = d_out + g * seg_out + (size_t)miss[i] * chunk_bytes;
            }
            if ((r = outer_restore(L, k, nm, ptr, cnt, chunk_bytes, s))) return r;
        }
        if ((r = hip_status(L->readers.record(s)))) return r;
    }
    return r;
}
}  // namespace

extern "C" {

int te_outer_last_launch_stats(te_outer_launch_stats *out) {
    if (!out) return TE_ERR_INVALID_ARG;
    *out = rs16_launch_stats();
    return TE_OK;
}

int te_outer_decode_device(uint32_t k, uint32_t n, const uint8_t *const *d_chunks, uint64_t chunk_bytes,
                           uint8_t *d_out, void *stream) {
    return outer_decode_segs(k, n, d_chunks, 1, chunk_bytes, d_out, 0, (hipStream_t)stream);
}

int te_outer_decode_device_batch(uint32_t k, uint32_t n, const uint8_t *const *d_chunks, uint32_t segments,
                                 uint64_t chunk_bytes, uint8_t *d_out, uint64_t seg_out, void *stream) {
    return outer_decode_segs(k, n, d_chunks, segments, chunk_bytes, d_out, seg_out, (hipStream_t)stream);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Snapshot codec (snapshot.hip; lib/snapshot/src/{encode,decode,chunk}.rs,
// network/protocol/src/snapshot.rs:143-275): OuterCoder and per-group Clay as one device pipeline
// ------------------------------------------------------------------------------------------
namespace {

struct SnapPlan {
    te_snapshot_plan_info info{};
    std::vector<te_snapshot_segment> segs;
};

// encode_snapshot's cut (encode.rs:62-71) and every segment's geometry
int snap_plan(const te_clay *c, uint64_t len, uint32_t n, SnapPlan &P) {
    if (!c || n == 0) return TE_ERR_INVALID_ARG;  // NoGroups
    const uint32_t k = te_snapshot_outer_k(n);
    if (n > k && rs16::use_high_rate(k, n - k) < 0) return TE_ERR_UNSUPPORTED;
    const uint64_t max_seg = te_snapshot_max_segment_bytes(n);
    te_snapshot_plan_info &I = P.info;
    I.total_groups = n;
    I.outer_k = k;
    I.compressed_len = len;
    I.max_segment_bytes = max_seg;
    I.segments = std::max<uint64_t>(1, (len + max_seg - 1) / max_seg);
    I.segment_bytes = std::max<uint64_t>(1, (len + I.segments - 1) / I.segments);
    I.chunks = I.segments * n;
    P.segs.resize(I.segments);
    uint64_t off = 0;
    for (uint64_t s = 0; s < I.segments; s++) {
        te_snapshot_segment &g = P.segs[s];
        g.start = std::min(s * I.segment_bytes, len);
        g.len = std::min(g.start + I.segment_bytes, len) - g.start;
        g.symbol_bytes = te_outer_chunk_bytes(k, TE_SNAPSHOT_SEGMENT_HEADER + g.len);
        g.payload_len = TE_SNAPSHOT_HEADER_SIZE + g.symbol_bytes;
        te_slicer_geometry(c, g.payload_len, &g.geom);
        g.slices_off = off;
        g.size = g.symbol_bytes;
        g.stripe_count = te_num_stripes(g.symbol_bytes, g.geom.stripe_size);
        off += (uint64_t)n * (uint64_t)c->h.n * g.geom.slice_len;
    }
    I.total_slice_bytes = off;
    return TE_OK;
}

// the payload scratch of segments [s0, s1) of the encode: SnapPackArgs' slots (kernels.hpp)
uint64_t snap_work_bytes(const SnapPlan &P, uint64_t s0, uint64_t s1) {
    const uint64_t n = P.info.total_groups;
    return 64u + (s1 - s0 - 1u) * n * (P.segs[s0].symbol_bytes + 64u) + n * (P.segs[s1 - 1u].symbol_bytes + 64u);
}
uint64_t snap_work_bytes(const SnapPlan &P) { return snap_work_bytes(P, 0, P.info.segments); }

te_slicer_cfg snap_cfg(const te_clay *c) {  // Slicer::clay_default(): rotated, chunk_index 0 (slicer.rs:151-159, 214)
    te_slicer_cfg cfg{};
    cfg.rotated = 1;
    cfg.encoding = TE_ENCODING_CLAY;
    cfg.params = (uint64_t)c->h.n | (uint64_t)c->h.k << 8 | (uint64_t)c->h.d << 16;
    cfg.chunk_index = 0;
    return cfg;
}

int snap_check_coder(const te_clay *c) {  // 20 leaves in a height-5 tree; dword-hashed slices
    if (c->h.n > (1 << TE_SLICE_TREE_HEIGHT) || c->h.n > (int)TE_COMMIT_MAX_LEAVES) return TE_ERR_UNSUPPORTED;
    return TE_OK;
}

// Handle locked, its device current: the four steps for segments [s0, s1) of the plan, enqueued on
// s.  d_src is segment s0's first byte, d_slices its first slice, d_leaf / d_roots its first
// chunk's; d_work holds snap_work_bytes(P, s0, s1).  Only the plan's last segment differs in symbol
// size, so a range is at most two runs.  Adds to c->sns and c->els (the entry points zero them).
int snapshot_encode_locked(te_clay *c, const SnapPlan &P, uint64_t s0, uint64_t s1, const uint8_t *d_src,
                           uint8_t *d_slices, uint8_t *d_leaf, uint8_t *d_roots, uint8_t *d_work, hipStream_t s,
                           Arena *arena = nullptr) {
    const te_snapshot_plan_info &I = P.info;
    const uint32_t n = I.total_groups, k = I.outer_k, ni = (uint32_t)c->h.n;
    const uint64_t S = s1 - s0, sym_a = P.segs[s0].symbol_bytes, sym_b = P.segs[s1 - 1u].symbol_bytes;
    const uint64_t seg_slots = (uint64_t)n * (sym_a + 64u), out0 = P.segs[s0].slices_off;
    if (S == 0 || S > 0xffffffffull / n) return TE_ERR_TOO_MUCH_DATA;
    c->sns.segments += S;
    c->sns.chunks += S * n;
    // 1. headers, data payloads, padding
    {
        SnapPackArgs a{};
        a.src = d_src;
        a.work = d_work;
        a.len = P.segs[s1 - 1u].start + P.segs[s1 - 1u].len - P.segs[s0].start;
        a.seg_bytes = I.segment_bytes;
        a.sym_a = sym_a;
        a.sym_b = sym_b;
        a.seg0 = s0;
        a.segs = (uint32_t)S;
        a.k = k;
        a.n = n;
        KTimer kt(s);
        TE_HIP(launch_snap_pack(a, s));
        kt.stop();
        c->sns.pack_launches++;
    }
    // runs of segments with one symbol size: [0, S - 1) and the last, or all of them
    struct Run { uint64_t first, count, sym; };
    std::vector<Run> runs;
    if (sym_a == sym_b) runs.push_back({0, S, sym_a});
    else { runs.push_back({0, S - 1, sym_a}); runs.push_back({S - 1, 1, sym_b}); }
    // 2. recovery symbols straight into their payload slots (8 bytes into the first payload)
    if (n > k) {
        const OuterCall call;
        for (const Run &r : runs) {
            uint8_t *in = d_work + 64u + r.first * seg_slots;
            bool waited = false;
            const int e = outer_encode_strided(k, n - k, in, r.sym, r.sym + 64u, (uint32_t)r.count, seg_slots,
                                               in + (uint64_t)k * (r.sym + 64u), seg_slots, s, false, &waited);
            if (e) return e;
            if (waited) c->sns.host_waits++;
        }
        const te_outer_launch_stats &os = rs16_launch_stats();
        c->sns.outer_launches += os.matrix_launches + os.transform_launches + os.low_reg_launches;
    }
    // 3. one Clay encode over every payload
    {
        std::vector<te_object> objs((size_t)(S * n));
        for (uint64_t sg = 0; sg < S; sg++) {
            const te_snapshot_segment &g = P.segs[s0 + sg];
            for (uint32_t p = 0; p < n; p++) {
                te_object &o = objs[(size_t)(sg * n + p)];
                o.data_off = 56u + sg * seg_slots + (uint64_t)p * (g.symbol_bytes + 64u);
                o.blob_len = g.payload_len;
                o.out_off = g.slices_off - out0 + (uint64_t)p * ni * g.geom.slice_len;
                o.chunk_index = 0;
            }
        }
        const te_slicer_cfg cfg = snap_cfg(c);
        const int e = encode_enqueue(c, &cfg, d_work, objs.data(), objs.size(), d_slices, s, false, arena);
        if (e) return e;
        c->sns.clay_objects += objs.size();
    }
    // 4. commitments, per run (one slice length each)
    if (d_leaf) {
        for (const Run &r : runs) {
            const te_snapshot_segment &g = P.segs[(size_t)(s0 + r.first)];
            const uint64_t t0 = r.first * n;
            const int e = te_commit_batch_device(d_slices + (g.slices_off - out0), (uint64_t)ni * g.geom.slice_len,
                                                 g.geom.slice_len, ni, (size_t)(r.count * n), TE_SLICE_TREE_HEIGHT,
                                                 d_leaf + t0 * ni * TE_HASH_SIZE,
                                                 d_roots ? d_roots + t0 * TE_HASH_SIZE : nullptr, nullptr, s);
            if (e) return e;
            c->sns.commit_launches++;
        }
    }
    return TE_OK;
}

// The host forms keep their device buffers between calls up to this size each; a larger one (a
// snapshot of many full segments) is released when the call returns, its streams drained.
constexpr size_t kSnapKeepBytes = (size_t)256 << 20;
void snap_trim(std::initializer_list<DevBuf *> bufs) {
    for (DevBuf *b : bufs)
        if (b->cap > kSnapKeepBytes) b->release();
}

// The decode's per-track outcome before any device work, and its scratch layout:
// [payload slots | headers | 64 bytes | packed segments].  A decoded payload is placed 64-byte
// aligned, so its symbol starts 8 bytes in: the Clay decode kernels store at the alignment their
// other callers use, and the rs16 kernels, which read 16-bit units, take the 8-mod-64 pointers.
struct SnapDecLayout {
    std::vector<int> status;          // per track
    std::vector<uint64_t> pay_off;    // per track (status TE_OK)
    std::vector<uint64_t> pay_len;
    uint64_t hdr_off = 0, packed_off = 0, packed_stride = 0, max_segs = 0, total = 0;
};
int snap_decode_layout(const te_clay *c, uint32_t n, const te_snapshot_track *tracks, const uint8_t *h_meta,
                       size_t ntracks, SnapDecLayout &L) {
    const uint32_t k = te_snapshot_outer_k(n);
    const uint32_t all = slice_bits(c);
    L.status.assign(ntracks, TE_OK);
    L.pay_off.assign(ntracks, 0);
    L.pay_len.assign(ntracks, 0);
    uint64_t off = 0, sym_max = 64, live = 0;
    for (size_t t = 0; t < ntracks; t++) {
        DecItem it{};
        int r = decode_validate(c, h_meta + t * TE_META_SIZE, tracks[t].obj.slice_len, tracks[t].obj.avail_mask & all, it);
        if (r == TE_OK && it.blob_len < TE_SNAPSHOT_HEADER_SIZE) r = TE_ERR_INVALID_LAYOUT;  // ChunkPayloadTooShort
        if ((L.status[t] = r)) continue;
        L.pay_off[t] = off;
        L.pay_len[t] = it.blob_len;
        off += (it.blob_len + 63u) / 64u * 64u + 64u;
        sym_max = std::max<uint64_t>(sym_max, it.blob_len - TE_SNAPSHOT_HEADER_SIZE);
        live++;
    }
    L.hdr_off = off;
    off += (8u * (uint64_t)ntracks + 63u) / 64u * 64u;
    L.packed_off = off + 64u;
    L.packed_stride = (uint64_t)k * ((sym_max + 63u) / 64u * 64u) + 64u;
    L.max_segs = std::max<uint64_t>(1, live / k);
    L.total = L.packed_off + L.max_segs * L.packed_stride + 64u;
    return TE_OK;
}

void snap_detail(const char *fmt, uint64_t a = 0, uint64_t b = 0, uint64_t d = 0) {
    snprintf(g_last_error, sizeof(g_last_error), fmt, (unsigned long long)a, (unsigned long long)b, (unsigned long long)d);
}

// Handle locked, its device current.
int snapshot_decode_locked(te_clay *c, uint32_t n, const uint8_t *d_slices, const te_snapshot_track *tracks,
                           const uint8_t *h_meta, const uint8_t *h_leaves, size_t ntracks, uint8_t *d_out, uint64_t out_cap,
                           uint8_t *d_work, size_t work_bytes, int *h_status, uint32_t *h_rejected, uint64_t *h_segment,
                           uint64_t *d_result, hipStream_t s) {
    const uint32_t k = te_snapshot_outer_k(n), ni = (uint32_t)c->h.n;
    SnapDecLayout L;
    snap_decode_layout(c, n, tracks, h_meta, ntracks, L);
    if (work_bytes < L.total) return TE_ERR_BUFFER_TOO_SMALL;
    g_last_error[0] = 0;  // callers tell NOT_ENOUGH_SLICES apart by the detail: none left from an earlier call
    c->sns = te_snapshot_stats{};
    c->dls = te_decode_launch_stats{};
    for (size_t t = 0; t < ntracks; t++) {
        h_status[t] = L.status[t];
        h_segment[t] = ~0ull;
        if (h_rejected) h_rejected[t] = 0;
    }
    // 1. Clay decode of every track that validates
    std::vector<size_t> live;
    for (size_t t = 0; t < ntracks; t++)
        if (!L.status[t]) live.push_back(t);
    const te_slicer_cfg cfg = snap_cfg(c);
    if (!live.empty() && h_leaves) {
        std::vector<te_decode_object> objs(live.size());
        std::vector<uint8_t> meta(live.size() * TE_META_SIZE), leaves(live.size() * ni * TE_HASH_SIZE);
        std::vector<uint32_t> rej(live.size());
        std::vector<int> st(live.size());
        for (size_t i = 0; i < live.size(); i++) {
            const size_t t = live[i];
            objs[i] = tracks[t].obj;
            objs[i].out_off = L.pay_off[t];
            if (objs[i].slice_len % 4u || objs[i].slices_off % 4u) return TE_ERR_INVALID_ARG;
            memcpy(&meta[i * TE_META_SIZE], h_meta + t * TE_META_SIZE, TE_META_SIZE);
            memcpy(&leaves[i * ni * TE_HASH_SIZE], h_leaves + t * ni * TE_HASH_SIZE, (size_t)ni * TE_HASH_SIZE);
        }
        const int e = decode_verified_locked(c, &cfg, d_slices, objs.data(), meta.data(), leaves.data(), objs.size(), d_work,
                                             rej.data(), st.data(), s);
        if (e) return e;
        c->sns.host_waits++;  // the verified masks
        std::vector<size_t> kept;
        for (size_t i = 0; i < live.size(); i++) {
            const size_t t = live[i];
            if (h_rejected) h_rejected[t] = rej[i];
            if ((h_status[t] = st[i]) == TE_OK) kept.push_back(t);
        }
        c->sns.clay_objects = live.size();
        live.swap(kept);
    } else if (!live.empty()) {
        std::vector<DecItem> items(live.size());
        for (size_t i = 0; i < live.size(); i++) {
            const size_t t = live[i];
            decode_validate(c, h_meta + t * TE_META_SIZE, tracks[t].obj.slice_len, tracks[t].obj.avail_mask & slice_bits(c),
                            items[i]);
            items[i].in_base = tracks[t].obj.slices_off;
            items[i].out_off = L.pay_off[t];
        }
        const int e = decode_enqueue(c, &cfg, d_slices, items.data(), items.size(), d_work, s, false);
        if (e) return e;
        c->sns.clay_objects = live.size();
    }
    c->sns.chunks = live.size();
    if (live.empty()) {  // decode.rs:95-97
        snap_detail("NoChunks: snapshot has no decoded chunks");
        return TE_ERR_NOT_ENOUGH_SLICES;
    }
    // 2. the headers, and the one wait
    Arena &A = c->snap;
    {
        std::vector<uint64_t> offs(live.size());
        for (size_t i = 0; i < live.size(); i++) offs[i] = L.pay_off[live[i]];
        A.img.clear();
        const size_t at = A.put(offs.data(), offs.size() * sizeof(uint64_t));
        int e = A.upload(s);
        if (e) return e;
        uint64_t *d_hdr = reinterpret_cast<uint64_t *>(d_work + L.hdr_off);
        KTimer kt(s);
        TE_HIP(launch_snap_headers(d_work, A.at<uint64_t>(at), (uint32_t)live.size(), d_hdr, s));
        kt.stop();
        c->sns.header_launches++;
        if ((e = A.mark_done(s))) return e;
        TE_HIP(c->snap_host.ensure(live.size() * sizeof(uint64_t)));
        TE_HIP(hipMemcpyAsync(c->snap_host.p, d_hdr, live.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if ((e = sync_sleep(s))) return e;
        c->sns.host_waits++;
    }
    // symbols_by_segment (snapshot.rs:159-172), in track order
    std::map<uint64_t, std::vector<size_t>> by_seg;
    for (size_t i = 0; i < live.size(); i++) {
        const uint64_t seg = reinterpret_cast<const uint64_t *>(c->snap_host.p)[i];
        h_segment[live[i]] = seg;
        by_seg[seg].push_back(live[i]);
    }
    // outer_decode_segments' checks (decode.rs:104-127): 0..segment_count contiguous, >= k symbols each
    {
        uint64_t want = 0;
        for (const auto &kv : by_seg) {
            if (kv.first != want) break;
            want++;
        }
        if (want != by_seg.size()) {
            snap_detail("MissingChunk: missing decoded chunk %llu", want);
            return TE_ERR_NOT_ENOUGH_SLICES;
        }
    }
    for (const auto &kv : by_seg)
        if (kv.second.size() < k) {
            snap_detail("InsufficientGroups: only %llu/%llu groups decoded for chunk %llu", kv.second.size(), k, kv.first);
            return TE_ERR_NOT_ENOUGH_SLICES;
        }
    const uint64_t S = by_seg.size();
    c->sns.segments = S;
    if (S > L.max_segs || S > 65535u) return TE_ERR_INVALID_LAYOUT;  // cannot happen with >= k tracks each
    // OuterCoder::decode's own checks (outer.rs:131-170), then its pointer table
    std::vector<uint64_t> sym(S);
    std::vector<const uint8_t *> ptr((size_t)S * n, nullptr);
    for (const auto &kv : by_seg) {
        const uint64_t cb = L.pay_len[kv.second.front()] - TE_SNAPSHOT_HEADER_SIZE;
        for (size_t t : kv.second) {
            if (L.pay_len[t] - TE_SNAPSHOT_HEADER_SIZE != cb || tracks[t].group >= n) return TE_ERR_INVALID_LAYOUT;
            ptr[(size_t)kv.first * n + tracks[t].group] = d_work + L.pay_off[t] + TE_SNAPSHOT_HEADER_SIZE;  // last wins
        }
        if ((uint64_t)k * cb + 64u > L.packed_stride) return TE_ERR_INVALID_LAYOUT;
        sym[kv.first] = cb;
    }
    // 3. outer decode, one call per run of segments with one symbol size
    uint8_t *d_packed = d_work + L.packed_off;
    for (uint64_t a = 0; a < S;) {
        uint64_t b = a + 1;
        while (b < S && sym[b] == sym[a]) b++;
        const int e = te_outer_decode_device_batch(k, n, ptr.data() + (size_t)a * n, (uint32_t)(b - a), sym[a],
                                                   d_packed + a * L.packed_stride, L.packed_stride, s);
        if (e) return e;
        const te_outer_launch_stats &os = rs16_launch_stats();
        c->sns.outer_launches += os.matrix_launches + os.decode_launches;
        a = b;
    }
    // 4. unpack
    {
        std::vector<uint64_t> cap(S);
        for (uint64_t g = 0; g < S; g++) cap[g] = (uint64_t)k * sym[g];
        A.img.clear();
        const size_t at = A.put(cap.data(), cap.size() * sizeof(uint64_t));
        int e = A.upload(s);
        if (e) return e;
        SnapUnpackArgs a{};
        a.packed = d_packed;
        a.cap = A.at<uint64_t>(at);
        a.out = d_out;
        a.result = d_result;
        a.stride = L.packed_stride;
        a.out_cap = out_cap;
        a.segs = (uint32_t)S;
        KTimer kt(s);
        TE_HIP(launch_snap_unpack(a, s));
        kt.stop();
        c->sns.unpack_launches++;
        if ((e = A.mark_done(s))) return e;
    }
    return TE_OK;
}

}  // namespace

extern "C" {

uint32_t te_snapshot_outer_k(uint32_t total_groups) { return total_groups == 0 ? 0u : (total_groups + 2u) / 3u; }

uint64_t te_snapshot_max_segment_bytes(uint32_t total_groups) {
    const uint64_t k = te_snapshot_outer_k(total_groups);
    return k == 0 ? 0u : k * TE_OUTER_MAX_CHUNK_BYTES - TE_SNAPSHOT_SEGMENT_HEADER;
}

int te_snapshot_plan(const te_clay *c, uint64_t compressed_len, uint32_t total_groups, te_snapshot_plan_info *plan,
                     te_snapshot_segment *segs, size_t cap) {
    if (!c || !plan) return TE_ERR_INVALID_ARG;
    SnapPlan P;
    const int r = snap_plan(c, compressed_len, total_groups, P);
    if (r) return r;
    *plan = P.info;
    if (!segs) return TE_OK;
    if (cap < P.segs.size()) return TE_ERR_BUFFER_TOO_SMALL;
    memcpy(segs, P.segs.data(), P.segs.size() * sizeof(te_snapshot_segment));
    return TE_OK;
}

size_t te_snapshot_work_bytes(const te_clay *c, uint64_t compressed_len, uint32_t total_groups) {
    SnapPlan P;
    if (snap_plan(c, compressed_len, total_groups, P)) return 0;
    return (size_t)snap_work_bytes(P);
}

int te_snapshot_encode_device(te_clay *c, const uint8_t *d_compressed, uint64_t len, uint32_t total_groups,
                              uint8_t *d_slices, uint8_t *d_leaf_hashes, uint8_t *d_roots, uint8_t *d_work,
                              size_t work_bytes, void *stream) {
    // d_slices is the commit step's input (te_commit_batch_device: 4-aligned), refused here, before
    // the pack and the encode are enqueued, not after them
    if (!c || (!d_compressed && len) || !d_slices || !d_work || (d_roots && !d_leaf_hashes) ||
        (reinterpret_cast<uintptr_t>(d_work) & 63u) || (d_leaf_hashes && (reinterpret_cast<uintptr_t>(d_slices) & 3u)))
        return TE_ERR_INVALID_ARG;
    SnapPlan P;
    int r = snap_plan(c, len, total_groups, P);
    if (r) return r;
    if ((r = snap_check_coder(c))) return r;
    if (work_bytes < snap_work_bytes(P)) return TE_ERR_BUFFER_TOO_SMALL;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    c->sns = te_snapshot_stats{};
    c->els = te_encode_launch_stats{};
    return snapshot_encode_locked(c, P, 0, P.info.segments, d_compressed, d_slices, d_leaf_hashes, d_roots, d_work,
                                  (hipStream_t)stream);
}

int te_snapshot_encode_host(te_clay *c, const uint8_t *h_compressed, uint64_t len, uint32_t total_groups,
                            uint8_t *h_slices, size_t cap, uint8_t *h_leaf_hashes, uint8_t *h_roots) {
    if (!c || (!h_compressed && len) || (h_roots && !h_leaf_hashes)) return TE_ERR_INVALID_ARG;
    SnapPlan P;
    int r = snap_plan(c, len, total_groups, P);
    if (r) return r;
    if ((r = snap_check_coder(c))) return r;
    if (!h_slices || cap < P.info.total_slice_bytes) return TE_ERR_BUFFER_TOO_SMALL;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    // Windows of whole segments through the encode pipeline's slots (te_encode_batch_host's: three
    // streams, each slot its own arena and buffers), so window w + 1's upload and kernels overlap
    // window w's slice download and the device holds three windows, not the snapshot.  A window is
    // as many segments as keep its slices within 128 MiB, at least one: a full segment at 50 groups
    // (~590 MiB of slices) is a window of its own.  The payloads live in the slot's input buffer,
    // behind the window's compressed bytes, and never leave the device.
    if ((r = ensure_stream(c))) return r;
    for (int q = 0; q < 2; q++)
        if (!c->pipe[q].s) TE_HIP(hipStreamCreateWithFlags(&c->pipe[q].s, hipStreamNonBlocking));
    auto slot_stream = [&](size_t q) { return q < 2 ? c->pipe[q].s : c->stream; };
    uint64_t window_bytes = (uint64_t)128 << 20;
    if (const char *e = tec_knob("TEC_SNAPSHOT_WINDOW_BYTES")) {  // tests: force several windows
        const uint64_t v = strtoull(e, nullptr, 10);
        if (v) window_bytes = v;
    }
    const uint64_t S = P.info.segments, n = total_groups, ni = (uint64_t)c->h.n;
    c->sns = te_snapshot_stats{};
    c->els = te_encode_launch_stats{};
    int rc = TE_OK;
    size_t w = 0;
    for (uint64_t s0 = 0; s0 < S && rc == TE_OK; w++) {
        auto slices_end = [&](uint64_t sg) { return sg < S ? P.segs[sg].slices_off : P.info.total_slice_bytes; };
        uint64_t s1 = s0 + 1;
        while (s1 < S && slices_end(s1 + 1) - slices_end(s0) <= window_bytes) s1++;
        te_clay::Slot &sl = c->pipe[w % te_clay::kPipe];
        const hipStream_t ss = slot_stream(w % te_clay::kPipe);
        const uint64_t work_b = (snap_work_bytes(P, s0, s1) + 63u) / 64u * 64u;
        const uint64_t in_b = P.segs[s1 - 1].start + P.segs[s1 - 1].len - P.segs[s0].start;
        const uint64_t out_b = slices_end(s1) - slices_end(s0), t0 = s0 * n, nt = (s1 - s0) * n;
        const uint64_t leaf_b = nt * ni * TE_HASH_SIZE, root_b = nt * TE_HASH_SIZE;
        if ((rc = hip_status(sl.in.ensure((size_t)(work_b + in_b + 64u)))) || (rc = hip_status(sl.out.ensure((size_t)out_b))) ||
            (rc = hip_status(sl.commit.ensure((size_t)(leaf_b + root_b + 64u)))))
            break;
        uint8_t *d_work = sl.in.as<uint8_t>(), *d_src = d_work + work_b;
        uint8_t *d_leaf = h_leaf_hashes ? sl.commit.as<uint8_t>() : nullptr;
        uint8_t *d_root = h_roots ? sl.commit.as<uint8_t>() + leaf_b : nullptr;
        if (in_b && (rc = hip_status(hipMemcpyAsync(d_src, h_compressed + P.segs[s0].start, (size_t)in_b,
                                                    hipMemcpyHostToDevice, ss))))
            break;
        if ((rc = snapshot_encode_locked(c, P, s0, s1, d_src, sl.out.as<uint8_t>(), d_leaf, d_root, d_work, ss, &sl.arena)))
            break;
        if ((rc = hip_status(hipMemcpyAsync(h_slices + slices_end(s0), sl.out.p, (size_t)out_b, hipMemcpyDeviceToHost, ss))))
            break;
        if (d_leaf && (rc = hip_status(hipMemcpyAsync(h_leaf_hashes + t0 * ni * TE_HASH_SIZE, d_leaf, (size_t)leaf_b,
                                                      hipMemcpyDeviceToHost, ss))))
            break;
        if (d_root &&
            (rc = hip_status(hipMemcpyAsync(h_roots + t0 * TE_HASH_SIZE, d_root, (size_t)root_b, hipMemcpyDeviceToHost, ss))))
            break;
        s0 = s1;
    }
    // also after a failure: copies from and to the caller's buffers may still be queued
    for (size_t q = 0; q < te_clay::kPipe; q++) {
        const int r2 = sync_sleep(slot_stream(q));
        if (rc == TE_OK) rc = r2;
    }
    for (auto &sl : c->pipe) snap_trim({&sl.in, &sl.out, &sl.commit});
    return rc;
}

size_t te_snapshot_decode_work_bytes(const te_clay *c, uint32_t total_groups, const te_snapshot_track *tracks,
                                     const uint8_t *h_meta, size_t ntracks) {
    if (!c || total_groups == 0 || ((!tracks || !h_meta) && ntracks)) return 0;
    SnapDecLayout L;
    snap_decode_layout(c, total_groups, tracks, h_meta, ntracks, L);
    return (size_t)L.total;
}

int te_snapshot_decode_device(te_clay *c, uint32_t total_groups, const uint8_t *d_slices,
                              const te_snapshot_track *tracks, const uint8_t *h_meta, const uint8_t *h_leaves,
                              size_t ntracks, uint8_t *d_out, uint64_t out_cap, uint8_t *d_work, size_t work_bytes,
                              int *h_track_status, uint32_t *h_rejected_mask, uint64_t *h_track_segment,
                              uint64_t *d_result, void *stream) {
    if (!c || total_groups == 0 || !d_work || !d_result || (!d_out && out_cap) ||
        ((!tracks || !h_meta || !d_slices || !h_track_status || !h_track_segment) && ntracks) ||
        (reinterpret_cast<uintptr_t>(d_work) & 63u) || ntracks > 0xffffffffull / (uint32_t)c->h.n)
        return TE_ERR_INVALID_ARG;
    const uint32_t k = te_snapshot_outer_k(total_groups);
    if (total_groups > k && rs16::use_high_rate(k, total_groups - k) < 0) return TE_ERR_UNSUPPORTED;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    return snapshot_decode_locked(c, total_groups, d_slices, tracks, h_meta, h_leaves, ntracks, d_out, out_cap, d_work,
                                  work_bytes, h_track_status, h_rejected_mask, h_track_segment, d_result,
                                  (hipStream_t)stream);
}

int te_snapshot_decode_host(te_clay *c, uint32_t total_groups, const uint8_t *h_slices, const te_snapshot_track *tracks,
                            const uint8_t *h_meta, const uint8_t *h_leaves, size_t ntracks, uint8_t *h_out, uint64_t cap,
                            uint64_t *out_len, int *h_track_status, uint32_t *h_rejected_mask, uint64_t *h_track_segment) {
    if (!c || total_groups == 0 || (!h_out && cap) ||
        ((!tracks || !h_meta || !h_slices || !h_track_status || !h_track_segment) && ntracks) ||
        ntracks > 0xffffffffull / (uint32_t)c->h.n)
        return TE_ERR_INVALID_ARG;
    const uint32_t k = te_snapshot_outer_k(total_groups), ni = (uint32_t)c->h.n, all = slice_bits(c);
    if (total_groups > k && rs16::use_high_rate(k, total_groups - k) < 0) return TE_ERR_UNSUPPORTED;
    if (device_count() <= 0) return TE_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    TE_HIP(dg.err);
    int r = ensure_stream(c);
    if (r) return r;
    hipStream_t s = c->stream;
    // device image of the tracks: a slot of n slices each, only the present ones uploaded
    std::vector<te_snapshot_track> dt(tracks, tracks + ntracks);
    uint64_t in_b = 0;
    for (size_t t = 0; t < ntracks; t++) {
        dt[t].obj.slices_off = in_b;
        in_b += ((uint64_t)ni * tracks[t].obj.slice_len + 63u) / 64u * 64u;
    }
    SnapDecLayout L;
    snap_decode_layout(c, total_groups, tracks, h_meta, ntracks, L);
    TE_HIP(c->snap_in.ensure((size_t)in_b + 64));
    TE_HIP(c->snap_work.ensure((size_t)L.total));
    TE_HIP(c->snap_out.ensure((size_t)cap + 64));
    TE_HIP(c->snap_commit.ensure(64));
    for (size_t t = 0; t < ntracks && r == TE_OK; t++)
        for (uint32_t i = 0; i < ni && r == TE_OK; i++)
            if (((tracks[t].obj.avail_mask & all) >> i) & 1u)
                r = hip_status(hipMemcpyAsync(
                    c->snap_in.as<uint8_t>() + dt[t].obj.slices_off + (uint64_t)i * tracks[t].obj.slice_len,
                    h_slices + tracks[t].obj.slices_off + (uint64_t)i * tracks[t].obj.slice_len,
                    (size_t)tracks[t].obj.slice_len, hipMemcpyHostToDevice, s));
    uint64_t *d_res = c->snap_commit.as<uint64_t>();
    uint64_t res[2] = {0, 0};
    if (r == TE_OK)
        r = snapshot_decode_locked(c, total_groups, c->snap_in.as<uint8_t>(), dt.data(), h_meta, h_leaves, ntracks,
                               c->snap_out.as<uint8_t>(), cap, c->snap_work.as<uint8_t>(), (size_t)L.total, h_track_status,
                               h_rejected_mask, h_track_segment, d_res, s);
    if (r == TE_OK) r = hip_status(hipMemcpyAsync(res, d_res, sizeof(res), hipMemcpyDeviceToHost, s));
    // also after a failure: uploads from the caller's slices may still be queued
    const int r2 = sync_sleep(s);
    if (r == TE_OK) r = r2;
    if (r == TE_OK) {
        if (out_len && (res[0] == TE_OK || res[0] == TE_ERR_BUFFER_TOO_SMALL)) *out_len = res[1];
        r = (int)res[0];
    }
    if (r == TE_OK && res[1]) r = hip_status(hipMemcpy(h_out, c->snap_out.p, (size_t)res[1], hipMemcpyDeviceToHost));
    snap_trim({&c->snap_in, &c->snap_work, &c->snap_out});
    return r;
}

int te_snapshot_launch_stats(te_clay *c, te_snapshot_stats *out) {
    if (!c || !out) return TE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->sns;
    return TE_OK;
}

}  // extern "C"
