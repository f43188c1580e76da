/*
 * tape_ec.h -- C ABI of the MI355X-native Tapedrive erasure-coding engine (libtapeec.so).
 *
 * Drop-in boundary for the reference hot path `lib/slicer` (crate tape-slicer).  Every entry
 * point below replaces one Rust item of lib/slicer's public surface (lib/slicer/src/lib.rs:15-27);
 * the file:line it replaces is cited next to it.  The Rust binding a maintainer would add
 * (an `extern "C"` block behind `ClayCoder`/`Slicer`) is shown in INTEGRATION.md.
 *
 * Conventions (mirroring the reference):
 *   - plain pointers + sizes, caller-allocated outputs, int status (0 = ok), no exceptions;
 *   - status codes map 1:1 onto EncodeError / DecodeError / RepairError
 *     (lib/slicer/src/errors.rs:5-37) plus engine errors;
 *   - all GF(2^8) compute runs on the GPU (gfx950).  With no HIP device the compute entry
 *     points return TE_ERR_NO_DEVICE: there is NO CPU fallback in this library.
 *   - host-only entry points (geometry, metadata, rotation maps, repair planning, helper-side
 *     gather) are pure integer bookkeeping and work without a GPU, as in the reference.
 *   - thread safety: a te_clay may be used from several threads; calls on one te_clay are
 *     serialised internally.  The GPU context is a process-wide singleton.
 */
#ifndef TAPE_EC_H
#define TAPE_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TE_META_SIZE 48      /* SliceMetadata::SIZE          lib/slicer/src/metadata.rs:44 */
#define TE_ROTATION_STEP 7   /* ROTATION_STEP                lib/slicer/src/slicer.rs:21   */
#define TE_GROUP_SIZE 20     /* GROUP_SIZE                   lib/core/src/erasure.rs:5     */
#define TE_ENCODING_CLAY 2   /* EncodingType::Clay           lib/core/src/encoding.rs:25   */
#define TE_CLAY_DEFAULT_PARAMS 0x100714ull /* ClayParams::DEFAULT (20,7,16) encoding.rs:236-239 */

typedef enum te_status {
    TE_OK = 0,
    /* EncodeError  errors.rs:5-11 */
    TE_ERR_TOO_MUCH_DATA = 1,
    TE_ERR_EMPTY_INPUT = 2,
    /* DecodeError  errors.rs:13-23 */
    TE_ERR_NOT_ENOUGH_SLICES = 3,
    TE_ERR_BAD_ENCODING = 4,
    TE_ERR_INVALID_LAYOUT = 5,
    /* RepairError  errors.rs:25-37 */
    TE_ERR_NOT_ENOUGH_HELPERS = 6,
    TE_ERR_INVALID_SLICE = 7,
    TE_ERR_CLAY = 8,
    TE_ERR_MISSING_HELPER = 9,
    /* MerkleError (lib/crypto/src/merkle/tree.rs:360-366) */
    TE_ERR_MERKLE_TREE_FULL = 10,
    TE_ERR_MERKLE_INVALID_PROOF = 11,
    TE_ERR_MERKLE_INVALID_INDEX = 12,
    TE_ERR_MERKLE_PROOF_LENGTH = 13,
    /* engine */
    TE_ERR_INVALID_ARG = 20,
    TE_ERR_NO_DEVICE = 21,
    TE_ERR_HIP = 22,
    TE_ERR_UNSUPPORTED = 23,
    TE_ERR_OUT_OF_MEMORY = 24,
    TE_ERR_BUFFER_TOO_SMALL = 25
} te_status;

const char *te_strerror(int status);
/* Number of usable gfx950 devices (0 on a CPU-only host).  Does not create a context. */
int te_device_count(void);
/* Make `device` the calling thread's current HIP device (hipSetDevice).  Handles do not depend on
 * it: a te_clay runs on the device it is bound to (te_clay_bind_device). */
int te_set_device(int device);
/* Detail of the last TE_ERR_HIP/OOM/NO_DEVICE on the calling thread (HIP error string). */
const char *te_last_error_detail(void);
/* Kernel timing (diagnostics for benchmarks): while enabled, every device batch call records a
 * HIP event pair on its stream around its kernel launches (after descriptor upload).
 * te_kernel_time_ms synchronises on the recorded events, returns their summed elapsed time and
 * count, and clears them.  Off by default; no effect on results. */
int te_kernel_timing(int enable);
int te_kernel_time_ms(double *total_ms, uint32_t *count);
/* Library build identification string. */
const char *te_version(void);

/* ------------------------------------------------------------------------------------------
 * ClayCoder                                                     lib/slicer/src/clay.rs:13-122
 * ------------------------------------------------------------------------------------------ */
typedef struct te_clay te_clay;
typedef struct te_clay_info {
    uint32_t n, k, m, d;     /* ErasureCoder::{n,k,m}, ClayCoder::d()   coder.rs:16-25, clay.rs:43-45 */
    uint32_t q, t, nu;       /* Clay layout: q = d-k+1, t = (n+nu)/q                                */
    uint32_t alpha, beta;    /* ClayCoder::alpha()/beta()                clay.rs:48-57              */
} te_clay_info;

/* ClayCoder::new(n, k, d)  clay.rs:24-34.  The reference panics on invalid params; this returns
 * TE_ERR_INVALID_ARG.  Profiles whose layout the GPU engine does not cover return
 * TE_ERR_UNSUPPORTED. */
int te_clay_new(uint32_t n, uint32_t k, uint32_t d, te_clay **out);
/* ClayCoder::from_params(ClayParams)  clay.rs:37-39 (packed n | k<<8 | d<<16, encoding.rs:193-197) */
int te_clay_from_params(uint64_t packed_params, te_clay **out);
void te_clay_free(te_clay *c);
/* Device binding (SURVEY 8b device-mask context; one SDK process may drive several GPUs): a handle
 * is bound to the device that was current on the creating thread; every allocation and launch it
 * makes runs on that device whatever the calling thread's current device is (the thread's device
 * is restored on return).  Re-binding drains and frees the handle's device state first. */
int te_clay_bind_device(te_clay *c, int device);
int te_clay_device(const te_clay *c);
/* Per-pattern decode kernels (no reference counterpart; an engine knob).  A hot erasure pattern
 * of a q = 10, t = 2 profile gets a kernel with its plane program and decoding matrix compiled
 * in (hipRTC, ~25 s of host time, off the caller's thread in mode 1); until then, and for every
 * other pattern, the table-driven kernel decodes it.  Clay(20,7,16) survivor sets run their
 * ahead-of-time class kernels instead, which time at or below the pattern kernels, unless this
 * function has been called on the handle.  mode: 0 off, 1 async (default; env
 * TEC_DEC_JIT=off|sync|async), 2 sync (compile in the decoding call).  A pattern is built once
 * `min_stripes` of its stripes have been decoded on the handle (default 1024, env
 * TEC_DEC_JIT_MIN). */
int te_clay_set_decode_jit(te_clay *c, int mode, uint64_t min_stripes);
/* Pattern kernels ready / compiling / failed on the handle, after waiting up to `timeout_ms` for
 * compiles in flight to finish. */
int te_clay_decode_jit_status(te_clay *c, uint32_t timeout_ms, uint32_t *ready, uint32_t *pending, uint32_t *failed);
/* Most distinct stripe patterns the handle's device-resident decode store holds (default and
 * maximum 16,384, ~26 KB of device memory and as much host memory each; the store grows by
 * doubling from 256 as patterns arrive).  A call with more distinct patterns than this uploads
 * them with the call. */
int te_clay_set_decode_store_cap(te_clay *c, uint32_t max_patterns);
/* The handle's device-resident decode pattern store (diagnostics): slots allocated (it grows by
 * doubling from 256 up to the cap) and filled, how often a full store was
 * emptied, how often it grew, and how many calls had more distinct stripe patterns than it holds
 * (those upload their patterns with the call instead). */
int te_clay_decode_store_stats(te_clay *c, uint32_t *capacity, uint32_t *used, uint64_t *clears, uint64_t *grows,
                               uint64_t *arena_calls);
/* Which kernels the handle's last decode call launched (diagnostics; host bookkeeping only, no
 * effect on results): one te_clay_decode / te_slicer_decode / te_decode_batch_device /
 * te_recover_batch_device call (or the decode part of their verified forms), summed over its parts
 * and windows when a recover batch is split.
 * Zeroed when such a call has passed its argument checks and starts its device work; all zero
 * before the first one.  class_g is that of the call's last class launches, class_streams the
 * most streams any part used. */
#define TE_DECODE_CLASSES 24
typedef struct te_decode_launch_stats {
    uint32_t class_launches[TE_DECODE_CLASSES]; /* launches per class kernel: 0..7 decode (known
                                                   column-0 nodes), 8 + 2*a0 + column: node recover */
    uint64_t class_stripes;      /* stripes of those launches */
    uint32_t class_g;            /* their column groups per workgroup: 1 per-call kernels, 2 batch
                                    kernels (0: no class launch) */
    uint32_t class_streams;      /* streams the class launches ran on side by side */
    uint32_t table_launches, generic_launches, jit_launches;  /* table-driven, generic, pattern kernels */
    uint32_t direct_out;         /* per-call decode: the kernels stored straight into the caller's
                                    page-locked `out` (no staging copy) */
    uint64_t table_stripes, generic_stripes, jit_stripes;
} te_decode_launch_stats;
int te_clay_decode_launch_stats(te_clay *c, te_decode_launch_stats *out);
/* Which kernels the handle's last encode call launched (diagnostics; host bookkeeping only, no
 * effect on results): one te_clay_encode / te_slicer_encode / te_encode_batch_device /
 * te_encode_batch_host / te_encode_commit_batch_host / te_stream_submit call, or the re-encode of
 * the parity-lost stripes in a te_recover_batch_device call (and its verified form), summed over
 * its windows and launch groups.  A launch group is the stripes of one (chunk size, slice length,
 * data end dword aligned or not, source address even or odd).
 * Zeroed when such a call has passed its argument checks and starts its device work; all zero
 * before the first one.  stage_g and stage_wgs are those of the call's last staged launch. */
typedef struct te_encode_launch_stats {
    uint32_t dma_launches;       /* LDS-DMA kernel (1 MB stripes of Clay(20,7,16)): every launch */
    uint32_t dma_level1_launches, dma_level2_launches; /* of those, the halves of split launches:
                                    the level-1 plane rows, then the level-2 chain */
    uint32_t stage_launches;     /* staged kernel (Clay(20,7,16) and (20,10,19), even addresses) */
    uint32_t stage_masked_launches; /* of those, with a data end that is not dword aligned */
    uint32_t stage_g;            /* their waves (64-word column groups) per workgroup, 1..6 (0: no
                                    staged launch) */
    uint32_t stage_wgs;          /* their workgroups per stripe */
    uint32_t generic_launches;   /* generic kernel: other profiles, odd source addresses, slices
                                    past the 31-bit offset limit */
    uint64_t dma_stripes, stage_stripes, generic_stripes; /* a split launch's stripes count once */
} te_encode_launch_stats;
int te_clay_encode_launch_stats(te_clay *c, te_encode_launch_stats *out);
/* The same for the handle's last repair call: one te_clay_repair / te_slicer_repair /
 * te_repair_batch_device / te_repair_verified_batch_device call, summed over its chunk sizes.
 * fold_g, fold_wgs, stage_g and stage_wgs are those of the call's last such launch. */
typedef struct te_repair_launch_stats {
    uint32_t fold_launches;      /* folded kernel: Clay(20,7,16), all 19 others up or one of the
                                    other column's first 7 down, sub-chunk >= 8 */
    uint32_t stage_launches;     /* staged kernel: every other helper set with a plane program */
    uint32_t generic_launches;   /* generic kernel: sub-chunk < 8, or a set without a program */
    uint32_t fold_g, fold_wgs;   /* waves per workgroup and workgroups per stripe (0: no launch) */
    uint32_t stage_g, stage_wgs;
    uint32_t pad_;
    uint64_t fold_stripes, stage_stripes, generic_stripes;
} te_repair_launch_stats;
int te_clay_repair_launch_stats(te_clay *c, te_repair_launch_stats *out);
int te_clay_get_info(const te_clay *c, te_clay_info *out);
/* ClayCoder::chunk_size_for  clay.rs:61-73 */
size_t te_clay_chunk_size_for(const te_clay *c, size_t input_len);
/* ClayCoder::track_chunk_size  clay.rs:81-84 */
size_t te_clay_track_chunk_size(const te_clay *c, size_t stripe_size, size_t blob_len);
/* ErasureCoder::encode for ClayCoder  clay.rs:99-104.  chunks: n*chunk_size bytes, chunk i at
 * i*chunk_size.  Empty input -> TE_ERR_EMPTY_INPUT.  (GPU) */
int te_clay_encode(te_clay *c, const uint8_t *data, size_t len, uint8_t *chunks, size_t cap,
                   size_t *chunk_size);
/* ErasureCoder::decode for ClayCoder  clay.rs:106-122.  chunks[i] == NULL marks chunk i missing.
 * out: k*chunk_size bytes (padded data; the Slicer trims).  (GPU) */
int te_clay_decode(te_clay *c, const uint8_t *const *chunks, size_t chunk_size, uint8_t *out,
                   size_t cap);
/* ClayCoder::plan_repair  repair.rs:53-70: helpers_out gets d shard ids (ascending),
 * sub_chunks_out gets beta plane indices (ascending).  Host only. */
int te_clay_plan_repair(const te_clay *c, uint32_t lost, const uint32_t *available, size_t navail,
                        uint32_t *helpers_out, uint32_t *sub_chunks_out);
/* ClayCoder::repair  repair.rs:75-88: helper_data[j] = beta*sub_chunk bytes of helpers[j].
 * out = chunk_size bytes.  (GPU) */
int te_clay_repair(te_clay *c, uint32_t lost, const uint32_t *helpers,
                   const uint8_t *const *helper_data, size_t nhelpers, size_t chunk_size,
                   uint8_t *out);

/* ------------------------------------------------------------------------------------------
 * Slicer<ClayCoder>                          lib/slicer/src/{adaptive,slicer,metadata}.rs
 * ------------------------------------------------------------------------------------------ */
size_t te_pick_stripe_size(size_t blob_len);                      /* adaptive.rs:31-39 */
size_t te_num_stripes(size_t blob_len, size_t stripe_size);       /* adaptive.rs:43-49 */
uint32_t te_shard_to_slice(int rotated, uint32_t n, uint32_t stripe, uint32_t shard); /* slicer.rs:34-42 */
uint32_t te_slice_to_shard(int rotated, uint32_t n, uint32_t stripe, uint32_t slice); /* slicer.rs:46-54 */

typedef struct te_slice_metadata {   /* SliceMetadata, 48-byte LE suffix   metadata.rs:22-37 */
    uint64_t version, blob_len, stripe_size, encoding, params, chunk_index;
} te_slice_metadata;
/* SliceMetadata::to_bytes  metadata.rs:66-69 */
void te_slice_metadata_to_bytes(const te_slice_metadata *m, uint8_t out[TE_META_SIZE]);
/* SliceMetadata::from_slice  metadata.rs:72-87 (rejects stripe sizes not in STRIPE_SIZES) */
int te_slice_metadata_from_slice(const uint8_t *slice, size_t len, te_slice_metadata *out);

typedef struct te_slicer_cfg {       /* Slicer fields   slicer.rs:124-132 */
    int rotated;                     /* MappingStrategy::Rotated if non-zero */
    uint64_t encoding, params;       /* EncodingProfile written to the metadata suffix */
    uint64_t chunk_index;            /* ChunkNumber salt */
} te_slicer_cfg;
typedef struct te_geometry {
    uint64_t stripe_size, num_stripes, chunk_size, sub_chunk_size, slice_len;
} te_geometry;
/* Slicer::encode geometry (pick_stripe_size + chunk_size_for + metadata) slicer.rs:237-262 */
int te_slicer_geometry(const te_clay *c, size_t blob_len, te_geometry *out);
/* Slicer::encode  slicer.rs:237-296 (+ encode_empty_blob :368-387).  slices: n*slice_len
 * bytes, slice i at i*slice_len.  (GPU) */
int te_slicer_encode(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *data, size_t len,
                     uint8_t *slices, size_t cap);
/* Slicer::decode  slicer.rs:298-364.  slices[i] == NULL marks slice i missing; all present
 * slices are slice_len bytes.  (GPU) */
int te_slicer_decode(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices,
                     size_t slice_len, uint8_t *out, size_t cap, size_t *out_len);

/* ------------------------------------------------------------------------------------------
 * Repair                                                       lib/slicer/src/repair.rs
 * ------------------------------------------------------------------------------------------ */
typedef struct te_repair_plan te_repair_plan;
typedef struct te_repair_plan_info {  /* RepairPlan  repair.rs:16-28 */
    uint32_t lost, num_stripes, d, beta;
    uint64_t chunk_size, sub_chunk_size;
} te_repair_plan_info;
/* Slicer::repair_plan_from_params  repair.rs:137-201 (host only) */
int te_repair_plan_from_params(const te_clay *c, int rotated, uint32_t lost,
                               const uint32_t *available, size_t navail, uint64_t blob_len,
                               uint64_t stripe_size, te_repair_plan **out);
/* Slicer::repair_plan  repair.rs:208-281 (layout from a reference slice; host only) */
int te_repair_plan_from_slice(const te_clay *c, int rotated, uint32_t lost,
                              const uint32_t *available, size_t navail,
                              const uint8_t *reference, size_t ref_len, te_repair_plan **out);
void te_repair_plan_free(te_repair_plan *p);
int te_repair_plan_get_info(const te_repair_plan *p, te_repair_plan_info *out);
/* StripeRepair/HelperPlan  repair.rs:30-47: helper_slices/helper_shards get d entries,
 * sub_chunks gets d*beta entries (helper-major). */
int te_repair_plan_stripe(const te_repair_plan *p, uint32_t stripe, uint32_t *lost_shard,
                          uint32_t *helper_slices, uint32_t *helper_shards, uint32_t *sub_chunks);
/* Bytes helper `slice` contributes under the plan. */
size_t te_extract_repair_data_size(const te_repair_plan *p, uint32_t helper_slice);
/* extract_repair_data  repair.rs:97-130 (helper-side gather; host only) */
int te_extract_repair_data(const te_repair_plan *p, const uint8_t *slice, size_t slice_len,
                           uint32_t helper_slice, uint8_t *out, size_t cap, size_t *out_len);
/* per_helper_reqs (network/node/src/features/spool/repair.rs:468-491) for one helper: the
 * RepairRequest (network/protocol/src/api/types.rs:75-85) the repairing node sends helper slice
 * `helper_slice` -- one StripeSubChunkRequest {stripe, sub_chunks} per stripe the helper serves,
 * in plan order; stripe k at stripes[k], its beta sub-chunk indices at sub_chunks[k*beta].
 * *count = the number of stripes (arrays NULL: count only). */
int te_repair_plan_helper_request(const te_repair_plan *p, uint32_t helper_slice, uint32_t *stripes,
                                  uint32_t *sub_chunks, size_t cap_stripes, size_t *count);
/* The helper node's extract_repair_data (network/node/src/features/spool/repair.rs:496-553):
 * serve a RepairRequest from the stored slice alone -- geometry from its metadata suffix and the
 * coder's alpha; stripe i's nsub[i] sub-chunk indices are consecutive in sub_chunks; output is
 * every requested sub-chunk in request order.  Layout errors return TE_ERR_INVALID_LAYOUT with
 * the reference's message in te_last_error_detail().  Host only. */
int te_serve_repair_request(te_clay *c, const uint8_t *slice, size_t slice_len, const uint32_t *stripes,
                            const uint32_t *nsub, const uint32_t *sub_chunks, size_t nstripes, uint8_t *out,
                            size_t cap, size_t *out_len);
/* Slicer::repair  repair.rs:324-367: helper_data/helper_lens indexed by SLICE id (n entries,
 * NULL = not provided).  out = num_stripes*chunk_size + 48 bytes.  (GPU) */
int te_slicer_repair(te_clay *c, const te_repair_plan *p, const uint8_t *const *helper_data,
                     const size_t *helper_lens, const uint8_t metadata[TE_META_SIZE],
                     uint8_t *out, size_t cap);

/* ------------------------------------------------------------------------------------------
 * Device-resident batch API (new; the batching seam of sdk/src/stream/write.rs:332-362 and
 * network/node/src/features/spool/repair.rs:94-226).  All pointers are DEVICE pointers;
 * descriptors are host arrays; work is enqueued on `hip_stream` (NULL = default stream) and
 * the call returns without synchronising.
 * ------------------------------------------------------------------------------------------ */
typedef struct te_object {
    uint64_t data_off;    /* object bytes at d_data + data_off */
    uint64_t blob_len;
    uint64_t out_off;     /* n slices at d_out + out_off, slice i at + i*slice_len */
    uint64_t chunk_index;
} te_object;
/* Batched Slicer::encode of nobj objects (each object's geometry from its blob_len). */
int te_encode_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_data,
                           const te_object *objs, size_t nobj, uint8_t *d_out, void *hip_stream);

/* Batched Slicer::encode HOST -> HOST: the shape of the sdk stream writer's encode stage
 * (sdk/src/stream/write.rs:332-362: object bytes in, n slices per object out).  Offsets in
 * `objs` are relative to h_data / h_out.  Objects are pipelined through the device in windows
 * of at most `window_bytes` (input + output; 0 = 128 MiB) over three streams, so the H2D copy of
 * one window, the kernels of the next and the D2H copy of a third overlap.  h_data/h_out
 * should be pinned (hipHostMalloc / hipHostRegister) for full PCIe rate.  Synchronous. */
int te_encode_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data,
                         const te_object *objs, size_t nobj, uint8_t *h_out, size_t window_bytes);
/* The same over several handles (typically one per device): objects are split into contiguous
 * ranges by bytes, one host thread per handle, each running te_encode_batch_host on its range.
 * The first error (by handle order) is returned.  Synchronous. */
int te_encode_batch_host_multi(te_clay *const *coders, size_t ncoders, const te_slicer_cfg *cfg,
                               const uint8_t *h_data, const te_object *objs, size_t nobj, uint8_t *h_out,
                               size_t window_bytes);
/* Host only: the split te_encode_batch_host_multi uses.  cuts[0..nparts] (nparts + 1 entries):
 * part p encodes objects [cuts[p], cuts[p+1]); contiguous, covering, by about equal input bytes
 * (blob_len + 1 per object).  Parts may be empty when nobj < nparts. */
int te_balance_object_ranges(const te_object *objs, size_t nobj, size_t nparts, size_t *cuts);
/* te_encode_batch_host plus the slice commitments of BlobEncoder::encode_with_proofs
 * (sdk/src/codec/encoder.rs:220-260; the stream writer's per-chunk step, sdk/src/stream/write.rs:
 * 332-362): per object o, leaf hashes hash_leaf(slice i) at h_leaf_hashes + (o*n + i)*32, the
 * root root_from_leaf_hashes::<height> at h_roots + o*32 and, if h_proofs is not NULL, proof i
 * (create_proof_from_leaf_hashes::<height>) at h_proofs + ((o*n + i)*height + level)*32.
 * Hashed on the device from the slices in HBM while they are copied out: objects go through the
 * device in groups of at most `window_bytes` (input + output; 0 = 4 GiB; three groups resident),
 * each copied in windows of <= 128 MiB, and one leaf launch hashes a whole group (its time is
 * one slice's SHA-256 whatever the group size, so groups are large).  The handle keeps the three
 * group buffers allocated between calls (te_clay_free frees them).  Requires
 * n <= 2^height, height <= 32 and slice_len % 4 == 0 (every Clay profile with even alpha).
 * Synchronous; objects keep their order. */
int te_encode_commit_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data,
                                const te_object *objs, size_t nobj, uint8_t *h_out, uint32_t height,
                                uint8_t *h_leaf_hashes, uint8_t *h_roots, uint8_t *h_proofs,
                                size_t window_bytes);

/* Ordered, asynchronous window submission: the stream writer's encode stage
 * (sdk/src/stream/write.rs:332-362 keeps up to min(cores, 4) chunk encodes in flight and hands them
 * on in order through FuturesOrdered) as one GPU pipeline per handle.
 *   te_stream_writer_new: over ncoders device-bound handles (one per GPU); window t goes to handle
 *     (t - 1) mod ncoders.  Consecutive windows share a hashing group of at most group_bytes
 *     (input + output; 0 = 8 GiB), hashed once it holds half of that (one leaf launch costs one
 *     slice's SHA-256, ~29 ms, whatever the group size), three groups resident per handle.  The
 *     writer owns its device buffers and runs on the handles' own streams; the handles must
 *     outlive it and must not be re-bound to another device meanwhile.
 *   te_stream_submit: enqueue one window -- te_encode_commit_batch_host's outputs for its objects
 *     (slices at h_out + out_off, leaf hashes, roots, proofs if h_proofs is not NULL) -- and return
 *     its ticket (1, 2, ... in submission order) without waiting for the device: window t+1's
 *     encode overlaps window t's hashing and copies.  Every host buffer of the window must stay
 *     valid (pinned for full overlap) until te_stream_wait has returned for its ticket.
 *   te_stream_wait: complete every window up to `ticket`, in submission order (a window whose
 *     hashing group is still open has it hashed now); returns the first failure among the
 *     windows it completes (TE_OK if none).
 *   te_stream_writer_free: waits for every window, then frees the writer. */
typedef struct te_stream_writer te_stream_writer;
int te_stream_writer_new(te_clay *const *coders, size_t ncoders, const te_slicer_cfg *cfg, uint32_t height,
                         size_t group_bytes, te_stream_writer **out);
int te_stream_submit(te_stream_writer *w, const uint8_t *h_data, const te_object *objs, size_t nobj, uint8_t *h_out,
                     uint8_t *h_leaf_hashes, uint8_t *h_roots, uint8_t *h_proofs, uint64_t *ticket);
int te_stream_wait(te_stream_writer *w, uint64_t ticket);
void te_stream_writer_free(te_stream_writer *w);

/* Who computes the leaf hashes of te_encode_commit_batch_host / te_stream_submit.  SHA-256 is
 * sequential within a slice, so the device hashes one slice per lane (~24 MB/s per lane, one leaf
 * launch ~ one slice's hash time): it wins for groups of many short slices (batches of 4 MiB
 * objects).  The SDK's stream shape -- 64 MiB chunks (MAX_TRACK_SIZE, sdk/src/stream/manifest.rs:22),
 * <= 4 encodes in flight (sdk/src/stream/write.rs:54-57), 9.7 MB slices -- is hashed faster by
 * host cores, as the SDK does (sdk/src/codec/encoder.rs:220-234): the slices are hashed from the
 * host output buffer by a worker pool (x86 SHA extensions when present) as soon as their D2H copy
 * has landed.  TE_HASH_AUTO picks per window (stream writer) or per group (one-shot call) from the
 * slice count, slice length and pool size; the results are identical either way. */
#define TE_HASH_AUTO 0
#define TE_HASH_DEVICE 1
#define TE_HASH_HOST 2
int te_set_commit_hashing(int mode);  /* process default (writers copy it when created) */
int te_stream_writer_set_hashing(te_stream_writer *w, int mode);
/* Host hashing pool size (0 = default: min(16, CPUs in this process's affinity mask)); waits
 * until the pool is idle. */
int te_set_host_hash_threads(int threads);
int te_host_hash_threads(void);
int te_host_sha_extensions(void);     /* 1 if the host SHA-256 uses the CPU's SHA extensions */
double te_host_hash_rate(void);       /* one pool thread's leaf-hash rate, bytes/s (measured at start) */
/* Slices one pool task hashes together, interleaved round by round (1..4): the lane count whose
 * measured per-thread rate is best on this host (a lone SHA-256 chain leaves the CPU's SHA unit
 * idle between dependent rounds). */
int te_host_hash_lanes(void);

/* Page-locked host memory for the host <-> device entry points (te_encode_*_host, te_stream_submit,
 * the per-call te_slicer_* / te_clay_* calls): copies from it run at full PCIe rate and need no
 * driver staging.  The callers of lib/slicer pass pageable Vec<u8>s (sdk/src/track/write.rs:273-308,
 * network/node/src/features/spool/repair.rs:312-339); a binding fills buffers from here instead
 * (rust/tape-slicer-gpu PinnedBuf), or pins an existing allocation in place with te_host_register.
 * Portable: pinned for every device.  Need a HIP device (TE_ERR_NO_DEVICE otherwise). */
int te_host_alloc(size_t bytes, void **out);
void te_host_free(void *p);
int te_host_register(void *p, size_t bytes);
int te_host_unregister(void *p);

typedef struct te_decode_object {
    uint64_t slices_off;  /* slice i at d_slices + slices_off + i*slice_len */
    uint64_t slice_len;
    uint32_t avail_mask;  /* bit i set = slice i present */
    uint32_t pad_;
    uint64_t out_off;     /* blob bytes written at d_out + out_off */
} te_decode_object;
/* Batched Slicer::decode.  Metadata is read on the host from `h_meta` (nobj*48 bytes: one
 * suffix per object, as the caller already holds them); no device->host sync is needed. */
int te_decode_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                           const te_decode_object *objs, const uint8_t *h_meta, size_t nobj,
                           uint8_t *d_out, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Ranged reads: the bytes [start, start + len) of an object from its slices.  The gateway answers
 * S3 Range requests (network/gateway/src/http/handlers/object/response.rs:45-173) and serves a
 * multi-track object with a {skip, take} per chunk (object/manifest.rs:35-52 chunk_range_plan) by
 * decoding each touched track in full and slicing the bytes afterwards (routes.rs:90-91,
 * response.rs:167-169).  Stripes are independent (slicer.rs:333-361), so the engine touches only
 * the stripes s0 = start / S .. s1 = (start + len - 1) / S of the window; each one is either
 *   TE_RANGE_COPY    every data chunk the window intersects is a present slice's (te_shard_to_slice
 *                    under the call's rotation, from avail_mask itself): its bytes are gathered
 *                    straight from the slices, nothing is decoded;
 *   TE_RANGE_DECODE  anything else: the stripe is decoded as in the full call (same pattern) and
 *                    only the window's bytes [lo, hi) of the stripe are stored.
 * With te_clay_set_range_chunk_path on (off by default) a third class takes stripes out of
 * TE_RANGE_DECODE:
 *   TE_RANGE_CHUNK   exactly one of the data chunks the window intersects is an absent slice's:
 *                    that chunk's piece is rebuilt by a node-recover class kernel (7 chunks read,
 *                    the window's bytes of 1 written) and the present chunks' pieces are gathered.
 *                    Clay(20,7,16) only, where a node recover of the stripe would run a class
 *                    kernel; two or more erased chunks in the window stay TE_RANGE_DECODE.
 * Meaning: Slicer::decode (slicer.rs:298-364) followed by bytes[start..start + len]; start = 0,
 * len = blob_len is byte-identical to the full decode.  start + len > blob_len (or an overflow) is
 * TE_ERR_INVALID_ARG; len == 0 is valid and writes nothing; fewer than k present slices is
 * TE_ERR_NOT_ENOUGH_SLICES even for a copy-only window (the reference decodes first).  The
 * per-pattern kernels of te_clay_set_decode_jit are not used by ranged calls.
 * Verified ranged reads are not offered: a leaf commits to a whole slice, so checking it costs the
 * whole slice's SHA-256 whatever the window.  A caller runs te_verify_leaves_device (or keeps a
 * verified mask per track) and passes the good mask as avail_mask.
 * ------------------------------------------------------------------------------------------ */
#define TE_RANGE_COPY 0
#define TE_RANGE_DECODE 1
#define TE_RANGE_CHUNK 2
/* Host only: the plan of a ranged read of an object of blob_len bytes encoded by this coder
 * (geometry as te_slicer_geometry).  *first_stripe = s0, *nstripes = touched stripes (0 for
 * len == 0); for touched stripe i (stripe s0 + i): classes[i], and the window [lo[i], hi[i]) in
 * stripe bytes.  classes / lo / hi may each be NULL, else hold *nstripes entries
 * (<= te_num_stripes).  Works for every profile and without a device. */
int te_slicer_range_plan(const te_clay *c, const te_slicer_cfg *cfg, uint64_t blob_len, uint32_t avail_mask,
                         uint64_t start, uint64_t len, uint64_t *first_stripe, uint64_t *nstripes,
                         uint32_t *classes, uint64_t *lo, uint64_t *hi);
/* The chunk path of ranged reads (TE_RANGE_CHUNK), per handle, 0 = off (the default) / 1 = on.
 * Off, every ranged call classifies, launches and counts exactly as without it.  On, a touched
 * stripe whose window holds exactly one erased data chunk x -- bytes [max(lo, x*cs),
 * min(hi, (x+1)*cs)) -- becomes one windowed recover job: lost node = shard x, the survivor set
 * the stripe's full decode would read, kernel class 8 + 2*a0 (a0 = its known column-0 nodes), the
 * per-call kernels up to 64 stripes in the call (decode stripes included) and the batch kernels
 * above.  Other profiles, sub-chunks below 8 bytes and objects past the class kernels' 31-bit
 * offsets keep TE_RANGE_DECODE.  Results are byte-identical either way. */
int te_clay_set_range_chunk_path(te_clay *c, int on);
int te_clay_range_chunk_path(const te_clay *c);
/* te_slicer_range_plan plus the chunk path: with chunk_path != 0, classes[i] is TE_RANGE_CHUNK
 * exactly where a ranged call with the knob on rebuilds one chunk, and shards[i] is that data
 * shard (UINT32_MAX for every other stripe).  chunk_path == 0: classes, lo and hi equal
 * te_slicer_range_plan's and every shards[i] is UINT32_MAX.  shards may be NULL.  The handle's own
 * knob is not read.  Host only, every profile. */
int te_slicer_range_plan_ex(const te_clay *c, const te_slicer_cfg *cfg, uint64_t blob_len, uint32_t avail_mask,
                            uint64_t start, uint64_t len, int chunk_path, uint64_t *first_stripe,
                            uint64_t *nstripes, uint32_t *classes, uint64_t *lo, uint64_t *hi, uint32_t *shards);
typedef struct te_decode_range_object {  /* te_decode_object plus the window */
    uint64_t slices_off;  /* slice i at d_slices + slices_off + i*slice_len */
    uint64_t slice_len;
    uint32_t avail_mask;  /* bit i set = slice i present */
    uint32_t pad_;
    uint64_t out_off;     /* the window's len bytes at d_out + out_off (any byte alignment) */
    uint64_t start, len;  /* object bytes [start, start + len) */
} te_decode_range_object;
/* Batched ranged read, mirroring te_decode_batch_device (one object per chunk_range_plan entry:
 * {skip, take} = {start, len}).  Exactly len bytes are written per object.  Kernel selection counts
 * the call's decode stripes, not the objects' stripes; the copy stripes of the whole call are one
 * gather launch.  Enqueued on hip_stream; returns without waiting. */
int te_decode_range_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                 const te_decode_range_object *objs, const uint8_t *h_meta, size_t nobj,
                                 uint8_t *d_out, void *hip_stream);
/* The per-call host form beside te_slicer_decode (the single-track object_response_ranged,
 * routes.rs:90-91): out gets the window's len bytes (cap >= len), *out_len = len.  Only the
 * touched stripes' chunks [s*cs, (s+1)*cs) of the slices each stripe's decode reads are staged to
 * the device (a copy stripe: only the present data-chunk bytes it reads; a TE_RANGE_CHUNK stripe:
 * its recover job's k chunks and the window's other present pieces); the metadata suffix is
 * read on the host.  A page-locked `out` is written by the kernels directly.  (GPU) */
int te_slicer_decode_range(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t slice_len,
                           uint64_t start, uint64_t len, uint8_t *out, size_t cap, size_t *out_len);
/* The handle's last ranged call (diagnostics; zeroed when such a call has passed its argument
 * checks; te_clay_decode_launch_stats reports which decode kernels ran for its decode stripes). */
typedef struct te_range_launch_stats {
    uint64_t stripes_touched;  /* = stripes_decoded + stripes_copied (+ te_range_chunk_stats.stripes_rebuilt) */
    uint64_t stripes_decoded;
    uint64_t stripes_copied;
    uint64_t gather_jobs;      /* chunk pieces the one gather launch copied */
    uint64_t bytes_staged;     /* te_slicer_decode_range: slice bytes staged for the device; 0 for
                                  the device form */
} te_range_launch_stats;
int te_clay_range_launch_stats(te_clay *c, te_range_launch_stats *out);
/* The chunk path's share of the handle's last ranged call (all zero with the knob off).  A rebuilt
 * stripe counts in te_range_launch_stats.stripes_touched and here, not in stripes_decoded or
 * stripes_copied; its present pieces count in both gather_jobs; te_clay_decode_launch_stats
 * reports its launch under class_launches[8 + 2*a0] and its stripe in class_stripes. */
typedef struct te_range_chunk_stats {
    uint64_t stripes_rebuilt;  /* TE_RANGE_CHUNK stripes: one windowed recover job each */
    uint64_t gather_jobs;      /* present chunk pieces of those stripes in the call's gather launch */
    uint64_t bytes_stored;     /* bytes the windowed recover jobs stored (sum of their windows) */
} te_range_chunk_stats;
int te_clay_range_chunk_launch_stats(te_clay *c, te_range_chunk_stats *out);

typedef struct te_repair_object {
    const te_repair_plan *plan;
    uint64_t helper_off[TE_GROUP_SIZE]; /* extract_repair_data output of slice i at d_helpers+off */
    uint64_t out_off;                   /* num_stripes*chunk_size + 48 bytes at d_out + out_off */
    uint8_t metadata[TE_META_SIZE];
} te_repair_object;
/* Batched Slicer::repair of nobj lost slices (each with its own plan). */
int te_repair_batch_device(te_clay *c, const uint8_t *d_helpers, const te_repair_object *objs,
                           size_t nobj, uint8_t *d_out, void *hip_stream);

typedef struct te_recover_object {
    uint64_t slices_off;  /* peer slice i at d_slices + slices_off + i*slice_len (if in avail_mask) */
    uint64_t slice_len;
    uint32_t avail_mask;  /* bit i set = slice i present (>= k of them) */
    uint32_t lost;        /* slice index to rebuild */
    uint64_t out_off;     /* the rebuilt slice (slice_len bytes) at d_out + out_off */
} te_recover_object;
/* Batched node recover, network/node/src/features/spool/recover.rs:411-442 `reconstruct`
 * (SURVEY §8f-2): Slicer::decode from the peer slices, Slicer::encode of the object with the
 * peers' chunk_index, keep slice `lost`.  h_meta: one 48-byte suffix per object (host). */
int te_recover_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                            const te_recover_object *objs, const uint8_t *h_meta, size_t nobj,
                            uint8_t *d_out, void *hip_stream);

/* Several lost slices of one object from one decode: `reconstruct` (recover.rs:411-442) decodes
 * k peer slices, re-encodes all n and keeps one; a node that owns L spools of a group, or a
 * gateway healing an object it has just read, wants L of them from the same k peers. */
typedef struct te_recover_multi_object {
    uint64_t slices_off, slice_len; /* peer slice i at d_slices + slices_off + i*slice_len */
    uint32_t avail_mask;   /* >= k bits */
    uint32_t lost_mask;    /* 1..n-k bits, disjoint from avail_mask */
    uint64_t out_off;      /* rebuilt slices, ascending slice index, packed:
                              j-th set bit of lost_mask at d_out + out_off + j*slice_len */
} te_recover_multi_object;
/* Batched multi-slice node recover.  Every rebuilt slice is what te_recover_batch_device writes
 * for that slice: its chunks, then the 48-byte suffix of h_meta (the peers' chunk_index).  The
 * survivors are the decode's (the absent shards padded to n - k erasures: of more than k
 * available slices the decode's k are read).  An object with one lost slice runs
 * te_recover_batch_device's path unchanged; two or more run one multi-output kernel pass per
 * stripe -- or a few, when the lost set is split to fit the kernel -- on q = 10, t = 2 profiles
 * (n = 20), and the decode + re-encode on any other.  out_off has no alignment rule.
 * TE_ERR_INVALID_ARG: lost_mask zero, a bit at or above n, more than n - k bits, or a bit of
 * avail_mask; TE_ERR_NOT_ENOUGH_SLICES below k available slices; the layout errors of
 * te_recover_batch_device for a suffix or slice length that does not validate.  An empty blob's
 * slices are one zero chunk and the suffix. */
int te_recover_multi_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                  const te_recover_multi_object *objs, const uint8_t *h_meta, size_t nobj,
                                  uint8_t *d_out, void *hip_stream);
/* One object, HOST -> HOST: slices[i] is slice i (slice_len bytes) or NULL; the present ones go up
 * once (pageable or page-locked), out[j] receives the j-th set bit of lost_mask (slice_len bytes).
 * A lost bit whose slice is present is TE_ERR_INVALID_ARG.  Synchronous. */
int te_slicer_recover_multi(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices,
                            size_t slice_len, uint32_t lost_mask, uint8_t *const *out);
/* The handle's last te_recover_multi_batch_device / te_slicer_recover_multi call, zeroed when the
 * call has passed its argument checks (host bookkeeping only).  The single-slice and generic
 * objects' kernels are in te_clay_decode_launch_stats / te_clay_encode_launch_stats. */
typedef struct te_recover_multi_stats {
    uint32_t multi_launches;   /* launches of the multi-output kernel (one per chunk size and slice length) */
    uint32_t passes;           /* most passes any stripe took: 1, or its sub-masks after a split (0: no launch) */
    uint64_t jobs;             /* (stripe, sub-mask) jobs of those launches */
    uint64_t out_rows;      /* output rows they stored: alpha per (stripe, lost node) */
    uint64_t stripes;          /* stripes of the multi-kernel objects */
    uint64_t split_stripes;    /* of those, stripes whose lost set was split */
    uint64_t single_objects;   /* objects sent to the single-slice path (one lost slice, or an empty blob) */
    uint64_t generic_objects;  /* objects decoded and re-encoded (profiles without plane programs,
                                  sub-chunks below 8 bytes, slices past the 31-bit offset limit) */
    uint64_t multi_objects;    /* objects on the multi-output kernel */
} te_recover_multi_stats;
int te_clay_recover_multi_launch_stats(te_clay *c, te_recover_multi_stats *out);

/* ------------------------------------------------------------------------------------------
 * Slice commitments: BlobEncoder::encode_with_proofs' step after encode
 * (sdk/src/codec/encoder.rs:226-234) -- hash_leaf per slice, the merkle root and a proof per
 * slice -- from lib/crypto/src/merkle/tree.rs.  Hashes are 32-byte SHA-256 digests.
 * ------------------------------------------------------------------------------------------ */
#define TE_HASH_SIZE 32
#define TE_SLICE_TREE_HEIGHT 5          /* SLICE_TREE_HEIGHT      lib/core/src/erasure.rs:9  */
#define TE_MAX_MERKLE_TREE_HEIGHT 32    /* MAX_MERKLE_TREE_HEIGHT tree.rs:6                  */
#define TE_COMMIT_MAX_LEAVES 64         /* leaves per object in te_commit_batch_device       */

/* hash_leaf (tree.rs:53-56): SHA-256("LEAF" || data).  Host. */
int te_hash_leaf(const uint8_t *data, size_t len, uint8_t out[TE_HASH_SIZE]);
/* hash_leaf of `count` messages of `len` bytes each at data + i*len (an object's slices, as
 * encoder.rs:226-229 hashes them one by one) into out + i*32, `lanes` (1..4; 0 = te_host_hash_lanes)
 * of them interleaved on the calling thread.  Host. */
int te_hash_leaves(const uint8_t *data, size_t len, size_t count, uint32_t lanes, uint8_t *out);
/* hash_pair (tree.rs:58-62): SHA-256("LEFT" || left || "RIGHT" || right).  Host. */
int te_hash_pair(const uint8_t left[TE_HASH_SIZE], const uint8_t right[TE_HASH_SIZE], uint8_t out[TE_HASH_SIZE]);
/* empty_subtree_root / EMPTY_ROOTS[height] (tree.rs:15-48, 64-68), height < 32.  Host. */
int te_empty_subtree_root(uint32_t height, uint8_t out[TE_HASH_SIZE]);
/* root_from_leaf_hashes::<height> (tree.rs:344-350): count <= 2^height (else TREE_FULL). */
int te_merkle_root_from_leaf_hashes(const uint8_t *hashes, size_t count, uint32_t height, uint8_t out[TE_HASH_SIZE]);
/* create_proof_from_leaf_hashes::<height> (tree.rs:353-358, 397-455): `height` hashes. */
int te_merkle_proof_from_leaf_hashes(const uint8_t *hashes, size_t count, size_t index, uint32_t height,
                                     uint8_t *proof_out);
/* verify_proof (tree.rs:462-481) over a pre-hashed leaf: 1 valid, 0 not valid. */
int te_merkle_verify_leaf_hash(const uint8_t leaf_hash[TE_HASH_SIZE], const uint8_t root[TE_HASH_SIZE],
                               const uint8_t *proof, size_t proof_len, uint64_t index, uint32_t height);
/* Batched commitments on the device (DEVICE pointers, enqueued on hip_stream): object o's n
 * slices at d_slices + o*obj_stride + i*slice_len (slice_len % 4 == 0, n <= 64) ->
 * leaf hashes d_leaf_hashes[(o*n + i)*32], roots d_roots[o*32] (NULL: leaves only), proofs
 * d_proofs[((o*n + i)*height + level)*32] (NULL: none).  The slices are read as 32-bit words:
 * a d_slices that is not 4-byte aligned, or an obj_stride or slice_len that is no multiple of 4, is
 * TE_ERR_INVALID_ARG, as are n == 0, n > 64, a NULL d_slices or d_leaf_hashes, d_proofs without
 * d_roots and, with d_roots, a height of 0 or above 32; n > 2^height with d_roots is
 * TE_ERR_MERKLE_TREE_FULL.  All of these are decided before any device call, and nothing is
 * written.  nobj == 0 is TE_OK and writes nothing. */
int te_commit_batch_device(const uint8_t *d_slices, uint64_t obj_stride, uint64_t slice_len, uint32_t n,
                           size_t nobj, uint32_t height, uint8_t *d_leaf_hashes, uint8_t *d_roots,
                           uint8_t *d_proofs, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Data verify: the verify half of the read flow.  verify_track_data (sdk/src/track/read.rs:145-186)
 * re-encodes an object's bytes with BlobEncoder::encode_with_root (sdk/src/codec/encoder.rs:166-193:
 * Slicer::encode, hash_leaf per slice, root_from_leaf_hashes) and compares the root with the
 * on-chain blob.commitment (read.rs:174-185).  Here the slices never leave HBM: the object's bytes
 * go up, 32 + 4 (+ 8) bytes per object come back.
 * ------------------------------------------------------------------------------------------ */
/* Root and check of nobj objects from their leaf hashes (DEVICE pointers, enqueued on hip_stream,
 * not waited for; read.rs:174-185 after encoder.rs:166-193's hashing).  Object o's n leaf hashes
 * at d_leaf_hashes + o*n*32 (as te_commit_batch_device writes them), its expected root at
 * d_expected_roots + o*32 and, if d_expected_leaves is not NULL, its BlobEncoding::leaves at
 * d_expected_leaves + o*n*32.  Outputs: d_roots + o*32 (or NULL) the observed root
 * root_from_leaf_hashes::<height>; d_ok[o] = 1 if it equals the expected root, else 0;
 * d_bad_leaf_mask[o] (or NULL; written only when d_expected_leaves is given) bit i set iff leaf i
 * differs from expected leaf i.  One wave per object.  TE_ERR_INVALID_ARG: n == 0, n > 64,
 * height > 32, n > 2^height, a NULL required pointer, a hash pointer that is not 4-byte aligned. */
int te_roots_check_device(const uint8_t *d_leaf_hashes, uint32_t n, size_t nobj, uint32_t height,
                          const uint8_t *d_expected_roots, const uint8_t *d_expected_leaves,
                          uint8_t *d_roots, uint32_t *d_ok, uint64_t *d_bad_leaf_mask, void *hip_stream);
/* verify_track_data's coded branch (read.rs:174-185; encoder.rs:166-193) over a batch, on the
 * device (DEVICE pointers, `objs` a host array; enqueued on hip_stream, nothing waited for): object
 * o's bytes at d_data + objs[o].data_off are encoded (te_encode_batch_device; chunk_index is part
 * of the 48-byte suffix and so of every leaf), each slice hashed and the root checked
 * (te_roots_check_device's outputs and optional arguments).  objs[o].out_off is ignored: the call
 * lays the slices out itself in d_work (te_verify_data_work_bytes bytes, 16-byte aligned; slices
 * 4-aligned, back to back, then the leaf hashes, which stay there for the caller: object o's at
 * d_work + te_verify_data_work_bytes - (nobj - o)*n*32).  Objects of different slice lengths are
 * hashed in runs of equal length, one leaf launch series per run.  A work_bytes below
 * te_verify_data_work_bytes is TE_ERR_BUFFER_TOO_SMALL.  Requires n <= 64, 1 <= height <= 32,
 * n <= 2^height and slice_len % 4 == 0. */
size_t te_verify_data_work_bytes(const te_clay *c, const te_object *objs, size_t nobj);
int te_verify_data_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_data,
                                const te_object *objs, size_t nobj, uint32_t height,
                                const uint8_t *d_expected_roots, const uint8_t *d_expected_leaves,
                                uint8_t *d_work, size_t work_bytes,
                                uint8_t *d_roots, uint32_t *d_ok, uint64_t *d_bad_leaf_mask, void *hip_stream);
/* The same HOST -> HOST (read.rs:174-185 / encoder.rs:166-193 over a batch): te_encode_commit_batch_host's
 * pipeline -- the same groups of at most `window_bytes` (input + slices; 0 = 8 GiB here: a group
 * costs one slice's hash chain whatever it holds, so fewer are faster) and copy windows, the H2D
 * and encode of one window beside the leaf launches of the group before -- with the slice D2H
 * switched off: per group the only copies back are the results, at most 32 + 4 + 8 bytes per
 * object.  h_expected_leaves, h_roots and h_bad_leaf_mask may be NULL.  Hashing is always on the
 * device: te_set_commit_hashing does not affect these calls (TE_HASH_HOST needs the slices on the
 * host, the copy this path removes).  What bounds it: one slice's SHA-256 chain per group (~24 MB/s
 * per lane, ~29 ms for a 4 MiB object's 715 KB slices), then the H2D copy: 1024 x 4 MiB objects
 * verify in 137 ms against 337 ms on te_encode_commit_batch_host.  The crossover: for slices above
 * about 3 MB (objects above about 18 MB; the SDK's 64 MiB chunks have 9.7 MB slices, ~0.4 s per
 * group: 435 against 195 ms for 32 of them) te_encode_commit_batch_host with host hashing remains
 * the faster route to the same roots.
 * h_data should be pinned for full PCIe rate; pageable memory works.  Synchronous. */
int te_verify_data_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_data,
                              const te_object *objs, size_t nobj, uint32_t height,
                              const uint8_t *h_expected_roots, const uint8_t *h_expected_leaves,
                              uint8_t *h_roots, uint32_t *h_ok, uint64_t *h_bad_leaf_mask,
                              size_t window_bytes);
/* verify_track_data for one object (read.rs:174-185; encoder.rs:166-193): one window of one
 * object through the handle's staging buffers (`data` may be pageable).  *ok = 1 if the root of
 * Slicer::encode(data) under cfg equals expected_root, else 0; observed_root (or NULL) receives
 * the root.  Synchronous. */
int te_slicer_verify_data(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *data, size_t len,
                          uint32_t height, const uint8_t expected_root[TE_HASH_SIZE],
                          uint8_t observed_root[TE_HASH_SIZE], int *ok);
/* The handle's last data-verify call (device batch, host batch or per-call): its objects, copy
 * windows, hashing groups (runs of equal slice length for the device forms), leaf_kernel and
 * root-check launches, and the bytes that crossed PCIe: h2d_bytes the objects' data,
 * h2d_expected_bytes the expected roots and leaves, d2h_bytes the results (no slice byte). */
typedef struct te_verify_data_stats {
    uint64_t objects, windows, groups, leaf_launches, root_check_launches;
    uint64_t h2d_bytes, h2d_expected_bytes, d2h_bytes;
} te_verify_data_stats;
int te_clay_verify_data_launch_stats(te_clay *c, te_verify_data_stats *out);

/* ------------------------------------------------------------------------------------------
 * Verified reads: the read side of the commitments.  Every reader of the reference checks a
 * slice against the object's leaves (BlobEncoding::leaves) before or after it touches the codec:
 * the gateway's object read (network/gateway/src/http/handlers/object/decode.rs:121-139), node
 * recover (network/node/src/features/spool/recover.rs:207-218), repair (repair.rs:339-341), sync
 * (sync.rs:266-289) and snapshot (network/protocol/src/snapshot.rs:255).
 * ------------------------------------------------------------------------------------------ */
/* BlobEncoding::verify_slice (lib/core/src/track/blob.rs:72-79): 1 if position < n and
 * hash_leaf(data) == leaves[position] (leaves: n * 32 bytes), else 0.  Any length.  Host. */
int te_verify_slice(const uint8_t *leaves, uint32_t n, uint32_t position, const uint8_t *data, size_t len);

typedef struct te_verify_item {
    uint64_t offset;     /* the slice's bytes at d_data + offset; offset % 4 == 0 */
    uint64_t len;        /* len % 4 == 0; 0 is hash_leaf(&[]) */
    uint32_t expected;   /* its leaf hash at d_expected + expected * 32 */
    uint32_t object;     /* on a match, d_good_mask[object] |= bit */
    uint32_t bit;
    uint32_t pad_;
} te_verify_item;
/* Host only: the order in which the leaf-verify kernel walks `items`, by SHA-256 block count,
 * descending (equal counts keep the caller's order), so that the lanes of a wave hash slices of
 * like length: order[j] = the caller's index of the j-th item walked. */
int te_verify_order(const te_verify_item *items, size_t nitems, uint32_t *order);
/* hash_leaf of nitems slices of any lengths on the device, checked against expected hashes: the
 * batch form of verify_slice for slices in HBM (DEVICE pointers, `items` a host array; enqueued on
 * hip_stream, returns without waiting).  Outputs are indexed as `items` is:
 *   d_digests   nitems * 32 bytes, required: hash_leaf of item i at d_digests + i * 32 (the call
 *               also parks each slice's running state there between its kernel launches);
 *   d_ok        nitems uint32, or NULL: 1 if item i's digest equals its expected hash, else 0;
 *   d_good_mask uint32 per object, or NULL: a matching item ORs its `bit` into d_good_mask[object].
 *               The call only ever sets bits: the caller zeroes the masks first.
 * d_expected NULL: digests only (d_ok and d_good_mask are then not written).
 * A len or an offset that is no multiple of 4 is TE_ERR_INVALID_ARG, as in te_commit_batch_device. */
int te_verify_leaves_device(te_clay *c, const uint8_t *d_data, const te_verify_item *items, size_t nitems,
                            const uint8_t *d_expected, uint8_t *d_digests, uint32_t *d_ok, uint32_t *d_good_mask,
                            void *hip_stream);
/* The gateway's object read (decode.rs:121-139) over a batch: te_decode_batch_device in which a
 * slice enters the decode only if hash_leaf(slice) == leaves[position].  h_leaves: nobj * n * 32
 * bytes (host), each object's BlobEncoding::leaves.  Every present slice is verified;
 * h_rejected_mask[o] (or NULL) = the present slices that failed (avail & ~good, the handler's
 * hash_mismatches).  An object with at least k verified slices decodes from them, h_status[o] =
 * TE_OK; any other gets h_status[o] = TE_ERR_NOT_ENOUGH_SLICES ("insufficient verified slices",
 * decode.rs:160-170) and nothing is written to its output range.  Returns TE_OK if the call ran;
 * per-object outcomes are in h_status (nobj ints, required).
 * The survivor set of each object is chosen on the host from the verified masks, so the call WAITS
 * ONCE on hip_stream, between the verify kernel and the decode; the decode itself is enqueued and
 * not waited for.  A caller who wants to overlap that wait with other work calls
 * te_verify_leaves_device and te_decode_batch_device on streams of their own.
 * slice_len % 4 == 0 and slices_off % 4 == 0 (TE_ERR_INVALID_ARG otherwise). */
int te_decode_verified_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                    const te_decode_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                    size_t nobj, uint8_t *d_out, uint32_t *h_rejected_mask, int *h_status,
                                    void *hip_stream);
/* Node recover with both of its checks (recover.rs:207-218): te_recover_batch_device from the peer
 * slices that verify against h_leaves (as te_decode_verified_batch_device: h_rejected_mask,
 * h_status, one wait), then verify_slice(lost, rebuilt) on the device: h_ok[o] = 1 if the rebuilt
 * slice hashes to leaves[lost], else 0 (0 too for an object that was not rebuilt).  The rebuilt
 * bytes are written either way; the caller discards a slice whose h_ok is 0 (recover.rs:216).
 * Waits for the results (h_ok is host memory).  out_off % 4 == 0. */
int te_recover_verified_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                     const te_recover_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                     size_t nobj, uint8_t *d_out, uint32_t *h_rejected_mask, uint32_t *h_ok,
                                     int *h_status, void *hip_stream);
/* Multi-slice node recover with both of its checks: the node that owns L spools of a group runs
 * recover.rs:77-244 once per spool, checking the peers and the rebuilt slice each time
 * (recover.rs:207-218) around `reconstruct` (recover.rs:411-442).  This is
 * te_recover_verified_batch_device's contract widened to a lost mask: every slice of avail_mask is
 * hashed against h_leaves (nobj * n * 32 bytes), h_rejected_mask[o] = avail & ~good, the survivors
 * are chosen on the host from the verified slices (one wait).  An object with fewer than k verified
 * slices gets h_status[o] = TE_ERR_NOT_ENOUGH_SLICES, nothing written to its output range and
 * h_ok_mask[o] = 0.  Every other object rebuilds as te_recover_multi_batch_device does (the same
 * routing), then one verify launch hashes all rebuilt slices of all objects: h_ok_mask[o] has the
 * bit of each lost slice whose rebuilt bytes hash to leaves[slice]; the bytes are written either
 * way.  lost_mask is what the caller asked for: a rejected peer does not become a lost slice.
 * Argument errors: te_recover_multi_batch_device's, and TE_ERR_INVALID_ARG for an out_off,
 * slices_off or slice_len that is no multiple of 4; all of them are returned before the call looks
 * for a device.  Waits for the results (h_ok_mask is host memory). */
int te_recover_multi_verified_batch_device(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *d_slices,
                                           const te_recover_multi_object *objs, const uint8_t *h_meta,
                                           const uint8_t *h_leaves, size_t nobj, uint8_t *d_out,
                                           uint32_t *h_rejected_mask, uint32_t *h_ok_mask, int *h_status,
                                           void *hip_stream);
/* Repair with its check (repair.rs:339-341): te_repair_batch_device, then verify_slice(plan.lost,
 * repaired) on the device into h_ok[o].  Helper fragments have no leaf of their own, so only the
 * result is checked.  h_leaves: nobj * n * 32 bytes.  The repaired bytes are written either way.
 * Waits for the results.  out_off % 4 == 0 and a repaired length that is a multiple of 4. */
int te_repair_verified_batch_device(te_clay *c, const uint8_t *d_helpers, const te_repair_object *objs,
                                    const uint8_t *h_leaves, size_t nobj, uint8_t *d_out, uint32_t *h_ok,
                                    void *hip_stream);
/* The per-call form for host slices: Slicer::decode (slicer.rs:298-364) behind the gateway's check
 * (decode.rs:121-139).  slices[i] == NULL marks slice i missing; leaves: n * 32 bytes.  Slices
 * whose hash_leaf differs from leaves[i] are left out of the decode and reported in
 * *rejected_mask (or NULL); fewer than k verified slices is TE_ERR_NOT_ENOUGH_SLICES.  The leaf
 * hashes follow te_set_commit_hashing: the host pool's SHA-256 (te_hash_leaves) or the leaf-verify
 * kernel over the uploaded slices (TE_HASH_AUTO: the host for the few slices of one call; the
 * device needs slice_len % 4 == 0 and the host hashes otherwise).  The results are identical. */
int te_slicer_decode_verified(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *const *slices, size_t slice_len,
                              const uint8_t *leaves, uint8_t *out, size_t cap, size_t *out_len,
                              uint32_t *rejected_mask);

/* ------------------------------------------------------------------------------------------
 * Host read pipeline: the read side's host boundary, the counterpart of te_encode_batch_host /
 * te_encode_commit_batch_host / te_stream_writer_*.  Every reader of the reference holds its
 * slices in host memory: BlobDecoder::decode in the SDK's read_track, and the gateway's
 * decode_track_bytes (network/gateway/src/http/handlers/object/decode.rs:28-91), one call per
 * track of a multi-track object.  All pointers below are HOST pointers; offsets in `objs` are
 * relative to h_slices / h_out.
 * ------------------------------------------------------------------------------------------ */
/* Host only: the windows the read pipeline cuts a batch into.  cuts[0..*nwindows] (*nwindows + 1
 * entries): window w holds objects [cuts[w], cuts[w+1]); contiguous, covering, in object order.
 * A window holds at most window_bytes (0 = 128 MiB), counted per object as its present slices'
 * bytes in (popcount(avail_mask) * slice_len) plus its blob_len out (from its metadata suffix in
 * h_meta); an object larger than that gets a window of its own.  *nwindows is always set (0 for
 * nobj == 0); cuts == NULL returns the count only, fewer than *nwindows + 1 entries (`cap`) is
 * TE_ERR_BUFFER_TOO_SMALL.  A suffix that does not parse is that suffix's error.  Works without a
 * device. */
int te_decode_window_plan(const te_clay *c, const te_decode_object *objs, const uint8_t *h_meta, size_t nobj,
                          size_t window_bytes, size_t *cuts, size_t cap, size_t *nwindows);
/* Batched Slicer::decode HOST -> HOST: te_decode_batch_device's meaning for slices in host memory.
 * Only the slices named in avail_mask are read from h_slices and uploaded (absent slots may be
 * unmapped); exactly blob_len bytes are written per object at h_out + out_off.  The windows of
 * te_decode_window_plan run over three streams, so the H2D copy of window w+1, the kernels of w
 * and the D2H copy of w-1 overlap.  h_slices / h_out should be pinned (te_host_alloc /
 * te_host_register) for full PCIe rate.  Every object is validated before anything is enqueued.
 * Synchronous. */
int te_decode_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices, const te_decode_object *objs,
                         const uint8_t *h_meta, size_t nobj, uint8_t *h_out, size_t window_bytes);
/* The gateway's object read (decode.rs:121-139) HOST -> HOST, with te_decode_verified_batch_device's
 * contract: every present slice is checked against h_leaves (nobj * n * 32 bytes),
 * h_rejected_mask[o] (or NULL) = the present slices that failed, an object with at least k verified
 * slices decodes from them (h_status[o] = TE_OK), any other gets TE_ERR_NOT_ENOUGH_SLICES and
 * nothing is written to its output range.  h_status: nobj ints, required.  Any slice_len.
 * The leaf hashes follow te_set_commit_hashing, per window:
 *   TE_HASH_HOST    the host pool hashes the slices in the caller's buffer before the upload; only
 *                   the verified slices of objects that decode are uploaded, and the host never
 *                   waits for the device inside the pipeline;
 *   TE_HASH_DEVICE  every present slice is uploaded and hashed by the leaf-verify kernel; the host
 *                   waits once per window for the masks, after it has enqueued the upload of the
 *                   next window (a window with a slice_len that is no multiple of 4 is hashed on
 *                   the host);
 *   TE_HASH_AUTO    whichever the stream writer's rule picks for the window's slice count and
 *                   lengths.
 * Outputs, masks and statuses are identical in every mode.  Synchronous. */
int te_decode_verified_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices,
                                  const te_decode_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                  size_t nobj, uint8_t *h_out, uint32_t *h_rejected_mask, int *h_status,
                                  size_t window_bytes);
/* Ordered, asynchronous window submission for reads: the counterpart of te_stream_writer_*.
 *   te_stream_reader_new: over ncoders device-bound handles; window t goes to handle
 *     (t - 1) mod ncoders.  The reader owns its device buffers and a host thread per handle, and
 *     runs on the handles' own streams; the handles must outlive it and must not be re-bound
 *     meanwhile.  It copies the process's te_set_commit_hashing mode.
 *   te_stream_read_submit: validate one window (every object, as the batch calls do) and enqueue
 *     it in verified form (h_leaves == NULL: unverified, h_status may then be NULL too); returns
 *     its ticket (1, 2, ... in submission order) without waiting for the device.  A window that
 *     fails validation gets no ticket.  objs, h_meta and h_leaves are copied; h_slices, h_out,
 *     h_rejected_mask and h_status must stay valid until the ticket has been waited for.  A
 *     handle's windows are pipelined as the batch call's are.
 *   te_stream_read_wait: complete every window up to `ticket`, in submission order; returns the
 *     first failure among them (TE_OK if none).  A window's h_out, h_status and h_rejected_mask are
 *     final once its ticket has been waited for.
 *   te_stream_reader_free: waits for every window, then frees the reader. */
typedef struct te_stream_reader te_stream_reader;
int te_stream_reader_new(te_clay *const *coders, size_t ncoders, const te_slicer_cfg *cfg, te_stream_reader **out);
int te_stream_read_submit(te_stream_reader *r, const uint8_t *h_slices, const te_decode_object *objs,
                          const uint8_t *h_meta, const uint8_t *h_leaves, size_t nobj, uint8_t *h_out,
                          uint32_t *h_rejected_mask, int *h_status, uint64_t *ticket);
int te_stream_read_wait(te_stream_reader *r, uint64_t ticket);
void te_stream_reader_free(te_stream_reader *r);
/* The handle's last te_decode_batch_host / te_decode_verified_batch_host call (zeroed when the call
 * has passed its argument checks), or the windows of the stream reader on the handle (zeroed by
 * te_stream_reader_new, summed over its windows as they are enqueued).  Diagnostics; all zero
 * before the first such call. */
typedef struct te_read_launch_stats {
    uint64_t windows;               /* pipeline windows */
    uint64_t objects;               /* objects of those windows */
    uint64_t slices_uploaded;       /* slices copied to the device */
    uint64_t bytes_h2d;             /* their bytes (descriptors and leaves not counted) */
    uint64_t bytes_d2h;             /* object bytes copied back: the blob_len of every decoded object */
    uint64_t slices_hashed_host;    /* leaf hashes by the host pool */
    uint64_t slices_hashed_device;  /* leaf hashes by the leaf-verify kernel */
    uint64_t host_waits;            /* times the host waited for the device inside the pipeline: one
                                       per device-hashed window; the final wait for the last windows'
                                       copies is not counted */
} te_read_launch_stats;
int te_clay_read_launch_stats(te_clay *c, te_read_launch_stats *out);

/* ------------------------------------------------------------------------------------------
 * Node rebuild pipeline: the node side's host boundary.  A node that has lost a spool drains
 * `pending_repairs` in batches of `repair_batch` tracks (network/node/src/features/spool/
 * repair.rs:94-226), each helper's fragment arriving as one host buffer; tracks that escalate
 * fetch k full peer slices and `reconstruct` (recover.rs:77-244, 411-442); both end in
 * verify_slice(position, rebuilt) (repair.rs:340, recover.rs:216) and put_slice.  All pointers
 * below are HOST pointers; offsets in `objs` are relative to the call's base pointers.
 * ------------------------------------------------------------------------------------------ */
/* Host only: the windows the rebuild pipeline cuts a batch into, in the shape of
 * te_decode_window_plan (cuts, cap, *nwindows, cuts == NULL = count only,
 * TE_ERR_BUFFER_TOO_SMALL).  Cutting is greedy, in object order, at most window_bytes per window
 * (0 = 128 MiB); an object above the limit gets a window alone.  A repair object (repair.rs:94-226)
 * counts as the sum of te_extract_repair_data_size(plan, h) over its plan's helpers in, plus
 * num_stripes * chunk_size + 48 out; a NULL plan is TE_ERR_INVALID_ARG. */
int te_repair_window_plan(const te_clay *c, const te_repair_object *objs, size_t nobj, size_t window_bytes,
                          size_t *cuts, size_t cap, size_t *nwindows);
/* The same for recover objects (recover.rs:77-244): popcount(avail_mask) * slice_len in, plus
 * slice_len out. */
int te_recover_window_plan(const te_clay *c, const te_recover_object *objs, size_t nobj, size_t window_bytes,
                           size_t *cuts, size_t cap, size_t *nwindows);
/* The repair loop's batch (repair.rs:94-226, verify_slice at repair.rs:340) HOST -> HOST:
 * te_repair_batch_device's meaning with helper_off / out_off as offsets into h_helpers / h_out.
 * Only the fragments of the helpers a plan names are read and uploaded (packed; the other entries of
 * helper_off are ignored).  h_leaves: nobj * n * 32 bytes, or NULL for the unverified form (h_ok may
 * then be NULL).  Verified: h_ok[o] = 1 if hash_leaf(repaired) == leaves[plan.lost], else 0; the
 * repaired bytes are written either way and the caller escalates an object whose h_ok is 0.  The
 * unverified form does not write h_ok.  Every object is validated before anything is enqueued and
 * before the call looks for a device: te_repair_batch_device's checks (a NULL plan or a plan of
 * another profile: TE_ERR_INVALID_ARG), and here up front what that call finds while it enqueues: a
 * named helper whose helper_off is UINT64_MAX is TE_ERR_MISSING_HELPER.  The windows of
 * te_repair_window_plan run over the handle's three pipeline streams.  The leaf hashes follow
 * te_set_commit_hashing per window, as te_decode_verified_batch_host's do: TE_HASH_HOST hashes the
 * repaired slices on the host pool after their D2H copy has landed, TE_HASH_DEVICE with the
 * leaf-verify kernel before it (a window with a repaired length or an out_off that is no multiple
 * of 4 is hashed on the host).  Results are identical in every mode.  Pageable buffers go through
 * page-locked staging; pinned ones (te_host_alloc / te_host_register) are copied directly.  Each of
 * h_helpers and h_out is of one kind throughout: the call asks once per buffer (h_helpers and h_out
 * themselves; te_recover_batch_host: the first present slice of h_slices, and h_out).
 * Synchronous. */
int te_repair_batch_host(te_clay *c, const uint8_t *h_helpers, const te_repair_object *objs, const uint8_t *h_leaves,
                         size_t nobj, uint8_t *h_out, uint32_t *h_ok, size_t window_bytes);
/* The escalation's batch (recover.rs:77-244, `reconstruct` recover.rs:411-442, verify_slice at
 * recover.rs:216) HOST -> HOST, with te_recover_verified_batch_device's contract: peer slices that
 * fail their leaf are left out and reported in h_rejected_mask[o]; an object with fewer than k
 * verified slices gets h_status[o] = TE_ERR_NOT_ENOUGH_SLICES, nothing is written to its output
 * range and its h_ok is 0; every other is rebuilt, h_ok[o] = 1 if the rebuilt slice hashes to
 * leaves[lost].  h_leaves == NULL is the unverified form: h_status, h_ok and h_rejected_mask may
 * then be NULL (h_ok and h_rejected_mask are not written; h_status, if given, is TE_OK throughout),
 * and fewer than k present slices is the call's error, as in te_recover_batch_device.
 * Only the slices named in avail_mask are read (absent slots may be unmapped); with host hashing
 * only the verified slices of objects that rebuild are uploaded.  Any slice_len and offsets: a
 * window not aligned to 4 is hashed on the host.  Synchronous. */
int te_recover_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices, const te_recover_object *objs,
                          const uint8_t *h_meta, const uint8_t *h_leaves, size_t nobj, uint8_t *h_out,
                          uint32_t *h_rejected_mask, uint32_t *h_ok, int *h_status, size_t window_bytes);
/* The windows of te_recover_multi_batch_host, in te_recover_window_plan's shape: a multi-slice
 * recover object (recover.rs:77-244 for each of its lost slices, one `reconstruct`
 * recover.rs:411-442, the checks of recover.rs:207-218) counts popcount(avail_mask) * slice_len in
 * plus popcount(lost_mask) * slice_len out.  Host only. */
int te_recover_multi_window_plan(const te_clay *c, const te_recover_multi_object *objs, size_t nobj,
                                 size_t window_bytes, size_t *cuts, size_t cap, size_t *nwindows);
/* A node's multi-spool escalation HOST -> HOST: the L lost slices of each object from one upload of
 * its peers (recover.rs:77-244 L times over: peers checked and the rebuilt slice checked,
 * recover.rs:207-218, around one `reconstruct`, recover.rs:411-442).  te_recover_batch_host's
 * contract and pipeline with te_recover_multi_verified_batch_device's masks: h_rejected_mask[o] the
 * peers that fail their leaf, h_status[o] = TE_ERR_NOT_ENOUGH_SLICES (output range untouched,
 * h_ok_mask[o] = 0) below k verified slices, else h_ok_mask[o] the bits of the lost slices whose
 * rebuilt bytes hash to their leaf.  The j-th set bit of lost_mask lands at
 * h_out + out_off + j * slice_len.  h_leaves == NULL is the unverified form: the mask and status
 * arrays may be NULL and fewer than k present slices is the call's error.  Every object is
 * validated (te_recover_multi_batch_device's checks) before anything is enqueued and before the
 * call looks for a device.  The windows of te_recover_multi_window_plan run over the handle's three
 * pipeline streams; hashing follows te_set_commit_hashing per window (a window with a slice_len,
 * slices_off or out_off that is no multiple of 4 hashes on the host) and the results are identical
 * in every mode.  Pageable or pinned: asked once per buffer, as te_recover_batch_host.  Zeroes and
 * fills te_clay_rebuild_launch_stats (windows, pieces, bytes) and te_clay_recover_multi_launch_stats
 * (summed over the call's windows).  Synchronous. */
int te_recover_multi_batch_host(te_clay *c, const te_slicer_cfg *cfg, const uint8_t *h_slices,
                                const te_recover_multi_object *objs, const uint8_t *h_meta, const uint8_t *h_leaves,
                                size_t nobj, uint8_t *h_out, uint32_t *h_rejected_mask, uint32_t *h_ok_mask,
                                int *h_status, size_t window_bytes);
/* The handle's last te_repair_batch_host / te_recover_batch_host call (repair.rs:94-226,
 * recover.rs:77-244), zeroed when the call has passed its argument checks.  The kernels of the
 * call, summed over its windows, stay in te_clay_repair_launch_stats / te_clay_decode_launch_stats. */
typedef struct te_rebuild_launch_stats {
    uint64_t windows;               /* pipeline windows */
    uint64_t objects;               /* objects of those windows */
    uint64_t pieces_uploaded;       /* repair: helper fragments; recover: peer slices copied to the device */
    uint64_t bytes_h2d;             /* their bytes (descriptors and leaves not counted) */
    uint64_t bytes_d2h;             /* rebuilt slice bytes copied back */
    uint64_t slices_hashed_host;    /* leaf hashes by the host pool (peer and rebuilt slices) */
    uint64_t slices_hashed_device;  /* leaf hashes by the leaf-verify kernel */
    uint64_t host_waits;            /* times the host waited for the device inside the pipeline, as in
                                       te_read_launch_stats: a device-hashed recover window's peer masks,
                                       and a window's results where the host goes on with them (hashing,
                                       masks, the scatter out of staging); the final wait is not counted */
} te_rebuild_launch_stats;
int te_clay_rebuild_launch_stats(te_clay *c, te_rebuild_launch_stats *out);

/* ------------------------------------------------------------------------------------------
 * OuterCoder (lib/slicer/src/outer.rs:19-197): single-level Reed-Solomon over
 * GF(2^16) in the Leopard construction of reed-solomon-simd 3.1.0 (parity unpinned: the crate
 * is not in the container).  n chunks, any k reconstruct; chunks 0..k-1 are the
 * data (systematic), k..n-1 the crate's recovery shards.  Chunk bytes are 64-byte aligned
 * (outer.rs:74-80), at most TE_OUTER_MAX_CHUNK_BYTES.
 * ------------------------------------------------------------------------------------------ */
#define TE_OUTER_MAX_CHUNK_BYTES (4u * 1024u * 1024u)  /* MAX_CHUNK_BYTES  outer.rs:12 */
/* chunk size for `len` data bytes: ceil(len / k) rounded up to 64, 64 for empty data. */
size_t te_outer_chunk_bytes(uint32_t k, size_t len);
/* OuterCoder::encode (outer.rs:70-118): out = n chunks of *chunk_bytes (data zero-padded to
 * k * chunk_bytes, then the n - k recovery chunks, computed on the GPU).  TE_ERR_TOO_MUCH_DATA
 * past the chunk limit; TE_ERR_UNSUPPORTED for shard counts the codec does not support. */
int te_outer_encode(uint32_t k, uint32_t n, const uint8_t *data, size_t len, uint8_t *out, size_t cap,
                    size_t *chunk_bytes);
/* OuterCoder::decode (outer.rs:126-197): chunks[i] for i < n (NULL = missing), all chunk_bytes
 * long; out = the k data chunks (k * chunk_bytes, data padding included).  Missing data chunks
 * are restored on the GPU from k received chunks.  TE_ERR_NOT_ENOUGH_SLICES below k chunks. */
int te_outer_decode(uint32_t k, uint32_t n, const uint8_t *const *chunks, size_t chunk_bytes, uint8_t *out,
                    size_t cap);
/* Batched device form of the encode (DEVICE pointers): `segments` segments, segment g's k
 * original shards at d_in + g*seg_in (shard j at + j*chunk_bytes), its m = n - k recovery shards
 * to d_out + g*seg_out (shard j at + j*chunk_bytes).  Runs on hip_stream and waits for it. */
int te_outer_encode_device(uint32_t k, uint32_t m, const uint8_t *d_in, uint64_t chunk_bytes, uint32_t segments,
                           uint64_t seg_in, uint8_t *d_out, uint64_t seg_out, void *hip_stream);
/* Device form of the decode (outer.rs:126-197) for snapshot reads: d_chunks = n DEVICE pointers
 * (host array; NULL = missing), each chunk_bytes long; d_out = the k data chunks (DEVICE,
 * k * chunk_bytes).  Received data chunks are copied, missing ones restored from the first k
 * received chunks on the GPU.  Enqueued on hip_stream; returns without waiting (the d_chunks
 * array is read before it returns).  The decoding tables are cached per erasure pattern. */
int te_outer_decode_device(uint32_t k, uint32_t n, const uint8_t *const *d_chunks, uint64_t chunk_bytes,
                           uint8_t *d_out, void *hip_stream);
/* The same for `segments` segments in one call (a snapshot read): segment g's chunk i at
 * d_chunks[g * n + i] (host array of DEVICE pointers, NULL = missing), its k data chunks to
 * d_out + g * seg_out.  Segments sharing an erasure pattern share launches (up to 256 shard
 * pointers each).  seg_out >= k * chunk_bytes when segments > 1 (TE_ERR_INVALID_ARG otherwise).
 * Every segment is validated before anything is enqueued.  Enqueued on hip_stream; returns
 * without waiting. */
int te_outer_decode_device_batch(uint32_t k, uint32_t n, const uint8_t *const *d_chunks, uint32_t segments,
                                 uint64_t chunk_bytes, uint8_t *d_out, uint64_t seg_out, void *hip_stream);
/* Which kernels the calling thread's last te_outer_* call launched (diagnostics; host bookkeeping
 * only, no effect on results).  The te_outer_* API has no handle, so the stats are per thread: one
 * te_outer_encode / te_outer_encode_device / te_outer_decode / te_outer_decode_device /
 * te_outer_decode_device_batch call, summed over its launches (a batch decode launches once per
 * erasure pattern and 256 shard pointers).  Filled by the launchers where the kernel instance is
 * picked.  Zeroed when such a call has passed its argument checks and starts its device work (an
 * encode of te_outer_encode counts as that one call); all zero before the first one.  The
 * geometry fields are those of the call's last such launch. */
typedef struct te_outer_launch_stats {
    uint32_t matrix_launches;    /* rs16_matrix_kernel: image <= 80 KiB, k <= 32, rows <= 64 */
    uint32_t matrix_ptr_launches; /* of those, shards by pointer argument (the decode) */
    uint32_t transform_launches; /* rs16_encode_kernel: the FFT encode, work vector in LDS */
    uint32_t low_reg_launches;   /* rs16_encode_low_kernel: low rate, k <= 32, work vector in VGPRs */
    uint32_t decode_launches;    /* rs16_decode_kernel: per-coefficient nibble tables */
    uint32_t matrix_g, matrix_kb; /* 4-row groups (1..16) and input slots (16 / 32) of the instance */
    uint32_t matrix_tail_bytes;  /* entry bytes of an odd G's last group: 2 / 4 / 8 (0: even G, or
                                    the last row on the VALU) */
    uint32_t matrix_tailv;       /* 1: the last row of rows = 8 h + 1 on the VALU */
    uint32_t matrix_grid, matrix_tiles; /* workgroups started, (segment, 512-thread column tile)
                                    pairs they loop over */
    uint32_t transform_high;     /* 1 high rate, 0 low rate */
    uint32_t transform_threads;  /* workgroup size picked for the LDS the shape needs */
    uint32_t transform_c;        /* transform size */
    uint32_t transform_lds;      /* dynamic LDS bytes of the launch */
    uint32_t low_reg_c;          /* transform size of the instance: 1, 2, 4, 8, 16, 32 */
    uint32_t decode_kb;          /* input slots of the instance: 4..32 (k <= 32), 0: any k */
    uint32_t decode_lds;         /* 1: tables staged in LDS (<= 48 KiB), 0: read from L2 */
    uint32_t lut_misses;         /* matrix images / decoding tables built and uploaded by the call */
    uint32_t lut_evictions;      /* least recently used tables it freed to stay within 64 */
    uint64_t matrix_segments, transform_segments, low_reg_segments, decode_segments;
} te_outer_launch_stats;
int te_outer_last_launch_stats(te_outer_launch_stats *out);

/* ------------------------------------------------------------------------------------------
 * Snapshot codec (lib/snapshot/src/{encode,decode,chunk}.rs, network/protocol/src/snapshot.rs:
 * 143-275): the one caller of lib/slicer that runs both coders.  The lz4-compressed log is cut
 * into segments; each segment gets a 4-byte length prefix (pack_segment) and is spread over the n
 * spool groups by OuterCoder(ceil(n / 3), n); each of the n symbols gets an 8-byte ChunkNumber
 * header (SnapshotChunkPayload::pack: the segment index, little endian) and is Clay-encoded by
 * Slicer::clay_default() (rotated, chunk_index 0) and committed (hash_leaf x 20,
 * root_from_leaf_hashes::<5>).  The engine takes and returns the compressed bytes: SnapshotLog,
 * lz4, track records, snapshot_chunk_key and signatures stay with the caller.
 * Chunk t = segment * total_groups + group is the reference's track_number (encode.rs:83) and the
 * order of every per-chunk output.  The handle `c` supplies the inner coder (Clay(20,7,16) for
 * the reference's snapshots; n <= 32).
 * ------------------------------------------------------------------------------------------ */
#define TE_SNAPSHOT_HEADER_SIZE 8    /* SnapshotChunkPayload::HEADER_SIZE  chunk.rs:37 */
#define TE_SNAPSHOT_SEGMENT_HEADER 4 /* SEGMENT_HEADER_SIZE                chunk.rs:63 */
/* snapshot_outer_k (chunk.rs:94-100): ceil(total_groups / 3), 0 for no groups.  Host only. */
uint32_t te_snapshot_outer_k(uint32_t total_groups);
/* snapshot_max_segment_bytes (chunk.rs:103-110): k * TE_OUTER_MAX_CHUNK_BYTES - 4.  Host only. */
uint64_t te_snapshot_max_segment_bytes(uint32_t total_groups);
typedef struct te_snapshot_segment {
    uint64_t start, len;       /* the segment is compressed bytes [start, start + len) */
    uint64_t symbol_bytes;     /* te_outer_chunk_bytes(k, 4 + len): each of its n outer symbols */
    uint64_t payload_len;      /* 8 + symbol_bytes: the Clay input of each of its n chunks */
    te_geometry geom;          /* te_slicer_geometry of a blob of payload_len */
    uint64_t slices_off;       /* its first chunk's slices in the output: chunk (s, g), slice i at
                                  slices_off + (g * n_inner + i) * geom.slice_len */
    /* the two BlobEncoding fields encode_chunk derives from the SYMBOL length, not from the
     * payload the slicer saw (encode.rs:136-146): size, and num_stripes(symbol.len(), stripe_size)
     * with the slicer's stripe size (geom.stripe_size, picked for the payload) */
    uint64_t size, stripe_count;
} te_snapshot_segment;
typedef struct te_snapshot_plan_info {
    uint32_t total_groups, outer_k;
    uint64_t compressed_len, max_segment_bytes;
    uint64_t segments;         /* max(1, ceil(len / max_segment_bytes))   encode.rs:63 */
    uint64_t segment_bytes;    /* max(1, ceil(len / segments))            encode.rs:64 */
    uint64_t chunks;           /* segments * total_groups */
    uint64_t total_slice_bytes; /* the encode's slice output */
} te_snapshot_plan_info;
/* encode_snapshot's cut (encode.rs:62-71).  segs gets plan->segments entries (NULL: the plan
 * only; fewer than that, `cap`, is TE_ERR_BUFFER_TOO_SMALL with *plan set).  compressed_len == 0
 * is one segment with an empty range and a 64-byte symbol.  total_groups == 0 is
 * TE_ERR_INVALID_ARG (NoGroups); a (k, n - k) the GF(2^16) codec does not support is
 * TE_ERR_UNSUPPORTED, as in te_outer_encode_device.  Host only. */
int te_snapshot_plan(const te_clay *c, uint64_t compressed_len, uint32_t total_groups, te_snapshot_plan_info *plan,
                     te_snapshot_segment *segs, size_t cap);

/* Bytes of device scratch te_snapshot_encode_device needs: every chunk's payload (header +
 * symbol), each symbol 64-byte aligned.  0 if the plan fails.  Host only. */
size_t te_snapshot_work_bytes(const te_clay *c, uint64_t compressed_len, uint32_t total_groups);
/* encode_snapshot's compute (encode.rs:62-154) on the device, enqueued on hip_stream; returns
 * without waiting.  d_compressed: `len` bytes at ANY byte address.  Outputs (DEVICE):
 *   d_slices       plan.total_slice_bytes, laid out as te_snapshot_segment.slices_off says;
 *                  4-byte aligned when d_leaf_hashes is given (TE_ERR_INVALID_ARG otherwise);
 *   d_leaf_hashes  chunk t's 20 leaves at (t * n_inner + i) * 32; NULL: no commitments;
 *   d_roots        chunk t's root (tree height TE_SLICE_TREE_HEIGHT) at t * 32; NULL: leaves only;
 *   d_work         te_snapshot_work_bytes of scratch, 64-byte aligned (TE_ERR_INVALID_ARG
 *                  otherwise; work_bytes too small is TE_ERR_BUFFER_TOO_SMALL).
 * Four steps: one pack launch writes every payload's header and the k data payloads of every
 * segment (length prefix, segment bytes, zero padding); the outer recovery symbols are computed
 * straight into their payload slots (one launch per distinct symbol size: only the last segment's
 * can differ; none for total_groups == 1); one batched Clay encode of all segments * n payloads;
 * one commit launch per distinct slice length.  Outer shapes only the transform kernels cover
 * (te_outer_launch_stats) upload their tables per call and wait for the stream once per launch
 * (counted in host_waits); OuterCoder(17, 50) and every shape with k <= 32 whose matrix image
 * fits does not. */
int te_snapshot_encode_device(te_clay *c, const uint8_t *d_compressed, uint64_t len, uint32_t total_groups,
                              uint8_t *d_slices, uint8_t *d_leaf_hashes, uint8_t *d_roots, uint8_t *d_work,
                              size_t work_bytes, void *hip_stream);
/* HOST -> HOST, in windows of whole segments through the slots of te_encode_batch_host's pipeline
 * (three streams): a window's compressed bytes are uploaded, the device form's four steps run on
 * it (its payloads in the slot's input buffer; they never visit the host), its slices and
 * commitments (h_leaf_hashes / h_roots may be NULL as above) are downloaded, and the next window's
 * upload and kernels overlap that download.  A window is as many segments as keep its slices
 * within 128 MiB, at least one; a full segment at 50 groups (~590 MiB of slices, ~210 MiB of
 * payloads) is a window of its own, so the device holds three windows, not the snapshot.  Slot
 * buffers above 256 MiB are released when the call returns.  te_snapshot_launch_stats sums over
 * the windows (pack_launches = windows).  Synchronous; on an error it still waits for the copies
 * it queued.  TE_ERR_BUFFER_TOO_SMALL when cap is below the plan's total_slice_bytes. */
int te_snapshot_encode_host(te_clay *c, const uint8_t *h_compressed, uint64_t len, uint32_t total_groups,
                            uint8_t *h_slices, size_t cap, uint8_t *h_leaf_hashes, uint8_t *h_roots);

/* One fetched chunk track of the snapshot reader (snapshot.rs:143-185): its group and its slices
 * (obj.out_off is ignored).  The segment is learnt from the decoded header only. */
typedef struct te_snapshot_track {
    uint32_t group;
    uint32_t pad_;
    te_decode_object obj;
} te_snapshot_track;
/* Bytes of device scratch te_snapshot_decode_device needs for these tracks (decoded payloads,
 * headers, the outer decode's packed segments).  Host only. */
size_t te_snapshot_decode_work_bytes(const te_clay *c, uint32_t total_groups, const te_snapshot_track *tracks,
                                     const uint8_t *h_meta, size_t ntracks);
/* The snapshot read (decode.rs:63-165) on the device.  h_meta: one 48-byte suffix per track;
 * h_leaves: ntracks * n_inner * 32 bytes (each track's BlobEncoding::leaves), or NULL for the
 * unverified form.  Steps:
 *   1. every track is Clay-decoded (te_decode_batch_device, or te_decode_verified_batch_device with
 *      its h_rejected_mask meaning when h_leaves is given).  A track that cannot decode -- fewer
 *      than k (verified) slices: TE_ERR_NOT_ENOUGH_SLICES; a suffix or layout that does not
 *      validate: that error; a payload shorter than 8 bytes: TE_ERR_INVALID_LAYOUT
 *      (ChunkPayloadTooShort) -- gets that status in h_track_status[t] and is skipped, as the
 *      reader skips a failed track (snapshot.rs:174-176); the outer code absorbs it.
 *   2. the decoded tracks' 8-byte headers are gathered by one kernel and the call WAITS ONCE on
 *      hip_stream to read them (the outer decode takes a host pointer table; the verified form
 *      has waited once before, for its masks).  h_track_segment[t] = the header's chunk number
 *      (UINT64_MAX for a skipped track); symbols are filed under it, whatever the caller expected
 *      (snapshot.rs:167-171).  outer_decode_segments' checks (decode.rs:95-127): no decoded track,
 *      a gap in 0..segment_count, or fewer than outer_k symbols in a segment return
 *      TE_ERR_NOT_ENOUGH_SLICES with the reference's message (NoChunks / MissingChunk /
 *      InsufficientGroups { got, need }; the epoch is the caller's) in te_last_error_detail, which
 *      the call clears once its arguments are checked: a TE_ERR_NOT_ENOUGH_SLICES from step 3
 *      carries no such text.
 *      Symbols of unequal length in a segment or a group >= total_groups are
 *      TE_ERR_INVALID_LAYOUT; a group repeated within a segment keeps its last track.
 *   3. te_outer_decode_device_batch per run of segments with one symbol size.
 *   4. one unpack launch checks every length prefix (4 + len <= k * symbol_bytes) and the total
 *      against out_cap, copies the segment bytes to their byte-aligned places in d_out (nothing
 *      is written when a check fails) and writes d_result[0] = status (TE_OK,
 *      TE_ERR_INVALID_LAYOUT or TE_ERR_BUFFER_TOO_SMALL), d_result[1] = the total length.
 * Steps 3-4 are enqueued and not waited for.  d_work: te_snapshot_decode_work_bytes, 64-byte
 * aligned.  h_track_status (ntracks ints) and h_track_segment (ntracks) are required,
 * h_rejected_mask may be NULL.  d_result: two uint64 (DEVICE). */
int te_snapshot_decode_device(te_clay *c, uint32_t total_groups, const uint8_t *d_slices,
                              const te_snapshot_track *tracks, const uint8_t *h_meta, const uint8_t *h_leaves,
                              size_t ntracks, uint8_t *d_out, uint64_t out_cap, uint8_t *d_work, size_t work_bytes,
                              int *h_track_status, uint32_t *h_rejected_mask, uint64_t *h_track_segment,
                              uint64_t *d_result, void *hip_stream);
/* HOST -> HOST: only the slices named in avail_mask are read from h_slices and uploaded; the
 * device form; d_result and the bytes are read back after the final wait.  *out_len is set on
 * TE_OK and on TE_ERR_BUFFER_TOO_SMALL (the length needed).  Every fetched track (a slot of n
 * slices each), the decoded payloads (about n / outer_k x the compressed length) and the output are
 * on the device at once: the segment of a track is known only after its Clay decode, so the outer
 * decode cannot start before the last track.  Device buffers above 256 MiB are released when the
 * call returns.  Synchronous; on an error it still waits for the copies it queued. */
int te_snapshot_decode_host(te_clay *c, uint32_t total_groups, const uint8_t *h_slices,
                            const te_snapshot_track *tracks, const uint8_t *h_meta, const uint8_t *h_leaves,
                            size_t ntracks, uint8_t *h_out, uint64_t cap, uint64_t *out_len, int *h_track_status,
                            uint32_t *h_rejected_mask, uint64_t *h_track_segment);
/* The handle's last te_snapshot_* encode or decode call (diagnostics; zeroed when the call has
 * passed its argument checks; all zero before the first one).  te_clay_encode_launch_stats /
 * te_clay_decode_launch_stats report the Clay kernels of the same call. */
typedef struct te_snapshot_stats {
    uint64_t segments, chunks;   /* encode: the plan's; decode: segments found, tracks decoded */
    uint64_t clay_objects;       /* payloads handed to the Clay encode / decode */
    uint32_t pack_launches, unpack_launches, header_launches;
    uint32_t outer_launches;     /* rs16 kernel launches (te_outer_launch_stats, summed) */
    uint32_t commit_launches;
    uint32_t host_waits;         /* times the call waited for the device before it returned: 0 for
                                    an encode, 1 for a decode (2 verified); the host forms' final
                                    wait is not counted */
} te_snapshot_stats;
int te_snapshot_launch_stats(te_clay *c, te_snapshot_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* TAPE_EC_H */
