"""ctypes binding of libtapeec.so (include/tape_ec.h).

The library is built in-tree (tape_amd/libtapeec.so, `make -C tape_amd`).  There is no Python or
CPU fallback for any compute entry point: if the shared object is missing, importing this module
raises, and compute calls on a host without a gfx950 device raise `NoDeviceError`.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TAPE_EC_LIB") or os.path.join(_HERE, "libtapeec.so")  # override: an alternate build
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tape_ec.h")

TE_OK = 0
TE_ERR_TOO_MUCH_DATA = 1
TE_ERR_EMPTY_INPUT = 2
TE_ERR_NOT_ENOUGH_SLICES = 3
TE_ERR_BAD_ENCODING = 4
TE_ERR_INVALID_LAYOUT = 5
TE_ERR_NOT_ENOUGH_HELPERS = 6
TE_ERR_INVALID_SLICE = 7
TE_ERR_CLAY = 8
TE_ERR_MISSING_HELPER = 9
TE_ERR_MERKLE_TREE_FULL = 10
TE_ERR_MERKLE_INVALID_PROOF = 11
TE_ERR_MERKLE_INVALID_INDEX = 12
TE_ERR_MERKLE_PROOF_LENGTH = 13
TE_ERR_INVALID_ARG = 20
TE_ERR_NO_DEVICE = 21
TE_ERR_HIP = 22
TE_ERR_UNSUPPORTED = 23
TE_ERR_OUT_OF_MEMORY = 24
TE_ERR_BUFFER_TOO_SMALL = 25
META_SIZE = 48


class te_clay_info(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("n", "k", "m", "d", "q", "t", "nu", "alpha", "beta")]


class te_slice_metadata(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("version", "blob_len", "stripe_size", "encoding", "params", "chunk_index")]


class te_slicer_cfg(C.Structure):
    _fields_ = [("rotated", C.c_int), ("encoding", C.c_uint64), ("params", C.c_uint64), ("chunk_index", C.c_uint64)]


class te_geometry(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("stripe_size", "num_stripes", "chunk_size", "sub_chunk_size", "slice_len")]


class te_repair_plan_info(C.Structure):
    _fields_ = [("lost", C.c_uint32), ("num_stripes", C.c_uint32), ("d", C.c_uint32), ("beta", C.c_uint32),
                ("chunk_size", C.c_uint64), ("sub_chunk_size", C.c_uint64)]


class te_object(C.Structure):
    _fields_ = [("data_off", C.c_uint64), ("blob_len", C.c_uint64), ("out_off", C.c_uint64),
                ("chunk_index", C.c_uint64)]


class te_decode_object(C.Structure):
    _fields_ = [("slices_off", C.c_uint64), ("slice_len", C.c_uint64), ("avail_mask", C.c_uint32),
                ("pad_", C.c_uint32), ("out_off", C.c_uint64)]


class te_decode_range_object(C.Structure):
    _fields_ = [("slices_off", C.c_uint64), ("slice_len", C.c_uint64), ("avail_mask", C.c_uint32),
                ("pad_", C.c_uint32), ("out_off", C.c_uint64), ("start", C.c_uint64), ("len", C.c_uint64)]


class te_range_launch_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("stripes_touched", "stripes_decoded", "stripes_copied", "gather_jobs",
                                          "bytes_staged")]


class te_range_chunk_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("stripes_rebuilt", "gather_jobs", "bytes_stored")]


RANGE_COPY, RANGE_DECODE, RANGE_CHUNK = 0, 1, 2  # TE_RANGE_COPY / TE_RANGE_DECODE / TE_RANGE_CHUNK


class te_recover_object(C.Structure):
    _fields_ = [("slices_off", C.c_uint64), ("slice_len", C.c_uint64), ("avail_mask", C.c_uint32),
                ("lost", C.c_uint32), ("out_off", C.c_uint64)]


class te_recover_multi_object(C.Structure):
    _fields_ = [("slices_off", C.c_uint64), ("slice_len", C.c_uint64), ("avail_mask", C.c_uint32),
                ("lost_mask", C.c_uint32), ("out_off", C.c_uint64)]


class te_recover_multi_stats(C.Structure):
    _fields_ = [("multi_launches", C.c_uint32), ("passes", C.c_uint32)] + \
               [(f, C.c_uint64) for f in ("jobs", "out_rows", "stripes", "split_stripes", "single_objects",
                                          "generic_objects", "multi_objects")]


class te_repair_object(C.Structure):
    _fields_ = [("plan", C.c_void_p), ("helper_off", C.c_uint64 * 20), ("out_off", C.c_uint64),
                ("metadata", C.c_uint8 * 48)]


class te_verify_item(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64), ("expected", C.c_uint32), ("object", C.c_uint32),
                ("bit", C.c_uint32), ("pad_", C.c_uint32)]


DECODE_CLASSES = 24  # TE_DECODE_CLASSES


class te_decode_launch_stats(C.Structure):
    _fields_ = [("class_launches", C.c_uint32 * DECODE_CLASSES), ("class_stripes", C.c_uint64),
                ("class_g", C.c_uint32), ("class_streams", C.c_uint32), ("table_launches", C.c_uint32),
                ("generic_launches", C.c_uint32), ("jit_launches", C.c_uint32), ("direct_out", C.c_uint32),
                ("table_stripes", C.c_uint64), ("generic_stripes", C.c_uint64), ("jit_stripes", C.c_uint64)]


class te_encode_launch_stats(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("dma_launches", "dma_level1_launches", "dma_level2_launches",
                                          "stage_launches", "stage_masked_launches", "stage_g", "stage_wgs",
                                          "generic_launches")] + \
               [(f, C.c_uint64) for f in ("dma_stripes", "stage_stripes", "generic_stripes")]


class te_repair_launch_stats(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("fold_launches", "stage_launches", "generic_launches", "fold_g", "fold_wgs",
                                          "stage_g", "stage_wgs", "pad_")] + \
               [(f, C.c_uint64) for f in ("fold_stripes", "stage_stripes", "generic_stripes")]


class te_read_launch_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("windows", "objects", "slices_uploaded", "bytes_h2d", "bytes_d2h",
                                          "slices_hashed_host", "slices_hashed_device", "host_waits")]


class te_rebuild_launch_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("windows", "objects", "pieces_uploaded", "bytes_h2d", "bytes_d2h",
                                          "slices_hashed_host", "slices_hashed_device", "host_waits")]


class te_outer_launch_stats(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("matrix_launches", "matrix_ptr_launches", "transform_launches",
                                          "low_reg_launches", "decode_launches", "matrix_g", "matrix_kb",
                                          "matrix_tail_bytes", "matrix_tailv", "matrix_grid", "matrix_tiles",
                                          "transform_high", "transform_threads", "transform_c", "transform_lds",
                                          "low_reg_c", "decode_kb", "decode_lds", "lut_misses", "lut_evictions")] + \
               [(f, C.c_uint64) for f in ("matrix_segments", "transform_segments", "low_reg_segments",
                                          "decode_segments")]


class te_snapshot_segment(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("start", "len", "symbol_bytes", "payload_len")] + \
               [("geom", te_geometry)] + [(f, C.c_uint64) for f in ("slices_off", "size", "stripe_count")]


class te_snapshot_plan_info(C.Structure):
    _fields_ = [("total_groups", C.c_uint32), ("outer_k", C.c_uint32)] + \
               [(f, C.c_uint64) for f in ("compressed_len", "max_segment_bytes", "segments", "segment_bytes", "chunks",
                                          "total_slice_bytes")]


class te_snapshot_track(C.Structure):
    _fields_ = [("group", C.c_uint32), ("pad_", C.c_uint32), ("obj", te_decode_object)]


class te_snapshot_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("segments", "chunks", "clay_objects")] + \
               [(f, C.c_uint32) for f in ("pack_launches", "unpack_launches", "header_launches", "outer_launches",
                                          "commit_launches", "host_waits")]


class te_verify_data_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("objects", "windows", "groups", "leaf_launches", "root_check_launches",
                                          "h2d_bytes", "h2d_expected_bytes", "d2h_bytes")]


def build(verbose: bool = False) -> str:
    """Compile libtapeec.so for gfx950 with hipcc (make -C tape_amd)."""
    subprocess.run(["make", "-s", "-C", _HERE], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def _load() -> C.CDLL:
    # torch wheels bundle their own HIP runtime with the same soname (libamdhip64.so.7); whichever
    # loads first serves the process.  Load torch's first so torch tensors/streams and our kernels
    # share one runtime (ours is ABI-compatible with it).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C tape_amd` "
                          "(the engine has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, sz, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int
    u32p, szp, u8p = C.POINTER(u32), C.POINTER(sz), C.c_void_p
    pp = C.POINTER(C.c_void_p)
    sig = {
        "te_strerror": (C.c_char_p, [i]),
        "te_device_count": (i, []),
        "te_set_device": (i, [i]),
        "te_clay_bind_device": (i, [vp, i]),
        "te_clay_device": (i, [vp]),
        "te_clay_set_decode_jit": (i, [vp, i, u64]),
        "te_clay_decode_jit_status": (i, [vp, u32, u32p, u32p, u32p]),
        "te_clay_set_decode_store_cap": (i, [vp, u32]),
        "te_clay_decode_store_stats": (i, [vp, u32p, u32p, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "te_clay_decode_launch_stats": (i, [vp, C.POINTER(te_decode_launch_stats)]),
        "te_clay_encode_launch_stats": (i, [vp, C.POINTER(te_encode_launch_stats)]),
        "te_clay_repair_launch_stats": (i, [vp, C.POINTER(te_repair_launch_stats)]),
        "te_version": (C.c_char_p, []),
        "te_kernel_timing": (C.c_int, [C.c_int]),
        "te_kernel_time_ms": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
        "te_last_error_detail": (C.c_char_p, []),
        "te_clay_new": (i, [u32, u32, u32, C.POINTER(vp)]),
        "te_clay_from_params": (i, [u64, C.POINTER(vp)]),
        "te_clay_free": (None, [vp]),
        "te_clay_get_info": (i, [vp, C.POINTER(te_clay_info)]),
        "te_clay_chunk_size_for": (sz, [vp, sz]),
        "te_clay_track_chunk_size": (sz, [vp, sz, sz]),
        "te_clay_encode": (i, [vp, u8p, sz, u8p, sz, szp]),
        "te_clay_decode": (i, [vp, pp, sz, u8p, sz]),
        "te_clay_plan_repair": (i, [vp, u32, u32p, sz, u32p, u32p]),
        "te_clay_repair": (i, [vp, u32, u32p, pp, sz, sz, u8p]),
        "te_pick_stripe_size": (sz, [sz]),
        "te_num_stripes": (sz, [sz, sz]),
        "te_shard_to_slice": (u32, [i, u32, u32, u32]),
        "te_slice_to_shard": (u32, [i, u32, u32, u32]),
        "te_slice_metadata_to_bytes": (None, [C.POINTER(te_slice_metadata), u8p]),
        "te_slice_metadata_from_slice": (i, [u8p, sz, C.POINTER(te_slice_metadata)]),
        "te_slicer_geometry": (i, [vp, sz, C.POINTER(te_geometry)]),
        "te_slicer_encode": (i, [vp, C.POINTER(te_slicer_cfg), u8p, sz, u8p, sz]),
        "te_slicer_decode": (i, [vp, C.POINTER(te_slicer_cfg), pp, sz, u8p, sz, szp]),
        "te_repair_plan_from_params": (i, [vp, i, u32, u32p, sz, u64, u64, C.POINTER(vp)]),
        "te_repair_plan_from_slice": (i, [vp, i, u32, u32p, sz, u8p, sz, C.POINTER(vp)]),
        "te_repair_plan_free": (None, [vp]),
        "te_repair_plan_get_info": (i, [vp, C.POINTER(te_repair_plan_info)]),
        "te_repair_plan_stripe": (i, [vp, u32, u32p, u32p, u32p, u32p]),
        "te_extract_repair_data_size": (sz, [vp, u32]),
        "te_extract_repair_data": (i, [vp, u8p, sz, u32, u8p, sz, szp]),
        "te_slicer_repair": (i, [vp, vp, pp, szp, u8p, u8p, sz]),
        "te_repair_plan_helper_request": (i, [vp, u32, u32p, u32p, sz, szp]),
        "te_serve_repair_request": (i, [vp, u8p, sz, u32p, u32p, u32p, sz, u8p, sz, szp]),
        "te_encode_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_object), sz, vp, vp]),
        "te_encode_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_object), sz, vp, sz]),
        "te_balance_object_ranges": (i, [C.POINTER(te_object), sz, sz, C.POINTER(sz)]),
        "te_encode_batch_host_multi": (i, [C.POINTER(vp), sz, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_object), sz,
                                           vp, sz]),
        "te_encode_commit_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_object), sz, vp,
                                            C.c_uint32, vp, vp, vp, sz]),
        "te_stream_writer_new": (i, [C.POINTER(vp), sz, C.POINTER(te_slicer_cfg), C.c_uint32, sz, C.POINTER(vp)]),
        "te_stream_submit": (i, [vp, vp, C.POINTER(te_object), sz, vp, vp, vp, vp, C.POINTER(u64)]),
        "te_stream_wait": (i, [vp, u64]),
        "te_stream_writer_free": (None, [vp]),
        "te_stream_writer_set_hashing": (i, [vp, i]),
        "te_set_commit_hashing": (i, [i]),
        "te_set_host_hash_threads": (i, [i]),
        "te_host_hash_threads": (i, []),
        "te_host_sha_extensions": (i, []),
        "te_host_hash_rate": (C.c_double, []),
        "te_host_hash_lanes": (i, []),
        "te_host_alloc": (i, [sz, C.POINTER(vp)]),
        "te_host_free": (None, [vp]),
        "te_host_register": (i, [vp, sz]),
        "te_host_unregister": (i, [vp]),
        "te_decode_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_decode_object), u8p, sz,
                                       vp, vp]),
        "te_slicer_range_plan": (i, [vp, C.POINTER(te_slicer_cfg), u64, u32, u64, u64, C.POINTER(u64), C.POINTER(u64),
                                     u32p, C.POINTER(u64), C.POINTER(u64)]),
        "te_decode_range_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_decode_range_object), u8p,
                                             sz, vp, vp]),
        "te_slicer_decode_range": (i, [vp, C.POINTER(te_slicer_cfg), pp, sz, u64, u64, u8p, sz, szp]),
        "te_clay_range_launch_stats": (i, [vp, C.POINTER(te_range_launch_stats)]),
        "te_slicer_range_plan_ex": (i, [vp, C.POINTER(te_slicer_cfg), u64, u32, u64, u64, i, C.POINTER(u64),
                                        C.POINTER(u64), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]),
        "te_clay_set_range_chunk_path": (i, [vp, i]),
        "te_clay_range_chunk_path": (i, [vp]),
        "te_clay_range_chunk_launch_stats": (i, [vp, C.POINTER(te_range_chunk_stats)]),
        "te_repair_batch_device": (i, [vp, vp, C.POINTER(te_repair_object), sz, vp, vp]),
        "te_recover_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_recover_object), u8p, sz,
                                        vp, vp]),
        "te_recover_multi_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_recover_multi_object), u8p,
                                              sz, vp, vp]),
        "te_slicer_recover_multi": (i, [vp, C.POINTER(te_slicer_cfg), pp, sz, u32, pp]),
        "te_clay_recover_multi_launch_stats": (i, [vp, C.POINTER(te_recover_multi_stats)]),
        "te_hash_leaf": (i, [u8p, sz, u8p]),
        "te_hash_leaves": (i, [u8p, sz, sz, u32, u8p]),
        "te_hash_pair": (i, [u8p, u8p, u8p]),
        "te_empty_subtree_root": (i, [u32, u8p]),
        "te_merkle_root_from_leaf_hashes": (i, [u8p, sz, u32, u8p]),
        "te_merkle_proof_from_leaf_hashes": (i, [u8p, sz, sz, u32, u8p]),
        "te_merkle_verify_leaf_hash": (i, [u8p, u8p, u8p, sz, u64, u32]),
        "te_commit_batch_device": (i, [vp, u64, u64, u32, sz, u32, vp, vp, vp, vp]),
        "te_roots_check_device": (i, [vp, u32, sz, u32, vp, vp, vp, vp, vp, vp]),
        "te_verify_data_work_bytes": (sz, [vp, C.POINTER(te_object), sz]),
        "te_verify_data_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_object), sz, u32, vp, vp,
                                            vp, sz, vp, vp, vp, vp]),
        "te_verify_data_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_object), sz, u32, vp, vp, vp,
                                          vp, vp, sz]),
        "te_slicer_verify_data": (i, [vp, C.POINTER(te_slicer_cfg), u8p, sz, u32, u8p, u8p, C.POINTER(i)]),
        "te_clay_verify_data_launch_stats": (i, [vp, C.POINTER(te_verify_data_stats)]),
        "te_verify_slice": (i, [u8p, u32, u32, u8p, sz]),
        "te_verify_order": (i, [C.POINTER(te_verify_item), sz, u32p]),
        "te_verify_leaves_device": (i, [vp, vp, C.POINTER(te_verify_item), sz, vp, vp, vp, vp, vp]),
        "te_decode_verified_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_decode_object), u8p,
                                                u8p, sz, vp, u32p, C.POINTER(i), vp]),
        "te_recover_verified_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_recover_object), u8p,
                                                 u8p, sz, vp, u32p, u32p, C.POINTER(i), vp]),
        "te_recover_multi_verified_batch_device": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_recover_multi_object),
                                                       u8p, u8p, sz, vp, u32p, u32p, C.POINTER(i), vp]),
        "te_repair_verified_batch_device": (i, [vp, vp, C.POINTER(te_repair_object), u8p, sz, vp, u32p, vp]),
        "te_slicer_decode_verified": (i, [vp, C.POINTER(te_slicer_cfg), pp, sz, u8p, u8p, sz, szp, u32p]),
        "te_decode_window_plan": (i, [vp, C.POINTER(te_decode_object), u8p, sz, sz, szp, sz, szp]),
        "te_decode_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_decode_object), u8p, sz, vp, sz]),
        "te_decode_verified_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_decode_object), u8p, u8p,
                                              sz, vp, u32p, C.POINTER(i), sz]),
        "te_stream_reader_new": (i, [C.POINTER(vp), sz, C.POINTER(te_slicer_cfg), C.POINTER(vp)]),
        "te_stream_read_submit": (i, [vp, vp, C.POINTER(te_decode_object), u8p, u8p, sz, vp, u32p, C.POINTER(i),
                                      C.POINTER(u64)]),
        "te_stream_read_wait": (i, [vp, u64]),
        "te_stream_reader_free": (None, [vp]),
        "te_clay_read_launch_stats": (i, [vp, C.POINTER(te_read_launch_stats)]),
        "te_repair_window_plan": (i, [vp, C.POINTER(te_repair_object), sz, sz, szp, sz, szp]),
        "te_recover_window_plan": (i, [vp, C.POINTER(te_recover_object), sz, sz, szp, sz, szp]),
        "te_repair_batch_host": (i, [vp, vp, C.POINTER(te_repair_object), u8p, sz, vp, u32p, sz]),
        "te_recover_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_recover_object), u8p, u8p, sz, vp,
                                      u32p, u32p, C.POINTER(i), sz]),
        "te_recover_multi_window_plan": (i, [vp, C.POINTER(te_recover_multi_object), sz, sz, szp, sz, szp]),
        "te_recover_multi_batch_host": (i, [vp, C.POINTER(te_slicer_cfg), vp, C.POINTER(te_recover_multi_object), u8p, u8p,
                                            sz, vp, u32p, u32p, C.POINTER(i), sz]),
        "te_clay_rebuild_launch_stats": (i, [vp, C.POINTER(te_rebuild_launch_stats)]),
        "te_outer_chunk_bytes": (sz, [u32, sz]),
        "te_outer_encode": (i, [u32, u32, u8p, sz, u8p, sz, szp]),
        "te_outer_decode": (i, [u32, u32, pp, sz, u8p, sz]),
        "te_outer_encode_device": (i, [u32, u32, vp, u64, u32, u64, vp, u64, vp]),
        "te_outer_decode_device": (i, [u32, u32, pp, u64, vp, vp]),
        "te_outer_decode_device_batch": (i, [u32, u32, pp, u32, u64, vp, u64, vp]),
        "te_outer_last_launch_stats": (i, [C.POINTER(te_outer_launch_stats)]),
        "te_snapshot_outer_k": (u32, [u32]),
        "te_snapshot_max_segment_bytes": (u64, [u32]),
        "te_snapshot_plan": (i, [vp, u64, u32, C.POINTER(te_snapshot_plan_info), C.POINTER(te_snapshot_segment), sz]),
        "te_snapshot_work_bytes": (sz, [vp, u64, u32]),
        "te_snapshot_encode_device": (i, [vp, vp, u64, u32, vp, vp, vp, vp, sz, vp]),
        "te_snapshot_encode_host": (i, [vp, vp, u64, u32, vp, sz, vp, vp]),
        "te_snapshot_decode_work_bytes": (sz, [vp, u32, C.POINTER(te_snapshot_track), u8p, sz]),
        "te_snapshot_decode_device": (i, [vp, u32, vp, C.POINTER(te_snapshot_track), u8p, u8p, sz, vp, u64, vp, sz,
                                          C.POINTER(i), u32p, C.POINTER(u64), vp, vp]),
        "te_snapshot_decode_host": (i, [vp, u32, vp, C.POINTER(te_snapshot_track), u8p, u8p, sz, vp, u64,
                                        C.POINTER(u64), C.POINTER(i), u32p, C.POINTER(u64)]),
        "te_snapshot_launch_stats": (i, [vp, C.POINTER(te_snapshot_stats)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    return L


lib = _load()


def declared_symbols() -> list[str]:
    """Every function the public header declares (te_*( ... ) prototypes)."""
    import re
    txt = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"\b(te_[a-z0-9_]+)\s*\(", txt)))


def strerror(code: int) -> str:
    return lib.te_strerror(code).decode()


def device_count() -> int:
    return int(lib.te_device_count())
