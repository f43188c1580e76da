"""Device-resident batch entry points over torch tensors (the stream-encode / repair-worker seam).

torch is plumbing here: it owns device memory and the HIP stream; the work is enqueued by
libtapeec.so's te_*_batch_device on that stream.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import lib
from .slicer import SLICE_TREE_HEIGHT, ClayCoder, DecodeError, RepairPlan, Slicer, _check


def _stream_ptr(stream) -> C.c_void_p:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _is_desc(objs) -> bool:
    return hasattr(objs, "_length_")  # a prepared ctypes descriptor array


def encode_descs(objs: list[tuple[int, int, int, int]]):
    """Prepared te_object array for encode_batch / encode_batch_host (build once, reuse)."""
    return (_lib.te_object * len(objs))(*[_lib.te_object(*o) for o in objs])


def encode_batch(slicer: Slicer, data, objs, out, stream=None) -> None:
    """objs: (data_off, blob_len, out_off, chunk_index) per object, or encode_descs(...) of them;
    data/out are uint8 cuda tensors."""
    arr = objs if _is_desc(objs) else encode_descs(objs)
    cfg = slicer._cfg()
    r = lib.te_encode_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(data.data_ptr()), arr, len(arr),
                                   C.c_void_p(out.data_ptr()), _stream_ptr(stream))
    _check(r, "encode")


def encode_batch_host(slicer: Slicer, data, objs: list[tuple[int, int, int, int]], out, window_bytes: int = 0) -> None:
    """Host -> host batched encode (te_encode_batch_host): data/out are host buffers (numpy arrays
    or CPU tensors, pinned for full PCIe rate); objs as for encode_batch, offsets into data/out."""
    arr = objs if _is_desc(objs) else encode_descs(objs)
    cfg = slicer._cfg()
    r = lib.te_encode_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(data)), arr, len(arr),
                                 C.c_void_p(_host_ptr(out)), window_bytes)
    _check(r, "encode")


def encode_batch_host_multi(slicers: list[Slicer], data, objs: list[tuple[int, int, int, int]], out,
                            window_bytes: int = 0) -> None:
    """te_encode_batch_host_multi: one host -> host pipeline per handle (typically one handle per
    device, ClayCoder.bind_device), objects split into contiguous ranges; same profile/config."""
    arr = objs if _is_desc(objs) else encode_descs(objs)
    cfg = slicers[0]._cfg()
    hs = (C.c_void_p * len(slicers))(*[s.coder.handle.value for s in slicers])
    r = lib.te_encode_batch_host_multi(hs, len(slicers), C.byref(cfg), C.c_void_p(_host_ptr(data)), arr, len(arr),
                                       C.c_void_p(_host_ptr(out)), window_bytes)
    _check(r, "encode")


def encode_commit_batch_host(slicer: Slicer, data, objs: list[tuple[int, int, int, int]], out, leaf_hashes, roots,
                             proofs=None, height: int = SLICE_TREE_HEIGHT, window_bytes: int = 0) -> None:
    """te_encode_commit_batch_host: BlobEncoder::encode_with_proofs (sdk/src/codec/encoder.rs:220-260)
    over a batch, host -> host: slices to `out` as encode_batch_host, plus per object n leaf hashes
    (`leaf_hashes`, nobj*n*32 bytes), the root (`roots`, nobj*32) and, if `proofs` is given, the n
    proofs of `height` hashes each (nobj*n*height*32).  Host buffers (pinned for PCIe rate)."""
    arr = objs if _is_desc(objs) else encode_descs(objs)
    cfg = slicer._cfg()
    pp = C.c_void_p(_host_ptr(proofs)) if proofs is not None else None
    r = lib.te_encode_commit_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(data)), arr, len(arr),
                                        C.c_void_p(_host_ptr(out)), height, C.c_void_p(_host_ptr(leaf_hashes)),
                                        C.c_void_p(_host_ptr(roots)), pp, window_bytes)
    _check(r, "encode")


def verify_data_work_bytes(slicer: Slicer, objs) -> int:
    """te_verify_data_work_bytes: the device work buffer verify_data_batch needs for `objs`."""
    arr = objs if _is_desc(objs) else encode_descs(objs)
    return int(lib.te_verify_data_work_bytes(slicer.coder.handle, arr, len(arr)))


def verify_data_batch(slicer: Slicer, data, objs, expected_roots, expected_leaves=None, roots=None, ok=None,
                      bad_leaf_mask=None, work=None, height: int = SLICE_TREE_HEIGHT, window_bytes: int = 0,
                      stream=None):
    """verify_track_data's coded branch (sdk/src/track/read.rs:174-185) over a batch: re-encode each
    object, hash its slices and check the root against expected_roots, the slices staying in HBM.
    objs: (data_off, blob_len, out_off, chunk_index) per object (out_off is ignored), or
    encode_descs(...) of them.

    data a cuda tensor: te_verify_data_batch_device -- every buffer a cuda tensor (expected_roots
    nobj*32 uint8; expected_leaves nobj*n*32 uint8 or None; roots nobj*32 uint8 or None; ok nobj int32;
    bad_leaf_mask nobj int64 or None; work uint8, verify_data_work_bytes long), enqueued on the stream,
    returns None.

    data a host buffer (numpy array or CPU tensor, pinned for full PCIe rate):
    te_verify_data_batch_host -- expected_roots / expected_leaves bytes or host arrays; returns
    (ok, roots, bad_leaf_mask): a list of bools, a list of 32-byte roots and a list of ints (None
    without expected_leaves).  Synchronous."""
    arr = objs if _is_desc(objs) else encode_descs(objs)
    cfg = slicer._cfg()
    nobj = len(arr)
    if hasattr(data, "is_cuda") and data.is_cuda:
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
        r = lib.te_verify_data_batch_device(slicer.coder.handle, C.byref(cfg), ptr(data), arr, nobj, height,
                                            ptr(expected_roots), ptr(expected_leaves), ptr(work),
                                            work.numel() if work is not None else 0, ptr(roots), ptr(ok),
                                            ptr(bad_leaf_mask), _stream_ptr(stream))
        _check_verify(r)
        return None
    n = slicer.coder.n()
    xr = bytes(expected_roots)
    if len(xr) != nobj * 32:
        raise ValueError(f"expected_roots: {len(xr)} bytes, expected {nobj} x 32")
    xrb = (C.c_uint8 * max(1, len(xr))).from_buffer_copy(xr or b"\0")
    xlb = _leaf_bytes(expected_leaves, nobj, n) if expected_leaves is not None else None
    rb = (C.c_uint8 * max(1, nobj * 32))()
    okb = (C.c_uint32 * max(1, nobj))()
    mb = (C.c_uint64 * max(1, nobj))() if xlb is not None else None
    r = lib.te_verify_data_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(data)), arr, nobj, height,
                                      xrb, xlb, rb, okb, mb, window_bytes)
    _check_verify(r)
    raw = bytes(rb)
    return ([bool(x) for x in okb[:nobj]], [raw[i * 32:(i + 1) * 32] for i in range(nobj)],
            [int(x) for x in mb[:nobj]] if mb is not None else None)


def _check_verify(r: int) -> None:
    if r == _lib.TE_ERR_MERKLE_TREE_FULL:
        raise ValueError("more slices than a tree of this height has leaves")
    _check(r, "encode")


def verify_data_launch_stats(coder: ClayCoder) -> dict:
    """te_clay_verify_data_launch_stats: objects, windows, groups, launches and PCIe bytes of the
    handle's last data-verify call."""
    st = _lib.te_verify_data_stats()
    _check(lib.te_clay_verify_data_launch_stats(coder.handle, C.byref(st)), "encode")
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


class StreamWriter:
    """te_stream_writer: the stream writer's ordered encode stage (sdk/src/stream/write.rs:332-362,
    FuturesOrdered over chunk encodes) as one GPU pipeline per handle.  submit() enqueues a window --
    te_encode_commit_batch_host's outputs for its objects -- and returns its ticket at once; wait()
    completes every window up to a ticket in submission order.  The window's host buffers (pinned
    for full overlap) are kept referenced here until its ticket has been waited for."""

    def __init__(self, slicers: list[Slicer], height: int = SLICE_TREE_HEIGHT, group_bytes: int = 0,
                 hashing: str = "auto"):
        self._cfg = slicers[0]._cfg()
        self._coders = [s.coder for s in slicers]  # the handles outlive the writer
        hs = (C.c_void_p * len(slicers))(*[s.coder.handle.value for s in slicers])
        h = C.c_void_p()
        _check(lib.te_stream_writer_new(hs, len(slicers), C.byref(self._cfg), height, group_bytes, C.byref(h)),
               "encode")
        self._h = h
        self._keep = {}
        self.set_hashing(hashing)

    def set_hashing(self, mode: str) -> None:
        """Who hashes the leaves (te_stream_writer_set_hashing): "auto" (per window, from its slice
        count and length), "device" (leaf kernel over groups of windows) or "host" (worker pool
        over the host slices as their D2H copies land -- the SDK's 64 MiB chunk shape)."""
        _check(lib.te_stream_writer_set_hashing(self._h, HASHING[mode]), "encode")

    def submit(self, data, objs, out, leaf_hashes, roots, proofs=None) -> int:
        arr = objs if _is_desc(objs) else encode_descs(objs)
        t = C.c_uint64()
        pp = C.c_void_p(_host_ptr(proofs)) if proofs is not None else None
        r = lib.te_stream_submit(self._h, C.c_void_p(_host_ptr(data)), arr, len(arr), C.c_void_p(_host_ptr(out)),
                                 C.c_void_p(_host_ptr(leaf_hashes)), C.c_void_p(_host_ptr(roots)), pp, C.byref(t))
        self._keep[t.value] = (data, arr, out, leaf_hashes, roots, proofs)
        _check(r, "encode")
        return t.value

    def wait(self, ticket: int) -> None:
        r = lib.te_stream_wait(self._h, ticket)
        for t in [t for t in self._keep if t <= ticket]:
            del self._keep[t]
        _check(r, "encode")

    def close(self) -> None:
        if self._h:
            lib.te_stream_writer_free(self._h)
            self._h = None
            self._keep.clear()

    def __del__(self):
        self.close()


HASHING = {"auto": 0, "device": 1, "host": 2}  # TE_HASH_AUTO / _DEVICE / _HOST


def set_commit_hashing(mode: str) -> None:
    """Process default for te_encode_commit_batch_host and new stream writers (te_set_commit_hashing)."""
    _check(lib.te_set_commit_hashing(HASHING[mode]), "encode")


def set_host_hash_threads(threads: int) -> None:
    """Host hashing pool size (te_set_host_hash_threads; 0 = min(16, affinity CPUs))."""
    _check(lib.te_set_host_hash_threads(threads), "encode")


def host_hash_threads() -> int:
    return lib.te_host_hash_threads()


def kernel_timing(enable: bool) -> None:
    """te_kernel_timing: record HIP events around every batch call's kernel launches."""
    _check(lib.te_kernel_timing(1 if enable else 0), "kernel timing")


def kernel_time_ms() -> tuple[float, int]:
    """(summed kernel ms, calls) since the last read (te_kernel_time_ms; synchronises)."""
    ms, n = C.c_double(0), C.c_uint32(0)
    _check(lib.te_kernel_time_ms(C.byref(ms), C.byref(n)), "kernel timing")
    return ms.value, n.value


def host_empty(nbytes: int):
    """A numpy uint8 array in page-locked host memory (te_host_alloc), freed with the array: the
    host buffers of encode_batch_host / StreamWriter.submit copy at full PCIe rate from it."""
    import weakref
    import numpy as np
    p = C.c_void_p()
    _check(lib.te_host_alloc(nbytes, C.byref(p)), "encode")
    raw = (C.c_uint8 * max(1, nbytes)).from_address(p.value)
    weakref.finalize(raw, lib.te_host_free, C.c_void_p(p.value))
    return np.frombuffer(raw, dtype=np.uint8)[:nbytes]


def host_register(arr) -> None:
    """Pin an existing host array in place (te_host_register); undo with host_unregister."""
    _check(lib.te_host_register(C.c_void_p(_host_ptr(arr)), arr.nbytes), "encode")


def host_unregister(arr) -> None:
    _check(lib.te_host_unregister(C.c_void_p(_host_ptr(arr))), "encode")


def _host_ptr(buf) -> int:
    if hasattr(buf, "data_ptr"):
        assert not buf.is_cuda, "host buffer expected"
        return buf.data_ptr()
    return buf.ctypes.data


def decode_descs(objs: list[tuple[int, int, int, int]]):
    """Prepared te_decode_object array for decode_batch (build once, reuse)."""
    return (_lib.te_decode_object * len(objs))(*[_lib.te_decode_object(o[0], o[1], o[2], 0, o[3]) for o in objs])


def decode_batch(slicer: Slicer, slices, objs, metas: bytes, out, stream=None) -> None:
    """objs: (slices_off, slice_len, avail_mask, out_off), or decode_descs(...) of them; metas:
    nobj*48 metadata bytes (host)."""
    arr = objs if _is_desc(objs) else decode_descs(objs)
    cfg = slicer._cfg()
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    r = lib.te_decode_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr, mb,
                                   len(arr), C.c_void_p(out.data_ptr()), _stream_ptr(stream))
    _check(r, "decode")


def _meta_bytes(metas: bytes):
    return (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")


def decode_window_plan(coder: ClayCoder, objs, metas: bytes, window_bytes: int = 0) -> list[int]:
    """te_decode_window_plan: the cuts of the host read pipeline's windows (window w = objects
    [cuts[w], cuts[w+1])); host only."""
    arr = objs if _is_desc(objs) else decode_descs(objs)
    nw = C.c_size_t()
    mb = _meta_bytes(metas)
    _check(lib.te_decode_window_plan(coder.handle, arr, mb, len(arr), window_bytes, None, 0, C.byref(nw)), "decode")
    cuts = (C.c_size_t * (nw.value + 1))()
    _check(lib.te_decode_window_plan(coder.handle, arr, mb, len(arr), window_bytes, cuts, nw.value + 1, C.byref(nw)),
           "decode")
    return [int(x) for x in cuts[:nw.value + 1]] if len(arr) else []


def decode_host(slicer: Slicer, slices, objs, metas: bytes, out, window_bytes: int = 0) -> None:
    """te_decode_batch_host: host -> host batched decode.  slices/out are host buffers (numpy arrays
    or CPU tensors, pinned for full PCIe rate: host_empty); objs / metas as for decode_batch, offsets
    into slices/out.  Only the slices named in each avail_mask are read.  Synchronous."""
    arr = objs if _is_desc(objs) else decode_descs(objs)
    cfg = slicer._cfg()
    r = lib.te_decode_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(slices)), arr,
                                 _meta_bytes(metas), len(arr), C.c_void_p(_host_ptr(out)), window_bytes)
    _check(r, "decode")


def decode_verified_host(slicer: Slicer, slices, objs, metas: bytes, leaves, out, window_bytes: int = 0):
    """te_decode_verified_batch_host: the gateway's object read (decode.rs:121-139) host -> host,
    pipelined in windows.  Arguments as decode_host plus each object's n leaf hashes; returns
    (status, rejected) per object as decode_verified_batch does.  Who hashes follows
    set_commit_hashing.  Synchronous."""
    arr = objs if _is_desc(objs) else decode_descs(objs)
    cfg = slicer._cfg()
    nobj = len(arr)
    lb = _leaf_bytes(leaves, nobj, slicer.coder.n())
    rej = (C.c_uint32 * max(1, nobj))()
    st = (C.c_int * max(1, nobj))()
    r = lib.te_decode_verified_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(slices)), arr,
                                          _meta_bytes(metas), lb, nobj, C.c_void_p(_host_ptr(out)), rej, st,
                                          window_bytes)
    _check(r, "decode")
    return [int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]]


def read_launch_stats(coder: ClayCoder) -> dict:
    """te_clay_read_launch_stats: windows, objects, uploads, bytes, hashing and host waits of the
    handle's last host read call (or of the stream reader's windows on it)."""
    st = _lib.te_read_launch_stats()
    _check(lib.te_clay_read_launch_stats(coder.handle, C.byref(st)), "decode")
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


class StreamReader:
    """te_stream_reader: ordered, asynchronous reads, the counterpart of StreamWriter.  submit()
    enqueues a window (verified against `leaves` if given) and returns its ticket at once; wait()
    completes every window up to a ticket in submission order and returns {ticket: (status,
    rejected)} for the windows it completed.  The window's host buffers are kept referenced here
    until its ticket has been waited for."""

    def __init__(self, slicers: list[Slicer]):
        self._h = None
        self._cfg = slicers[0]._cfg()
        self._coders = [s.coder for s in slicers]  # the handles outlive the reader
        hs = (C.c_void_p * len(slicers))(*[s.coder.handle.value for s in slicers])
        h = C.c_void_p()
        _check(lib.te_stream_reader_new(hs, len(slicers), C.byref(self._cfg), C.byref(h)), "decode")
        self._h = h
        self._keep = {}

    def submit(self, slices, objs, metas: bytes, out, leaves=None) -> int:
        arr = objs if _is_desc(objs) else decode_descs(objs)
        nobj = len(arr)
        lb = _leaf_bytes(leaves, nobj, self._coders[0].n()) if leaves is not None else None
        rej = (C.c_uint32 * max(1, nobj))()
        st = (C.c_int * max(1, nobj))()
        t = C.c_uint64()
        r = lib.te_stream_read_submit(self._h, C.c_void_p(_host_ptr(slices)), arr, _meta_bytes(metas), lb, nobj,
                                      C.c_void_p(_host_ptr(out)), rej, st, C.byref(t))
        _check(r, "decode")
        self._keep[t.value] = (slices, out, rej, st, nobj)
        return t.value

    def wait(self, ticket: int) -> dict:
        r = lib.te_stream_read_wait(self._h, ticket)
        res = {}
        for t in sorted(t for t in self._keep if t <= ticket):
            _, _, rej, st, nobj = self._keep.pop(t)
            res[t] = ([int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]])
        _check(r, "decode")
        return res

    def close(self) -> None:
        if self._h:
            lib.te_stream_reader_free(self._h)
            self._h = None
            self._keep.clear()

    def __del__(self):
        self.close()


def decode_range_descs(objs: list[tuple[int, int, int, int, int, int]]):
    """Prepared te_decode_range_object array for decode_range_batch (build once, reuse)."""
    return (_lib.te_decode_range_object * len(objs))(
        *[_lib.te_decode_range_object(o[0], o[1], o[2], 0, o[3], o[4], o[5]) for o in objs])


def decode_range_batch(slicer: Slicer, slices, objs, metas: bytes, out, stream=None) -> None:
    """te_decode_range_batch_device: bytes [start, start + len) of each object (the gateway's ranged
    reads, one object per chunk_range_plan {skip, take}).  objs: (slices_off, slice_len, avail_mask,
    out_off, start, len), or decode_range_descs(...) of them; exactly len bytes land at out_off.
    metas: nobj*48 metadata bytes (host)."""
    arr = objs if _is_desc(objs) else decode_range_descs(objs)
    cfg = slicer._cfg()
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    r = lib.te_decode_range_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr, mb,
                                         len(arr), C.c_void_p(out.data_ptr()), _stream_ptr(stream))
    _check(r, "decode")


def range_launch_stats(coder: ClayCoder) -> dict:
    """te_clay_range_launch_stats: the stripe outcomes of the handle's last ranged call."""
    st = _lib.te_range_launch_stats()
    _check(lib.te_clay_range_launch_stats(coder.handle, C.byref(st)), "decode")
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


def set_range_chunk_path(coder: ClayCoder, on: bool) -> None:
    """te_clay_set_range_chunk_path: ranged reads rebuild a window's lone erased data chunk on the
    windowed recover class kernels (TE_RANGE_CHUNK) instead of decoding the stripe.  Off by default."""
    _check(lib.te_clay_set_range_chunk_path(coder.handle, 1 if on else 0), "decode")


def range_chunk_path(coder: ClayCoder) -> bool:
    """te_clay_range_chunk_path: the handle's knob."""
    return bool(lib.te_clay_range_chunk_path(coder.handle))


def range_chunk_launch_stats(coder: ClayCoder) -> dict:
    """te_clay_range_chunk_launch_stats: the chunk path's share of the handle's last ranged call --
    stripes rebuilt, their gather jobs, bytes the windowed recover jobs stored (zero with the knob off)."""
    st = _lib.te_range_chunk_stats()
    _check(lib.te_clay_range_chunk_launch_stats(coder.handle, C.byref(st)), "decode")
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


def recover_batch(slicer: Slicer, slices, objs: list[tuple[int, int, int, int, int]], metas: bytes, out,
                  stream=None) -> None:
    """Node recover (recover.rs:411-442 `reconstruct`) on the device: objs are (slices_off,
    slice_len, avail_mask, lost, out_off); metas nobj*48 metadata bytes (host)."""
    arr = (_lib.te_recover_object * len(objs))(*[_lib.te_recover_object(*o) for o in objs])
    cfg = slicer._cfg()
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    r = lib.te_recover_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr, mb,
                                    len(arr), C.c_void_p(out.data_ptr()), _stream_ptr(stream))
    _check(r, "recover")


def recover_multi_batch(slicer: Slicer, slices, objs: list[tuple[int, int, int, int, int]], metas: bytes, out,
                        stream=None) -> None:
    """te_recover_multi_batch_device: several lost slices of each object from one decode.  objs are
    (slices_off, slice_len, avail_mask, lost_mask, out_off); the j-th set bit of lost_mask is rebuilt
    at out + out_off + j*slice_len.  metas as for recover_batch."""
    arr = (_lib.te_recover_multi_object * max(1, len(objs)))(*[_lib.te_recover_multi_object(*o) for o in objs])
    cfg = slicer._cfg()
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    r = lib.te_recover_multi_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr, mb,
                                          len(objs), C.c_void_p(out.data_ptr()), _stream_ptr(stream))
    _check(r, "recover")


def recover_multi_launch_stats(coder: ClayCoder) -> dict:
    """te_clay_recover_multi_launch_stats: the handle's last multi-slice recover -- launches of the
    multi-output kernel, the most passes a stripe took, its jobs and stored rows, stripes and split
    stripes, and the objects sent to the single-slice, generic and multi-output paths."""
    st = _lib.te_recover_multi_stats()
    _check(lib.te_clay_recover_multi_launch_stats(coder.handle, C.byref(st)), "recover")
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


def _leaf_bytes(leaves, nobj: int, n: int):
    """nobj * n * 32 bytes of leaves (bytes, or a list per object of n 32-byte hashes) as a ctypes array."""
    b = bytes(leaves) if isinstance(leaves, (bytes, bytearray, memoryview)) else \
        b"".join(bytes(h) for obj in leaves for h in obj)
    if len(b) != nobj * n * 32:
        raise ValueError(f"leaves: {len(b)} bytes, expected {nobj} x {n} x 32")
    return (C.c_uint8 * max(1, len(b))).from_buffer_copy(b or b"\0")


def decode_verified_batch(slicer: Slicer, slices, objs, metas: bytes, leaves, out, stream=None):
    """te_decode_verified_batch_device: the gateway's object read (decode.rs:121-139) over a batch.
    objs / metas as for decode_batch; leaves: each object's n leaf hashes (BlobEncoding::leaves).
    A slice enters the decode only if hash_leaf(slice) == leaves[position].  Returns (status,
    rejected): per object TE_OK or TE_ERR_NOT_ENOUGH_SLICES (its output range is then untouched),
    and the mask of present slices that failed.  Waits once on the stream for the verify kernel; the
    decode is enqueued."""
    arr = objs if _is_desc(objs) else decode_descs(objs)
    cfg = slicer._cfg()
    nobj = len(arr)
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    lb = _leaf_bytes(leaves, nobj, slicer.coder.n())
    rej = (C.c_uint32 * max(1, nobj))()
    st = (C.c_int * max(1, nobj))()
    r = lib.te_decode_verified_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr, mb,
                                            lb, nobj, C.c_void_p(out.data_ptr()), rej, st, _stream_ptr(stream))
    _check(r, "decode")
    return [int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]]


def recover_verified_batch(slicer: Slicer, slices, objs: list[tuple[int, int, int, int, int]], metas: bytes, leaves,
                           out, stream=None):
    """te_recover_verified_batch_device: node recover with both checks of recover.rs:207-218 --
    peers verified before the rebuild, the rebuilt slice against leaves[lost] after.  objs as for
    recover_batch.  Returns (status, rejected, ok) per object; the rebuilt bytes are written whether
    ok or not.  Waits for the results."""
    arr = (_lib.te_recover_object * max(1, len(objs)))(*[_lib.te_recover_object(*o) for o in objs])
    cfg = slicer._cfg()
    nobj = len(objs)
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    lb = _leaf_bytes(leaves, nobj, slicer.coder.n())
    rej = (C.c_uint32 * max(1, nobj))()
    ok = (C.c_uint32 * max(1, nobj))()
    st = (C.c_int * max(1, nobj))()
    r = lib.te_recover_verified_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr, mb,
                                             lb, nobj, C.c_void_p(out.data_ptr()), rej, ok, st, _stream_ptr(stream))
    _check(r, "recover")
    return [int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]], [int(x) for x in ok[:nobj]]


def recover_multi_descs(objs: list[tuple[int, int, int, int, int]]):
    """Prepared te_recover_multi_object array: (slices_off, slice_len, avail_mask, lost_mask, out_off) each."""
    return (_lib.te_recover_multi_object * max(1, len(objs)))(*[_lib.te_recover_multi_object(*o) for o in objs])


def recover_multi_verified_batch(slicer: Slicer, slices, objs: list[tuple[int, int, int, int, int]], metas: bytes,
                                 leaves, out, stream=None):
    """te_recover_multi_verified_batch_device: recover_multi_batch with both checks of
    recover.rs:207-218 -- the peers verified before the rebuild, every rebuilt slice against its leaf
    after.  objs as for recover_multi_batch.  Returns (status, rejected, ok_mask) per object: ok_mask
    has the bit of each lost slice whose rebuilt bytes match (0 for an object that was not rebuilt);
    the bytes are written either way.  Waits for the results."""
    nobj = len(objs)
    arr = objs if _is_desc(objs) else recover_multi_descs(objs)
    cfg = slicer._cfg()
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas if metas else b"\0")
    lb = _leaf_bytes(leaves, nobj, slicer.coder.n())
    rej = (C.c_uint32 * max(1, nobj))()
    ok = (C.c_uint32 * max(1, nobj))()
    st = (C.c_int * max(1, nobj))()
    r = lib.te_recover_multi_verified_batch_device(slicer.coder.handle, C.byref(cfg), C.c_void_p(slices.data_ptr()), arr,
                                                   mb, lb, nobj, C.c_void_p(out.data_ptr()), rej, ok, st,
                                                   _stream_ptr(stream))
    _check(r, "recover")
    return [int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]], [int(x) for x in ok[:nobj]]


def reconstruct(slicer: Slicer, lost: int, peer_slices: list[tuple[int, bytes]]) -> bytes:
    """recover.rs:411-442 `reconstruct`: decode the peers' slices, re-encode, return slice `lost`
    (one object, host bytes in and out, through recover_batch)."""
    import torch
    if not peer_slices:
        raise ValueError("no peer slices provided")
    slen = len(peer_slices[0][1])
    n = slicer.coder.n()
    if not 0 <= lost < n:
        raise ValueError(f"lost slice {lost} out of range")
    host = bytearray(n * slen)
    mask = 0
    for i, d in peer_slices:
        # validate_layout (slicer.rs:79-105): every slice the same length, indices in range, once
        if not 0 <= i < n or mask >> i & 1:
            raise DecodeError("InvalidLayout")
        if len(d) != slen:
            raise DecodeError("InvalidLayout")
        host[i * slen:(i + 1) * slen] = d
        mask |= 1 << i
    dev = torch.frombuffer(host, dtype=torch.uint8).cuda()
    out = torch.empty(slen, dtype=torch.uint8, device="cuda")
    recover_batch(slicer, dev, [(0, slen, mask, lost, 0)], bytes(peer_slices[0][1][-48:]), out)
    torch.cuda.synchronize()
    return out.cpu().numpy().tobytes()


def repair_descs(objs: list[tuple[RepairPlan, dict[int, int], int, bytes]]):
    """Prepared te_repair_object array for repair_batch (build once, reuse; the plans must stay
    alive while it is used)."""
    arr = (_lib.te_repair_object * len(objs))()
    for i, (plan, offs, out_off, meta) in enumerate(objs):
        arr[i].plan = plan.handle.value if hasattr(plan.handle, "value") else plan.handle
        for s in range(20):
            arr[i].helper_off[s] = offs.get(s, 0xFFFFFFFFFFFFFFFF)
        arr[i].out_off = out_off
        for j, b in enumerate(meta):
            arr[i].metadata[j] = b
    return arr


def repair_batch(coder: ClayCoder, helpers, objs, out, stream=None) -> None:
    """objs: (plan, {helper_slice: offset in helpers tensor}, out_off, metadata48) per object, or
    repair_descs(...) of them."""
    arr = objs if _is_desc(objs) else repair_descs(objs)
    r = lib.te_repair_batch_device(coder.handle, C.c_void_p(helpers.data_ptr()), arr, len(arr),
                                   C.c_void_p(out.data_ptr()), _stream_ptr(stream))
    _check(r, "repair")


def repair_verified_batch(coder: ClayCoder, helpers, objs, leaves, out, stream=None) -> list[int]:
    """te_repair_verified_batch_device: repair_batch, then the repaired slice against
    leaves[plan.lost] on the device (repair.rs:339-341).  Returns ok per object; the repaired bytes
    are written either way.  Waits for the results."""
    arr = objs if _is_desc(objs) else repair_descs(objs)
    nobj = len(arr)
    lb = _leaf_bytes(leaves, nobj, coder.n())
    ok = (C.c_uint32 * max(1, nobj))()
    r = lib.te_repair_verified_batch_device(coder.handle, C.c_void_p(helpers.data_ptr()), arr, lb, nobj,
                                            C.c_void_p(out.data_ptr()), ok, _stream_ptr(stream))
    _check(r, "repair")
    return [int(x) for x in ok[:nobj]]


def recover_descs(objs: list[tuple[int, int, int, int, int]]):
    """Prepared te_recover_object array: (slices_off, slice_len, avail_mask, lost, out_off) each."""
    return (_lib.te_recover_object * max(1, len(objs)))(*[_lib.te_recover_object(*o) for o in objs])


def _window_plan(fn, coder: ClayCoder, arr, nobj: int, window_bytes: int, what: str) -> list[int]:
    nw = C.c_size_t()
    _check(fn(coder.handle, arr, nobj, window_bytes, None, 0, C.byref(nw)), what)
    cuts = (C.c_size_t * (nw.value + 1))()
    _check(fn(coder.handle, arr, nobj, window_bytes, cuts, nw.value + 1, C.byref(nw)), what)
    return [int(x) for x in cuts[:nw.value + 1]] if nobj else []


def repair_window_plan(coder: ClayCoder, objs, window_bytes: int = 0) -> list[int]:
    """te_repair_window_plan: the cuts of repair_host's windows (window w = objects [cuts[w],
    cuts[w+1])); host only.  objs as for repair_batch."""
    arr = objs if _is_desc(objs) else repair_descs(objs)
    return _window_plan(lib.te_repair_window_plan, coder, arr, len(arr), window_bytes, "repair")


def recover_window_plan(coder: ClayCoder, objs, window_bytes: int = 0) -> list[int]:
    """te_recover_window_plan: the cuts of recover_host's windows; host only.  objs as for
    recover_batch."""
    nobj = len(objs)
    arr = objs if _is_desc(objs) else recover_descs(objs)
    return _window_plan(lib.te_recover_window_plan, coder, arr, nobj, window_bytes, "recover")


def repair_host(coder: ClayCoder, helpers, objs, out, leaves=None, window_bytes: int = 0):
    """te_repair_batch_host: the node's repair loop (repair.rs:94-226) host -> host, pipelined in
    windows.  helpers/out are host buffers (numpy arrays or CPU tensors; pinned ones, host_empty,
    are copied directly); objs as for repair_batch with offsets into them.  With leaves (each
    object's n leaf hashes) returns ok per object (repair.rs:340), else None; the repaired bytes are
    written either way.  Who hashes follows set_commit_hashing.  Synchronous."""
    arr = objs if _is_desc(objs) else repair_descs(objs)
    nobj = len(arr)
    lb = _leaf_bytes(leaves, nobj, coder.n()) if leaves is not None else None
    ok = (C.c_uint32 * max(1, nobj))() if leaves is not None else None
    r = lib.te_repair_batch_host(coder.handle, C.c_void_p(_host_ptr(helpers)), arr, lb, nobj,
                                 C.c_void_p(_host_ptr(out)), ok, window_bytes)
    _check(r, "repair")
    return [int(x) for x in ok[:nobj]] if ok is not None else None


def recover_host(slicer: Slicer, slices, objs, metas: bytes, out, leaves=None, window_bytes: int = 0):
    """te_recover_batch_host: the escalation (recover.rs:77-244) host -> host, pipelined in windows.
    objs / metas as for recover_batch with offsets into the host buffers slices/out; only the slices
    named in each avail_mask are read.  With leaves returns (status, rejected, ok) per object as
    recover_verified_batch does, else None.  Synchronous."""
    nobj = len(objs)
    arr = objs if _is_desc(objs) else recover_descs(objs)
    cfg = slicer._cfg()
    verified = leaves is not None
    lb = _leaf_bytes(leaves, nobj, slicer.coder.n()) if verified else None
    rej = (C.c_uint32 * max(1, nobj))() if verified else None
    ok = (C.c_uint32 * max(1, nobj))() if verified else None
    st = (C.c_int * max(1, nobj))() if verified else None
    r = lib.te_recover_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(slices)), arr,
                                  _meta_bytes(metas), lb, nobj, C.c_void_p(_host_ptr(out)), rej, ok, st, window_bytes)
    _check(r, "recover")
    if not verified:
        return None
    return [int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]], [int(x) for x in ok[:nobj]]


def recover_multi_window_plan(coder: ClayCoder, objs, window_bytes: int = 0) -> list[int]:
    """te_recover_multi_window_plan: the cuts of recover_multi_batch_host's windows; host only.  objs
    as for recover_multi_batch: an object counts its present and its lost slices, a slice length each."""
    nobj = len(objs)
    arr = objs if _is_desc(objs) else recover_multi_descs(objs)
    return _window_plan(lib.te_recover_multi_window_plan, coder, arr, nobj, window_bytes, "recover")


def recover_multi_batch_host(slicer: Slicer, slices, objs, metas: bytes, out, leaves=None, window_bytes: int = 0):
    """te_recover_multi_batch_host: a node's multi-spool escalation (recover.rs:77-244 for every lost
    slice of an object, from one upload of its peers) host -> host, pipelined in windows.  objs /
    metas as for recover_multi_batch with offsets into the host buffers slices/out; only the slices
    named in each avail_mask are read.  With leaves returns (status, rejected, ok_mask) per object as
    recover_multi_verified_batch does, else None.  Synchronous."""
    nobj = len(objs)
    arr = objs if _is_desc(objs) else recover_multi_descs(objs)
    cfg = slicer._cfg()
    verified = leaves is not None
    lb = _leaf_bytes(leaves, nobj, slicer.coder.n()) if verified else None
    rej = (C.c_uint32 * max(1, nobj))() if verified else None
    ok = (C.c_uint32 * max(1, nobj))() if verified else None
    st = (C.c_int * max(1, nobj))() if verified else None
    r = lib.te_recover_multi_batch_host(slicer.coder.handle, C.byref(cfg), C.c_void_p(_host_ptr(slices)), arr,
                                        _meta_bytes(metas), lb, nobj, C.c_void_p(_host_ptr(out)), rej, ok, st,
                                        window_bytes)
    _check(r, "recover")
    if not verified:
        return None
    return [int(x) for x in st[:nobj]], [int(x) for x in rej[:nobj]], [int(x) for x in ok[:nobj]]


def rebuild_launch_stats(coder: ClayCoder) -> dict:
    """te_clay_rebuild_launch_stats: windows, objects, uploads, bytes, hashing and host waits of the
    handle's last repair_host / recover_host call."""
    st = _lib.te_rebuild_launch_stats()
    _check(lib.te_clay_rebuild_launch_stats(coder.handle, C.byref(st)), "repair")
    return {f: int(getattr(st, f)) for f, _ in st._fields_}
