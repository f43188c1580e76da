"""Snapshot codec (lib/snapshot/src/{encode,decode,chunk}.rs, network/protocol/src/snapshot.rs:
143-275): OuterCoder(ceil(n / 3), n) over length-prefixed segments of the lz4-compressed log, an
8-byte ChunkNumber header per symbol, Slicer::clay_default() and the slice commitments per chunk --
run by libtapeec as one device pipeline (te_snapshot_*).  The engine takes and returns the
compressed bytes; SnapshotLog, lz4, track records and keys stay with the caller."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _lib
from ._lib import lib
from .slicer import ClayCoder, ClayParams, _check, _engine_error

HEADER_SIZE = 8          # SnapshotChunkPayload::HEADER_SIZE  chunk.rs:37
SEGMENT_HEADER_SIZE = 4  # chunk.rs:63
HASH_SIZE = 32
NO_SEGMENT = (1 << 64) - 1


class SnapshotError(Exception):
    """SnapshotError (lib/snapshot/src/lib.rs): NoGroups, NoChunks, MissingChunk, InsufficientGroups,
    ChunkPayload (a length prefix past its segment), OutputTooSmall."""

    def __init__(self, variant: str, detail: str = ""):
        self.variant = variant
        self.detail = detail
        super().__init__(f"{variant}: {detail}" if detail else variant)


_default = None


def _coder(coder: ClayCoder | None) -> ClayCoder:
    global _default
    if coder is not None:
        return coder
    if _default is None:
        _default = ClayCoder.from_params(ClayParams.default())
    return _default


def snapshot_outer_k(total_groups: int) -> int:
    """snapshot_outer_k (chunk.rs:94-100)."""
    return int(lib.te_snapshot_outer_k(total_groups))


def snapshot_max_segment_bytes(total_groups: int) -> int:
    """snapshot_max_segment_bytes (chunk.rs:103-110)."""
    return int(lib.te_snapshot_max_segment_bytes(total_groups))


def _raise_plan(r: int) -> None:
    if r == _lib.TE_ERR_INVALID_ARG:
        raise SnapshotError("NoGroups")
    if r:
        raise _engine_error(r)


def plan(compressed_len: int, total_groups: int, coder: ClayCoder | None = None) -> dict:
    """te_snapshot_plan: encode_snapshot's cut (encode.rs:62-71).  The plan's fields plus
    "segs": one dict per segment (start, len, symbol_bytes, payload_len, the inner geometry,
    slices_off, size, stripe_count).  Works without a device."""
    c = _coder(coder)
    info = _lib.te_snapshot_plan_info()
    _raise_plan(lib.te_snapshot_plan(c.handle, compressed_len, total_groups, C.byref(info), None, 0))
    segs = (_lib.te_snapshot_segment * int(info.segments))()
    _raise_plan(lib.te_snapshot_plan(c.handle, compressed_len, total_groups, C.byref(info), segs, len(segs)))
    out = {f: int(getattr(info, f)) for f, _ in info._fields_}
    out["segs"] = []
    for g in segs:
        d = {f: int(getattr(g, f)) for f, _ in g._fields_ if f != "geom"}
        d.update({f: int(getattr(g.geom, f)) for f, _ in g.geom._fields_})
        out["segs"].append(d)
    return out


@dataclass
class SnapshotChunk:
    """One SnapshotChunk (encode.rs:30-41) without its track record: BlobEncoding's leaves,
    commitment, size and stripe_count, and the 20 slices."""
    group: int
    chunk: int
    leaves: list[bytes]
    root: bytes
    slices: list[bytes]
    size: int
    stripe_size: int
    stripe_count: int
    track_number: int


def encode(compressed: bytes, total_groups: int, coder: ClayCoder | None = None) -> list[SnapshotChunk]:
    """encode_snapshot's compute (encode.rs:62-154) through te_snapshot_encode_host: the chunks in
    track_number order (chunk * total_groups + group)."""
    c = _coder(coder)
    P = plan(len(compressed), total_groups, c)
    ni = c.n()
    nch = P["chunks"]
    out = (C.c_uint8 * max(1, P["total_slice_bytes"]))()
    leaves = (C.c_uint8 * (nch * ni * HASH_SIZE))()
    roots = (C.c_uint8 * (nch * HASH_SIZE))()
    buf = (C.c_uint8 * max(1, len(compressed))).from_buffer_copy(bytes(compressed) or b"\0")
    r = lib.te_snapshot_encode_host(c.handle, buf, len(compressed), total_groups, out, len(out), leaves, roots)
    _check(r, "encode")
    raw, lv, rt = memoryview(out), bytes(leaves), bytes(roots)
    chunks = []
    for s, g in enumerate(P["segs"]):
        sl = g["slice_len"]
        for grp in range(total_groups):
            t = s * total_groups + grp
            base = g["slices_off"] + grp * ni * sl
            chunks.append(SnapshotChunk(
                group=grp, chunk=s,
                leaves=[lv[(t * ni + i) * HASH_SIZE:(t * ni + i + 1) * HASH_SIZE] for i in range(ni)],
                root=rt[t * HASH_SIZE:(t + 1) * HASH_SIZE],
                slices=[bytes(raw[base + i * sl:base + (i + 1) * sl]) for i in range(ni)],
                size=g["size"], stripe_size=g["stripe_size"], stripe_count=g["stripe_count"], track_number=t))
    return chunks


def track_descs(tracks):
    """te_snapshot_track array from (group, slices_off, slice_len, avail_mask) tuples."""
    arr = (_lib.te_snapshot_track * max(1, len(tracks)))()
    for i, (grp, off, sl, mask) in enumerate(tracks):
        arr[i].group = grp
        arr[i].obj = _lib.te_decode_object(off, sl, mask, 0, 0)
    return arr


def _raise_decode(r: int) -> None:
    if r == 0:
        return
    detail = lib.te_last_error_detail().decode()
    if r == _lib.TE_ERR_NOT_ENOUGH_SLICES and ":" in detail and detail.split(":")[0] in (
            "NoChunks", "MissingChunk", "InsufficientGroups"):
        raise SnapshotError(detail.split(":")[0], detail.split(":", 1)[1].strip())
    if r == _lib.TE_ERR_INVALID_ARG:
        raise SnapshotError("NoGroups")
    if r == _lib.TE_ERR_BUFFER_TOO_SMALL:
        raise SnapshotError("OutputTooSmall")
    if r == _lib.TE_ERR_INVALID_LAYOUT:
        raise SnapshotError("ChunkPayload", "invalid layout")
    _check(r, "decode")


def decode(tracks: list[tuple[int, list[tuple[int, bytes]]]], total_groups: int,
           leaves: list[list[bytes]] | None = None, coder: ClayCoder | None = None, max_len: int | None = None,
           report: dict | None = None) -> bytes:
    """The snapshot read (decode.rs:63-165) through te_snapshot_decode_host.  tracks: per fetched
    chunk track its group and its (leaf_index, slice) pairs; leaves: per track its 20 leaf hashes for
    the verified form.  Returns the compressed bytes.  report (a dict) receives "status",
    "rejected" and "segment" per track."""
    c = _coder(coder)
    ni = c.n()
    descs, metas, blob, off = [], [], bytearray(), 0
    for grp, slices in tracks:
        sl = len(slices[0][1]) if slices else 0
        mask = 0
        slot = bytearray(ni * sl)
        for i, d in slices:
            if len(d) != sl or not 0 <= i < ni:
                raise SnapshotError("ClayDecode", "InvalidLayout")
            mask |= 1 << i
            slot[i * sl:(i + 1) * sl] = d
        descs.append((grp, off, sl, mask))
        metas.append(bytes(slices[0][1][-_lib.META_SIZE:]).rjust(_lib.META_SIZE, b"\0") if slices else bytes(_lib.META_SIZE))
        blob += slot
        off += len(slot)
    nt = len(tracks)
    arr = track_descs(descs)
    meta = b"".join(metas) or b"\0"
    lv = None
    if leaves is not None:
        lv = b"".join(b"".join(bytes(h) for h in tl) for tl in leaves) or b"\0"
    if max_len is None:
        max_len = len(blob)
    hbuf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
    out = (C.c_uint8 * max(1, max_len))()
    status = (C.c_int * max(1, nt))()
    rej = (C.c_uint32 * max(1, nt))()
    seg = (C.c_uint64 * max(1, nt))()
    got = C.c_uint64()
    r = lib.te_snapshot_decode_host(c.handle, total_groups, hbuf, arr, meta, lv, nt, out, max_len, C.byref(got), status,
                                    rej, seg)
    if report is not None:
        report["status"] = [int(status[i]) for i in range(nt)]
        report["rejected"] = [int(rej[i]) for i in range(nt)]
        report["segment"] = [int(seg[i]) for i in range(nt)]
        report["code"] = int(r)
    _raise_decode(r)
    return bytes(out)[:got.value]


def _sp(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def work_bytes(compressed_len: int, total_groups: int, coder: ClayCoder | None = None) -> int:
    return int(lib.te_snapshot_work_bytes(_coder(coder).handle, compressed_len, total_groups))


def encode_device(d_compressed, length: int, total_groups: int, d_slices, d_leaf_hashes, d_roots, d_work,
                  coder: ClayCoder | None = None, stream=None, src_offset: int = 0) -> None:
    """te_snapshot_encode_device over uint8 cuda tensors; the compressed bytes start at
    d_compressed[src_offset] (any byte alignment).  Enqueued on the stream."""
    c = _coder(coder)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    r = lib.te_snapshot_encode_device(c.handle, C.c_void_p(d_compressed.data_ptr() + src_offset), length, total_groups,
                                      p(d_slices), p(d_leaf_hashes), p(d_roots), p(d_work), d_work.numel(), _sp(stream))
    _check(r, "encode")


def decode_work_bytes(descs, metas: bytes, total_groups: int, coder: ClayCoder | None = None) -> int:
    arr = descs if hasattr(descs, "_length_") else track_descs(descs)
    n = len(descs)
    return int(lib.te_snapshot_decode_work_bytes(_coder(coder).handle, total_groups, arr, metas or b"\0", n))


def decode_device(d_slices, descs, metas: bytes, total_groups: int, d_out, out_cap: int, d_work, d_result,
                  leaves: bytes | None = None, coder: ClayCoder | None = None, stream=None) -> dict:
    """te_snapshot_decode_device over cuda tensors (d_result: two int64).  descs: (group, slices_off,
    slice_len, avail_mask) per track.  Returns {"code", "status", "rejected", "segment"}; raises
    nothing: d_result carries the unpack's status once the stream has run."""
    c = _coder(coder)
    nt = len(descs)
    arr = track_descs(descs)
    status = (C.c_int * max(1, nt))()
    rej = (C.c_uint32 * max(1, nt))()
    seg = (C.c_uint64 * max(1, nt))()
    r = lib.te_snapshot_decode_device(c.handle, total_groups, C.c_void_p(d_slices.data_ptr()), arr, metas or b"\0", leaves,
                                      nt, C.c_void_p(d_out.data_ptr()), out_cap, C.c_void_p(d_work.data_ptr()),
                                      d_work.numel(), status, rej, seg, C.c_void_p(d_result.data_ptr()), _sp(stream))
    return {"code": int(r), "detail": lib.te_last_error_detail().decode() if r else "",
            "status": [int(status[i]) for i in range(nt)], "rejected": [int(rej[i]) for i in range(nt)],
            "segment": [int(seg[i]) for i in range(nt)]}


def launch_stats(coder: ClayCoder | None = None) -> dict:
    """te_snapshot_launch_stats of the coder's last snapshot call."""
    st = _lib.te_snapshot_stats()
    r = lib.te_snapshot_launch_stats(_coder(coder).handle, C.byref(st))
    if r:
        raise _engine_error(r)
    return {f: int(getattr(st, f)) for f, _ in st._fields_}


__all__ = ["SnapshotError", "SnapshotChunk", "snapshot_outer_k", "snapshot_max_segment_bytes", "plan", "encode", "decode",
           "encode_device", "decode_device", "work_bytes", "decode_work_bytes", "track_descs", "launch_stats",
           "HEADER_SIZE", "SEGMENT_HEADER_SIZE", "NO_SEGMENT"]
