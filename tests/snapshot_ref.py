"""TEST INFRASTRUCTURE ONLY: the snapshot codec as a composition of the existing oracles
(oracle/rs16.py OracleOuter, oracle/oracle.py slicer_encode / slicer_decode, oracle/merkle_oracle.py
commit_slices), put together as lib/snapshot/src/encode.rs:46-154 and decode.rs:63-165 do it.
Nothing here touches libtapeec."""
from __future__ import annotations

from functools import lru_cache

from oracle import merkle_oracle as MO
from oracle import oracle as O
from oracle import rs16

MAX_CHUNK_BYTES = rs16.MAX_CHUNK_BYTES
HEADER_SIZE = 8
SEGMENT_HEADER_SIZE = 4
GROUP_SIZE = 20


@lru_cache(maxsize=None)
def clay():
    return O.OracleClay(20, 7, 16)


def outer_k(total_groups: int) -> int:  # chunk.rs:94-100
    return 0 if total_groups == 0 else -(-total_groups // 3)


def max_segment_bytes(total_groups: int) -> int:  # chunk.rs:103-110
    k = outer_k(total_groups)
    return 0 if k == 0 else k * MAX_CHUNK_BYTES - SEGMENT_HEADER_SIZE


def cut(length: int, total_groups: int) -> list[tuple[int, int]]:
    """encode.rs:62-71: the (start, end) of every segment."""
    mx = max_segment_bytes(total_groups)
    total = max(-(-length // mx), 1)
    size = max(-(-length // total), 1)
    return [(min(i * size, length), min(i * size + size, length)) for i in range(total)]


def pack_segment(seg: bytes) -> bytes:  # chunk.rs:67-72
    return len(seg).to_bytes(4, "little") + bytes(seg)


def unpack_segment(packed: bytes) -> bytes:  # chunk.rs:75-87
    if len(packed) < SEGMENT_HEADER_SIZE:
        raise ValueError("ChunkPayloadTooShort")
    n = int.from_bytes(packed[:4], "little")
    if 4 + n > len(packed):
        raise ValueError("ChunkPayloadTooShort")
    return packed[4:4 + n]


def payload(chunk: int, symbol: bytes) -> bytes:  # SnapshotChunkPayload::pack chunk.rs:39-44
    return chunk.to_bytes(8, "little") + bytes(symbol)


def encode_chunk(chunk: int, symbol: bytes) -> dict:
    """encode.rs:110-154: slices, leaves, commitment and the BlobEncoding fields taken from the
    SYMBOL length (size, stripe_count) with the slicer's stripe size (picked for the payload)."""
    packed = payload(chunk, symbol)
    slices = O.slicer_encode(clay(), packed, rotated=True, chunk_index=0)
    leaves, root, _ = MO.commit_slices(slices)
    stripe = O.pick_stripe_size(len(packed))
    return {"slices": slices, "leaves": leaves, "root": root, "size": len(symbol), "stripe_size": stripe,
            "stripe_count": O.num_stripes(len(symbol), stripe)}


@lru_cache(maxsize=None)
def encode(compressed: bytes, total_groups: int) -> tuple:
    """encode_snapshot's chunks in track_number order (encode.rs:69-104), computed once per input."""
    k = outer_k(total_groups)
    if k == 0:
        raise ValueError("NoGroups")
    outer = rs16.OracleOuter(k, total_groups)
    chunks = []
    for ci, (a, b) in enumerate(cut(len(compressed), total_groups)):
        for g, symbol in enumerate(outer.encode(pack_segment(compressed[a:b]))):
            c = encode_chunk(ci, symbol)
            c.update(group=g, chunk=ci, track_number=ci * total_groups + g)
            chunks.append(c)
    return tuple(chunks)


def decode(tracks: list[tuple[int, dict[int, bytes]]], total_groups: int) -> bytes:
    """snapshot.rs:159-172 + decode.rs:63-165: tracks are (group, {leaf_index: slice}); a track
    whose Clay decode fails is skipped."""
    by_seg: dict[int, list[tuple[int, bytes]]] = {}
    for group, slices in tracks:
        try:
            plain = O.slicer_decode(clay(), slices, rotated=True)
        except ValueError:
            continue
        if len(plain) < HEADER_SIZE:
            continue
        by_seg.setdefault(int.from_bytes(plain[:8], "little"), []).append((group, plain[8:]))
    if not by_seg:
        raise ValueError("NoChunks")
    k = outer_k(total_groups)
    for i in range(max(by_seg) + 1):
        if i not in by_seg:
            raise ValueError(f"MissingChunk {i}")
    out = b""
    for ci in sorted(by_seg):
        if len(by_seg[ci]) < k:
            raise ValueError(f"InsufficientGroups {len(by_seg[ci])}/{k}")
        out += unpack_segment(rs16.OracleOuter(k, total_groups).decode(by_seg[ci]))
    return out
