"""Case tables of tests/test_gpu_snapshot_edges.py: the byte alignments and segment edges of the
snapshot codec's two copy kernels (tape_amd/csrc/snapshot.hip), in plain Python (no device, no
library; the oracles of tests/snapshot_ref.py build the doctored chunks).
tests/test_snapshot_edge_cases.py checks every property claimed here by enumeration.

Pack (snap_pack_kernel): the packed segment is [u32 LE length | bytes | zeros], cut into k data
shards of `symbol` bytes.  Unit u of it is read from the source address `src + 16 u - 4`, so the
source address mod 4 picks the funnel shift and (4 + length) & 15 is where the data ends inside
its last 16-byte unit; load16_unaligned's masked path runs for the unit that holds the end and for
unit 0.  Everything past the end must come out zero whatever follows the data in the source.

Unpack (snap_unpack_kernel): segment i lands at dst_i = out + sum of the lengths before it.  The
kernel works on the absolute 16-byte units that [dst, dst + len) touches and writes the first and
last of them byte by byte: what matters is (dst & 15, len & 15), whether a short segment stays
inside one unit, empty segments, and the prefix scan over more than blockDim.x = 256 segments."""
from functools import lru_cache

import numpy as np

import snapshot_ref as R

# ---- pack -----------------------------------------------------------------------------------------
PACK_GROUPS = (3, 20)  # total_groups: outer k = 1 and k = 7
PACK_SHIFTS = (0, 1, 2, 3)  # source address mod 4


def _pack_ends(k):
    """The values of 4 + length for outer k, shortest list: either side of every data-shard
    boundary, lengths 0..3, and one end per position in the last unit that those leave out."""
    ends = [64 * j + d for j in range(1, k + 1) for d in (-1, 0, 1)] + [4, 5, 6, 7]
    rest = [r for r in range(16) if r not in {e & 15 for e in ends}]
    for i, r in enumerate(rest):  # spread over the shards; 64 k + r has the larger symbol
        j = 1 + i % k if r < 8 else i % (k + 1)
        ends.append(64 * j + r)
    return sorted(ends)


PACK_CASES = [(n, e - 4) for n in PACK_GROUPS for e in _pack_ends(R.outer_k(n))]

TWO_SEG = (3, 4_194_425)  # tests/test_gpu_snapshot.py: segments of 2,097,213 and 2,097,212 bytes
TWO_SEG_SHIFTS = (0, 1, 2, 3)


def poison(count, seed):
    """Nonzero pseudo-random bytes: what surrounds the data in the source tensor."""
    return np.random.default_rng(seed).integers(1, 256, count, dtype=np.uint8).tobytes()


# ---- unpack ---------------------------------------------------------------------------------------
def _circuit():
    """An Eulerian circuit of the graph on Z/16 whose node a has the edges a -> a + r, r = 0..15
    (Hierholzer), as its 256 edge labels, turned so that it starts with node 0's loop r = 0."""
    used = [0] * 16
    stack, out = [(0, None)], []
    while stack:
        a, r_in = stack[-1]
        if used[a] < 16:
            r = (7 * used[a] + 3 * a) % 16  # a fixed order of a's edges, different at each node
            used[a] += 1
            stack.append(((a + r) % 16, r))
        else:
            stack.pop()
            if r_in is not None:
                out.append(r_in)
    out.reverse()
    a = 0
    for i, r in enumerate(out):
        if (a, r) == (0, 0):
            return out[i:] + out[:i]
        a = (a + r) % 16
    raise AssertionError("no loop at node 0")


def euler_lengths(extra):
    """256 + extra values r_i in 0..15.  With a_0 = 0 and a_(i+1) = (a_i + r_i) mod 16, the first
    256 pairs (a_i, r_i) are all different -- every (offset & 15, length & 15) once -- and a_256 = 0
    again, so the `extra` values that follow, the head once more, repeat the head's pairs."""
    c = _circuit()
    return c + [c[i % 256] for i in range(extra)]


_R = euler_lengths(4)
if _R[-1]:
    _R.append(0)  # UNPACK_SMALL ends, as it starts, with an empty segment

UNPACK_SMALL = list(_R)
UNPACK_MIXED = [r + 16 * (1 + i % 3) for i, r in enumerate(_R)]
UNPACK_WIDE = [5, 40_003, 9, 0, 20_000, 1]
UNPACK_LISTS = {"small": UNPACK_SMALL, "mixed": UNPACK_MIXED, "wide": UNPACK_WIDE}
OUT_BASES = (0, 5)  # byte offset of d_out inside its tensor (the tensor is 16-byte aligned)

UNPACK_GROUPS = 3   # total_groups of the doctored snapshots: outer k = 1, one track per segment
FETCHED = range(7)  # the slices of a track that a test fetches


def offsets(lengths, base=0):
    out, at = [], base
    for n in lengths:
        out.append(at)
        at += n
    return out


def symbol_bytes(length, k=1):
    """OuterCoder::chunk_bytes of a packed segment of `length` data bytes."""
    return R.rs16.OracleOuter.chunk_bytes(k, 4 + length)


def unpack_stride(lengths, k=1):
    """snap_decode_layout's packed_stride (tape_amd/csrc/engine.cpp)."""
    return k * max(symbol_bytes(n, k) for n in lengths) + 64


def unpack_gx(lengths, k=1):
    """launch_snap_unpack's workgroups per segment."""
    return min(1024, max(1, -(-(unpack_stride(lengths, k) // 16) // 1024)))


def group_of(i):
    """The group fetched for segment i: the data group, and the first recovery group for every 16th."""
    return 1 if i % 16 == 15 else 0


def parts_of(lengths, seed):
    blob = np.random.default_rng(seed).bytes(sum(lengths))
    return [blob[a:a + n] for a, n in zip(offsets(lengths), lengths)]


def chunk_of(i, packed):
    """The chunk of group group_of(i) of a hand-made segment: header chunk number i over `packed`."""
    g = group_of(i)
    c = R.encode_chunk(i, R.rs16.OracleOuter(1, UNPACK_GROUPS).encode(packed)[g])
    c.update(group=g, chunk=i)
    return c


@lru_cache(maxsize=None)
def unpack_case(name):
    """(parts, chunks) of UNPACK_LISTS[name], computed once."""
    lengths = UNPACK_LISTS[name]
    parts = parts_of(lengths, 0x5EED + len(lengths))
    return parts, tuple(chunk_of(i, R.pack_segment(p)) for i, p in enumerate(parts))


def ref_tracks(chunks):
    """snapshot_ref.decode's view of the chunks: (group, {leaf_index: slice})."""
    return [(c["group"], {i: c["slices"][i] for i in FETCHED}) for c in chunks]


def prefix_past_capacity(part):
    """A packed segment over `part` whose length prefix is one byte more than its symbol holds."""
    cap = symbol_bytes(len(part))
    return (cap - 3).to_bytes(4, "little") + part
