"""Host-only geometry of the snapshot codec (te_snapshot_outer_k, te_snapshot_max_segment_bytes,
te_snapshot_plan; lib/snapshot/src/chunk.rs:94-110, encode.rs:62-71, 136-146) against their
restatement in tests/snapshot_ref.py.  No device."""
import ctypes as C

import pytest

import snapshot_ref as R
from oracle import oracle as O
from oracle import rs16
from tape_amd import _lib, snapshot
from tape_amd._lib import lib
from tape_amd.slicer import ClayCoder, ClayParams

GROUPS = (1, 3, 20, 50)


@pytest.fixture(scope="module")
def coder():
    return ClayCoder.from_params(ClayParams.default())


def c_plan(coder, length, n, cap=None):
    info = _lib.te_snapshot_plan_info()
    r = lib.te_snapshot_plan(coder.handle, length, n, C.byref(info), None, 0)
    if r:
        return r, info, []
    segs = (_lib.te_snapshot_segment * int(info.segments))()
    r = lib.te_snapshot_plan(coder.handle, length, n, C.byref(info), segs, len(segs) if cap is None else cap)
    return r, info, list(segs)


def test_outer_k_table():  # chunk.rs:159-166
    assert [lib.te_snapshot_outer_k(n) for n in (0, 1, 3, 20, 50, 100)] == [0, 1, 1, 7, 17, 34]
    assert [snapshot.snapshot_outer_k(n) for n in (0, 1, 3, 20, 50, 100)] == [0, 1, 1, 7, 17, 34]


def test_max_segment_bytes():  # chunk.rs:103-110
    assert lib.te_snapshot_max_segment_bytes(0) == 0
    for n in (1, 3, 20, 50, 100):
        assert lib.te_snapshot_max_segment_bytes(n) == R.outer_k(n) * rs16.MAX_CHUNK_BYTES - 4 == R.max_segment_bytes(n)
        assert snapshot.snapshot_max_segment_bytes(n) == R.max_segment_bytes(n)


def lengths(n):
    mx = R.max_segment_bytes(n)
    return [0, 1, 59, 60, 61, mx, mx + 1]


@pytest.mark.parametrize("n", GROUPS)
def test_plan(coder, n):
    k = R.outer_k(n)
    for length in lengths(n):
        r, info, segs = c_plan(coder, length, n)
        assert r == 0
        cuts = R.cut(length, n)
        assert info.total_groups == n and info.outer_k == k and info.compressed_len == length
        assert info.segments == len(cuts) == max(1, -(-length // R.max_segment_bytes(n)))
        assert info.segment_bytes == max(1, -(-length // len(cuts)))
        assert info.chunks == len(cuts) * n
        pos = off = 0
        for g, (a, b) in zip(segs, cuts):
            assert (g.start, g.start + g.len) == (a, b) and g.start == pos  # contiguous, in order
            pos = b
            sym = rs16.OracleOuter.chunk_bytes(k, 4 + (b - a))
            assert g.symbol_bytes == sym <= rs16.MAX_CHUNK_BYTES and g.payload_len == 8 + sym
            S, ns, cs, sl = O.geometry(R.clay(), 8 + sym)
            assert (g.geom.stripe_size, g.geom.num_stripes, g.geom.chunk_size, g.geom.slice_len) == (S, ns, cs, sl)
            assert g.size == sym
            assert g.stripe_count == O.num_stripes(sym, O.pick_stripe_size(8 + sym))  # encode.rs:136-137
            assert g.slices_off == off
            off += n * 20 * sl
        assert pos == length and info.total_slice_bytes == off
    # compressed_len == 0: one segment, an empty range, a 64-byte symbol
    r, info, segs = c_plan(coder, 0, n)
    assert (info.segments, segs[0].start, segs[0].len, segs[0].symbol_bytes) == (1, 0, 0, 64)


def test_stripe_count_is_the_symbols(coder):
    """encode_chunk takes stripe_count from num_stripes(symbol.len(), stripe_size) while the slicer
    striped the payload, 8 bytes longer (encode.rs:136-146).  The two differ when the symbol is a
    whole number of stripes: symbols are multiples of 64, so with pick_stripe_size's 100,000-byte
    stripes (payload <= 1,000,000) at 200,000 (2 against 3 stripes), and at 1,000,000, where the
    payload crosses into 1,000,000-byte stripes (1 against 2)."""
    for length, sym, count, payload_count in ((199_996, 200_000, 2, 3), (999_996, 1_000_000, 1, 2)):
        r, info, segs = c_plan(coder, length, 3)  # k = 1: the symbol is the packed segment
        g = segs[0]
        assert r == 0 and g.symbol_bytes == sym
        assert g.stripe_count == count and g.geom.num_stripes == payload_count
        assert g.size == sym and g.payload_len == sym + 8
        ref = R.encode_chunk(0, bytes(sym))
        assert (ref["stripe_count"], ref["size"], ref["stripe_size"]) == (count, sym, g.geom.stripe_size)


def test_two_segments_differ(coder):
    r, info, segs = c_plan(coder, 4_194_425, 3)
    assert r == 0 and info.segments == 2
    assert [(g.len, g.symbol_bytes) for g in segs] == [(2_097_213, 2_097_280), (2_097_212, 2_097_216)]


def test_errors(coder):
    info = _lib.te_snapshot_plan_info()
    assert lib.te_snapshot_plan(coder.handle, 100, 0, C.byref(info), None, 0) == _lib.TE_ERR_INVALID_ARG  # NoGroups
    assert lib.te_snapshot_plan(None, 100, 3, C.byref(info), None, 0) == _lib.TE_ERR_INVALID_ARG
    r, info, _ = c_plan(coder, R.max_segment_bytes(3) + 1, 3, cap=1)  # two segments, room for one
    assert r == _lib.TE_ERR_BUFFER_TOO_SMALL and info.segments == 2
    # a (k, n - k) the GF(2^16) codec cannot take: min(next_pow2(k), next_pow2(m)) + max(k, m) > 65536
    n = 196_605  # k = 65,535, m = 131,070
    assert rs16.use_high_rate(R.outer_k(n), n - R.outer_k(n)) < 0
    assert lib.te_snapshot_plan(coder.handle, 100, n, C.byref(info), None, 0) == _lib.TE_ERR_UNSUPPORTED
    assert lib.te_snapshot_work_bytes(coder.handle, 100, 0) == 0
    with pytest.raises(snapshot.SnapshotError, match="NoGroups"):
        snapshot.plan(100, 0)


@pytest.mark.parametrize("n", GROUPS)
def test_python_mirror_agrees(coder, n):
    for length in lengths(n):
        r, info, segs = c_plan(coder, length, n)
        P = snapshot.plan(length, n, coder)
        for f, _ in info._fields_:
            assert P[f] == getattr(info, f)
        assert len(P["segs"]) == len(segs)
        for d, g in zip(P["segs"], segs):
            for f in ("start", "len", "symbol_bytes", "payload_len", "slices_off", "size", "stripe_count"):
                assert d[f] == getattr(g, f)
            for f, _ in g.geom._fields_:
                assert d[f] == getattr(g.geom, f)


def test_work_bytes(coder):
    """Every payload slot holds its 8-byte header and symbol, the symbol on a 64-byte boundary."""
    for n, length in ((50, 5000), (3, 4_194_425), (1, 1)):
        _, info, segs = c_plan(coder, length, n)
        need = 56 + sum(n * (g.symbol_bytes + 64) for g in segs)
        assert need <= lib.te_snapshot_work_bytes(coder.handle, length, n) <= need + 64
