"""The case tables of the snapshot kernels' edge tests (tests/snapshot_edge_cases.py) hold what
their GPU tests rely on, checked by enumeration; and the doctored snapshots built from them decode,
on the reference, to their parts.  No GPU."""
import pytest

import snapshot_edge_cases as E
import snapshot_ref as R

LISTS = sorted(E.UNPACK_LISTS)


def ends(n):
    return [4 + length for g, length in E.PACK_CASES if g == n]


def test_pack_groups_and_shifts():
    assert {n for n, _ in E.PACK_CASES} == {3, 20} == set(E.PACK_GROUPS)
    assert (R.outer_k(3), R.outer_k(20)) == (1, 7)
    assert len(set(E.PACK_CASES)) == len(E.PACK_CASES)
    assert E.PACK_SHIFTS == (0, 1, 2, 3) == E.TWO_SEG_SHIFTS


@pytest.mark.parametrize("n", E.PACK_GROUPS)
def test_pack_every_end_position_in_the_last_unit(n):
    assert {e & 15 for e in ends(n)} == set(range(16))


@pytest.mark.parametrize("n", E.PACK_GROUPS)
def test_pack_shortest_lengths(n):
    assert {0, 1, 2, 3} <= {length for g, length in E.PACK_CASES if g == n}


@pytest.mark.parametrize("n", E.PACK_GROUPS)
def test_pack_either_side_of_every_shard_boundary(n):
    k = R.outer_k(n)
    want = {64 * j + d for j in range(1, k + 1) for d in (-1, 0, 1)}
    assert want <= set(ends(n))
    if k == 1:
        assert want == {63, 64, 65}
    # the boundaries are those of the data shards: 64-byte symbols up to 64 k, 128 past it
    assert E.symbol_bytes(64 * k - 4, k) == 64 and E.symbol_bytes(64 * k - 3, k) == 128
    assert {R.rs16.OracleOuter.chunk_bytes(k, e) for e in ends(n)} == {64, 128}


@pytest.mark.parametrize("n", E.PACK_GROUPS)
def test_pack_list_is_the_shortest(n):
    """The boundary ends and the lengths 0..3 are forced, and they leave 9 positions of the last unit
    open: no list with fewer cases meets the conditions."""
    k = R.outer_k(n)
    forced = {64 * j + d for j in range(1, k + 1) for d in (-1, 0, 1)} | {4, 5, 6, 7}
    open_positions = set(range(16)) - {e & 15 for e in forced}
    assert len(ends(n)) == len(forced) + len(open_positions) == (16 if k == 1 else 34)


def test_pack_payload_sizes():
    """encode_chunk's payload: 8 bytes of header and a 64- or 128-byte symbol."""
    assert {8 + E.symbol_bytes(length, R.outer_k(n)) for n, length in E.PACK_CASES} == {72, 136}


def test_two_seg_shape():
    n, length = E.TWO_SEG
    cut = R.cut(length, n)
    assert [b - a for a, b in cut] == [2_097_213, 2_097_212]
    # segment 1 starts at every address mod 4 over the shifts, and segment 0's end with it
    assert {(s + cut[1][0]) & 3 for s in E.TWO_SEG_SHIFTS} == {0, 1, 2, 3}


def test_poison_has_no_zero_byte():
    p = E.poison(4096, 1)
    assert len(p) == 4096 and 0 not in p and len(set(p)) > 200
    assert p == E.poison(4096, 1) != E.poison(4096, 2)


def test_euler_lengths():
    r = E.euler_lengths(0)
    assert len(r) == 256 and all(0 <= x <= 15 for x in r)
    a, pairs = 0, []
    for x in r:
        pairs.append((a, x))
        a = (a + x) % 16
    assert a == 0  # a circuit
    assert sorted(pairs) == [(p, q) for p in range(16) for q in range(16)]
    assert r == E.euler_lengths(0)  # deterministic
    more = E.euler_lengths(7)
    assert more[:256] == r and more[256:] == r[:7]


def test_unpack_list_lengths():
    assert len(E.UNPACK_SMALL) == len(E.UNPACK_MIXED) >= 260 > 256
    assert all(0 <= n < 16 for n in E.UNPACK_SMALL)
    assert E.UNPACK_SMALL[:256] == E.euler_lengths(0)
    assert E.UNPACK_MIXED == [r + 16 * (1 + i % 3) for i, r in enumerate(E.UNPACK_SMALL)]
    assert max(E.UNPACK_MIXED) <= 63
    assert E.UNPACK_WIDE == [5, 40_003, 9, 0, 20_000, 1]
    assert E.OUT_BASES == (0, 5)


@pytest.mark.parametrize("base", E.OUT_BASES)
@pytest.mark.parametrize("name", ["small", "mixed"])
def test_unpack_every_offset_and_length_pair(name, base):
    lengths = E.UNPACK_LISTS[name]
    got = {(d & 15, n & 15) for d, n in zip(E.offsets(lengths, 64 + base), lengths)}
    assert got == {(p, q) for p in range(16) for q in range(16)}


@pytest.mark.parametrize("base", E.OUT_BASES)
def test_unpack_small_segment_shapes(base):
    lengths = E.UNPACK_SMALL
    segs = list(zip(E.offsets(lengths, 64 + base), lengths))
    # inside one 16-byte unit, touching neither of its ends
    assert any(n > 0 and d & 15 and (d & 15) + n < 16 for d, n in segs)
    # under 16 bytes and across a unit boundary
    assert any((d & 15) + n > 16 for d, n in segs)
    empty = [i for i, n in enumerate(lengths) if n == 0]
    last = len(lengths) - 1
    assert 0 in empty and last in empty
    # empty ones between non-empty ones, beyond the first and the last
    middle = [i for i in empty if 0 < i < last and lengths[i - 1] and lengths[i + 1]]
    assert len(middle) >= 3
    assert len(empty) >= 16 and len(lengths) > 256


def test_unpack_mixed_has_both_symbol_sizes():
    assert {E.symbol_bytes(n) for n in E.UNPACK_MIXED} == {64, 128}
    assert {E.symbol_bytes(n) for n in E.UNPACK_SMALL} == {64}
    assert E.unpack_gx(E.UNPACK_MIXED) == E.unpack_gx(E.UNPACK_SMALL) == 1


def test_unpack_wide_runs_several_workgroups_per_segment():
    stride = E.unpack_stride(E.UNPACK_WIDE)
    assert stride > 16 * 1024 and stride % 64 == 0
    assert E.unpack_gx(E.UNPACK_WIDE) == -(-(stride // 16) // 1024) >= 2
    for base in E.OUT_BASES:
        segs = list(zip(E.offsets(E.UNPACK_WIDE, 64 + base), E.UNPACK_WIDE))
        for d, n in segs:
            if n >= 20_000:  # the long ones start and end off a unit boundary
                assert d & 15 and (d + n) & 15


def test_fetched_groups():
    groups = [E.group_of(i) for i in range(len(E.UNPACK_SMALL))]
    assert set(groups) == {0, 1} and groups.count(1) == len(groups) // 16
    assert E.group_of(258) == 0  # the error-path test doctors a data group


def test_prefix_past_capacity():
    part = E.unpack_case("mixed")[0][258]
    packed = E.prefix_past_capacity(part)
    assert len(packed) == 4 + len(part)
    cap = len(R.rs16.OracleOuter(1, 3).encode(packed)[0])
    assert 4 + int.from_bytes(packed[:4], "little") == cap + 1
    with pytest.raises(ValueError, match="ChunkPayloadTooShort"):
        R.unpack_segment(packed + bytes(cap - len(packed)))


@pytest.mark.parametrize("name", LISTS)
def test_reference_decodes_the_doctored_snapshot(name):
    parts, chunks = E.unpack_case(name)
    assert [len(p) for p in parts] == E.UNPACK_LISTS[name]
    assert [(c["chunk"], c["group"]) for c in chunks] == [(i, E.group_of(i)) for i in range(len(parts))]
    assert R.decode(E.ref_tracks(chunks), E.UNPACK_GROUPS) == b"".join(parts)
