"""GPU parity of the snapshot codec (te_snapshot_*; lib/snapshot/src/{encode,decode,chunk}.rs,
network/protocol/src/snapshot.rs:143-275) against the composition of the oracles in
tests/snapshot_ref.py.  Every comparison is bit-exact."""
import random

import numpy as np
import pytest

import snapshot_ref as R
import tape_amd as T
from tape_amd import _lib, snapshot
from tape_amd.slicer import ClayCoder, ClayParams

pytestmark = pytest.mark.gpu

NI = 20  # GROUP_SIZE: slices per chunk
TWO_SEG = (3, 4_194_425)  # segments of 2,097,213 and 2,097,212 bytes: symbols of 2,097,280 and 2,097,216
ENCODE_CASES = [(1, 1), (3, 0), (3, 61), (20, 1), (20, 1000), (50, 5000), (50, 17 * 64 - 4), (50, 17 * 64 - 3)]


@pytest.fixture(scope="module")
def coder():
    return ClayCoder.from_params(ClayParams.default())


def data_of(n, length):
    return np.random.default_rng(n * 1_000_003 + length).bytes(length)


def dev(b: bytes, pad: int = 0):
    import torch
    a = np.frombuffer(bytes(b) + bytes(pad), np.uint8) if len(b) + pad else np.zeros(1, np.uint8)
    return torch.from_numpy(a.copy()).cuda()


def encode_device(coder, data, n, shift=0):
    """te_snapshot_encode_device with the compressed bytes `shift` bytes into their tensor:
    (slices, leaves, roots) as bytes, the plan, both stats."""
    import torch
    P = snapshot.plan(len(data), n, coder)
    src = dev(bytes(shift) + data, 8)
    out = torch.full((max(1, P["total_slice_bytes"]),), 0xEE, dtype=torch.uint8, device="cuda")
    leaves = torch.zeros(P["chunks"] * NI * 32, dtype=torch.uint8, device="cuda")
    roots = torch.zeros(P["chunks"] * 32, dtype=torch.uint8, device="cuda")
    work = torch.full((snapshot.work_bytes(len(data), n, coder),), 0xEE, dtype=torch.uint8, device="cuda")
    snapshot.encode_device(src, len(data), n, out, leaves, roots, work, coder, src_offset=shift)
    torch.cuda.synchronize()
    st = snapshot.launch_stats(coder)
    es = _lib.te_encode_launch_stats()
    assert _lib.lib.te_clay_encode_launch_stats(coder.handle, es) == 0
    return out.cpu().numpy().tobytes(), leaves.cpu().numpy().tobytes(), roots.cpu().numpy().tobytes(), P, st, es


def check_against_ref(got, data, n):
    slices, leaves, roots, P, _, _ = got
    ref = R.encode(data, n)
    assert len(ref) == P["chunks"]
    for c in ref:
        g, t = P["segs"][c["chunk"]], c["track_number"]
        sl = g["slice_len"]
        base = g["slices_off"] + c["group"] * NI * sl
        assert len(c["slices"][0]) == sl
        for i in range(NI):
            assert slices[base + i * sl:base + (i + 1) * sl] == c["slices"][i], (t, i)
            assert leaves[(t * NI + i) * 32:(t * NI + i + 1) * 32] == c["leaves"][i], (t, i)
        assert roots[t * 32:(t + 1) * 32] == c["root"], t
        assert (g["size"], g["stripe_count"]) == (c["size"], c["stripe_count"])


@pytest.mark.parametrize("n,length", ENCODE_CASES)
def test_encode_matches_oracle(coder, n, length):
    data = data_of(n, length)
    got = encode_device(coder, data, n)
    check_against_ref(got, data, n)
    st, es = got[4], got[5]
    assert (st["segments"], st["chunks"], st["clay_objects"]) == (1, n, n)
    assert (st["pack_launches"], st["outer_launches"], st["commit_launches"], st["host_waits"]) == \
        (1, 0 if n == 1 else 1, 1, 0)
    assert es.generic_launches == 0 and es.stage_launches + es.dma_launches >= 1
    # the host form equals the device form
    host = snapshot.encode(data, n, coder)
    P = got[3]
    for c in host:
        g = P["segs"][c.chunk]
        base = g["slices_off"] + c.group * NI * g["slice_len"]
        assert b"".join(c.slices) == got[0][base:base + NI * g["slice_len"]]
        assert b"".join(c.leaves) == got[1][c.track_number * NI * 32:(c.track_number + 1) * NI * 32]
        assert c.root == got[2][c.track_number * 32:(c.track_number + 1) * 32]


def test_encode_source_misalignment(coder):
    data = data_of(20, 1000)
    base = encode_device(coder, data, 20)
    check_against_ref(base, data, 20)
    for shift in (1, 2, 3):
        got = encode_device(coder, data, 20, shift)
        assert got[:3] == base[:3], shift
        assert got[5].generic_launches == 0


def test_encode_two_segments_of_different_symbol_size(coder):
    n, length = TWO_SEG
    data = data_of(n, length)
    got = encode_device(coder, data, n, shift=1)
    P, st = got[3], got[4]
    assert [(g["len"], g["symbol_bytes"]) for g in P["segs"]] == [(2_097_213, 2_097_280), (2_097_212, 2_097_216)]
    check_against_ref(got, data, n)
    assert (st["segments"], st["chunks"], st["pack_launches"], st["outer_launches"], st["commit_launches"],
            st["host_waits"]) == (2, 6, 1, 2, 2, 0)
    assert got[5].generic_launches == 0


# ---------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------
def tracks_of(chunks, pick):
    """(group, {leaf_index: slice}) per chunk; pick(chunk) -> the leaf indices fetched (None: skip)."""
    out = []
    for c in chunks:
        idx = pick(c)
        if idx is not None:
            out.append((c["group"], {i: c["slices"][i] for i in idx}, c["leaves"]))
    return out


def decode_device(coder, tracks, n, cap, verified=False, guard=64):
    """te_snapshot_decode_device: (report, result status, result length, output bytes + guard)."""
    import torch
    descs, metas, blob, off = [], b"", bytearray(), 0
    for group, slices, _ in tracks:
        sl = len(next(iter(slices.values())))
        slot = bytearray(b"\xEE" * (NI * sl))
        mask = 0
        for i, d in slices.items():
            slot[i * sl:(i + 1) * sl] = d
            mask |= 1 << i
        descs.append((group, off, sl, mask))
        metas += next(iter(slices.values()))[-48:]
        blob += slot + bytes(-len(slot) % 64)
        off = len(blob)
    leaves = b"".join(b"".join(t[2]) for t in tracks) if verified else None
    d_slices = dev(bytes(blob))
    work = torch.zeros(max(64, snapshot.decode_work_bytes(descs, metas, n, coder)), dtype=torch.uint8, device="cuda")
    out = torch.full((cap + guard,), 0xAA, dtype=torch.uint8, device="cuda")
    res = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rep = snapshot.decode_device(d_slices, descs, metas, n, out, cap, work, res, leaves, coder)
    torch.cuda.synchronize()
    rep["stats"] = snapshot.launch_stats(coder)
    r = res.cpu().tolist()
    return rep, r[0], r[1], out.cpu().numpy().tobytes()


def expect_decoded(coder, tracks, n, data, verified=False):
    rep, status, length, out = decode_device(coder, tracks, n, len(data), verified)
    assert rep["code"] == 0, rep
    assert (status, length) == (0, len(data))
    assert out[:len(data)] == data and out[len(data):] == b"\xAA" * 64
    assert rep["stats"]["host_waits"] == (2 if verified else 1)
    assert (rep["stats"]["header_launches"], rep["stats"]["unpack_launches"]) == (1, 1)
    return rep


DECODE_CASES = ENCODE_CASES + [TWO_SEG]  # every encode above


@pytest.mark.parametrize("n,length", DECODE_CASES)
def test_decode_first_seven_slices(coder, n, length):  # the reference's own test (encode.rs tests)
    data = data_of(n, length)
    tracks = tracks_of(R.encode(data, n), lambda c: range(7))
    assert R.decode([(g, s) for g, s, _ in tracks], n) == data
    rep = expect_decoded(coder, tracks, n, data)
    assert rep["segment"] == [c["chunk"] for c in R.encode(data, n)]
    assert rep["stats"]["segments"] == len(R.cut(length, n)) and rep["stats"]["chunks"] == len(tracks)


@pytest.mark.parametrize("n,length", DECODE_CASES)
def test_decode_random_seven_of_twenty(coder, n, length):
    data = data_of(n, length)
    rng = random.Random(n * 31 + length)
    tracks = tracks_of(R.encode(data, n), lambda c: sorted(rng.sample(range(NI), 7)))
    rng.shuffle(tracks)
    expect_decoded(coder, tracks, n, data)


# n = 1 has no recovery group (OuterCoder(1, 1)): every other encode above
@pytest.mark.parametrize("n,length", [c for c in DECODE_CASES if c[0] > 1])
def test_decode_outer_k_recovery_groups_only(coder, n, length):
    """Exactly outer_k tracks per segment, none of them a data group: every data shard is GF(2^16)
    work on the 8-mod-64 symbol pointers.  TWO_SEG makes that two runs of different symbol size."""
    data = data_of(n, length)
    k = R.outer_k(n)
    tracks = tracks_of(R.encode(data, n), lambda c: range(13, 20) if k <= c["group"] < 2 * k else None)
    segs = len(R.cut(length, n))
    assert len(tracks) == k * segs
    rep = expect_decoded(coder, tracks, n, data)
    assert rep["stats"]["outer_launches"] >= (2 if (n, length) == TWO_SEG else 1)


def test_decode_several_segments_of_one_symbol_size_from_recovery_groups(coder):
    """A batch of three segments in one outer call, each rebuilt from a recovery group alone
    (doctored segments: a real snapshot has more than one only past 4 MiB)."""
    parts = [data_of(3, 100 + i) for i in range(3)]
    chunks = doctored([(i, R.pack_segment(p)) for i, p in enumerate(parts)], 3)
    tracks = tracks_of(chunks, lambda c: range(7) if c["group"] == 1 + c["chunk"] % 2 else None)
    assert R.decode([(g, s) for g, s, _ in tracks], 3) == b"".join(parts)
    rep = expect_decoded(coder, tracks, 3, b"".join(parts))
    assert rep["stats"]["segments"] == 3 and rep["stats"]["outer_launches"] >= 1


def test_decode_repeated_group_within_a_segment(coder):
    """outer.rs:140-170 keeps the last symbol given for a group: two tracks of group 0, of
    different data, decode to the second one's, as OracleOuter.decode does."""
    x, y = data_of(3, 50), data_of(3, 51)[:50]
    chunks = doctored([(0, R.pack_segment(x))], 3)[:1] + doctored([(0, R.pack_segment(y))], 3)[:1]
    tracks = tracks_of(chunks, lambda c: range(7))
    assert [g for g, _, _ in tracks] == [0, 0]
    assert R.decode([(g, s) for g, s, _ in tracks], 3) == y
    expect_decoded(coder, tracks, 3, y)


def test_decode_verified_rejects_a_corrupted_slice(coder):
    n, length = 20, 1000
    data = data_of(n, length)
    tracks = tracks_of(R.encode(data, n), lambda c: range(8) if c["group"] == 2 else range(7))
    bad = bytearray(tracks[2][1][3])
    bad[5] ^= 0x40
    tracks[2][1][3] = bytes(bad)
    rep = expect_decoded(coder, tracks, n, data, verified=True)
    assert rep["rejected"] == [0, 0, 1 << 3] + [0] * (n - 3)
    assert rep["status"] == [0] * n


def test_decode_skips_a_track_with_six_good_slices(coder):
    n, length = 20, 1000
    data = data_of(n, length)
    tracks = tracks_of(R.encode(data, n), lambda c: range(7))
    bad = bytearray(tracks[0][1][6])
    bad[0] ^= 1
    tracks[0][1][6] = bytes(bad)  # verified: 6 good slices left
    tracks[1] = (tracks[1][0], {i: tracks[1][1][i] for i in range(6)}, tracks[1][2])  # 6 fetched
    rep = expect_decoded(coder, tracks, n, data, verified=True)
    assert rep["status"][:3] == [_lib.TE_ERR_NOT_ENOUGH_SLICES, _lib.TE_ERR_NOT_ENOUGH_SLICES, 0]
    assert rep["rejected"][0] == 1 << 6 and rep["segment"][:3] == [snapshot.NO_SEGMENT, snapshot.NO_SEGMENT, 0]
    assert rep["stats"]["chunks"] == n - 2
    # unverified: the track with six slices is skipped the same way
    rep = expect_decoded(coder, tracks[1:], n, data)
    assert rep["status"][0] == _lib.TE_ERR_NOT_ENOUGH_SLICES


def test_decode_insufficient_groups(coder):
    n, length = 20, 1000
    data = data_of(n, length)
    k = R.outer_k(n)
    tracks = tracks_of(R.encode(data, n), lambda c: range(7) if c["group"] < k - 1 else None)
    rep, status, _, out = decode_device(coder, tracks, n, length)
    assert rep["code"] == _lib.TE_ERR_NOT_ENOUGH_SLICES
    assert rep["detail"].startswith("InsufficientGroups") and "only 6/7 groups" in rep["detail"]
    assert out == b"\xAA" * len(out)
    with pytest.raises(snapshot.SnapshotError, match="InsufficientGroups"):
        snapshot.decode([(g, list(s.items())) for g, s, _ in tracks], n, coder=coder)
    with pytest.raises(snapshot.SnapshotError, match="NoChunks"):
        snapshot.decode([], n, coder=coder)


def doctored(segments, n):
    """Chunks of hand-made segments: segments[i] = (header chunk number, packed segment bytes)."""
    k = R.outer_k(n)
    out = []
    for chunk, packed in segments:
        for g, sym in enumerate(R.rs16.OracleOuter(k, n).encode(packed)):
            c = R.encode_chunk(chunk, sym)
            c.update(group=g, chunk=chunk)
            out.append(c)
    return out


def test_decode_missing_middle_segment(coder):
    chunks = doctored([(0, R.pack_segment(b"a" * 10)), (2, R.pack_segment(b"c" * 10))], 3)
    rep, _, _, _ = decode_device(coder, tracks_of(chunks, lambda c: range(7)), 3, 64)
    assert rep["code"] == _lib.TE_ERR_NOT_ENOUGH_SLICES
    assert rep["detail"].startswith("MissingChunk") and "chunk 1" in rep["detail"]


def test_decode_files_a_track_under_its_headers_segment(coder):
    """snapshot.rs:167-171: the segment is the decoded header's, wherever the track came from."""
    a, b = data_of(3, 100), data_of(3, 77)
    chunks = doctored([(1, R.pack_segment(b)), (0, R.pack_segment(a))], 3)  # segment 1's tracks first
    tracks = tracks_of(chunks, lambda c: range(7))
    rep = expect_decoded(coder, tracks, 3, a + b)
    assert rep["segment"] == [1, 1, 1, 0, 0, 0]
    assert R.decode([(g, s) for g, s, _ in tracks], 3) == a + b


def test_decode_length_prefix_past_its_segment(coder):
    packed = (1000).to_bytes(4, "little") + bytes(60)  # 4 + 1000 > 64
    tracks = tracks_of(doctored([(0, packed)], 3), lambda c: range(7))
    rep, status, _, out = decode_device(coder, tracks, 3, 2048)
    assert rep["code"] == 0 and status == _lib.TE_ERR_INVALID_LAYOUT
    assert out == b"\xAA" * len(out)
    with pytest.raises(snapshot.SnapshotError, match="ChunkPayload"):
        snapshot.decode([(g, list(s.items())) for g, s, _ in tracks], 3, coder=coder)


def test_decode_unequal_symbols_in_a_segment(coder):  # outer.rs:136-138
    chunks = doctored([(0, R.pack_segment(b"x" * 10))], 3)[:1] + doctored([(0, R.pack_segment(b"y" * 100))], 3)[1:2]
    rep, _, _, _ = decode_device(coder, tracks_of(chunks, lambda c: range(7)), 3, 256)
    assert rep["code"] == _lib.TE_ERR_INVALID_LAYOUT


def test_decode_out_cap_one_byte_short(coder):
    n, length = 20, 1000
    data = data_of(n, length)
    tracks = tracks_of(R.encode(data, n), lambda c: range(7))
    rep, status, need, out = decode_device(coder, tracks, n, length - 1, guard=128)
    assert rep["code"] == 0 and (status, need) == (_lib.TE_ERR_BUFFER_TOO_SMALL, length)
    assert out == b"\xAA" * (length - 1 + 128)  # nothing written, before or past out_cap
    with pytest.raises(snapshot.SnapshotError, match="OutputTooSmall"):
        snapshot.decode([(g, list(s.items())) for g, s, _ in tracks], n, coder=coder, max_len=length - 1)


@pytest.mark.parametrize("n,length", [(20, 1000), (3, 199_996)])
def test_round_trip_through_the_python_mirror(coder, n, length):
    """encode and decode of tape_amd.snapshot (the host forms), and the reference's symbol-length
    quirk on the way: 199,996 bytes at n = 3 make a 200,000-byte symbol, 2 stripes by encode_chunk's
    count, 3 by the slicer's."""
    data = data_of(n, length)
    chunks = snapshot.encode(data, n, coder)
    ref = R.encode(data, n)
    assert [(c.size, c.stripe_count, c.stripe_size) for c in chunks] == \
        [(c["size"], c["stripe_count"], c["stripe_size"]) for c in ref]
    assert [c.root for c in chunks] == [c["root"] for c in ref]
    rng = random.Random(length)
    tracks = [(c.group, [(i, c.slices[i]) for i in sorted(rng.sample(range(NI), 7))]) for c in chunks]
    rep = {}
    assert snapshot.decode(tracks, n, coder=coder, report=rep) == data
    assert rep["status"] == [0] * len(tracks) and rep["segment"] == [c.chunk for c in chunks]
    assert snapshot.decode(tracks, n, leaves=[c.leaves for c in chunks], coder=coder) == data
    assert T.snapshot.launch_stats(coder)["host_waits"] == 2


@pytest.mark.parametrize("window", [None, "1"])
def test_host_forms_on_two_segments_of_different_symbol_size(coder, window, monkeypatch):
    """te_snapshot_encode_host equals the device form where the last segment's symbols are shorter,
    in one window and (TEC_SNAPSHOT_WINDOW_BYTES) in a window per segment; te_snapshot_decode_host
    reads it back from the recovery group alone."""
    n, length = TWO_SEG
    data = data_of(n, length)
    want = encode_device(coder, data, n)
    P = want[3]
    if window:
        monkeypatch.setenv("TEC_DEBUG_KNOBS", "1")
        monkeypatch.setenv("TEC_SNAPSHOT_WINDOW_BYTES", window)
    host = snapshot.encode(data, n, coder)
    st = snapshot.launch_stats(coder)
    assert (st["segments"], st["chunks"], st["clay_objects"], st["pack_launches"], st["host_waits"]) == \
        (2, 6, 6, 2 if window else 1, 0)
    assert [c.track_number for c in host] == list(range(6))
    for c in host:
        g = P["segs"][c.chunk]
        base = g["slices_off"] + c.group * NI * g["slice_len"]
        assert b"".join(c.slices) == want[0][base:base + NI * g["slice_len"]], c.track_number
        assert b"".join(c.leaves) == want[1][c.track_number * NI * 32:(c.track_number + 1) * NI * 32]
        assert c.root == want[2][c.track_number * 32:(c.track_number + 1) * 32]
    tracks = [(c.group, [(i, c.slices[i]) for i in range(13, 20)]) for c in host if c.group == 1]
    assert snapshot.decode(tracks, n, coder=coder) == data
    assert snapshot.launch_stats(coder)["outer_launches"] >= 2


def test_encode_through_the_transform_kernels(coder, monkeypatch):
    """Shapes without a matrix image (here forced: TEC_RS16_NO_MATRIX) take the transform kernels,
    with the payload stride in place of chunk_bytes, and wait once per outer launch."""
    monkeypatch.setenv("TEC_DEBUG_KNOBS", "1")
    monkeypatch.setenv("TEC_RS16_NO_MATRIX", "1")
    n, length = 20, 1000
    data = data_of(n, length)
    got = encode_device(coder, data, n)
    check_against_ref(got, data, n)
    assert (got[4]["outer_launches"], got[4]["host_waits"]) == (1, 1)
