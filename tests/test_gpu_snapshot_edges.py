"""The snapshot codec's copy kernels (tape_amd/csrc/snapshot.hip: snap_pack_kernel,
snap_unpack_kernel, load16_unaligned) at every byte alignment and segment edge of
tests/snapshot_edge_cases.py, through te_snapshot_encode_device / te_snapshot_decode_device and
against tests/snapshot_ref.py.  Every comparison is bit-exact.

The encode's source lies between nonzero bytes, so a byte read from outside [lo, hi) shows in the
slices; the decode's output lies between guard bytes at either offset of d_out in its unit."""
import numpy as np
import pytest

import snapshot_edge_cases as E
import snapshot_ref as R
from tape_amd import _lib, snapshot
from tape_amd.slicer import ClayCoder, ClayParams
from test_gpu_snapshot import NI, TWO_SEG, check_against_ref, data_of, dev, tracks_of

pytestmark = pytest.mark.gpu

LEAD = 64   # bytes before the data in its tensor (plus the shift), and guard bytes around the output
GUARD = b"\xAA"


@pytest.fixture(scope="module")
def coder():
    return ClayCoder.from_params(ClayParams.default())


# ---------------------------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------------------------
def encode_poisoned(coder, data, n, shift):
    """te_snapshot_encode_device of `data` at byte LEAD + shift of a tensor whose other bytes are
    nonzero: (slices, leaves, roots) as bytes, the plan, both stats."""
    import torch
    P = snapshot.plan(len(data), n, coder)
    src = dev(E.poison(LEAD + shift, 2 * shift) + data + E.poison(LEAD, 2 * shift + 1))
    out = torch.full((max(1, P["total_slice_bytes"]),), 0xEE, dtype=torch.uint8, device="cuda")
    leaves = torch.zeros(P["chunks"] * NI * 32, dtype=torch.uint8, device="cuda")
    roots = torch.zeros(P["chunks"] * 32, dtype=torch.uint8, device="cuda")
    work = torch.full((snapshot.work_bytes(len(data), n, coder),), 0xEE, dtype=torch.uint8, device="cuda")
    snapshot.encode_device(src, len(data), n, out, leaves, roots, work, coder, src_offset=LEAD + shift)
    torch.cuda.synchronize()
    st = snapshot.launch_stats(coder)
    es = _lib.te_encode_launch_stats()
    assert _lib.lib.te_clay_encode_launch_stats(coder.handle, es) == 0
    return out.cpu().numpy().tobytes(), leaves.cpu().numpy().tobytes(), roots.cpu().numpy().tobytes(), P, st, es


@pytest.mark.parametrize("n,length", E.PACK_CASES)
def test_encode_every_data_end_and_source_alignment(coder, n, length):
    data = data_of(n, length)
    for shift in E.PACK_SHIFTS:
        got = encode_poisoned(coder, data, n, shift)
        check_against_ref(got, data, n)  # slices, leaves and roots; the reference is cached per data
        st, es = got[4], got[5]
        assert (st["segments"], st["chunks"], st["clay_objects"]) == (1, n, n), shift
        assert (st["pack_launches"], st["outer_launches"], st["commit_launches"], st["host_waits"]) == (1, 1, 1, 0), shift
        assert es.generic_launches == 0 and es.stage_launches + es.dma_launches >= 1, shift


@pytest.mark.parametrize("shift", E.TWO_SEG_SHIFTS)
def test_encode_two_segments_at_every_source_alignment(coder, shift):
    """Segment 0's last unit is followed in the source by segment 1's bytes, segment 1's by the
    poison: both ends at every address mod 4 (the lengths 2,097,213 and 2,097,212 differ by one)."""
    assert TWO_SEG == E.TWO_SEG
    n, length = TWO_SEG
    data = data_of(n, length)
    got = encode_poisoned(coder, data, n, shift)
    P, st = got[3], got[4]
    assert [(g["len"], g["symbol_bytes"]) for g in P["segs"]] == [(2_097_213, 2_097_280), (2_097_212, 2_097_216)]
    check_against_ref(got, data, n)
    assert (st["segments"], st["chunks"], st["pack_launches"], st["outer_launches"], st["commit_launches"],
            st["host_waits"]) == (2, 6, 1, 2, 2, 0)
    assert got[5].generic_launches == 0


# ---------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------
def decode_at(coder, chunks, cap, base):
    """te_snapshot_decode_device over slices 0..6 of every chunk's track, d_out = buf[LEAD + base:]
    of a guard-filled tensor of LEAD + base + cap + LEAD bytes: (report, result status, result
    length, the whole tensor)."""
    import torch
    tracks = tracks_of(chunks, lambda c: E.FETCHED)
    descs, metas, blob = [], b"", bytearray()
    for group, slices, _ in tracks:
        sl = len(slices[0])
        slot = bytearray(b"\xEE" * (NI * sl))
        mask = 0
        for i, d in slices.items():
            slot[i * sl:(i + 1) * sl] = d
            mask |= 1 << i
        descs.append((group, len(blob), sl, mask))
        metas += slices[0][-48:]
        blob += slot + bytes(-len(slot) % 64)
    d_slices = dev(bytes(blob))
    n = E.UNPACK_GROUPS
    work = torch.zeros(max(64, snapshot.decode_work_bytes(descs, metas, n, coder)), dtype=torch.uint8, device="cuda")
    buf = torch.full((LEAD + base + cap + LEAD,), GUARD[0], dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    res = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    rep = snapshot.decode_device(d_slices, descs, metas, n, buf[LEAD + base:], cap, work, res, None, coder)
    torch.cuda.synchronize()
    rep["stats"] = snapshot.launch_stats(coder)
    r = res.cpu().tolist()
    return rep, r[0], r[1], buf.cpu().numpy().tobytes()


def first_difference(got, want):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return f"{a.size} bytes for {b.size}"
    bad = np.flatnonzero(a != b)
    return None if bad.size == 0 else f"{bad.size} bytes differ, the first at {int(bad[0])}"


@pytest.mark.parametrize("base", E.OUT_BASES)
@pytest.mark.parametrize("name", sorted(E.UNPACK_LISTS))
def test_decode_every_segment_edge(coder, name, base):
    parts, chunks = E.unpack_case(name)
    data = b"".join(parts)
    assert R.decode(E.ref_tracks(chunks), E.UNPACK_GROUPS) == data
    rep, status, length, buf = decode_at(coder, chunks, len(data), base)
    assert rep["code"] == 0 and rep["status"] == [0] * len(chunks), rep
    assert rep["segment"] == list(range(len(chunks)))
    assert (status, length) == (0, len(data))
    at = LEAD + base
    assert first_difference(buf[at:at + len(data)], data) is None
    assert buf[:at] == GUARD * at and buf[at + len(data):] == GUARD * LEAD
    st = rep["stats"]
    assert (st["header_launches"], st["unpack_launches"], st["segments"]) == (1, 1, len(parts))


def test_decode_length_prefix_past_its_capacity_beyond_the_first_256_segments(coder):
    """Segment 258's prefix says one byte more than its symbol holds: a thread finds it on its
    second trip through the prefix loop, and nothing is written."""
    parts, chunks = E.unpack_case("mixed")
    bad = 258
    assert 256 <= bad < len(chunks)
    doctored = list(chunks)
    doctored[bad] = E.chunk_of(bad, E.prefix_past_capacity(parts[bad]))
    with pytest.raises(ValueError, match="ChunkPayloadTooShort"):
        R.decode(E.ref_tracks(doctored), E.UNPACK_GROUPS)
    total = sum(map(len, parts))
    rep, status, _, buf = decode_at(coder, doctored, total, 5)
    assert rep["code"] == 0 and status == _lib.TE_ERR_INVALID_LAYOUT
    assert buf == GUARD * len(buf)
    assert rep["stats"]["unpack_launches"] == 1


def test_decode_many_segments_out_cap_one_byte_short(coder):
    parts, chunks = E.unpack_case("mixed")
    total = sum(map(len, parts))
    rep, status, need, buf = decode_at(coder, chunks, total - 1, 5)
    assert rep["code"] == 0 and (status, need) == (_lib.TE_ERR_BUFFER_TOO_SMALL, total)
    assert buf == GUARD * len(buf)
    assert rep["stats"]["unpack_launches"] == 1
