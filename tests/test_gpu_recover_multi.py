"""Multi-slice node recover (te_recover_multi_batch_device, te_slicer_recover_multi,
tape_amd/csrc/recover_multi.hip) against the CPU oracle's Slicer::encode, bit for bit, metadata
suffix included.

Every call writes into a buffer pre-filled with 0xA5 and the whole buffer is compared with the
expected image, so a byte stored outside the rebuilt slices, or one left unwritten inside them,
fails.  The slices that are not available to a call are poisoned in its input.  Each test asserts
the path it took from te_clay_recover_multi_launch_stats (and the decode / encode launch stats for
the delegated paths).

Small geometry: Clay(20,7,16) with a 20,000-byte object (one stripe, sub-chunks of 30 bytes: 8
words a row, the last a tail word), a 300,000-byte one (three full stripes, 36 words a row) and a
250,001-byte one (a short last stripe), in one batch, rotated and identity layouts.  Production
geometry: 4 MiB objects (sub-chunks of 1,430 bytes: two waves a workgroup, three workgroups a
stripe)."""
import ctypes as C
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib, batch

pytestmark = pytest.mark.gpu
N, POISON, GUARD = 20, 0xA5, 64
MiB = 1024 * 1024
SMALL = (20_000, 300_000, 250_001)

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()


def _slicer(rotated):
    key = ("slicer", rotated)
    if key not in _cache:
        _cache[key] = T.Slicer.clay_default() if rotated else T.Slicer.new(T.ClayCoder(20, 7, 16))
    return _cache[key]


def _objects(oracle, rotated, lens):
    """Oracle-encoded objects, made once per (layout, lengths) and left unchanged: (n, slice_len) each."""
    key = ("objs", rotated, lens)
    if key not in _cache:
        o = oracle.OracleClay(20, 7, 16)
        _cache[key] = [oracle.slicer_encode_np(o, oracle.splitmix64_bytes(0x6D756C74 ^ ln ^ int(rotated), ln) if ln
                                               else np.zeros(0, np.uint8), rotated=rotated) for ln in lens]
    return _cache[key]


def _bits(xs):
    return sum(1 << i for i in xs)


def _run(slicer, objs, specs, misalign=0, fn=batch.recover_multi_batch, single=False):
    """One call over specs = [(object index, avail slices, lost slices)].  Returns (got, expected)
    host images of the whole output buffer."""
    import torch
    ins, descs, metas, exp = [], [], b"", [np.full(GUARD + misalign, POISON, np.uint8)]
    in_at, out_at = 0, GUARD + misalign
    for oi, avail, lost in specs:
        sl = objs[oi]
        slen = sl.shape[1]
        img = np.full_like(sl, 0x3C)  # what is not available is never what the call needs
        for i in avail:
            img[i] = sl[i]
        ins.append(img.reshape(-1))
        lost = sorted(lost)
        if single:
            for j, i in enumerate(lost):
                descs.append((in_at, slen, _bits(avail), i, out_at + j * slen))
                metas += sl[avail[0]][-48:].tobytes()
        else:
            descs.append((in_at, slen, _bits(avail), _bits(lost), out_at))
            metas += sl[avail[0]][-48:].tobytes()
        for i in lost:
            exp.append(sl[i])
        gap = np.full(GUARD + (3 if misalign else 0), POISON, np.uint8)  # the next object's offset stays odd
        exp.append(gap)
        in_at += sl.size
        out_at += len(lost) * slen + gap.size
    exp = np.concatenate(exp)
    d_in = torch.from_numpy(np.concatenate(ins)).cuda()
    d_out = torch.full((exp.size,), POISON, dtype=torch.uint8, device="cuda")
    fn(slicer, d_in, descs, metas, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), exp


def _same(got, exp, what):
    if np.array_equal(got, exp):
        return
    at = int(np.nonzero(got != exp)[0][0])
    raise AssertionError(f"{what}: first mismatch at byte {at} of {exp.size}: got {int(got[at]):#x}, expected {int(exp[at]):#x}")


# lost sets by slice (= node in an identity layout and in a rotated layout's stripe 0), 7 survivors each
LOST_SETS = {
    "column0_pair": ([0, 2, 3, 10, 11, 12, 13], [1, 4]),
    "column1_pair": ([0, 1, 2, 3, 4, 10, 11], [12, 17]),
    "data_and_parity_across": ([0, 1, 3, 4, 5, 10, 11], [2, 15]),
    "all_13": ([0, 3, 5, 9, 11, 14, 18], [i for i in range(N) if i not in (0, 3, 5, 9, 11, 14, 18)]),
    "ten_available_three_lost": ([0, 1, 2, 3, 4, 10, 11, 12, 13, 14], [5, 15, 19]),
}


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "identity"])
@pytest.mark.parametrize("case", list(LOST_SETS))
def test_small_geometry_lost_sets(oracle, rotated, case):
    s, objs = _slicer(rotated), _objects(oracle, rotated, SMALL)
    avail, lost = LOST_SETS[case]
    specs = [(i, avail, lost) for i in range(len(SMALL))]
    got, exp = _run(s, objs, specs)
    st = batch.recover_multi_launch_stats(s.coder)
    _same(got, exp, case)
    assert (st["multi_objects"], st["single_objects"], st["generic_objects"]) == (3, 0, 0), st
    assert st["multi_launches"] == 2 and st["stripes"] == 7, st  # two chunk sizes; 1 + 3 + 3 stripes
    assert st["out_rows"] == 7 * len(lost) * 100 and st["jobs"] >= 7, st
    assert st["passes"] >= 1 and (st["split_stripes"] > 0) == (st["passes"] > 1), st
    d = s.coder.decode_launch_stats()
    assert d["table_launches"] == 0 and d["generic_launches"] == 0 and not d["class_launches"], d


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_output_offset_not_a_multiple_of_four(oracle, misalign):
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    avail, lost = LOST_SETS["data_and_parity_across"]
    got, exp = _run(s, objs, [(i, avail, lost) for i in range(len(SMALL))], misalign=misalign)
    _same(got, exp, f"out_off % 4 == {misalign}")
    assert batch.recover_multi_launch_stats(s.coder)["multi_objects"] == 3


def test_mask_split(oracle):
    """All 13 erased nodes never fit one pass (tests/native/rec_multi_check.cpp checks that on the CPU
    for every sampled survivor set): the stripe's sub-masks run as passes over the same slices."""
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    rnd = random.Random(13)
    specs = []
    for i in range(len(SMALL)):
        avail = sorted(rnd.sample(range(N), 7))
        specs.append((i, avail, [j for j in range(N) if j not in avail]))
    got, exp = _run(s, objs, specs)
    st = batch.recover_multi_launch_stats(s.coder)
    _same(got, exp, "split")
    assert st["passes"] >= 2 and st["split_stripes"] == st["stripes"] == 7 and st["jobs"] >= 14, st
    assert st["out_rows"] == 7 * 13 * 100, st


def test_single_slice_routing(oracle):
    """popcount(lost_mask) == 1, every slice index: the single-slice path's bytes and launches."""
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    rnd = random.Random(1)
    specs = []
    for lost in range(N):
        specs.append((lost % len(SMALL), sorted(rnd.sample([i for i in range(N) if i != lost], 7)), [lost]))
    want, exp = _run(s, objs, specs, fn=batch.recover_batch, single=True)
    want_launch = s.coder.decode_launch_stats()
    _same(want, exp, "te_recover_batch_device")
    got, _ = _run(s, objs, specs)
    st = batch.recover_multi_launch_stats(s.coder)
    assert np.array_equal(got, want)
    assert (st["single_objects"], st["multi_objects"], st["generic_objects"]) == (N, 0, 0), st
    assert st["multi_launches"] == 0 and st["passes"] == 0 and st["jobs"] == 0, st
    assert s.coder.decode_launch_stats() == want_launch  # the same kernels, launch for launch


def test_mixed_batch_single_and_multi(oracle):
    s, objs = _slicer(False), _objects(oracle, False, SMALL)
    specs = [(0, [1, 2, 3, 4, 5, 6, 7], [0]), (1, [0, 2, 4, 6, 8, 10, 12], [1, 3, 19]), (2, [13, 14, 15, 16, 17, 18, 19], [5])]
    got, exp = _run(s, objs, specs)
    st = batch.recover_multi_launch_stats(s.coder)
    _same(got, exp, "mixed")
    assert (st["single_objects"], st["multi_objects"], st["multi_launches"], st["stripes"]) == (2, 1, 1, 3), st


def test_production_sub_chunk(oracle):
    """Two 4 MiB objects (sc = 1,430), random 7-of-20 survivors, four lost slices each."""
    s, objs = _slicer(True), _objects(oracle, True, (4 * MiB, 4 * MiB - 5))
    assert s.geometry(4 * MiB).sub_chunk_size == 1430
    rnd = random.Random(4)
    specs = []
    for i in range(2):
        avail = sorted(rnd.sample(range(N), 7))
        specs.append((i, avail, sorted(rnd.sample([j for j in range(N) if j not in avail], 4))))
    got, exp = _run(s, objs, specs)
    st = batch.recover_multi_launch_stats(s.coder)
    _same(got, exp, "4 MiB")
    ns = int(s.geometry(4 * MiB).num_stripes)
    assert st["multi_launches"] == 1 and st["multi_objects"] == 2 and st["stripes"] == 2 * ns, st
    assert st["out_rows"] == 2 * ns * 4 * 100, st


def test_batch_geometry_two_waves(oracle):
    """More than 64 jobs: the batch geometry (two waves a workgroup, three workgroups a stripe at
    sc = 1,430) instead of the per-call one the two-object case runs."""
    s, objs = _slicer(True), _objects(oracle, True, (4 * MiB, 4 * MiB - 5))
    rnd = random.Random(14)
    specs = []
    for i in range(14):
        avail = sorted(rnd.sample(range(N), 7))
        specs.append((i % 2, avail, sorted(rnd.sample([j for j in range(N) if j not in avail], 2))))
    got, exp = _run(s, objs, specs)
    st = batch.recover_multi_launch_stats(s.coder)
    _same(got, exp, "14 x 4 MiB")
    assert st["multi_launches"] == 1 and st["jobs"] >= 70 and st["stripes"] == 70, st


def test_empty_blob_is_metadata_only(oracle):
    s, objs = _slicer(True), _objects(oracle, True, (0,))
    got, exp = _run(s, objs, [(0, [0, 1, 2, 3, 4, 5, 6], [7, 19])])
    _same(got, exp, "empty blob")
    st = batch.recover_multi_launch_stats(s.coder)
    assert st["single_objects"] == 1 and st["multi_launches"] == 0, st


def test_generic_path_other_profile(oracle):
    """Clay(12,8,11) has no plane programs: the existing decode, then the existing encode, two lost
    slices kept."""
    key = ("generic",)
    if key not in _cache:
        o = oracle.OracleClay(12, 8, 11)
        data = oracle.splitmix64_bytes(0x12811, 250_001)
        sl = oracle.slicer_encode(o, data.tobytes(), rotated=True)
        _cache[key] = np.stack([np.frombuffer(x, np.uint8) for x in sl])
    sl = _cache[key]
    s = T.Slicer.with_profile(T.ClayCoder(12, 8, 11), T.STRIPE_SIZES[0], True, T.EncodingProfile.clay_default())
    import torch
    n, slen = sl.shape
    avail, lost = [0, 1, 2, 4, 5, 7, 8, 10, 11], [3, 9]
    img = np.full_like(sl, 0x3C)
    for i in avail:
        img[i] = sl[i]
    exp = np.concatenate([np.full(GUARD + 1, POISON, np.uint8), sl[3], sl[9], np.full(GUARD, POISON, np.uint8)])
    d_out = torch.full((exp.size,), POISON, dtype=torch.uint8, device="cuda")
    batch.recover_multi_batch(s, torch.from_numpy(img.reshape(-1)).cuda(), [(0, slen, _bits(avail), _bits(lost), GUARD + 1)],
                              sl[0][-48:].tobytes(), d_out)
    torch.cuda.synchronize()
    _same(d_out.cpu().numpy(), exp, "Clay(12,8,11)")
    st = batch.recover_multi_launch_stats(s.coder)
    assert (st["generic_objects"], st["multi_objects"], st["single_objects"], st["multi_launches"]) == (1, 0, 0, 0), st
    d = s.coder.decode_launch_stats()
    assert d["generic_launches"] >= 1 and d["table_launches"] == 0, d


def test_host_form_pageable(oracle):
    """te_slicer_recover_multi from pageable numpy buffers into pageable outputs."""
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    sl = objs[2]
    slen = sl.shape[1]
    avail, lost = [1, 2, 6, 8, 12, 15, 17, 19], [0, 7, 13]
    keep = {i: np.ascontiguousarray(sl[i]).copy() for i in avail}
    ptrs = (C.c_void_p * N)(*[keep[i].ctypes.data if i in keep else None for i in range(N)])
    outs = [np.full(slen + 2 * GUARD, POISON, np.uint8) for _ in lost]
    optrs = (C.c_void_p * len(lost))(*[o.ctypes.data + GUARD for o in outs])
    cfg = s._cfg()
    r = _lib.lib.te_slicer_recover_multi(s.coder.handle, C.byref(cfg), ptrs, slen, _bits(lost), optrs)
    assert r == 0, _lib.strerror(r)
    guard = np.full(GUARD, POISON, np.uint8)
    for o, i in zip(outs, lost):
        _same(o, np.concatenate([guard, sl[i], guard]), f"slice {i}")
    for i in avail:
        assert np.array_equal(keep[i], sl[i])  # the inputs are left as they were
    st = batch.recover_multi_launch_stats(s.coder)
    assert st["multi_objects"] == 1 and st["multi_launches"] == 1 and st["stripes"] == 3, st


def test_recover_many_round_trip(oracle):
    s = _slicer(True)
    data = oracle.splitmix64_bytes(99, 123_457).tobytes()
    sl = s.encode(data)
    avail = [0, 4, 5, 9, 10, 16, 18]
    got = s.recover_many([(i, sl[i]) for i in avail], [19, 2, 11, 7])
    assert sorted(got) == [2, 7, 11, 19]
    for i, b in got.items():
        assert b == sl[i], f"slice {i}"
    one = s.recover_many([(i, sl[i]) for i in avail], [3])  # a single lost slice: the single-slice path
    assert one == {3: sl[3]}
    assert batch.recover_multi_launch_stats(s.coder)["single_objects"] == 1
    with pytest.raises(T.slicer.EngineError):
        s.recover_many([(i, sl[i]) for i in avail], [4, 6])  # slice 4 is present
