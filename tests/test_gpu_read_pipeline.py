"""The host read pipeline on the device: te_decode_batch_host, te_decode_verified_batch_host and
te_stream_reader_* against the CPU oracle (slices encoded and decoded by oracle/clay_oracle.c) and
against te_decode_batch_device on the same inputs.

The slices lie in a host buffer whose absent slots are poisoned (0xA5), and every output range has
a poisoned guard band on both sides: an absent slot must never be read into a result, and no byte
outside an object's blob_len bytes may change.  The shapes are the smallest at which the pipeline
can go wrong: nine objects of 0 B .. 4 MiB + 9 B over five windows (the three-slot ring wraps),
single-object and oversize windows, survivor sets of the data slices, the parity slices, random
7-of-20 and more than k present."""
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib, batch

pytestmark = pytest.mark.gpu
N, K = 20, 7
MiB = 1 << 20
GUARD = 64
POISON = 0xA5
H = T.SLICE_TREE_HEIGHT
SIZES = [1, 4_099, 999_999, 1_000_001, 4 * MiB, 0, 250_000, 2_300_000, 4 * MiB + 9]
WINDOW = 7 * MiB  # five windows: [0, 1, 2] [3] [4: oversize] [5, 6, 7] [8: oversize]
CUTS = [0, 3, 4, 5, 8, 9]

_CACHE = {}


def _objects(oracle):
    """The nine objects, built once and left unchanged: data, the oracle's slices and leaves, a
    survivor set, and the oracle's decode of the survivors (the expected output)."""
    if "objs" in _CACHE:
        return _CACHE["objs"]
    from oracle import merkle_oracle as MO
    o = oracle.OracleClay(N, K, 16)
    rng = random.Random(0x5EAD)
    sets = [list(range(K)),                      # all data chunks' slices of stripe 0
            list(range(N - K, N)),               # parity only: the worst case
            sorted(rng.sample(range(N), K)),     # random 7-of-20
            list(range(N)),                      # everything present
            sorted(rng.sample(range(N), K)),
            sorted(rng.sample(range(N), 9)),     # the empty blob, more than k present
            list(range(K)),
            sorted(rng.sample(range(N), K + 1)),
            list(range(N - K, N))]
    objs = []
    for i, L in enumerate(SIZES):
        data = oracle.splitmix64_bytes(0xD0 + i, L).tobytes()
        slices = oracle.slicer_encode(o, data)
        exp = oracle.slicer_decode(o, {j: slices[j] for j in sets[i]})
        assert exp == data
        objs.append({"len": L, "data": np.frombuffer(data, np.uint8), "slices": slices, "sl": len(slices[0]),
                     "leaves": MO.commit_slices(slices, H)[0], "present": sets[i],
                     "mask": sum(1 << j for j in sets[i]), "meta": slices[0][-48:]})
    _CACHE["objs"] = objs
    return objs


class Layout:
    """Host buffers of a batch: slices (absent slots poisoned), outputs with guard bands."""

    def __init__(self, objs, pinned=False, corrupt=()):
        self.objs = objs
        self.s_off, self.o_off, a, b = [], [], 0, GUARD
        for ob in objs:
            self.s_off.append(a)
            self.o_off.append(b)
            a += N * ob["sl"]
            b += ob["len"] + GUARD
        alloc = batch.host_empty if pinned else (lambda nbytes: np.empty(nbytes, np.uint8))
        self.slices = alloc(a)
        self.out = alloc(b)
        self.slices[:] = POISON
        self.out[:] = POISON
        for i, ob in enumerate(objs):
            for j in ob["present"]:
                at = self.s_off[i] + j * ob["sl"]
                self.slices[at:at + ob["sl"]] = np.frombuffer(ob["slices"][j], np.uint8)
        for i, j, byte in corrupt:  # flip one byte of slice j of object i
            at = self.s_off[i] + j * objs[i]["sl"] + (byte % objs[i]["sl"])
            self.slices[at] ^= 0x40
        self.descs = [(self.s_off[i], ob["sl"], ob["mask"], self.o_off[i]) for i, ob in enumerate(objs)]
        self.metas = b"".join(ob["meta"] for ob in objs)
        self.leaves = [ob["leaves"] for ob in objs]

    def check(self, untouched=(), only=None):
        """every decoded object exact, `untouched` objects' ranges and every guard still poisoned"""
        idx = range(len(self.objs)) if only is None else only
        for i in idx:
            ob, at = self.objs[i], self.o_off[i]
            got = self.out[at:at + ob["len"]]
            if i in untouched:
                assert (got == POISON).all(), ("an object that did not decode was written", i)
            else:
                assert np.array_equal(got, ob["data"]), ("decoded bytes differ from the oracle's", i)
            assert (self.out[at - GUARD:at] == POISON).all(), ("guard before object written", i)
            assert (self.out[at + ob["len"]:at + ob["len"] + GUARD] == POISON).all(), ("guard after object written", i)


def _present_bytes(objs, masks=None):
    masks = [ob["mask"] for ob in objs] if masks is None else masks
    return sum(bin(m).count("1") * ob["sl"] for ob, m in zip(objs, masks)), sum(bin(m).count("1") for m in masks)


@pytest.mark.parametrize("pinned", [False, True])
def test_batch_over_five_windows(oracle, pinned):
    """Nine objects over five windows (the ring of three slots wraps), pageable and page-locked
    buffers; bit-exact with the oracle and with te_decode_batch_device on the same inputs."""
    import torch
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    lay = Layout(objs, pinned=pinned)
    assert batch.decode_window_plan(s.coder, lay.descs, lay.metas, WINDOW) == CUTS
    batch.decode_host(s, lay.slices, lay.descs, lay.metas, lay.out, WINDOW)
    lay.check()
    st = batch.read_launch_stats(s.coder)
    nbytes, nslices = _present_bytes(objs)
    assert st == {"windows": 5, "objects": 9, "slices_uploaded": nslices, "bytes_h2d": nbytes,
                  "bytes_d2h": sum(SIZES), "slices_hashed_host": 0, "slices_hashed_device": 0, "host_waits": 0}
    # the device form on the same bytes
    d_out = torch.full((lay.out.size,), POISON, dtype=torch.uint8, device="cuda")
    batch.decode_batch(s, torch.from_numpy(np.asarray(lay.slices)).cuda(), lay.descs, lay.metas, d_out)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), np.asarray(lay.out))


@pytest.mark.parametrize("case", ["one_object", "oversize_alone", "window_zero", "empty_batch"])
def test_window_shapes(oracle, case):
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    pick, window, windows = {"one_object": ([3], WINDOW, 1),
                             "oversize_alone": ([1, 4, 0], 1 * MiB, 3),   # 4 MiB in a 1 MiB window
                             "window_zero": (list(range(9)), 0, 1),       # 0 = 128 MiB: one window
                             "empty_batch": ([], 0, 0)}[case]
    lay = Layout([objs[i] for i in pick])
    batch.decode_host(s, lay.slices, lay.descs, lay.metas, lay.out, window)
    lay.check()
    st = batch.read_launch_stats(s.coder)
    assert (st["windows"], st["objects"]) == (windows, len(pick))
    assert st["bytes_d2h"] == sum(objs[i]["len"] for i in pick)
    assert st["bytes_h2d"] == _present_bytes(lay.objs)[0]


def _verified_case(objs):
    """One corrupted slice in objects 3 (all 20 present) and 7 (8 present): both still decode.  One in
    object 1 (7 present): k - 1 good slices left, in a window with objects 0 and 2."""
    corrupt = [(3, 11, 0), (7, objs[7]["present"][2], -1), (1, 15, 333)]
    rejected = [0] * 9
    for i, j, _ in corrupt:
        rejected[i] = 1 << j
    status = [0] * 9
    status[1] = _lib.TE_ERR_NOT_ENOUGH_SLICES
    return corrupt, rejected, status


def test_verified_identical_in_every_hash_mode(oracle):
    """Corrupted slices are reported and left out, the outputs stay exact; an object left with k - 1
    good slices fails alone and its range is untouched.  Host, device and auto hashing give the same
    outputs, masks and statuses; the stats show where the hashing ran."""
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    corrupt, rejected, status = _verified_case(objs)
    nbytes, nslices = _present_bytes(objs)
    good = [ob["mask"] & ~r if not st else 0 for ob, r, st in zip(objs, rejected, status)]
    good_bytes, good_slices = _present_bytes(objs, good)
    seen = {}
    try:
        for mode in ("host", "device", "auto"):
            batch.set_commit_hashing(mode)
            lay = Layout(objs, corrupt=corrupt)
            got = batch.decode_verified_host(s, lay.slices, lay.descs, lay.metas, lay.leaves, lay.out, WINDOW)
            assert got == (status, rejected), mode
            lay.check(untouched={1})
            st = batch.read_launch_stats(s.coder)
            seen[mode] = np.asarray(lay.out).copy()
            assert (st["windows"], st["objects"], st["bytes_d2h"]) == (5, 9, sum(SIZES) - objs[1]["len"]), (mode, st)
            assert st["slices_hashed_host"] + st["slices_hashed_device"] == nslices, (mode, st)
            if mode == "host":
                # hashed where the slices lie; only the verified slices of objects that decode go up
                assert (st["slices_hashed_host"], st["host_waits"]) == (nslices, 0), st
                assert (st["slices_uploaded"], st["bytes_h2d"]) == (good_slices, good_bytes), st
            if mode == "device":
                # every present slice goes up and is hashed there: one host wait per window
                assert (st["slices_hashed_device"], st["host_waits"]) == (nslices, 5), st
                assert (st["slices_uploaded"], st["bytes_h2d"]) == (nslices, nbytes), st
            if mode == "auto":
                assert st["host_waits"] <= 5 and st["bytes_h2d"] in range(good_bytes, nbytes + 1), st
    finally:
        batch.set_commit_hashing("auto")
    assert np.array_equal(seen["host"], seen["device"]) and np.array_equal(seen["host"], seen["auto"])


@pytest.mark.parametrize("mode", ["host", "device"])
def test_verified_clean_pinned_bytes(oracle, mode):
    """Nothing corrupted, page-locked buffers: H2D bytes are the present slices', D2H bytes the
    objects', in both modes."""
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    lay = Layout(objs, pinned=True)
    nbytes, nslices = _present_bytes(objs)
    try:
        batch.set_commit_hashing(mode)
        got = batch.decode_verified_host(s, lay.slices, lay.descs, lay.metas, lay.leaves, lay.out, WINDOW)
    finally:
        batch.set_commit_hashing("auto")
    assert got == ([0] * 9, [0] * 9)
    lay.check()
    st = batch.read_launch_stats(s.coder)
    assert (st["bytes_h2d"], st["slices_uploaded"], st["bytes_d2h"]) == (nbytes, nslices, sum(SIZES)), st
    assert st["host_waits"] == (5 if mode == "device" else 0)


def _stream_windows(lay):
    return [(a, b, lay.descs[a:b], lay.metas[a * 48:b * 48], lay.leaves[a:b]) for a, b in ((0, 3), (3, 5), (5, 8), (8, 9))]


def _run_reader(oracle, slicers, mode):
    objs = _objects(oracle)
    corrupt, rejected, status = _verified_case(objs)
    lay = Layout(objs, pinned=True, corrupt=corrupt)
    try:
        batch.set_commit_hashing(mode)  # a reader copies the mode when it is created
        rd = batch.StreamReader(slicers)
    finally:
        batch.set_commit_hashing("auto")
    wins = _stream_windows(lay)
    tickets = [rd.submit(lay.slices, d, m, lay.out, leaves=lv) for _, _, d, m, lv in wins]
    assert tickets == [1, 2, 3, 4]
    res = rd.wait(2)  # completes windows 1 and 2, in order; 3 and 4 may still be in flight
    assert sorted(res) == [1, 2]
    for t in (1, 2):
        a, b = wins[t - 1][:2]
        assert res[t] == (status[a:b], rejected[a:b])
    lay.check(untouched={1}, only=range(0, 5))
    res = rd.wait(4)
    assert sorted(res) == [3, 4]
    for t in (3, 4):
        a, b = wins[t - 1][:2]
        assert res[t] == (status[a:b], rejected[a:b])
    lay.check(untouched={1})
    # the pipeline persists across waits: an unverified window, then free with it still in flight
    lay2 = Layout(objs[2:5], pinned=True)
    t = rd.submit(lay2.slices, lay2.descs, lay2.metas, lay2.out)
    assert t == 5
    rd.close()  # waits for everything
    lay2.check()
    return rd


@pytest.mark.parametrize("mode", ["host", "device"])
def test_stream_reader_windows_in_order(oracle, mode):
    _run_reader(oracle, [T.Slicer.clay_default()], mode)


@pytest.mark.skipif(T.device_count() < 2, reason="needs two HIP devices")
def test_stream_reader_two_devices(oracle):
    s0, s1 = T.Slicer.clay_default(), T.Slicer.clay_default()
    s1.coder.bind_device(1)
    _run_reader(oracle, [s0, s1], "auto")


def test_stream_reader_errors(oracle):
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    rd = batch.StreamReader([s])
    with pytest.raises(T.EngineError):
        rd.wait(1)  # never submitted
    lay = Layout(objs[:2])
    bad = [lay.descs[0], (lay.descs[1][0], lay.descs[1][1], 0x3F, lay.descs[1][3])]
    with pytest.raises(T.DecodeError):
        rd.submit(lay.slices, bad, lay.metas, lay.out)  # unverified and too few slices: no ticket
    assert rd.submit(lay.slices, lay.descs, lay.metas, lay.out) == 1
    rd.wait(1)
    lay.check()
    rd.close()
