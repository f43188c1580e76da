"""The node rebuild pipeline on the device: te_repair_batch_host and te_recover_batch_host against
the CPU oracle's encoded slice `lost` of each object, and against te_repair_batch_device /
te_recover_batch_device on the same inputs.

24 objects of mixed length (the empty blob, 1 B, sub-chunks below 8 B for the generic kernel, the
20 KB sub-chunk-30 B shape, short last stripes, three 4 MiB objects); object i loses slice i mod 20,
so every index occurs.  Host buffers carry a poison pattern in every byte the engine must not read
into a result or write."""
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib, batch
from tape_amd._lib import lib

pytestmark = pytest.mark.gpu
N, K = 20, 7
MiB = 1 << 20
GUARD = 64
POISON = 0xA5
H = T.SLICE_TREE_HEIGHT
SIZES = [0, 1, 1_000, 20_000, 1_000_001, 4 * MiB, 2_300_000, 700, 4 * MiB, 20_000, 333, 250_000,
         1, 4_099, 20_000, 999_999, 3_000, 4 * MiB, 0, 20_000, 64_000, 5, 1_000_001, 123_456]
WINDOW = MiB  # a 4 MiB object (16 fragments + 1 slice = ~1.8 MB; 8 slices = ~4.8 MB) is above it
MODES = ("host", "device", "auto")
_CACHE = {}


def _objects(oracle):
    """Built once and left unchanged: per object the oracle's slices and leaves, the lost index."""
    if "objs" in _CACHE:
        return _CACHE["objs"]
    from oracle import merkle_oracle as MO
    o = oracle.OracleClay(N, K, 16)
    s = T.Slicer.clay_default()
    objs = []
    for i, L in enumerate(SIZES):
        data = oracle.splitmix64_bytes(0xE0 + i, L).tobytes()
        slices = oracle.slicer_encode(o, data)
        objs.append({"len": L, "slices": slices, "sl": len(slices[0]), "leaves": MO.commit_slices(slices, H)[0],
                     "lost": i % N, "meta": slices[0][-48:], "geo": s.geometry(L)})
    assert len(objs) == 24 and {ob["lost"] for ob in objs} == set(range(N))
    sc = [int(ob["geo"].sub_chunk_size) for ob in objs]
    assert sc[2] < 8 and sc[3] == 30 and min(sc[5], sc[8], sc[17]) >= 8  # generic, the 30 B shape, staged / folded
    g = objs[4]["geo"]  # a short last stripe
    assert int(g.num_stripes) > 1 and objs[4]["len"] % int(g.stripe_size) not in (0, int(g.stripe_size))
    assert all(ob["sl"] % 4 == 0 for ob in objs)  # no Clay(20,7,16) slice length is odd: out_off is used instead
    _CACHE["objs"] = objs
    return objs


def _alloc(pinned, nbytes):
    buf = batch.host_empty(nbytes) if pinned else np.empty(nbytes, np.uint8)
    buf[:] = POISON
    return buf


class RepairLayout:
    """Fragments packed in a host buffer (a poisoned gap before each object's), outputs with guard
    bands; odd objects have slice lost + 10 down too.  `shift`: out_off of that object is odd."""

    def __init__(self, objs, pinned=False, corrupt=(), shift=None):
        s = T.Slicer.clay_default()
        self.objs, self.plans, self.descs, self.o_off, self.frag = objs, [], [], [], []
        blobs, cur, b = [], 0, GUARD
        for i, ob in enumerate(objs):
            lost = ob["lost"]
            avail = [j for j in range(N) if j != lost and not (i % 2 and j == (lost + 10) % N)]
            p = s.repair_plan(lost, avail, ob["slices"][avail[0]])
            offs = {lost: 1 << 50}  # not a helper of the plan: ignored
            blobs.append(bytes([POISON]) * 16)
            cur += 16
            for h in avail:
                d = T.extract_repair_data(ob["slices"][h], p, h)
                if d:
                    offs[h] = cur
                    self.frag.append((i, cur, len(d)))
                    blobs.append(d)
                    cur += len(d)
            at = b + (1 if shift == i else 0)
            self.plans.append(p)
            self.o_off.append(at)
            self.descs.append((p, offs, at, ob["meta"]))
            b = (at + ob["sl"] + GUARD + 3) & ~3  # only the shifted object is unaligned
        self.helpers = _alloc(pinned, cur)
        self.helpers[:] = np.frombuffer(b"".join(blobs), np.uint8)
        for i, byte in corrupt:  # flip one byte of one fragment of object i
            mine = [f for f in self.frag if f[0] == i]
            _, at, ln = mine[byte % len(mine)]
            self.helpers[at + byte % ln] ^= 0x20
        self.out = _alloc(pinned, b)
        self.frag_bytes = sum(f[2] for f in self.frag)
        self.arr = batch.repair_descs(self.descs)
        self.leaves = [ob["leaves"] for ob in objs]

    def check(self, wrong=()):
        for i, ob in enumerate(self.objs):
            at = self.o_off[i]
            got = self.out[at:at + ob["sl"]].tobytes()
            if i in wrong:
                assert got != ob["slices"][ob["lost"]] and got[-48:] == ob["meta"], i
            else:
                assert got == ob["slices"][ob["lost"]], ("repaired slice differs from the oracle's", i)
            assert (self.out[at - GUARD + 1:at] == POISON).all() and \
                (self.out[at + ob["sl"]:at + ob["sl"] + GUARD - 1] == POISON).all(), ("guard written", i)


def _masks(objs):
    """Survivor sets from a fixed seed: the first eight with exactly 7 peers of which a0 = 0..7 hold a
    column-0 shard of stripe 0, the others random 7-to-12-of-20."""
    rng = random.Random(0xC1A7)
    out = []
    for i, ob in enumerate(objs):
        others = [j for j in range(N) if j != ob["lost"]]
        if i < 8:
            col0 = [j for j in others if lib.te_slice_to_shard(1, N, 0, j) < 10]
            col1 = [j for j in others if j not in col0]
            pick = rng.sample(col0, i) + rng.sample(col1, K - i)
            assert sum(1 for j in pick if lib.te_slice_to_shard(1, N, 0, j) < 10) == i
        else:
            pick = rng.sample(others, rng.randint(K, 12))
        out.append(sorted(pick))
    return out


class RecoverLayout:
    """n slots per object in a host buffer, absent slots poisoned; outputs with guard bands."""

    def __init__(self, objs, present, pinned=False, corrupt=()):
        self.objs, self.present = objs, present
        self.s_off, self.o_off, a, b = [], [], 0, GUARD
        for ob in objs:
            self.s_off.append(a)
            self.o_off.append(b)
            a += N * ob["sl"]
            b += ob["sl"] + GUARD
        self.slices = _alloc(pinned, a)
        self.out = _alloc(pinned, b)
        for i, ob in enumerate(objs):
            for j in present[i]:
                at = self.s_off[i] + j * ob["sl"]
                self.slices[at:at + ob["sl"]] = np.frombuffer(ob["slices"][j], np.uint8)
        for i, j, byte in corrupt:  # flip one byte of slice j of object i
            self.slices[self.s_off[i] + j * objs[i]["sl"] + byte % objs[i]["sl"]] ^= 0x40
        self.descs = [(self.s_off[i], ob["sl"], sum(1 << j for j in present[i]), ob["lost"], self.o_off[i])
                      for i, ob in enumerate(objs)]
        self.metas = b"".join(ob["meta"] for ob in objs)
        self.leaves = [ob["leaves"] for ob in objs]

    def check(self, untouched=()):
        for i, ob in enumerate(self.objs):
            at = self.o_off[i]
            got = self.out[at:at + ob["sl"]]
            if i in untouched:
                assert (got == POISON).all(), ("an object that was not rebuilt was written", i)
            else:
                assert got.tobytes() == ob["slices"][ob["lost"]], ("rebuilt slice differs from the oracle's", i)
            assert (self.out[at - GUARD:at] == POISON).all() and \
                (self.out[at + ob["sl"]:at + ob["sl"] + GUARD] == POISON).all(), ("guard written", i)


@pytest.mark.parametrize("pinned", [False, True])
def test_repair_over_windows(oracle, pinned):
    import torch
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    lay = RepairLayout(objs, pinned=pinned)
    cuts = batch.repair_window_plan(s.coder, lay.arr, WINDOW)
    assert len(cuts) - 1 >= 5 and any(b - a == 1 and a in (5, 8, 17) for a, b in zip(cuts, cuts[1:]))
    assert batch.repair_host(s.coder, lay.helpers, lay.arr, lay.out, window_bytes=WINDOW) is None
    lay.check()
    st = batch.rebuild_launch_stats(s.coder)
    assert st["windows"] == len(cuts) - 1 and st["objects"] == len(objs)
    assert st["bytes_h2d"] == lay.frag_bytes and st["pieces_uploaded"] == len(lay.frag)
    assert st["bytes_d2h"] == sum(ob["sl"] for ob in objs)
    assert st["slices_hashed_host"] == st["slices_hashed_device"] == 0
    ks = s.coder.repair_launch_stats()  # summed over the windows: folded, staged and generic kernels all ran
    assert ks["fold_stripes"] + ks["stage_stripes"] + ks["generic_stripes"] == sum(int(ob["geo"].num_stripes) for ob in objs)
    assert ks["generic_launches"] >= 1 and ks["fold_launches"] >= 3
    first = lay.out.copy()
    lay.out[:] = POISON
    batch.repair_host(s.coder, lay.helpers, lay.arr, lay.out, window_bytes=0)  # one window
    lay.check()
    assert np.array_equal(first, lay.out)
    assert batch.rebuild_launch_stats(s.coder)["windows"] == 1
    if pinned:  # the device call on the same inputs
        d_out = torch.full((len(lay.out),), POISON, dtype=torch.uint8, device="cuda")
        batch.repair_batch(s.coder, torch.from_numpy(np.asarray(lay.helpers).copy()).cuda(), lay.arr, d_out)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), lay.out)


@pytest.mark.parametrize("pinned", [False, True])
def test_verified_repair_every_mode(oracle, pinned):
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    bad = (3, 8, 21)
    lay = RepairLayout(objs, pinned=pinned, corrupt=[(3, 7), (8, 123_457), (21, 2)], shift=13)
    cuts = batch.repair_window_plan(s.coder, lay.arr, WINDOW)
    odd = next(b - a for a, b in zip(cuts, cuts[1:]) if a <= 13 < b)  # the window with the odd out_off
    got = {}
    try:
        for mode in MODES:
            batch.set_commit_hashing(mode)
            lay.out[:] = POISON
            ok = batch.repair_host(s.coder, lay.helpers, lay.arr, lay.out, leaves=lay.leaves, window_bytes=WINDOW)
            assert ok == [0 if i in bad else 1 for i in range(len(objs))], mode
            lay.check(wrong=bad)
            st = batch.rebuild_launch_stats(s.coder)
            assert st["slices_hashed_host"] + st["slices_hashed_device"] == len(objs), (mode, st)
            if mode == "host":
                assert st["slices_hashed_device"] == 0
            if mode == "device":  # only the unaligned window falls back to the host
                assert st["slices_hashed_host"] == odd and st["slices_hashed_device"] == len(objs) - odd, st
            got[mode] = (ok, lay.out.copy())
    finally:
        batch.set_commit_hashing("auto")
    for mode in MODES[1:]:
        assert got[mode][0] == got["host"][0] and np.array_equal(got[mode][1], got["host"][1]), mode


@pytest.mark.parametrize("pinned", [False, True])
def test_recover_over_windows(oracle, pinned):
    import torch
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    present = _masks(objs)
    assert any(ob["lost"] < K for ob in objs) and any(ob["lost"] >= K for ob in objs)  # data and parity slices
    lay = RecoverLayout(objs, present, pinned=pinned)
    cuts = batch.recover_window_plan(s.coder, lay.descs, WINDOW)
    assert len(cuts) - 1 >= 5
    assert batch.recover_host(s, lay.slices, lay.descs, lay.metas, lay.out, window_bytes=WINDOW) is None
    lay.check()
    st = batch.rebuild_launch_stats(s.coder)
    assert st["windows"] == len(cuts) - 1 and st["objects"] == len(objs)
    assert st["pieces_uploaded"] == sum(len(p) for p in present)
    assert st["bytes_h2d"] == sum(len(p) * ob["sl"] for p, ob in zip(present, objs))
    assert st["bytes_d2h"] == sum(ob["sl"] for ob in objs)
    # the unverified form leaves h_ok and h_rejected_mask alone, and reports TE_OK where h_status is given
    import ctypes as C
    n = len(objs)
    ok, rej, stat = (C.c_uint32 * n)(*[7] * n), (C.c_uint32 * n)(*[9] * n), (C.c_int * n)(*[5] * n)
    cfg = s._cfg()
    mb = (C.c_uint8 * len(lay.metas)).from_buffer_copy(lay.metas)
    lay.out[:] = POISON
    assert lib.te_recover_batch_host(s.coder.handle, C.byref(cfg), C.c_void_p(lay.slices.ctypes.data),
                                     batch.recover_descs(lay.descs), mb, None, n, C.c_void_p(lay.out.ctypes.data),
                                     rej, ok, stat, WINDOW) == 0
    lay.check()
    assert list(ok) == [7] * n and list(rej) == [9] * n and list(stat) == [0] * n
    if pinned:  # the device call on the same inputs
        d_out = torch.full((len(lay.out),), POISON, dtype=torch.uint8, device="cuda")
        batch.recover_batch(s, torch.from_numpy(np.asarray(lay.slices).copy()).cuda(), lay.descs, lay.metas, d_out)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), lay.out)


@pytest.mark.parametrize("pinned", [False, True])
def test_verified_recover_every_mode(oracle, pinned):
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    present = _masks(objs)
    # object 10 is given at least 9 peers and keeps k after one corrupted peer; objects 2 and 5 have
    # exactly 7 peers, so one corrupted peer leaves 6 verified
    present[10] = sorted(set(present[10]) | set([j for j in range(N) if j != objs[10]["lost"]][:9]))
    corrupt = [(10, present[10][2], 77), (2, present[2][0], 5), (5, present[5][6], 1_000_000)]
    short = (2, 5)
    lay = RecoverLayout(objs, present, pinned=pinned, corrupt=corrupt)
    got = {}
    try:
        for mode in MODES:
            batch.set_commit_hashing(mode)
            lay.out[:] = POISON
            status, rej, ok = batch.recover_host(s, lay.slices, lay.descs, lay.metas, lay.out, leaves=lay.leaves,
                                                 window_bytes=WINDOW)
            assert status == [_lib.TE_ERR_NOT_ENOUGH_SLICES if i in short else _lib.TE_OK for i in range(len(objs))], mode
            want_rej = [0] * len(objs)
            for i, j, _ in corrupt:
                want_rej[i] = 1 << j
            assert rej == want_rej, mode
            assert ok == [0 if i in short else 1 for i in range(len(objs))], mode
            lay.check(untouched=short)
            st = batch.rebuild_launch_stats(s.coder)
            if mode == "host":  # only the verified slices of objects that rebuild go up
                assert st["slices_hashed_device"] == 0
                assert st["pieces_uploaded"] == sum(len(p) for i, p in enumerate(present) if i not in short) - 1
            if mode == "device":
                assert st["slices_hashed_host"] == 0 and st["host_waits"] >= st["windows"]
                assert st["slices_hashed_device"] == sum(len(p) for p in present) + len(objs) - len(short)
            got[mode] = (status, rej, ok, lay.out.copy())
    finally:
        batch.set_commit_hashing("auto")
    for mode in MODES[1:]:
        assert got[mode][:3] == got["host"][:3] and np.array_equal(got[mode][3], got["host"][3]), mode


def test_back_to_back_calls_share_slots_and_arenas(oracle):
    """Each batch call twice in a row on one handle, then a host read: the slots, the descriptor
    arenas and the streams are shared."""
    objs = _objects(oracle)
    s = T.Slicer.clay_default()
    rep = RepairLayout(objs)
    rec = RecoverLayout(objs, _masks(objs))
    for _ in range(2):
        rep.out[:] = POISON
        ok = batch.repair_host(s.coder, rep.helpers, rep.arr, rep.out, leaves=rep.leaves, window_bytes=WINDOW)
        assert ok == [1] * len(objs)
        rep.check()
    for _ in range(2):
        rec.out[:] = POISON
        status, rej, ok = batch.recover_host(s, rec.slices, rec.descs, rec.metas, rec.out, leaves=rec.leaves,
                                             window_bytes=WINDOW)
        assert status == [0] * len(objs) and rej == [0] * len(objs) and ok == [1] * len(objs)
        rec.check()
    sub = [4, 5, 3, 0, 8]
    descs, a = [], 0
    for i in sub:
        descs.append((rec.s_off[i], objs[i]["sl"], sum(1 << j for j in rec.present[i]), a))
        a += objs[i]["len"]
    out = np.full(a + 1, POISON, np.uint8)
    batch.decode_host(s, rec.slices, descs, b"".join(objs[i]["meta"] for i in sub), out, 3 * MiB)
    want = b"".join(oracle.splitmix64_bytes(0xE0 + i, objs[i]["len"]).tobytes() for i in sub)
    assert out[:a].tobytes() == want and out[a] == POISON
