"""The verified and pipelined forms of the multi-slice rebuild on the device:
te_recover_multi_verified_batch_device and te_recover_multi_batch_host against the CPU oracle's
Slicer::encode, bit for bit, and their masks and statuses against the oracle's leaves.

test_gpu_recover_multi.py's method and geometry: every call writes into a buffer pre-filled with
0xA5 that is compared whole with the expected image, the slices a call may not read are poisoned in
its input; Clay(20,7,16) objects of 20,000 / 300,000 / 250,001 bytes (one stripe of 30-byte
sub-chunks, three full stripes, a short last stripe) in rotated and identity layouts, and one pair
of 4 MiB objects for the 1,430-byte sub-chunk."""
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib, batch

pytestmark = pytest.mark.gpu
N, K, POISON, ABSENT, GUARD = 20, 7, 0xA5, 0x3C, 64
MiB = 1024 * 1024
H = T.SLICE_TREE_HEIGHT
SMALL = (20_000, 300_000, 250_001)
MODES = ("host", "device", "auto")
NOT_ENOUGH = _lib.TE_ERR_NOT_ENOUGH_SLICES

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    batch.set_commit_hashing("auto")
    _cache.clear()


def _slicer(rotated):
    key = ("slicer", rotated)
    if key not in _cache:
        _cache[key] = T.Slicer.clay_default() if rotated else T.Slicer.new(T.ClayCoder(20, 7, 16))
    return _cache[key]


def _leaves(sl):
    from oracle import merkle_oracle as MO
    return b"".join(bytes(h) for h in MO.commit_slices([x.tobytes() for x in sl], H)[0])


def _objects(oracle, rotated, lens):
    """Oracle-encoded objects and their leaves, made once per (layout, lengths) and left unchanged:
    ((n, slice_len) array, n * 32 bytes of leaves) each."""
    key = ("objs", rotated, lens)
    if key not in _cache:
        o = oracle.OracleClay(20, 7, 16)
        out = []
        for ln in lens:
            sl = oracle.slicer_encode_np(o, oracle.splitmix64_bytes(0x70697065 ^ ln ^ int(rotated), ln) if ln
                                         else np.zeros(0, np.uint8), rotated=rotated)
            out.append((sl, _leaves(sl)))
        _cache[key] = out
    return _cache[key]


def _generic_object(oracle):
    """A Clay(12,8,11) object: no plane programs, so the decode + re-encode path."""
    key = ("generic",)
    if key not in _cache:
        sl = oracle.slicer_encode(oracle.OracleClay(12, 8, 11), oracle.splitmix64_bytes(0x12811, 250_001).tobytes(), rotated=True)
        sl = np.stack([np.frombuffer(x, np.uint8) for x in sl])
        _cache[key] = (sl, _leaves(sl))
    return _cache[key]


def _bits(xs):
    return sum(1 << i for i in xs)


class Layout:
    """specs = [(object, avail, lost)] laid out as one call's buffers.  corrupt: {spec index: peer
    slice} gets a flipped byte; wrong_leaf: {spec index: lost slice} gets a leaf that cannot match;
    dead: the spec indices that must not rebuild (their output range stays poison)."""

    def __init__(self, objs, specs, n=N, corrupt=None, wrong_leaf=None, dead=(), misalign=0):
        corrupt, wrong_leaf = corrupt or {}, wrong_leaf or {}
        ins, self.descs, self.metas, leaves, exp = [], [], b"", [], [np.full(GUARD + misalign, POISON, np.uint8)]
        in_at, out_at = 0, GUARD + misalign
        for x, (oi, avail, lost) in enumerate(specs):
            sl, lv = objs[oi]
            slen = sl.shape[1]
            img = np.full_like(sl, ABSENT)  # what is not available is never what the call needs
            for i in avail:
                img[i] = sl[i]
            if x in corrupt:
                img[corrupt[x], slen // 2] ^= 0x10
            ins.append(img.reshape(-1))
            lost = sorted(lost)
            self.descs.append((in_at, slen, _bits(avail), _bits(lost), out_at))
            self.metas += sl[avail[0]][-48:].tobytes()
            lv = bytearray(lv)
            if x in wrong_leaf:
                lv[wrong_leaf[x] * 32] ^= 0xFF
            leaves.append(bytes(lv))
            for i in lost:
                exp.append(np.full(slen, POISON, np.uint8) if x in dead else sl[i])
            gap = np.full(GUARD, POISON, np.uint8)  # slice lengths are multiples of 4: every out_off keeps `misalign`
            exp.append(gap)
            in_at += sl.size
            out_at += len(lost) * slen + gap.size
        self.exp = np.concatenate(exp)
        self.src = np.concatenate(ins)
        self.leaves = b"".join(leaves)
        self.lost = [d[3] for d in self.descs]
        assert len(self.leaves) == len(specs) * n * 32

    def host(self, pinned):
        src = batch.host_empty(self.src.size) if pinned else np.empty(self.src.size, np.uint8)
        src[:] = self.src
        out = batch.host_empty(self.exp.size) if pinned else np.empty(self.exp.size, np.uint8)
        out[:] = POISON
        return src, out


def _same(got, exp, what):
    if np.array_equal(got, exp):
        return
    at = int(np.nonzero(got != exp)[0][0])
    raise AssertionError(f"{what}: first mismatch at byte {at} of {exp.size}: got {int(got[at]):#x}, expected {int(exp[at]):#x}")


def _device_call(s, lay):
    import torch
    d_in = torch.from_numpy(lay.src).cuda()
    d_out = torch.full((lay.exp.size,), POISON, dtype=torch.uint8, device="cuda")
    res = batch.recover_multi_verified_batch(s, d_in, lay.descs, lay.metas, lay.leaves, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), res


LOST_SETS = {
    "column0_pair": ([0, 2, 3, 10, 11, 12, 13], [1, 4]),
    "data_and_parity_across": ([0, 1, 3, 4, 5, 10, 11], [2, 15]),
    "all_13": ([0, 3, 5, 9, 11, 14, 18], [i for i in range(N) if i not in (0, 3, 5, 9, 11, 14, 18)]),
    "ten_available_three_lost": ([0, 1, 2, 3, 4, 10, 11, 12, 13, 14], [5, 15, 19]),
}


# ---- 1. the verified device form ----
@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "identity"])
@pytest.mark.parametrize("case", list(LOST_SETS))
def test_verified_device_lost_sets(oracle, rotated, case):
    s, objs = _slicer(rotated), _objects(oracle, rotated, SMALL)
    avail, lost = LOST_SETS[case]
    lay = Layout(objs, [(i, avail, lost) for i in range(len(SMALL))])
    got, (status, rej, ok) = _device_call(s, lay)
    _same(got, lay.exp, case)
    assert status == [0, 0, 0] and rej == [0, 0, 0] and ok == lay.lost
    st = batch.recover_multi_launch_stats(s.coder)
    assert (st["multi_objects"], st["single_objects"], st["generic_objects"]) == (3, 0, 0), st
    if case == "all_13":
        assert st["passes"] >= 2 and st["split_stripes"] == st["stripes"] == 7, st


def test_verified_device_corrupted_peer_among_ten(oracle):
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    avail, lost = LOST_SETS["ten_available_three_lost"]
    lay = Layout(objs, [(i, avail, lost) for i in range(len(SMALL))], corrupt={1: 3, 2: 14})
    got, (status, rej, ok) = _device_call(s, lay)
    _same(got, lay.exp, "one bad peer of ten")
    assert status == [0, 0, 0] and rej == [0, 1 << 3, 1 << 14] and ok == lay.lost


def test_verified_device_corrupted_peer_among_seven(oracle):
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    avail, lost = LOST_SETS["data_and_parity_across"]
    lay = Layout(objs, [(i, avail, lost) for i in range(len(SMALL))], corrupt={1: 10}, dead={1})
    got, (status, rej, ok) = _device_call(s, lay)
    _same(got, lay.exp, "six verified peers")  # the object's output range is untouched
    assert status == [0, NOT_ENOUGH, 0] and rej == [0, 1 << 10, 0] and ok == [lay.lost[0], 0, lay.lost[2]]


def test_verified_device_wrong_leaf_clears_one_bit(oracle):
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    avail, lost = LOST_SETS["ten_available_three_lost"]
    lay = Layout(objs, [(i, avail, lost) for i in range(len(SMALL))], wrong_leaf={2: 15})
    got, (status, rej, ok) = _device_call(s, lay)
    _same(got, lay.exp, "wrong leaf")  # the bytes are written either way
    assert status == [0, 0, 0] and rej == [0, 0, 0]
    assert ok == [lay.lost[0], lay.lost[1], lay.lost[2] & ~(1 << 15)]


# ---- 2. the host form over windows ----
def _mixed_specs():
    """One lost slice, a pair, thirteen, an empty blob, ten available with a bad peer, seven with a
    bad peer (verified: too few), another pair; objects index _objects(..., SMALL + (0,))."""
    a13, l13 = LOST_SETS["all_13"]
    a10, l10 = LOST_SETS["ten_available_three_lost"]
    a2, l2 = LOST_SETS["data_and_parity_across"]
    return [(0, [1, 2, 3, 4, 5, 6, 7], [0]), (1, *LOST_SETS["column0_pair"]), (2, a13, l13), (3, [0, 1, 2, 3, 4, 5, 6], [7, 19]),
            (1, a10, l10), (2, a2, l2), (0, a2, l2), (1, a13, [1, 2])]


WINDOW = 400_000  # a 300,000-byte object's nine slices are ~387 KB


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("verified", [True, False], ids=["verified", "unverified"])
def test_host_windows_every_mode(oracle, pinned, verified):
    s, objs = _slicer(True), _objects(oracle, True, SMALL + (0,))
    specs = _mixed_specs()
    if verified:
        lay = Layout(objs, specs, corrupt={4: 12, 5: 4}, dead={5})
        want = ([0, 0, 0, 0, 0, NOT_ENOUGH, 0, 0], [0, 0, 0, 0, 1 << 12, 1 << 4, 0, 0],
                [m if x != 5 else 0 for x, m in enumerate(lay.lost)])
    else:
        lay = Layout(objs, specs)
    cuts = batch.recover_multi_window_plan(s.coder, lay.descs, WINDOW)
    assert len(cuts) - 1 >= 4, cuts  # slot 0 is used again
    try:
        for mode in MODES:
            batch.set_commit_hashing(mode)
            src, out = lay.host(pinned)
            res = batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves if verified else None,
                                                 window_bytes=WINDOW)
            _same(out, lay.exp, f"{mode}")
            assert np.array_equal(src, lay.src)
            assert res == (want if verified else None), mode
            rb, st = batch.rebuild_launch_stats(s.coder), batch.recover_multi_launch_stats(s.coder)
            assert rb["windows"] == len(cuts) - 1 and rb["objects"] == len(specs), rb
            ran = len(specs) - (1 if verified else 0)
            assert (st["single_objects"], st["multi_objects"], st["generic_objects"]) == (2, ran - 2, 0), st
            assert st["multi_launches"] >= 4 and st["passes"] >= 2, st
            if verified and mode == "device":
                assert rb["slices_hashed_device"] > 0 and rb["slices_hashed_host"] == 0, rb
            if not verified or mode == "host":
                assert rb["slices_hashed_device"] == 0, rb
    finally:
        batch.set_commit_hashing("auto")


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_host_generic_path_other_profile(oracle, pinned):
    obj = _generic_object(oracle)
    s = T.Slicer.with_profile(T.ClayCoder(12, 8, 11), T.STRIPE_SIZES[0], True, T.EncodingProfile.clay_default())
    specs = [(0, [0, 1, 2, 4, 5, 7, 8, 10, 11], [3, 9]), (0, [0, 1, 2, 3, 4, 5, 6, 7, 8], [9, 10, 11])]
    lay = Layout([obj], specs, n=12, corrupt={0: 11})
    try:
        for mode in MODES:
            batch.set_commit_hashing(mode)
            src, out = lay.host(pinned)
            res = batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves, window_bytes=1)
            _same(out, lay.exp, f"Clay(12,8,11) {mode}")
            assert res == ([0, 0], [1 << 11, 0], lay.lost), mode
            st = batch.recover_multi_launch_stats(s.coder)
            assert (st["generic_objects"], st["multi_objects"], st["single_objects"], st["multi_launches"]) == (2, 0, 0, 0), st
            assert batch.rebuild_launch_stats(s.coder)["windows"] == 2
    finally:
        batch.set_commit_hashing("auto")


def test_host_odd_out_off_hashes_on_the_host(oracle):
    s, objs = _slicer(True), _objects(oracle, True, SMALL + (0,))
    lay = Layout(objs, _mixed_specs(), corrupt={4: 12, 5: 4}, dead={5}, misalign=1)
    assert all(d[4] % 4 for d in lay.descs)
    try:
        batch.set_commit_hashing("device")
        src, out = lay.host(True)
        res = batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves, window_bytes=WINDOW)
    finally:
        batch.set_commit_hashing("auto")
    _same(out, lay.exp, "odd out_off")
    assert res == ([0, 0, 0, 0, 0, NOT_ENOUGH, 0, 0], [0, 0, 0, 0, 1 << 12, 1 << 4, 0, 0],
                   [m if x != 5 else 0 for x, m in enumerate(lay.lost)])
    rb = batch.rebuild_launch_stats(s.coder)
    assert rb["slices_hashed_host"] > 0 and rb["slices_hashed_device"] == 0, rb


# ---- 3. the survivors go up once ----
@pytest.mark.parametrize("verified", [True, False], ids=["verified", "unverified"])
def test_upload_counters_against_the_single_slice_call(oracle, verified):
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    rnd = random.Random(3)
    L = 4
    specs = []
    for i in range(6):
        avail = sorted(rnd.sample(range(N), 7 + i % 3))
        specs.append((i % 3, avail, sorted(rnd.sample([j for j in range(N) if j not in avail], L))))
    lay = Layout(objs, specs)
    src, out = lay.host(True)
    batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves if verified else None,
                                   window_bytes=WINDOW)
    _same(out, lay.exp, "multi")
    multi = batch.rebuild_launch_stats(s.coder)
    # the existing entry point: the same objects and survivors, the first lost slice of each
    single_descs = [(d[0], d[1], d[2], sp[2][0], d[4]) for d, sp in zip(lay.descs, specs)]
    out1 = batch.host_empty(lay.exp.size)
    out1[:] = POISON
    batch.recover_host(s, src, single_descs, lay.metas, out1, leaves=lay.leaves if verified else None, window_bytes=WINDOW)
    single = batch.rebuild_launch_stats(s.coder)
    for d, sp in zip(lay.descs, specs):
        assert np.array_equal(out1[d[4]:d[4] + d[1]], objs[sp[0]][0][sp[2][0]])
    assert single["pieces_uploaded"] > 0 and single["bytes_d2h"] > 0
    assert multi["bytes_h2d"] == single["bytes_h2d"] and multi["pieces_uploaded"] == single["pieces_uploaded"], (multi, single)
    assert multi["bytes_d2h"] == L * single["bytes_d2h"], (multi, single)


# ---- 4. the production sub-chunk ----
def test_host_production_sub_chunk(oracle):
    s, objs = _slicer(True), _objects(oracle, True, (4 * MiB, 4 * MiB - 5))
    assert s.geometry(4 * MiB).sub_chunk_size == 1430
    rnd = random.Random(4)
    specs = []
    for i in range(2):
        avail = sorted(rnd.sample(range(N), 7))
        specs.append((i, avail, sorted(rnd.sample([j for j in range(N) if j not in avail], 4))))
    lay = Layout(objs, specs)
    src, out = lay.host(True)
    res = batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves)
    _same(out, lay.exp, "4 MiB")
    assert res == ([0, 0], [0, 0], lay.lost)
    rb, st = batch.rebuild_launch_stats(s.coder), batch.recover_multi_launch_stats(s.coder)
    ns = int(s.geometry(4 * MiB).num_stripes)
    assert rb["windows"] == 1 and st["multi_objects"] == 2 and st["stripes"] == 2 * ns, (rb, st)
    assert st["out_rows"] == 2 * ns * 4 * 100, st


# ---- 5. back-to-back calls on one handle ----
def test_back_to_back_calls_share_slots_and_programs(oracle):
    s, objs = _slicer(False), _objects(oracle, False, SMALL)
    rnd = random.Random(5)
    specs = []
    for i in range(6):
        avail = sorted(rnd.sample(range(N), 7))
        specs.append((i % 3, avail, sorted(rnd.sample([j for j in range(N) if j not in avail], 2 + i))))
    lay = Layout(objs, specs)
    src, out = lay.host(False)
    batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves, window_bytes=WINDOW)
    _same(out, lay.exp, "first call")
    store, first = s.coder.decode_store_stats(), batch.recover_multi_launch_stats(s.coder)
    assert store["used"] > 0
    src, out = lay.host(False)
    res = batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out, leaves=lay.leaves, window_bytes=WINDOW)
    _same(out, lay.exp, "second call")
    assert res == ([0] * 6, [0] * 6, lay.lost)
    assert s.coder.decode_store_stats() == store  # every program was there: none compiled, none uploaded
    assert batch.recover_multi_launch_stats(s.coder) == first


# ---- 6. Slicer.recover_many(leaves=...) ----
def test_recover_many_with_leaves(oracle):
    from oracle import merkle_oracle as MO
    s = _slicer(True)
    data = oracle.splitmix64_bytes(99, 123_457).tobytes()
    sl = s.encode(data)
    leaves = MO.commit_slices(sl, H)[0]
    avail = [0, 4, 5, 9, 10, 16, 18, 19]
    peers = [(i, sl[i]) for i in avail]
    got, ok, rej = s.recover_many(peers, [17, 2, 11, 7], leaves=leaves)
    assert got == {i: sl[i] for i in (2, 7, 11, 17)} and ok == _bits([2, 7, 11, 17]) and rej == 0
    bad = bytearray(sl[9])
    bad[100] ^= 1
    got, ok, rej = s.recover_many([(i, bytes(bad) if i == 9 else d) for i, d in peers], [2, 11], leaves=b"".join(leaves))
    assert got == {2: sl[2], 11: sl[11]} and ok == _bits([2, 11]) and rej == 1 << 9
    wrong = [bytes(32) if i == 11 else h for i, h in enumerate(leaves)]
    got, ok, rej = s.recover_many(peers, [2, 11], leaves=wrong)
    assert got == {2: sl[2], 11: sl[11]} and ok == 1 << 2 and rej == 0
    with pytest.raises(T.DecodeError):
        s.recover_many([(i, bytes(bad) if i == 9 else d) for i, d in peers[:7]], [2], leaves=leaves)
    # without leaves: the return value of today
    assert s.recover_many(peers, [11, 2]) == {2: sl[2], 11: sl[11]}


# ---- the repair windows share stage C: their h_ok is written whatever the caller left in it ----
@pytest.mark.parametrize("mode", MODES)
def test_repair_host_overwrites_a_prefilled_ok_array(oracle, mode):
    """te_repair_batch_host with a wrong leaf for one object and h_ok pre-filled with ones: the
    object whose repaired slice does not match its leaf reads 0, in every hashing mode."""
    import ctypes as C
    s, objs = _slicer(True), _objects(oracle, True, SMALL)
    descs, blobs, leaves, cur, out_at = [], [], [], 0, GUARD
    plans, want = [], []
    for i, (sl, lv) in enumerate(objs):
        lost = 3 + 5 * i
        avail = [j for j in range(N) if j != lost]
        p = s.repair_plan(lost, avail, sl[avail[0]].tobytes())
        offs = {}
        for h in avail:
            d = T.extract_repair_data(sl[h].tobytes(), p, h)
            if d:
                offs[h] = cur
                blobs.append(d)
                cur += len(d)
        plans.append(p)
        descs.append((p, offs, out_at, sl[0][-48:].tobytes()))
        want.append((out_at, sl[lost]))
        out_at += sl.shape[1] + GUARD
        lv = bytearray(lv)
        if i == 1:
            lv[lost * 32 + 5] ^= 0x01  # object 1's leaf cannot match
        leaves.append(bytes(lv))
    helpers = np.frombuffer(b"".join(blobs), np.uint8).copy()
    out = np.full(out_at, POISON, np.uint8)
    arr = batch.repair_descs(descs)
    lb = (C.c_uint8 * (len(objs) * N * 32)).from_buffer_copy(b"".join(leaves))
    ok = (C.c_uint32 * len(objs))(*[0xFFFFFFFF] * len(objs))
    try:
        batch.set_commit_hashing(mode)
        r = _lib.lib.te_repair_batch_host(s.coder.handle, C.c_void_p(helpers.ctypes.data), arr, lb, len(objs),
                                          C.c_void_p(out.ctypes.data), ok, 0)
    finally:
        batch.set_commit_hashing("auto")
    assert r == 0, _lib.strerror(r)
    assert list(ok) == [1, 0, 1], mode
    for at, sl in want:  # the repaired bytes are written either way
        assert np.array_equal(out[at:at + sl.size], sl)
    st = batch.rebuild_launch_stats(s.coder)
    assert st["slices_hashed_host"] + st["slices_hashed_device"] == len(objs), st
    if mode == "host":
        assert st["slices_hashed_host"] == len(objs), st
