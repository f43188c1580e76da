"""Data verify on the device: te_verify_data_batch_device, te_verify_data_batch_host and
te_slicer_verify_data against oracle.slicer_encode + oracle/merkle_oracle.py, bit-exact, and
against each other.

Eight objects: the empty blob, 1 B, 1,000 B (sub-chunk below 8 B: the generic kernel), 20,000 B (the
30 B sub-chunk shape), 1,000,001 B (a short last stripe), 2,300,000 B, one 4 MiB object (the only
production-size one) and 333 B; rotated and identity mapping, tree heights 5 and 7.  The host
buffer carries poison around the objects.  The oracle's slices are built once per module."""
import ctypes as C

import numpy as np
import pytest
import torch

import tape_amd as T
from tape_amd import _lib, batch
from tape_amd._lib import lib

pytestmark = pytest.mark.gpu
N, K = 20, 7
MiB = 1 << 20
GUARD = 64
POISON = 0xA5
SIZES = [0, 1, 1_000, 20_000, 1_000_001, 2_300_000, 4 * MiB, 333]
HEIGHTS = (5, 7)
WINDOW = MiB  # the 4 MiB object exceeds one window
_CACHE = {}


def _slicer(rotated):
    key = ("slicer", rotated)
    if key not in _CACHE:
        _CACHE[key] = T.Slicer.clay_default() if rotated else T.Slicer.new(T.ClayCoder(N, K, 16))
    return _CACHE[key]


def _commit(oracle, data, rotated, chunk_index=0):
    """The oracle's leaves of one object and its root per height."""
    from oracle import merkle_oracle as MO
    key = ("clay",)
    if key not in _CACHE:
        _CACHE[key] = oracle.OracleClay(N, K, 16)
    slices = oracle.slicer_encode(_CACHE[key], data, rotated=rotated, chunk_index=chunk_index)
    leaves = [MO.hash_leaf(s) for s in slices]
    return {"leaves": leaves, "roots": {h: MO.root_from_leaf_hashes(leaves, h) for h in HEIGHTS},
            "sl": len(slices[0])}


def _objects(oracle, rotated):
    """Built once per mapping and left unchanged."""
    key = ("objs", rotated)
    if key not in _CACHE:
        objs = []
        for i, L in enumerate(SIZES):
            data = oracle.splitmix64_bytes(0xD0 + i, L).tobytes()
            objs.append(dict(_commit(oracle, data, rotated), data=data, len=L))
        s = _slicer(rotated)
        sc = [int(s.geometry(L).sub_chunk_size) for L in SIZES]
        assert sc[2] < 8 and sc[3] == 30 and sc[6] >= 8  # generic kernel, the 30 B shape, the fast kernels
        g = s.geometry(SIZES[4])
        assert int(g.num_stripes) > 1 and SIZES[4] % int(g.stripe_size)  # a short last stripe
        assert len({ob["sl"] for ob in objs}) > 4  # several runs of equal slice length
        _CACHE[key] = objs
    return _CACHE[key]


class Layout:
    """The objects' bytes in one host buffer, poison before, between and after them."""

    def __init__(self, datas, pinned=False, chunk_index=None):
        offs, cur = [], GUARD
        for d in datas:
            offs.append(cur)
            cur += len(d) + GUARD
        self.buf = batch.host_empty(cur) if pinned else np.empty(cur, np.uint8)
        self.buf[:] = POISON
        for d, o in zip(datas, offs):
            self.buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
        self.image = self.buf.copy()
        ci = chunk_index or [0] * len(datas)
        # out_off is ignored by every verify call: give it values no buffer could hold
        self.descs = [(o, len(d), (1 << 50) + 3 * i, ci[i]) for i, (d, o) in enumerate(zip(datas, offs))]
        self.total = sum(len(d) for d in datas)

    def unchanged(self):
        return bool((self.buf == self.image).all())


def _join(hashes):
    return b"".join(hashes)


def _host(slicer, lay, xroots, xleaves, height, window=WINDOW):
    ok, roots, mask = batch.verify_data_batch(slicer, lay.buf, lay.descs, _join(xroots),
                                              expected_leaves=xleaves, height=height, window_bytes=window)
    assert lay.unchanged()
    return ok, roots, mask, batch.verify_data_launch_stats(slicer.coder)


def _device(slicer, lay, xroots, xleaves, height):
    nobj = len(lay.descs)
    d_data = torch.from_numpy(lay.buf.copy()).cuda()
    d_xr = torch.frombuffer(bytearray(_join(xroots)), dtype=torch.uint8).cuda()
    d_xl = torch.frombuffer(bytearray(_join(h for ob in xleaves for h in ob)), dtype=torch.uint8).cuda() \
        if xleaves is not None else None
    wb = batch.verify_data_work_bytes(slicer, lay.descs)
    raw = torch.full((GUARD + wb + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    work = raw[GUARD:GUARD + wb]
    roots = torch.full((GUARD + nobj * 32 + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    ok = torch.full((nobj + 2,), -1, dtype=torch.int32, device="cuda")
    mask = torch.full((nobj + 2,), -1, dtype=torch.int64, device="cuda")
    batch.verify_data_batch(slicer, d_data, lay.descs, d_xr, expected_leaves=d_xl, roots=roots[GUARD:GUARD + nobj * 32],
                            ok=ok[1:1 + nobj], bad_leaf_mask=mask[1:1 + nobj], work=work, height=height)
    torch.cuda.synchronize()
    st = batch.verify_data_launch_stats(slicer.coder)
    assert d_data.cpu().numpy().tobytes() == lay.image.tobytes()
    r = raw.cpu().numpy()
    assert (r[:GUARD] == POISON).all() and (r[-GUARD:] == POISON).all()
    rr = roots.cpu().numpy()
    assert (rr[:GUARD] == POISON).all() and (rr[-GUARD:] == POISON).all()
    okh, mh = ok.cpu().tolist(), mask.cpu().tolist()
    assert okh[0] == okh[-1] == -1 and mh[0] == mh[-1] == -1
    rb = rr[GUARD:GUARD + nobj * 32].tobytes()
    # the leaf hashes stay at the end of the work buffer
    lb = r[GUARD + wb - nobj * N * 32:GUARD + wb].tobytes()
    leaves = [[lb[(o * N + i) * 32:(o * N + i + 1) * 32] for i in range(N)] for o in range(nobj)]
    masks = [m & (2 ** 64 - 1) for m in mh[1:-1]] if xleaves is not None else None
    if xleaves is None:
        assert mh[1:-1] == [-1] * nobj  # not written without expected leaves
    return [bool(x) for x in okh[1:-1]], [rb[o * 32:(o + 1) * 32] for o in range(nobj)], masks, st, leaves


def _per_call(slicer, datas, xroots, height, chunk_index=None):
    oks, roots = [], []
    for i, (d, x) in enumerate(zip(datas, xroots)):
        ci = chunk_index[i] if chunk_index else 0
        oks.append(slicer.verify_data(d, x, chunk_index=ci, height=height))
        st = slicer.verify_data_launch_stats()
        assert (st["objects"], st["windows"], st["root_check_launches"]) == (1, 1, 1)
        assert st["h2d_bytes"] == len(d) and st["d2h_bytes"] <= 44
        roots.append(slicer.encode_root(d, chunk_index=ci, height=height))
    return oks, roots


def _bad_sets(true_leaves, leaves):
    return sum(1 << i for i in range(N) if true_leaves[i] != leaves[i])


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("rotated", [True, False])
def test_all_true(oracle, rotated, height):
    objs, s = _objects(oracle, rotated), _slicer(rotated)
    nobj = len(objs)
    datas = [ob["data"] for ob in objs]
    xroots = [ob["roots"][height] for ob in objs]
    xleaves = [ob["leaves"] for ob in objs]
    ok, roots, mask, st, leaves = _device(s, Layout(datas), xroots, xleaves, height)
    assert ok == [True] * nobj and roots == xroots and mask == [0] * nobj and leaves == xleaves
    assert st["objects"] == nobj and st["root_check_launches"] == 1 and st["h2d_bytes"] == st["d2h_bytes"] == 0
    sl = [ob["sl"] for ob in objs]
    runs = 1 + sum(a != b for a, b in zip(sl, sl[1:]))  # one leaf launch series per run of equal slice lengths
    assert st["groups"] == runs and runs >= 6 and st["leaf_launches"] >= runs
    for pinned in (True, False):
        lay = Layout(datas, pinned=pinned)
        ok, roots, mask, st = _host(s, lay, xroots, xleaves, height)
        assert ok == [True] * nobj and roots == xroots and mask == [0] * nobj
        # no slice byte left the device
        assert st["d2h_bytes"] <= nobj * 44 and st["h2d_bytes"] == lay.total and st["windows"] > 1
        assert st["objects"] == nobj and st["root_check_launches"] == st["groups"] >= 1
        assert st["leaf_launches"] >= runs
    # without expected leaves: no mask, fewer bytes either way
    ok, roots, mask, st = _host(s, Layout(datas), xroots, None, height)
    assert ok == [True] * nobj and roots == xroots and mask is None
    assert st["d2h_bytes"] <= nobj * 36 and st["h2d_expected_bytes"] == nobj * 32
    ok, roots, mask, st, _ = _device(s, Layout(datas), xroots, None, height)
    assert ok == [True] * nobj and roots == xroots
    oks, roots = _per_call(s, datas, xroots, height)
    assert oks == [True] * nobj and roots == xroots


@pytest.mark.parametrize("rotated", [True, False])
def test_roots_equal_encode_commit(oracle, rotated):
    """The same roots as te_encode_commit_batch_host computes on the same inputs."""
    objs, s = _objects(oracle, rotated), _slicer(rotated)
    nobj, height = len(objs), 5
    lay = Layout([ob["data"] for ob in objs], pinned=True)
    descs, cur = [], 0
    for (off, ln, _, ci), ob in zip(lay.descs, objs):
        descs.append((off, ln, cur, ci))
        cur += N * ob["sl"]
    out = batch.host_empty(cur)
    leaf = np.zeros(nobj * N * 32, np.uint8)
    roots = np.zeros(nobj * 32, np.uint8)
    batch.encode_commit_batch_host(s, lay.buf, descs, out, leaf, roots, height=height)
    want = [roots[o * 32:(o + 1) * 32].tobytes() for o in range(nobj)]
    ok, got, mask, st = _host(s, lay, want, [[leaf[(o * N + i) * 32:(o * N + i + 1) * 32].tobytes() for i in range(N)]
                                             for o in range(nobj)], height, window=0)
    assert ok == [True] * nobj and got == want and mask == [0] * nobj
    assert got == [ob["roots"][height] for ob in objs]
    assert st["groups"] == 1 and st["d2h_bytes"] <= nobj * 44


@pytest.mark.parametrize("victim", [1, 4, 6])
def test_one_byte_flipped(oracle, victim):
    rotated, height = True, 5
    objs, s = _objects(oracle, rotated), _slicer(rotated)
    nobj = len(objs)
    datas = [ob["data"] for ob in objs]
    flipped = bytearray(datas[victim])
    flipped[(len(flipped) * 2) // 3] ^= 0x04
    datas[victim] = bytes(flipped)
    bad = _commit(oracle, datas[victim], rotated)
    # computed from the oracle, not assumed: which leaves the flip changes
    want_mask = [_bad_sets(objs[o]["leaves"], bad["leaves"]) if o == victim else 0 for o in range(nobj)]
    assert want_mask[victim] != 0
    want_ok = [o != victim for o in range(nobj)]
    want_roots = [bad["roots"][height] if o == victim else objs[o]["roots"][height] for o in range(nobj)]
    assert want_roots[victim] != objs[victim]["roots"][height]
    xroots = [ob["roots"][height] for ob in objs]   # the true commitments
    xleaves = [ob["leaves"] for ob in objs]
    ok, roots, mask, st, leaves = _device(s, Layout(datas), xroots, xleaves, height)
    assert (ok, roots, mask) == (want_ok, want_roots, want_mask)
    assert leaves[victim] == bad["leaves"]
    for pinned in (True, False):
        ok, roots, mask, st = _host(s, Layout(datas, pinned=pinned), xroots, xleaves, height)
        assert (ok, roots, mask) == (want_ok, want_roots, want_mask)
    oks, roots = _per_call(s, datas, xroots, height)
    assert (oks, roots) == (want_ok, want_roots)


@pytest.mark.parametrize("rotated", [True, False])
def test_chunk_index_enters_every_leaf(oracle, rotated):
    """chunk_index is part of the 48-byte suffix of every slice, so of every leaf and of the root."""
    height = 7
    objs, s = _objects(oracle, rotated), _slicer(rotated)
    pick = [0, 1, 3, 4, 7]
    ci = [5, (1 << 40) + 3, 1, 77, (1 << 64) - 1]
    datas = [objs[i]["data"] for i in pick]
    com = [_commit(oracle, d, rotated, chunk_index=c) for d, c in zip(datas, ci)]
    xroots = [c["roots"][height] for c in com]
    xleaves = [c["leaves"] for c in com]
    for i, c in zip(pick, com):
        assert c["roots"][height] != objs[i]["roots"][height]
        assert all(a != b for a, b in zip(c["leaves"], objs[i]["leaves"]))
    nobj = len(pick)
    ok, roots, mask, st, leaves = _device(s, Layout(datas, chunk_index=ci), xroots, xleaves, height)
    assert ok == [True] * nobj and roots == xroots and mask == [0] * nobj and leaves == xleaves
    ok, roots, mask, st = _host(s, Layout(datas, pinned=True, chunk_index=ci), xroots, xleaves, height)
    assert ok == [True] * nobj and roots == xroots and mask == [0] * nobj
    oks, roots = _per_call(s, datas, xroots, height, chunk_index=ci)
    assert oks == [True] * nobj and roots == xroots
    # against chunk index 0's commitments every object fails, in every leaf
    zroots = [objs[i]["roots"][height] for i in pick]
    zleaves = [objs[i]["leaves"] for i in pick]
    ok, roots, mask, st = _host(s, Layout(datas, chunk_index=ci), zroots, zleaves, height)
    assert ok == [False] * nobj and roots == xroots and mask == [(1 << N) - 1] * nobj


def test_work_buffer_too_small(oracle):
    objs, s = _objects(oracle, True), _slicer(True)
    lay = Layout([objs[2]["data"]])
    cfg = s._cfg()
    arr = batch.encode_descs(lay.descs)
    wb = batch.verify_data_work_bytes(s, arr)
    t = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(1, dtype=torch.int32, device="cuda")
    r = lib.te_verify_data_batch_device(s.coder.handle, C.byref(cfg), C.c_void_p(t.data_ptr()), arr, 1, 5,
                                        C.c_void_p(t.data_ptr()), None, C.c_void_p(t.data_ptr()), wb - 1, None,
                                        C.c_void_p(ok.data_ptr()), None, None)
    assert r == _lib.TE_ERR_BUFFER_TOO_SMALL
