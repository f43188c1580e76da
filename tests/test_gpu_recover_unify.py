"""One rebuild path for one lost slice and for several: a lost index is a lost mask of one bit.

The single-slice entry points (te_recover_verified_batch_device, te_recover_batch_host) against the
multi-slice ones called with one-bit masks -- the same bytes, statuses and rejected masks, and
h_ok == (h_ok_mask >> lost) & 1; a mixed batch through te_recover_batch_device whose staged and
unstaged objects each take their own path; and the generic path (decode, re-encode, gather) in
several windows for several lost slices.

test_gpu_recover_multi.py's method: oracle-encoded objects at its SMALL lengths, every call writes
into a buffer pre-filled with 0xA5 that is compared whole with the expected image, and the slices a
call may not read are poisoned in its input."""
import ctypes as C
import os

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib, batch

import test_gpu_recover_multi as M
import test_gpu_recover_multi_pipeline as P

pytestmark = pytest.mark.gpu
N, POISON = P.N, P.POISON
NOT_ENOUGH = P.NOT_ENOUGH
WINDOW = P.WINDOW


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    batch.set_commit_hashing("auto")
    P._cache.clear()
    M._cache.clear()


# ---- 1. the single forms equal the multi forms with one-bit masks ----
# a clean object; one corrupted peer of eight; one corrupted peer of seven (too few verified peers);
# a wrong leaf for the lost slice; an empty blob.  Objects index P._objects(..., SMALL + (0,)).
SPECS = [(0, [0, 1, 2, 4, 5, 10, 12, 19], [3]), (1, [1, 2, 3, 5, 8, 13, 14, 18], [0]), (2, [0, 2, 4, 6, 8, 10, 12], [15]),
         (1, [3, 4, 5, 6, 7, 8, 9], [11]), (3, [0, 1, 2, 3, 4, 5, 6], [19])]
CORRUPT, WRONG_LEAF, DEAD = {1: 13, 2: 8}, {3: 11}, {2}
WANT = ([0, 0, NOT_ENOUGH, 0, 0], [0, 1 << 13, 1 << 8, 0, 0], [1, 1, 0, 0, 1])


def _layout(oracle, verified):
    objs = P._objects(oracle, True, P.SMALL + (0,))
    # without leaves nothing tells a corrupted peer from a good one: every object rebuilds
    lay = P.Layout(objs, SPECS, corrupt=CORRUPT, wrong_leaf=WRONG_LEAF, dead=DEAD if verified else ())
    single = [(d[0], d[1], d[2], sp[2][0], d[4]) for d, sp in zip(lay.descs, SPECS)]
    return lay, single


def _ok_bits(ok_mask):
    return [(m >> sp[2][0]) & 1 for m, sp in zip(ok_mask, SPECS)]


def test_verified_device_single_equals_one_bit_masks(oracle):
    import torch
    s = P._slicer(True)
    lay, single = _layout(oracle, True)
    got_m, res_m = P._device_call(s, lay)
    stats_m = (s.coder.decode_launch_stats(), batch.recover_multi_launch_stats(s.coder))
    d_out = torch.full((lay.exp.size,), POISON, dtype=torch.uint8, device="cuda")
    res_s = batch.recover_verified_batch(s, torch.from_numpy(lay.src).cuda(), single, lay.metas, lay.leaves, d_out)
    torch.cuda.synchronize()
    got_s = d_out.cpu().numpy()
    P._same(got_m, lay.exp, "multi form")
    P._same(got_s, lay.exp, "single form")
    assert res_m[:2] == WANT[:2] and res_s[:2] == WANT[:2]
    assert res_s[2] == WANT[2] and res_s[2] == _ok_bits(res_m[2])
    assert res_m[2] == [ok << sp[2][0] for ok, sp in zip(WANT[2], SPECS)]
    # the same kernels, launch for launch, and the same objects on each path
    assert (s.coder.decode_launch_stats(), batch.recover_multi_launch_stats(s.coder)) == stats_m
    assert stats_m[1]["single_objects"] == 4 and stats_m[1]["multi_objects"] == stats_m[1]["generic_objects"] == 0, stats_m


@pytest.mark.parametrize("mode", ["host", "device"])
def test_host_pipeline_with_leaves_single_equals_one_bit_masks(oracle, mode):
    s = P._slicer(True)
    lay, single = _layout(oracle, True)
    cuts = batch.recover_multi_window_plan(s.coder, lay.descs, WINDOW)
    assert len(cuts) - 1 >= 3 and cuts == batch.recover_window_plan(s.coder, single, WINDOW), cuts
    try:
        batch.set_commit_hashing(mode)
        src, out_m = lay.host(True)
        res_m = batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out_m, leaves=lay.leaves, window_bytes=WINDOW)
        stats_m = (s.coder.decode_launch_stats(), batch.rebuild_launch_stats(s.coder))
        src, out_s = lay.host(True)
        res_s = batch.recover_host(s, src, single, lay.metas, out_s, leaves=lay.leaves, window_bytes=WINDOW)
        stats_s = (s.coder.decode_launch_stats(), batch.rebuild_launch_stats(s.coder))
    finally:
        batch.set_commit_hashing("auto")
    P._same(out_m, lay.exp, "multi form")
    P._same(out_s, lay.exp, "single form")
    assert res_m[:2] == WANT[:2] and res_s[:2] == WANT[:2]
    assert res_s[2] == WANT[2] and res_s[2] == _ok_bits(res_m[2])
    assert stats_s == stats_m and stats_m[1]["windows"] == len(cuts) - 1
    hashed = "slices_hashed_host" if mode == "host" else "slices_hashed_device"
    assert stats_m[1][hashed] > 0, stats_m


def test_host_pipeline_without_leaves_single_equals_one_bit_masks(oracle):
    s = P._slicer(True)
    lay, single = _layout(oracle, False)
    cuts = batch.recover_multi_window_plan(s.coder, lay.descs, WINDOW)
    assert len(cuts) - 1 >= 3 and cuts == batch.recover_window_plan(s.coder, single, WINDOW), cuts
    src, out_m = lay.host(False)
    assert batch.recover_multi_batch_host(s, src, lay.descs, lay.metas, out_m, window_bytes=WINDOW) is None
    stats_m = (s.coder.decode_launch_stats(), batch.rebuild_launch_stats(s.coder))
    # the single form through the C ABI with outcome arrays it must leave alone: unverified, the
    # call writes no status, no rejected mask and no h_ok
    src, out_s = lay.host(False)
    nobj = len(single)
    rej, ok, st = [(C.c_uint32 * nobj)(*[0xDEADBEEF] * nobj) for _ in range(2)] + [(C.c_int * nobj)(*[-7] * nobj)]
    cfg = s._cfg()
    r = _lib.lib.te_recover_batch_host(s.coder.handle, C.byref(cfg), C.c_void_p(src.ctypes.data), batch.recover_descs(single),
                                       batch._meta_bytes(lay.metas), None, nobj, C.c_void_p(out_s.ctypes.data), rej, ok, st,
                                       WINDOW)
    assert r == 0, _lib.strerror(r)
    assert list(ok) == [0xDEADBEEF] * nobj and list(rej) == [0xDEADBEEF] * nobj
    assert (s.coder.decode_launch_stats(), batch.rebuild_launch_stats(s.coder)) == stats_m
    assert np.array_equal(out_s, out_m)
    # the objects whose peers are what the oracle made are the oracle's slices (a corrupted peer
    # goes unnoticed without leaves: those two objects are only the same in both forms)
    for x, (d, sp) in enumerate(zip(lay.descs, SPECS)):
        if x not in CORRUPT:
            sl = P._objects(oracle, True, P.SMALL + (0,))[sp[0]][0]
            assert np.array_equal(out_s[d[4]:d[4] + d[1]], sl[sp[2][0]]), x
    guard = np.full(P.GUARD, POISON, np.uint8)
    assert np.array_equal(out_s[:P.GUARD], guard) and np.array_equal(out_s[-P.GUARD:], guard)


# ---- 2. a mixed batch through the single device form ----
def test_mixed_staged_and_unstaged_batch_single_form(oracle):
    """An empty blob, a staged geometry (20,000 bytes: sub-chunks of 30) and an unstaged one (999
    bytes: sub-chunks of 2, tests/native/rec_multi_check.cpp asserts its route) in one call: the
    staged kernels run the first two, the decode + re-encode the third, its lost slice a parity
    shard of its stripe."""
    s, objs = M._slicer(True), M._objects(oracle, True, (0, 20_000, 999))
    specs = [(0, [0, 1, 2, 3, 4, 5, 6], [9]), (1, [1, 2, 3, 4, 5, 6, 8], [0]), (2, [0, 1, 2, 3, 4, 5, 6], [12]),
             (2, [5, 6, 7, 8, 9, 10, 11], [2])]
    got, exp = M._run(s, objs, specs, fn=batch.recover_batch, single=True)
    M._same(got, exp, "mixed batch")
    d, e, st = s.coder.decode_launch_stats(), s.coder.encode_launch_stats(), batch.recover_multi_launch_stats(s.coder)
    assert sum(d["class_launches"].values()) + d["table_launches"] >= 1, d  # the staged part
    assert d["generic_launches"] >= 1, d                                     # the unstaged part's decode
    # ... and its re-encode: only the stripe whose lost shard is parity (slice 12), not the data one (slice 2)
    assert e["dma_stripes"] + e["stage_stripes"] + e["generic_stripes"] == 1, e
    assert (st["single_objects"], st["generic_objects"], st["multi_objects"]) == (2, 2, 0), st


# ---- 3. the generic path in several windows for several lost slices ----
@pytest.mark.parametrize("window", ["1", None], ids=["window_per_object", "one_window"])
def test_generic_path_windows_several_lost(oracle, window):
    """Three Clay(12,8,11) objects (no plane programs), rotated, three stripes each, with lost slices
    {3, 5}, {3, 9} and {10}: by te_slice_to_shard there are stripes whose lost shards are all data
    (nothing to re-encode, the gather reads the decoded object), all parity, and one of each (both
    gather sources in one stripe)."""
    import torch
    obj = P._generic_object(oracle)
    s = T.Slicer.with_profile(T.ClayCoder(12, 8, 11), T.STRIPE_SIZES[0], True, T.EncodingProfile.clay_default())
    ns = int(s.geometry(250_001).num_stripes)
    specs = [(0, [0, 1, 2, 4, 6, 7, 8, 9, 10], [3, 5]), (0, [0, 1, 2, 4, 5, 7, 8, 10, 11], [3, 9]), (0, [0, 1, 2, 3, 4, 5, 6, 7], [10])]
    # per object and stripe: how many of its lost slices hold a parity shard (shards 8..11)
    parity = [[sum(int(_lib.lib.te_slice_to_shard(1, 12, st, sl)) >= 8 for sl in lost) for st in range(ns)] for _, _, lost in specs]
    assert ns == 3 and 0 in parity[0] and 2 in parity[0] and 1 in parity[1] and 0 in parity[2] and 1 in parity[2], parity
    lay = P.Layout([obj], specs, n=12)
    d_out = torch.full((lay.exp.size,), POISON, dtype=torch.uint8, device="cuda")
    if window:
        os.environ["TEC_DEBUG_KNOBS"] = "1"  # measurement knobs are read only with this set
        os.environ["TEC_RECOVER_WINDOW_BYTES"] = window
    try:
        batch.recover_multi_batch(s, torch.from_numpy(lay.src).cuda(), lay.descs, lay.metas, d_out)
        torch.cuda.synchronize()
    finally:
        if window:
            del os.environ["TEC_RECOVER_WINDOW_BYTES"]
            del os.environ["TEC_DEBUG_KNOBS"]
    P._same(d_out.cpu().numpy(), lay.exp, f"window {window}")
    st, d, e = batch.recover_multi_launch_stats(s.coder), s.coder.decode_launch_stats(), s.coder.encode_launch_stats()
    assert (st["generic_objects"], st["multi_objects"], st["single_objects"], st["multi_launches"]) == (3, 0, 0, 0), st
    assert d["generic_stripes"] == 3 * ns and d["table_launches"] == 0, d
    assert d["generic_launches"] >= 3 if window else d["generic_launches"] < 3, d  # a decode per window
    # a stripe whose lost shards are all data is not re-encoded
    assert e["dma_stripes"] + e["stage_stripes"] + e["generic_stripes"] == sum(p > 0 for o in parity for p in o), e
