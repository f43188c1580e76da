"""The node rebuild pipeline without a GPU: te_repair_window_plan / te_recover_window_plan against
plain Python arithmetic, the argument rules of te_repair_batch_host / te_recover_batch_host, the
ctypes mirror of te_rebuild_launch_stats, and the Rust side's declarations (checked textually).

A window is cut greedily in object order.  A repair object costs the fragments of its plan's
helpers in (te_extract_repair_data_size per helper) plus num_stripes * chunk_size + 48 out; a
recover object its present slices in (popcount(avail_mask) * slice_len) plus slice_len out."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import tape_amd as T
from tape_amd import _lib, batch
from tape_amd._lib import lib

N, K = 20, 7
MiB = 1 << 20
FULL = (1 << N) - 1
SEVEN = sum(1 << i for i in range(13, 20))
SIZES = [0, 1, 4_099, 20_000, 1_000_001, 4 * MiB, 5 * MiB + 3]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["windows", "objects", "pieces_uploaded", "bytes_h2d", "bytes_d2h", "slices_hashed_host",
         "slices_hashed_device", "host_waits"]


def _slicer():
    return T.Slicer.clay_default()


def _meta(s, blob_len):
    g = s.geometry(blob_len)
    m = _lib.te_slice_metadata(1, blob_len, int(g.stripe_size), s.profile.encoding, s.profile.params, 0)
    out = (C.c_uint8 * 48)()
    lib.te_slice_metadata_to_bytes(C.byref(m), out)
    return bytes(out), int(g.slice_len)


def _repair_batch(s, sizes, downs=None):
    """(plans kept alive, descriptor tuples, cost per object): object i loses slice (3 * i) mod 20;
    where downs[i] is set, slice lost + 10 (a node of the other column in every stripe) is down
    too.  The cost is computed here from te_extract_repair_data_size and te_slicer_geometry, not by
    the planner (the empty blob's plan, made from its length alone, has the minimal chunk: its own
    num_stripes * chunk_size)."""
    plans, objs, cost, a, b = [], [], [], 0, 0
    for i, L in enumerate(sizes):
        lost = (3 * i) % N
        down = (lost + 10) % N if downs and downs[i] else None
        avail = [j for j in range(N) if j != lost and j != down]
        g = s.geometry(L)
        p = s.repair_plan_from_params(lost, avail, L, int(g.stripe_size))
        need = [int(lib.te_extract_repair_data_size(p.handle, h)) for h in range(N)]
        assert need[lost] == 0 and (down is None or need[down] == 0)
        offs = {}
        for h in range(N):
            if need[h]:
                offs[h] = a
                a += need[h]
        out_len = int(g.num_stripes) * int(g.chunk_size) + 48
        assert out_len == int(g.slice_len)
        if L == 0:
            info = _lib.te_repair_plan_info()
            assert lib.te_repair_plan_get_info(p.handle, C.byref(info)) == 0
            out_len = info.num_stripes * info.chunk_size + 48
        meta, _ = _meta(s, L)
        plans.append(p)
        objs.append((p, offs, b, meta))
        cost.append(sum(need) + out_len)
        b += out_len
    return plans, objs, cost


def _recover_batch(s, sizes, masks):
    objs, metas, cost, a, b = [], b"", [], 0, 0
    for i, (L, m) in enumerate(zip(sizes, masks)):
        meta, sl = _meta(s, L)
        objs.append((a, sl, m, (5 * i) % N, b))
        metas += meta
        cost.append(bin(m & FULL).count("1") * sl + sl)
        a += N * sl
        b += sl
    return objs, metas, cost


def _py_cuts(cost, window):
    window = window or 128 * MiB
    cuts, acc = [0], 0
    for i, c in enumerate(cost):
        if i > cuts[-1] and acc + c > window:
            cuts.append(i)
            acc = 0
        acc += c
    return cuts + [len(cost)] if cost else [0]


def _assert_cuts(cuts, cost, window):
    """contiguous, covering, order-preserving, every window within the limit or a single object"""
    assert cuts[0] == 0 and cuts[-1] == len(cost)
    assert all(a < b for a, b in zip(cuts, cuts[1:]))
    for a, b in zip(cuts, cuts[1:]):
        assert sum(cost[a:b]) <= window or b - a == 1, (a, b)
        if b < len(cost):  # greedy: the next object did not fit
            assert sum(cost[a:b + 1]) > window, (a, b)


def _raw(fn, s, arr, nobj, window, cap=None, count_only=False):
    nw = C.c_size_t(77)
    cap = nobj + 1 if cap is None else cap
    cuts = (C.c_size_t * max(1, cap))(*([99] * max(1, cap)))
    r = fn(s.coder.handle, arr, nobj, window, None if count_only else cuts, cap, C.byref(nw))
    return r, nw.value, [int(x) for x in cuts[:nw.value + 1]] if r == 0 and not count_only else None


def test_repair_window_plan_matches_python():
    s = _slicer()
    downs = [0, 1, 0, 1, 0, 1, 1]
    plans, objs, cost = _repair_batch(s, SIZES, downs)
    arr = batch.repair_descs(objs)
    # a repair moves 16 fragments of beta / alpha = 1/10 of a slice in and one slice out
    g = s.geometry(4 * MiB)
    assert cost[5] == 16 * (int(g.slice_len) - 48) // 10 + int(g.slice_len)
    for w in (0, 1, cost[0] + cost[1], sum(cost[:4]), sum(cost[:4]) - 1, cost[5], MiB, 3 * MiB, sum(cost)):
        r, nw, cuts = _raw(lib.te_repair_window_plan, s, arr, len(objs), w)
        assert r == 0 and cuts == _py_cuts(cost, w) and nw == len(cuts) - 1, w
        _assert_cuts(cuts, cost, w or 128 * MiB)
        assert batch.repair_window_plan(s.coder, arr, w) == cuts
    # an object above the limit gets a window alone; window_bytes = 0 means 128 MiB
    assert _raw(lib.te_repair_window_plan, s, arr, len(objs), cost[5] - 1)[2][-3:] == [5, 6, 7]
    assert _raw(lib.te_repair_window_plan, s, arr, len(objs), 0) == (0, 1, [0, 7])
    big = [4 * MiB] * 80  # 80 x (16 fragments + 1 slice) of a 4 MiB object: past 128 MiB
    plans2, objs2, cost2 = _repair_batch(s, big)
    assert sum(cost2) > 128 * MiB
    arr2 = batch.repair_descs(objs2)
    r, nw, cuts = _raw(lib.te_repair_window_plan, s, arr2, len(objs2), 0)
    assert r == 0 and cuts == _py_cuts(cost2, 128 * MiB) and nw == 2
    del plans, plans2


def test_recover_window_plan_matches_python():
    s = _slicer()
    masks = [SEVEN, FULL, 0x7F, SEVEN | 1, FULL | 1 << 25, 0x3FFF, 0xFE]
    objs, metas, cost = _recover_batch(s, SIZES, masks)
    arr = batch.recover_descs(objs)
    assert cost[1] == 21 * objs[1][1] and cost[4] == 21 * objs[4][1]  # bits past n do not count
    for w in (0, 1, cost[0] + cost[1], sum(cost[:4]), sum(cost[:4]) - 1, cost[5], MiB, 3 * MiB, sum(cost)):
        r, nw, cuts = _raw(lib.te_recover_window_plan, s, arr, len(objs), w)
        assert r == 0 and cuts == _py_cuts(cost, w) and nw == len(cuts) - 1, w
        _assert_cuts(cuts, cost, w or 128 * MiB)
        assert batch.recover_window_plan(s.coder, objs, w) == cuts
    assert _raw(lib.te_recover_window_plan, s, arr, len(objs), 0) == (0, 1, [0, 7])
    many = [(0, 4 * MiB, FULL, 0, 0)] * 3  # 3 x 21 x 4 MiB = 252 MiB: 0 cuts at 128 MiB
    assert batch.recover_window_plan(s.coder, many, 0) == [0, 1, 2, 3]
    assert batch.recover_window_plan(s.coder, [(0, MiB, FULL, 0, 0)] * 7, 0) == [0, 6, 7]


@pytest.mark.parametrize("which", ["repair", "recover"])
def test_window_plan_count_only_empty_and_small_cap(which):
    s = _slicer()
    if which == "repair":
        plans, objs, _ = _repair_batch(s, SIZES[:4])
        arr, fn = batch.repair_descs(objs), lib.te_repair_window_plan
    else:
        objs, _, _ = _recover_batch(s, SIZES[:4], [SEVEN] * 4)
        arr, fn = batch.recover_descs(objs), lib.te_recover_window_plan
    assert _raw(fn, s, arr, 4, 1, count_only=True) == (0, 4, None)
    assert _raw(fn, s, arr, 4, 1, cap=0, count_only=True) == (0, 4, None)
    assert _raw(fn, s, arr, 4, 1, cap=4)[:2] == (_lib.TE_ERR_BUFFER_TOO_SMALL, 4)  # needs 5 entries
    assert _raw(fn, s, arr, 4, 1, cap=5) == (0, 4, [0, 1, 2, 3, 4])
    assert _raw(fn, s, None, 0, 1) == (0, 0, [0])                     # nobj = 0: no window
    assert _raw(fn, s, None, 0, 0, count_only=True) == (0, 0, None)
    nw = C.c_size_t()
    assert fn(None, arr, 4, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    assert fn(s.coder.handle, None, 4, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    assert fn(s.coder.handle, arr, 4, 0, None, 0, None) == _lib.TE_ERR_INVALID_ARG
    assert (batch.repair_window_plan if which == "repair" else batch.recover_window_plan)(s.coder, []) == []


def test_repair_host_validates_then_needs_a_device():
    s = _slicer()
    h = s.coder.handle
    plans, objs, _ = _repair_batch(s, [1_000_001, 4_099], [0, 1])
    good = batch.repair_descs(objs)
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below returns before any copy
    lv = (C.c_uint8 * (2 * N * 32))()
    ok = (C.c_uint32 * 2)()

    def call(arr=good, c=h, helpers=fake, out=fake, leaves=lv, pok=ok):
        return lib.te_repair_batch_host(c, helpers, arr, leaves, 2, out, pok, 0)

    for bad in (lambda: call(c=None), lambda: call(arr=None), lambda: call(helpers=None), lambda: call(out=None),
                lambda: call(pok=None)):
        assert bad() == _lib.TE_ERR_INVALID_ARG
    null_plan = batch.repair_descs(objs)
    null_plan[1].plan = None  # the second object: the whole batch is checked
    assert call(arr=null_plan) == _lib.TE_ERR_INVALID_ARG
    assert call(arr=null_plan, leaves=None, pok=None) == _lib.TE_ERR_INVALID_ARG
    nw = C.c_size_t()
    assert lib.te_repair_window_plan(h, null_plan, 2, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    # a plan of another profile: Clay(12, 8, 11)
    other = T.Slicer.with_profile(T.ClayCoder(12, 8, 11), 1_000_000, True,
                                  T.EncodingProfile.clay(T.ClayParams.new(12, 8, 11)))
    p12 = other.repair_plan_from_params(0, list(range(1, 12)), 4_099, int(other.geometry(4_099).stripe_size))
    foreign = batch.repair_descs([objs[0], (p12, {j: 0 for j in range(1, 12)}, 0, objs[1][3])])
    assert call(arr=foreign) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_repair_window_plan(h, foreign, 2, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    # a helper the plan names has no fragment; one it does not name may be absent
    named = sorted(objs[1][1])
    missing = batch.repair_descs([objs[0], (objs[1][0], {j: o for j, o in objs[1][1].items() if j != named[3]},
                                            objs[1][2], objs[1][3])])
    assert call(arr=missing) == _lib.TE_ERR_MISSING_HELPER
    if _lib.device_count() == 0:
        assert call() == _lib.TE_ERR_NO_DEVICE
        assert call(leaves=None, pok=None) == _lib.TE_ERR_NO_DEVICE
        assert lib.te_repair_batch_host(h, None, None, None, 0, None, None, 0) == _lib.TE_ERR_NO_DEVICE
        import numpy as np
        buf = np.zeros(16, np.uint8)
        with pytest.raises(T.NoDeviceError):
            batch.repair_host(s.coder, buf, objs, buf)
        with pytest.raises(T.NoDeviceError):
            batch.repair_host(s.coder, buf, objs, buf, leaves=bytes(2 * N * 32))
    del plans


def test_recover_host_validates_then_needs_a_device():
    s = _slicer()
    cfg = s._cfg()
    h = s.coder.handle
    objs, metas, _ = _recover_batch(s, [1_000_001, 4_099], [SEVEN, FULL])
    good = batch.recover_descs(objs)
    fake = C.c_void_p(1 << 20)
    mb = (C.c_uint8 * len(metas)).from_buffer_copy(metas)
    lv = (C.c_uint8 * (2 * N * 32))()
    ok, rej, st = (C.c_uint32 * 2)(), (C.c_uint32 * 2)(), (C.c_int * 2)(9, 9)

    def verified(arr=good, c=h, pcfg=C.byref(cfg), slices=fake, meta=mb, leaves=lv, out=fake, pok=ok, status=st):
        return lib.te_recover_batch_host(c, pcfg, slices, arr, meta, leaves, 2, out, rej, pok, status, 0)

    def plain(arr=good, **kw):
        return verified(arr=arr, leaves=None, pok=None, status=None, **kw)

    for bad in (lambda: verified(c=None), lambda: verified(pcfg=None), lambda: verified(arr=None),
                lambda: verified(slices=None), lambda: verified(meta=None), lambda: verified(out=None),
                lambda: verified(pok=None), lambda: verified(status=None), lambda: plain(c=None),
                lambda: plain(meta=None)):
        assert bad() == _lib.TE_ERR_INVALID_ARG
    # lost >= n, on the second object
    lost20 = batch.recover_descs([objs[0], (objs[1][0], objs[1][1], FULL, N, objs[1][4])])
    assert verified(arr=lost20) == _lib.TE_ERR_INVALID_SLICE
    assert plain(arr=lost20) == _lib.TE_ERR_INVALID_SLICE
    # fewer than k present: the unverified call's error, the verified call's per-object outcome
    few = batch.recover_descs([objs[0], (objs[1][0], objs[1][1], 0x3F | 1 << 25, 3, objs[1][4])])
    assert plain(arr=few) == _lib.TE_ERR_NOT_ENOUGH_SLICES
    off = batch.recover_descs([(objs[0][0], objs[0][1] + 1, SEVEN, 0, objs[0][4]), objs[1]])
    assert plain(arr=off) == _lib.TE_ERR_INVALID_LAYOUT
    assert verified(arr=off) == _lib.TE_ERR_INVALID_LAYOUT
    if _lib.device_count() == 0:
        assert verified() == _lib.TE_ERR_NO_DEVICE
        assert plain() == _lib.TE_ERR_NO_DEVICE
        assert verified(arr=few) == _lib.TE_ERR_NO_DEVICE
        assert lib.te_recover_batch_host(h, C.byref(cfg), None, None, None, None, 0, None, None, None, None, 0) == \
            _lib.TE_ERR_NO_DEVICE
        import numpy as np
        buf = np.zeros(16, np.uint8)
        with pytest.raises(T.NoDeviceError):
            batch.recover_host(s, buf, objs, metas, buf)
        with pytest.raises(T.NoDeviceError):
            batch.recover_host(s, buf, objs, metas, buf, leaves=bytes(2 * N * 32))


def _header_struct(name):
    txt = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [(d.split()[1], d.split()[0]) for d in body.split(";") if d.split()]


def test_rebuild_launch_stats_mirror_and_zero_state():
    fields = _header_struct("te_rebuild_launch_stats")
    assert [f for f, _ in fields] == NAMES == [f for f, _ in _lib.te_rebuild_launch_stats._fields_]
    assert all(t == "uint64_t" for _, t in fields)
    assert C.sizeof(_lib.te_rebuild_launch_stats) == 64
    declared = set(_lib.declared_symbols())
    for sym in ("te_repair_window_plan", "te_recover_window_plan", "te_repair_batch_host", "te_recover_batch_host",
                "te_clay_rebuild_launch_stats"):
        assert sym in declared and hasattr(lib, sym), sym
    s = _slicer()
    assert lib.te_clay_rebuild_launch_stats(None, None) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_clay_rebuild_launch_stats(s.coder.handle, None) == _lib.TE_ERR_INVALID_ARG
    assert batch.rebuild_launch_stats(s.coder) == dict.fromkeys(NAMES, 0)  # all zero before the first call
    # each entry point cites the reference's repair loop or its escalation
    txt = open(_lib.HEADER_PATH).read()
    for sym in ("te_repair_window_plan", "te_repair_batch_host"):
        doc = txt[:txt.index("int %s(" % sym)].rsplit("/*", 1)[1]
        assert "repair.rs:94-226" in doc, sym
    for sym in ("te_recover_window_plan", "te_recover_batch_host"):
        doc = txt[:txt.index("int %s(" % sym)].rsplit("/*", 1)[1]
        assert "recover.rs:77-244" in doc, sym


# ---------------------------------------------------------------- the Rust side ----------------
RS = os.path.join(ROOT, "rust", "tapeec-sys", "src", "lib.rs")
SHIM = os.path.join(ROOT, "rust", "tape-slicer-gpu", "src", "rebuild.rs")


def test_generated_binding_is_current_and_has_the_rebuild_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_rust_sys.py"), "--check"])
    assert r.returncode == 0, "rust/tapeec-sys/src/lib.rs is stale: run scripts/gen_rust_sys.py"
    rs = open(RS).read()
    declared = set(re.findall(r"pub fn (te_\w+)", rs))
    assert {"te_repair_window_plan", "te_recover_window_plan", "te_repair_batch_host", "te_recover_batch_host",
            "te_clay_rebuild_launch_stats"} <= declared
    assert "pub fn te_repair_window_plan(c: *const te_clay," in rs  # host only: a const handle
    assert ("pub fn te_repair_batch_host(c: *mut te_clay, h_helpers: *const u8, objs: *const te_repair_object, "
            "h_leaves: *const u8, nobj: usize, h_out: *mut u8, h_ok: *mut u32, window_bytes: usize) -> c_int;") in rs
    body = re.search(r"pub struct te_rebuild_launch_stats \{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):\s*(\w+)", body) == [(f, "u64") for f in NAMES]


def test_shim_offers_repair_batch_and_recover_batch():
    lib_rs = open(os.path.join(ROOT, "rust", "tape-slicer-gpu", "src", "lib.rs")).read()
    assert "pub mod rebuild;" in lib_rs
    shim = open(SHIM).read()
    assert re.search(r"pub fn repair_batch\(coder: &mut ClayCoder, helpers: &PinnedBuf, objects: &\[RepairObject<'_>\], "
                     r"leaves: Option<&\[u8\]>,\s*out: &mut PinnedBuf, window_bytes: usize\)", shim)
    assert re.search(r"pub fn recover_batch\(coder: &mut ClayCoder, cfg: &ObjectCfg, slices: &PinnedBuf, "
                     r"objects: &\[RecoverObject\],\s*metas: &\[u8\], leaves: Option<&\[u8\]>, out: &mut PinnedBuf, "
                     r"window_bytes: usize\)", shim)
    called = set(re.findall(r"ffi::(te_\w+)\(", shim))
    assert {"te_repair_batch_host", "te_recover_batch_host", "te_clay_rebuild_launch_stats"} <= called
    # offsets are checked against the buffers before the engine reads them
    assert shim.count("helpers.len()") >= 1 and shim.count("slices.len()") >= 1 and shim.count("out.capacity()") >= 2
    lit = re.search(r"= ffi::te_rebuild_launch_stats \{(.*?)\}", shim, flags=re.S).group(1)
    assert re.findall(r"(\w+): 0", lit) == NAMES
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "repair_batch(" in doc and "recover_batch(" in doc and "repair::run" in doc
