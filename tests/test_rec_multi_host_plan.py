"""The multi-slice rebuild's host side without a GPU: te_recover_multi_window_plan against plain
Python arithmetic, the argument rules of te_recover_multi_verified_batch_device and
te_recover_multi_batch_host (every one of them answered before the call looks for a device), and the
header, the ctypes mirror and the generated Rust binding agreeing on the three entry points.

A window is cut greedily in object order; a multi object costs its present slices in plus its lost
slices out, a slice length each: (popcount(avail_mask) + popcount(lost_mask)) * slice_len."""
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
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["te_recover_multi_verified_batch_device", "te_recover_multi_window_plan", "te_recover_multi_batch_host"]


def _slicer():
    return T.Slicer.clay_default()


def _meta(s, blob_len):
    g = s.geometry(blob_len)
    m = _lib.te_slice_metadata(1, blob_len, int(g.stripe_size), s.profile.encoding, s.profile.params, 0)
    out = (C.c_uint8 * 48)()
    lib.te_slice_metadata_to_bytes(C.byref(m), out)
    return bytes(out), int(g.slice_len)


def _batch(s, sizes, masks):
    """Descriptor tuples (slices_off, slice_len, avail, lost, out_off), metas and each object's cost."""
    objs, metas, cost, a, b = [], b"", [], 0, 0
    for L, (avail, lost) in zip(sizes, masks):
        meta, slen = _meta(s, L)
        objs.append((a, slen, avail, lost, b))
        metas += meta
        nl = bin(lost & FULL).count("1")
        cost.append((bin(avail & FULL).count("1") + nl) * slen)
        a += N * slen
        b += nl * slen
    return objs, metas, cost


def _cuts(cost, limit):
    """The rule, restated: at least one object per window, then as many as fit."""
    limit = limit or 128 * MiB
    cuts, total = [0], 0
    for i, c in enumerate(cost):
        if i > cuts[-1] and total + c > limit:
            cuts.append(i)
            total = 0
        total += c
    return cuts + [len(cost)] if cost else []


SIZES = [0, 1, 4_099, 20_000, 1_000_001, 4 * MiB, 5 * MiB + 3, 300_000]
MASKS = [(SEVEN, 1), (SEVEN, 0x1FFF), (0x7F, 3 << 10), (FULL & ~0x30, 0x30), (SEVEN | 1, 2 | 1 << 25), (SEVEN, 0x0FF0),
         (0x3FFF, 1 << 19), (SEVEN, 0x1FFF)]


def test_window_plan_matches_python():
    s = _slicer()
    objs, _, cost = _batch(s, SIZES, MASKS)
    slen4 = objs[5][1]
    assert cost[5] == 15 * slen4 and cost[1] == 20 * objs[1][1] and cost[4] == 9 * objs[4][1]  # bits >= n do not count
    for limit in (0, 1, 10_000, cost[3], cost[3] + cost[4], MiB, 8 * MiB, 14 * slen4, 15 * slen4, 1 << 40):
        got = batch.recover_multi_window_plan(s.coder, objs, limit)
        assert got == _cuts(cost, limit), limit
    # an object above the limit is a window alone; every window otherwise stays within it
    cuts = batch.recover_multi_window_plan(s.coder, objs, 8 * MiB)
    assert len(cuts) - 1 >= 3
    for a, b in zip(cuts, cuts[1:]):
        assert b > a and (b - a == 1 or sum(cost[a:b]) <= 8 * MiB)
    assert any(b - a == 1 and cost[a] > 8 * MiB for a, b in zip(cuts, cuts[1:]))
    assert batch.recover_multi_window_plan(s.coder, objs, 1) == list(range(len(objs) + 1))


def test_window_plan_count_only_empty_and_small_cap():
    s = _slicer()
    objs, _, cost = _batch(s, SIZES, MASKS)
    arr = batch.recover_multi_descs(objs)
    want = _cuts(cost, MiB)
    nw = C.c_size_t(99)
    assert lib.te_recover_multi_window_plan(s.coder.handle, arr, len(objs), MiB, None, 0, C.byref(nw)) == 0
    assert nw.value == len(want) - 1
    cuts = (C.c_size_t * len(want))()
    assert lib.te_recover_multi_window_plan(s.coder.handle, arr, len(objs), MiB, cuts, len(want) - 1, C.byref(nw)) == \
        _lib.TE_ERR_BUFFER_TOO_SMALL
    assert nw.value == len(want) - 1
    assert lib.te_recover_multi_window_plan(s.coder.handle, arr, len(objs), MiB, cuts, len(want), C.byref(nw)) == 0
    assert list(cuts) == want
    assert lib.te_recover_multi_window_plan(s.coder.handle, None, 0, MiB, None, 0, C.byref(nw)) == 0 and nw.value == 0
    assert batch.recover_multi_window_plan(s.coder, [], MiB) == []
    for bad in (lambda: lib.te_recover_multi_window_plan(None, arr, 1, 0, None, 0, C.byref(nw)),
                lambda: lib.te_recover_multi_window_plan(s.coder.handle, None, 1, 0, None, 0, C.byref(nw)),
                lambda: lib.te_recover_multi_window_plan(s.coder.handle, arr, 1, 0, None, 0, None)):
        assert bad() == _lib.TE_ERR_INVALID_ARG


def _calls(s, objs, metas):
    cfg = s._cfg()
    h = s.coder.handle
    nobj = len(objs)
    good = batch.recover_multi_descs(objs)
    fake = C.c_void_p(1 << 20)
    mb = (C.c_uint8 * len(metas)).from_buffer_copy(metas)
    lv = (C.c_uint8 * (nobj * N * 32))()
    ok, rej, st = (C.c_uint32 * nobj)(), (C.c_uint32 * nobj)(), (C.c_int * nobj)(*[9] * nobj)

    def host(arr=good, c=h, pcfg=C.byref(cfg), slices=fake, meta=mb, leaves=lv, out=fake, pok=ok, status=st):
        return lib.te_recover_multi_batch_host(c, pcfg, slices, arr, meta, leaves, nobj, out, rej, pok, status, 0)

    def plain(arr=good, **kw):
        return host(arr=arr, leaves=None, pok=None, status=None, **kw)

    def device(arr=good, c=h, pcfg=C.byref(cfg), slices=fake, meta=mb, leaves=lv, out=fake, pok=ok, status=st):
        return lib.te_recover_multi_verified_batch_device(c, pcfg, slices, arr, meta, leaves, nobj, out, rej, pok, status, None)

    return host, plain, device, st


def test_argument_errors_come_before_the_device():
    s = _slicer()
    objs, metas, _ = _batch(s, [1_000_001, 4_099], [(SEVEN, 3), (FULL & ~0x1800, 0x1800)])
    host, plain, device, st = _calls(s, objs, metas)
    IA = _lib.TE_ERR_INVALID_ARG
    for bad in (lambda: host(c=None), lambda: host(pcfg=None), lambda: host(arr=None), lambda: host(slices=None),
                lambda: host(meta=None), lambda: host(out=None), lambda: host(pok=None), lambda: host(status=None),
                lambda: plain(c=None), lambda: plain(meta=None),
                lambda: device(c=None), lambda: device(pcfg=None), lambda: device(arr=None), lambda: device(meta=None),
                lambda: device(leaves=None), lambda: device(pok=None), lambda: device(status=None)):
        assert bad() == IA

    def second(avail=objs[1][2], lost=objs[1][3], slices_off=objs[1][0], slen=objs[1][1], out_off=objs[1][4]):
        return batch.recover_multi_descs([objs[0], (slices_off, slen, avail, lost, out_off)])

    # the lost mask, on the second object: empty, a bit at n, more than n - k bits, a bit of avail_mask
    for arr in (second(lost=0), second(lost=1 << N), second(avail=SEVEN, lost=0x3FFF), second(lost=0x1801)):
        assert host(arr=arr) == IA and plain(arr=arr) == IA and device(arr=arr) == IA
    # the verified device form's alignment rules; the host forms take any offset
    for arr in (second(out_off=objs[1][4] + 2), second(slices_off=objs[1][0] + 1)):
        assert device(arr=arr) == IA
    # a slice length that is not the object's: odd for the device form first, a layout error otherwise
    assert device(arr=second(slen=objs[1][1] + 1)) == IA
    # (+ 400: still whole sub-chunks, so the length passes Slicer::decode's checks and fails the geometry's)
    longer = second(slen=objs[1][1] + 400)
    assert device(arr=longer) == _lib.TE_ERR_INVALID_LAYOUT
    assert host(arr=longer) == _lib.TE_ERR_INVALID_LAYOUT and plain(arr=longer) == _lib.TE_ERR_INVALID_LAYOUT
    # fewer than k present: the unverified call's error, a verified call's per-object outcome
    few = second(avail=0x3F, lost=0x1800)
    assert plain(arr=few) == _lib.TE_ERR_NOT_ENOUGH_SLICES
    if _lib.device_count() == 0:
        ND = _lib.TE_ERR_NO_DEVICE
        assert host() == ND and plain() == ND and device() == ND
        assert host(arr=few) == ND and device(arr=few) == ND
        assert host(arr=second(out_off=objs[1][4] + 1)) == ND  # an odd out_off is the host form's to hash on the host
        assert list(st) == [9, 9]  # nothing was written
        cfg = s._cfg()
        assert lib.te_recover_multi_batch_host(s.coder.handle, C.byref(cfg), None, None, None, None, 0, None, None, None,
                                               None, 0) == ND
        import numpy as np
        buf = np.zeros(16, np.uint8)
        with pytest.raises(T.NoDeviceError):
            batch.recover_multi_batch_host(s, buf, objs, metas, buf)
        with pytest.raises(T.NoDeviceError):
            batch.recover_multi_batch_host(s, buf, objs, metas, buf, leaves=bytes(2 * N * 32))
        peer = bytes(objs[1][1] - 48) + metas[48:]  # slices of the second object, by its suffix
        with pytest.raises(T.NoDeviceError):
            s.recover_many([(i, peer) for i in range(7)], [8, 9], leaves=bytes(N * 32))


def _decl(txt, name):
    m = re.search(r"\bint %s\((.*?)\);" % name, txt, flags=re.S)
    assert m, name
    return m.group(1)


def test_header_mirror_and_binding_agree():
    hdr = open(_lib.HEADER_PATH).read()
    rs = open(os.path.join(ROOT, "rust", "tapeec-sys", "src", "lib.rs")).read()
    for name in NEW:
        nargs = len(_decl(hdr, name).split(","))
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*c_int;" % name, rs, flags=re.S)
        assert m, f"{name} missing from the generated binding"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs, name
        # each entry point names the node's code it stands for
        doc = hdr[:hdr.index("int %s(" % name)].rsplit("/*", 1)[1]
        for cite in ("recover.rs:77-244", "recover.rs:207-218", "recover.rs:411-442"):
            assert cite in doc, (name, cite)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_rust_sys.py"), "--check"])
    assert r.returncode == 0, "rust/tapeec-sys/src/lib.rs is stale: run scripts/gen_rust_sys.py"
