"""The host read pipeline without a GPU: te_decode_window_plan against plain Python arithmetic, the
argument rules of te_decode_batch_host / te_decode_verified_batch_host / te_stream_reader_*, and
the ctypes mirror of te_read_launch_stats.

A window is cut greedily in object order: an object costs its present slices' bytes in
(popcount(avail_mask) * slice_len) plus its blob_len out; a window takes objects while their sum
stays within window_bytes, and always at least one."""
import ctypes as C
import re

import pytest

import tape_amd as T
from tape_amd import _lib, batch
from tape_amd._lib import lib

N, K = 20, 7
MiB = 1 << 20
SIZES = [1, 4_099, 1_000_001, 4 * MiB]
SEVEN = sum(1 << i for i in range(13, 20))
FULL = (1 << N) - 1


def _slicer():
    return T.Slicer.clay_default()


def _meta(s, blob_len):
    g = s.geometry(blob_len)
    m = _lib.te_slice_metadata(1, blob_len, int(g.stripe_size), s.profile.encoding, s.profile.params, 0)
    out = (C.c_uint8 * 48)()
    lib.te_slice_metadata_to_bytes(C.byref(m), out)
    return bytes(out), int(g.slice_len)


def _batch(s, sizes, masks):
    """(descriptor tuples, metas, cost per object)"""
    objs, metas, cost, a, b = [], b"", [], 0, 0
    for L, m in zip(sizes, masks):
        meta, sl = _meta(s, L)
        objs.append((a, sl, m, b))
        metas += meta
        cost.append(bin(m & FULL).count("1") * sl + L)
        a += N * sl
        b += L
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


def _raw_plan(s, objs, metas, window, cap=None, count_only=False):
    arr = batch.decode_descs(objs)
    mb = (C.c_uint8 * max(1, len(metas))).from_buffer_copy(metas or b"\0")
    nw = C.c_size_t(77)
    cap = len(objs) + 1 if cap is None else cap
    cuts = (C.c_size_t * max(1, cap))(*([99] * max(1, cap)))
    r = lib.te_decode_window_plan(s.coder.handle, arr, mb, len(objs), window, None if count_only else cuts, cap,
                                  C.byref(nw))
    return r, nw.value, [int(x) for x in cuts[:nw.value + 1]] if r == 0 and not count_only else None


def _assert_cuts(cuts, cost, window):
    """contiguous, covering, order-preserving, every window within the limit or a single object"""
    assert cuts[0] == 0 and cuts[-1] == len(cost)
    assert all(a < b for a, b in zip(cuts, cuts[1:]))
    for a, b in zip(cuts, cuts[1:]):
        assert sum(cost[a:b]) <= window or b - a == 1, (a, b)
        if b < len(cost):  # greedy: the next object did not fit
            assert sum(cost[a:b + 1]) > window, (a, b)


def test_window_plan_edges():
    s = _slicer()
    objs, metas, cost = _batch(s, SIZES, [SEVEN] * 4)
    # one window holds exactly two objects; the third and fourth exceed the limit: windows of their own
    w = cost[0] + cost[1]
    assert _raw_plan(s, objs, metas, w) == (0, 3, [0, 2, 3, 4])
    _assert_cuts([0, 2, 3, 4], cost, w)
    # one byte less and the second object no longer fits beside the first
    assert _raw_plan(s, objs, metas, w - 1) == (0, 4, [0, 1, 2, 3, 4])
    # an object lands exactly on the limit: 1 B + 4,099 B + 1,000,001 B objects sum to the window
    w = cost[0] + cost[1] + cost[2]
    assert _raw_plan(s, objs, metas, w) == (0, 2, [0, 3, 4])
    assert _raw_plan(s, objs, metas, w - 1) == (0, 3, [0, 2, 3, 4])
    # the window is exactly the third object: it gets a window alone, on the limit
    assert _raw_plan(s, objs, metas, cost[2]) == (0, 3, [0, 2, 3, 4])
    # everything in one window; 0 means 128 MiB
    assert _raw_plan(s, objs, metas, sum(cost)) == (0, 1, [0, 4])
    assert _raw_plan(s, objs, metas, 0) == (0, 1, [0, 4])
    # a limit below every object: one window each
    assert _raw_plan(s, objs, metas, 1) == (0, 4, [0, 1, 2, 3, 4])


def test_window_plan_counts_present_slices_and_matches_python():
    s = _slicer()
    sizes = SIZES + [0, 999_999, 4 * MiB, 250_000, 1]
    masks = [SEVEN, FULL, 0x7F, SEVEN | 1, FULL, 0x3FFF, SEVEN, FULL | 1 << 25, 0xFE]
    objs, metas, cost = _batch(s, sizes, masks)
    assert cost[1] == N * objs[1][1] + 4_099 and cost[4] == N * objs[4][1]  # 20 present; the empty blob
    assert cost[7] == N * objs[7][1] + 250_000                             # bits past n do not count
    for w in (0, 1, cost[0] + cost[1], sum(cost[:3]), 5 * MiB, 9 * MiB, 12 * MiB, 30 * MiB, sum(cost)):
        r, nw, cuts = _raw_plan(s, objs, metas, w)
        assert r == 0 and cuts == _py_cuts(cost, w) and nw == len(cuts) - 1, w
        _assert_cuts(cuts, cost, w or 128 * MiB)
    assert batch.decode_window_plan(s.coder, objs, metas, 9 * MiB) == _py_cuts(cost, 9 * MiB)


def test_window_plan_count_only_empty_and_small_cap():
    s = _slicer()
    objs, metas, cost = _batch(s, SIZES, [SEVEN] * 4)
    assert _raw_plan(s, objs, metas, 1, count_only=True) == (0, 4, None)
    assert _raw_plan(s, objs, metas, 1, cap=0, count_only=True) == (0, 4, None)
    assert _raw_plan(s, objs, metas, 1, cap=4)[:2] == (_lib.TE_ERR_BUFFER_TOO_SMALL, 4)  # needs 5 entries
    assert _raw_plan(s, objs, metas, 1, cap=5) == (0, 4, [0, 1, 2, 3, 4])
    assert _raw_plan(s, [], b"", 1) == (0, 0, [0])                  # nobj = 0: no window
    assert _raw_plan(s, [], b"", 0, count_only=True) == (0, 0, None)
    assert batch.decode_window_plan(s.coder, [], b"") == []
    nw = C.c_size_t()
    arr = batch.decode_descs(objs)
    mb = (C.c_uint8 * len(metas)).from_buffer_copy(metas)
    assert lib.te_decode_window_plan(None, arr, mb, 4, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_decode_window_plan(s.coder.handle, None, mb, 4, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_decode_window_plan(s.coder.handle, arr, None, 4, 0, None, 0, C.byref(nw)) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_decode_window_plan(s.coder.handle, arr, mb, 4, 0, None, 0, None) == _lib.TE_ERR_INVALID_ARG
    bad = (C.c_uint8 * 48)()  # no version, no stripe size: the suffix's own error
    one = batch.decode_descs(objs[:1])
    assert lib.te_decode_window_plan(s.coder.handle, one, bad, 1, 0, None, 0, C.byref(nw)) not in (0, _lib.TE_ERR_INVALID_ARG)


def test_entry_points_validate_then_need_a_device():
    """Every object is validated before anything is enqueued -- and before the call looks for a
    device; without one the compute calls return TE_ERR_NO_DEVICE: there is no CPU fallback."""
    s = _slicer()
    cfg = s._cfg()
    objs, metas, _ = _batch(s, [1_000_001, 4_099], [SEVEN, FULL])
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below returns before any copy
    mb = (C.c_uint8 * len(metas)).from_buffer_copy(metas)
    lv = (C.c_uint8 * (2 * N * 32))()
    st = (C.c_int * 2)(9, 9)
    rej = (C.c_uint32 * 2)()
    h = s.coder.handle

    def plain(arr, meta=mb, slices=fake, out=fake, c=h, pcfg=C.byref(cfg)):
        return lib.te_decode_batch_host(c, pcfg, slices, arr, meta, 2, out, 0)

    def verified(arr, meta=mb, leaves=lv, status=st, slices=fake, out=fake):
        return lib.te_decode_verified_batch_host(h, C.byref(cfg), slices, arr, meta, leaves, 2, out, rej, status, 0)

    good = batch.decode_descs(objs)
    for call in (lambda: plain(good, c=None), lambda: plain(good, pcfg=None), lambda: plain(None),
                 lambda: plain(good, meta=None), lambda: plain(good, slices=None), lambda: plain(good, out=None),
                 lambda: verified(None), lambda: verified(good, meta=None), lambda: verified(good, leaves=None),
                 lambda: verified(good, status=None), lambda: verified(good, slices=None),
                 lambda: verified(good, out=None)):
        assert call() == _lib.TE_ERR_INVALID_ARG
    # fewer than k present slices: the unverified call's error (the second object, so the whole
    # batch is checked); bits past n do not count
    few = batch.decode_descs([objs[0], (objs[1][0], objs[1][1], 0x3F | 1 << 25, objs[1][3])])
    assert plain(few) == _lib.TE_ERR_NOT_ENOUGH_SLICES
    none = batch.decode_descs([objs[0], (objs[1][0], objs[1][1], 0, objs[1][3])])
    assert plain(none) == _lib.TE_ERR_NOT_ENOUGH_SLICES
    # a metadata suffix that disagrees with slice_len: its stripes do not divide slice_len - 48 + 1
    off = batch.decode_descs([(objs[0][0], objs[0][1] + 1, SEVEN, objs[0][3]), objs[1]])
    assert plain(off) == _lib.TE_ERR_INVALID_LAYOUT
    assert verified(off) == _lib.TE_ERR_INVALID_LAYOUT
    off2 = batch.decode_descs([objs[0], (objs[1][0], 47, FULL, objs[1][3])])
    assert plain(off2) == _lib.TE_ERR_INVALID_LAYOUT
    assert verified(off2) == _lib.TE_ERR_INVALID_LAYOUT
    if _lib.device_count() == 0:
        assert plain(good) == _lib.TE_ERR_NO_DEVICE
        assert verified(good) == _lib.TE_ERR_NO_DEVICE
        assert verified(few) == _lib.TE_ERR_NO_DEVICE  # too few slices is the object's outcome, not the call's
        assert lib.te_decode_batch_host(h, C.byref(cfg), None, None, None, 0, None, 0) == _lib.TE_ERR_NO_DEVICE
        import numpy as np
        buf = np.zeros(16, np.uint8)
        with pytest.raises(T.NoDeviceError):
            batch.decode_host(s, buf, objs, metas, buf)
        with pytest.raises(T.NoDeviceError):
            batch.decode_verified_host(s, buf, objs, metas, bytes(2 * N * 32), buf)
        with pytest.raises(T.NoDeviceError):
            batch.StreamReader([s])


def test_stream_reader_argument_rules():
    s = _slicer()
    cfg = s._cfg()
    hs = (C.c_void_p * 1)(s.coder.handle.value)
    r = C.c_void_p(123)
    assert lib.te_stream_reader_new(None, 1, C.byref(cfg), C.byref(r)) == _lib.TE_ERR_INVALID_ARG and r.value is None
    assert lib.te_stream_reader_new(hs, 0, C.byref(cfg), C.byref(r)) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_stream_reader_new(hs, 1, None, C.byref(r)) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_stream_reader_new(hs, 1, C.byref(cfg), None) == _lib.TE_ERR_INVALID_ARG
    null = (C.c_void_p * 1)(None)
    assert lib.te_stream_reader_new(null, 1, C.byref(cfg), C.byref(r)) == _lib.TE_ERR_INVALID_ARG
    if _lib.device_count() == 0:
        assert lib.te_stream_reader_new(hs, 1, C.byref(cfg), C.byref(r)) == _lib.TE_ERR_NO_DEVICE and r.value is None
    t = C.c_uint64(5)
    assert lib.te_stream_read_submit(None, None, None, None, None, 0, None, None, None, C.byref(t)) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_stream_read_wait(None, 1) == _lib.TE_ERR_INVALID_ARG
    lib.te_stream_reader_free(None)


def _header_struct(name):
    txt = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        toks = decl.replace(",", " , ").split()
        if not toks:
            continue
        fields += [(t, toks[0]) for t in toks[1:] if t != ","]
    return fields


def test_read_launch_stats_mirror_and_zero_state():
    fields = _header_struct("te_read_launch_stats")
    names = ["windows", "objects", "slices_uploaded", "bytes_h2d", "bytes_d2h", "slices_hashed_host",
             "slices_hashed_device", "host_waits"]
    assert [f for f, _ in fields] == names == [f for f, _ in _lib.te_read_launch_stats._fields_]
    off = 0
    for f, ctype in fields:
        assert ctype == "uint64_t"
        assert getattr(_lib.te_read_launch_stats, f).offset == off and getattr(_lib.te_read_launch_stats, f).size == 8
        off += 8
    assert C.sizeof(_lib.te_read_launch_stats) == off == 64
    # the read entry points take te_decode_object as te_decode_batch_device does
    assert C.sizeof(_lib.te_decode_object) == 32
    declared = set(_lib.declared_symbols())
    for sym in ("te_decode_window_plan", "te_decode_batch_host", "te_decode_verified_batch_host",
                "te_stream_reader_new", "te_stream_read_submit", "te_stream_read_wait", "te_stream_reader_free",
                "te_clay_read_launch_stats"):
        assert sym in declared and hasattr(lib, sym), sym
    s = _slicer()
    assert lib.te_clay_read_launch_stats(None, None) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_clay_read_launch_stats(s.coder.handle, None) == _lib.TE_ERR_INVALID_ARG
    assert batch.read_launch_stats(s.coder) == dict.fromkeys(names, 0)  # all zero before the first call
