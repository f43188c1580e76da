"""Ranged reads on the device: te_slicer_decode_range and te_decode_range_batch_device against the
original object bytes x[start:start + len], through every store path the window's head clip
touches -- the per-call `_small` class kernels, the batched G = 2 class kernels, the table-driven
kernel and the generic kernel -- and the gather of copy stripes.

Every output lands in a poisoned buffer with guard bytes on both sides of the object's len bytes;
every byte outside must come back unchanged.  Each case asserts its kernel path from
te_clay_decode_launch_stats and its stripe counts from te_clay_range_launch_stats against the
plan computed in plain Python (tests/test_range_plan.py checks the same arithmetic on the host).

Run as a program (`python tests/test_gpu_decode_range.py table`) this file is the child process of
test_table_kernel_windows: the same windows with the class kernels switched off by the engine's
measurement knob, which is read once per process."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tape_amd as T  # noqa: E402
from tape_amd import _lib, batch  # noqa: E402
from tape_amd._lib import lib  # noqa: E402
from tape_amd.slicer import ClayParams, EncodingProfile  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = 0xA5


def _slicer(params=(20, 7, 16), rotated=True):
    n, k, d = params
    coder = T.ClayCoder(n, k, d)
    s = T.Slicer.with_rotation(coder) if rotated else T.Slicer(coder)
    s.profile = EncodingProfile.clay(ClayParams(n | k << 8 | d << 16))
    return s


_ENC = {}


def _encoded(params, blob_len, rotated=True):
    """(slicer, data, slices array, slice_len), encoded once per object by the engine (checked
    against the oracle in test_gpu_parity.py) and left unchanged."""
    key = (params, blob_len, rotated)
    if key not in _ENC:
        s = _slicer(params, rotated)
        data = np.random.default_rng(blob_len + params[1]).integers(0, 256, blob_len, dtype=np.uint8)
        g = s.geometry(blob_len)
        sl = int(g.slice_len)
        out = np.empty(params[0] * sl, np.uint8)
        cfg = s._cfg()
        assert lib.te_slicer_encode(s.coder.handle, C.byref(cfg), C.c_void_p(data.ctypes.data), blob_len,
                                    C.c_void_p(out.ctypes.data), out.size) == 0
        _ENC[key] = (s, data, out, sl)
    return _ENC[key]


def _py_plan(s, n, blob_len, avail, start, ln):
    """[(copy?, lo, hi)] per touched stripe, in plain arithmetic."""
    g = s.geometry(blob_len)
    S, cs = int(g.stripe_size), int(g.chunk_size)
    rotated = s.strategy == T.MappingStrategy.Rotated
    if ln == 0:
        return []
    out = []
    for st in range(start // S, (start + ln - 1) // S + 1):
        lo = max(start - st * S, 0)
        hi = min(start + ln, (st + 1) * S, blob_len) - st * S
        sl_of = lambda x: (x + (st * 7) % n) % n if rotated else x  # noqa: E731
        out.append((all(avail >> sl_of(x) & 1 for x in range(lo // cs, (hi - 1) // cs + 1)), lo, hi))
    return out


def _windows(s, blob_len):
    """The edges of the head clip: every byte alignment, windows inside one word, across a word
    boundary, lo in the last 5 bytes of a sub-chunk row, on and around a chunk and a stripe
    boundary, ending inside the short last stripe, the whole object."""
    g = s.geometry(blob_len)
    S, cs, sc, ns = int(g.stripe_size), int(g.chunk_size), int(g.sub_chunk_size), int(g.num_stripes)
    base = (ns - 1) * S if ns > 1 and blob_len - (ns - 1) * S > 3 * cs else 0  # a stripe other than 0 when there is one
    w = [(base + cs + 5 * sc + 8 + a, 37) for a in range(4)]                      # the four alignments
    w += [(base + 401, 1), (base + 401, 2), (base + 400, 3), (base + 401, 3), (base + 403, 1)]  # inside one word
    w += [(base + 403, 2), (base + 402, 5)]                                       # across a word boundary
    w += [(base + 2 * cs + 3 * sc - d, 9) for d in (1, 2, 3, 4, 5)]               # the row's last 5 bytes
    w += [(base + sc - d, 3) for d in (1, 2, 3, 4)]                               # ... with hi in the same tail word
    w += [(base + 2 * cs + d, 11) for d in (-1, 0, 1)]                            # a chunk boundary
    if ns > 1:
        w += [(S + d, 11) for d in (-1, 0, 1)] + [(S - 2, 3), (S - 7, 2 * S + 9 - S)]  # a stripe boundary
        w += [(S - 3, blob_len - 5 - (S - 3))]                                    # every stripe, both ends inside
    w += [(blob_len - 777, 500), (blob_len - 3, 3), (blob_len - 1, 1)] if blob_len > 1000 else []
    w += [(0, 1), (0, blob_len)]
    return [(a, b) for a, b in w if 0 <= a and a + b <= blob_len and b > 0]


def _check_stats(s, k, plan, cs, sc, path, where):
    rs = batch.range_launch_stats(s.coder)
    ndec = sum(1 for c, _, _ in plan if not c)
    assert rs["stripes_touched"] == len(plan), (rs, where)
    assert rs["stripes_decoded"] == ndec and rs["stripes_copied"] == len(plan) - ndec, (rs, plan, where)
    assert rs["gather_jobs"] == sum((hi - 1) // cs - lo // cs + 1 for c, lo, hi in plan if c), (rs, where)
    assert 0 < rs["bytes_staged"] <= k * len(plan) * cs, (rs, where)
    st = s.coder.decode_launch_stats()
    got = {"class": st["class_stripes"], "table": st["table_stripes"], "generic": st["generic_stripes"]}
    want = {"class": 0, "table": 0, "generic": 0}
    want[path] = ndec
    assert got == want and st["jit_launches"] == 0, (st, where)
    if path == "class" and ndec:
        assert st["class_g"] == 1, (st, where)  # a per-call decode: the one-wave `_small` kernels
    return st


def _run_percall(params, blob_len, path, nsets=2, windows=None):
    """te_slicer_decode_range of every window into a page-locked block (the kernels store into it
    directly) at the four alignments of `out`, under nsets survivor sets."""
    n, k, _ = params
    s, data, enc, sl = _encoded(params, blob_len)
    g = s.geometry(blob_len)
    cs, sc = int(g.chunk_size), int(g.sub_chunk_size)
    rng = random.Random(blob_len * 31 + k)
    cfg = s._cfg()
    block = batch.host_empty(blob_len + 2 * GUARD + 3)
    for si in range(nsets):
        # Clay(20,7,16): the worst case (parity only), then a random set; the other profiles: random
        # sets (a survivor set that is one whole column of Clay(20,10,19) has no plane program
        # and decodes on the generic kernel, in the full decode alike)
        survivors = list(range(n - k, n)) if si == 0 and k == 7 else sorted(rng.sample(range(n), k))
        avail = sum(1 << i for i in survivors)
        keep = {i: enc[i * sl:(i + 1) * sl].copy() for i in survivors}
        ptrs = (C.c_void_p * n)()
        for i, a in keep.items():
            ptrs[i] = a.ctypes.data
        for wi, (start, ln) in enumerate(windows or _windows(s, blob_len)):
            off = (wi + si) % 4
            block[:] = POISON
            got = C.c_size_t()
            r = lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, sl, start, ln,
                                           C.c_void_p(block.ctypes.data + GUARD + off), ln, C.byref(got))
            where = (params, blob_len, survivors, start, ln, off)
            assert r == 0 and got.value == ln, (r, where)
            assert (block[GUARD + off:GUARD + off + ln] == data[start:start + ln]).all(), where
            assert (block[:GUARD + off] == POISON).all(), ("bytes before the window were written", where)
            assert (block[GUARD + off + ln:] == POISON).all(), ("bytes after the window were written", where)
            st = _check_stats(s, k, _py_plan(s, n, blob_len, avail, start, ln), cs, sc, path, where)
            assert st["direct_out"] == 1, (st, where)


# 250,000 B: sub-chunk 144 B (36 words); 70,001 B: one stripe with its own chunk size, sub-chunk
# 102 B = 2 mod 4 (the aliased last word); 2,300,000 B: the production row of 1,430 B
@pytest.mark.parametrize("blob_len", [250_000, 70_001, 2_300_000])
def test_percall_class_kernel_windows(blob_len):
    s = _slicer()
    sc = int(s.geometry(blob_len).sub_chunk_size)
    assert sc == {250_000: 144, 70_001: 102, 2_300_000: 1430}[blob_len]
    _run_percall((20, 7, 16), blob_len, "class")


def test_full_window_equals_full_decode_percall():
    s, data, enc, sl = _encoded((20, 7, 16), 250_000)
    chunks = [(i, enc[i * sl:(i + 1) * sl].tobytes()) for i in (1, 4, 6, 9, 12, 15, 19)]
    full = s.decode(chunks)
    assert full == data.tobytes()
    assert s.decode_range(chunks, 0, len(full)) == full


def test_python_mirror():
    s, data, enc, sl = _encoded((20, 7, 16), 250_000)
    chunks = [(i, enc[i * sl:(i + 1) * sl].tobytes()) for i in (0, 2, 3, 8, 11, 16, 18)]
    full = s.decode(chunks)
    for start, ln in ((0, 0), (0, 1), (99_999, 2), (100_001, 57_123), (249_999, 1), (123_457, 3), (7, 249_990)):
        assert s.decode_range(chunks, start, ln) == full[start:start + ln], (start, ln)
    with pytest.raises(T.EngineError):
        s.decode_range(chunks, 249_999, 2)


@pytest.mark.parametrize("blob_len", [250_000, 70_001])
def test_all_slices_present_is_copy_only(blob_len):
    """All 20 slices: every window of the grid is gathered from the data chunks -- no decode
    launch, although the full decode would pad 13 erasures and decode every stripe."""
    n = 20
    s, data, enc, sl = _encoded((20, 7, 16), blob_len)
    cfg = s._cfg()
    ptrs = (C.c_void_p * n)()
    keep = [enc[i * sl:(i + 1) * sl].copy() for i in range(n)]
    for i, a in enumerate(keep):
        ptrs[i] = a.ctypes.data
    block = np.empty(blob_len + 2 * GUARD + 3, np.uint8)  # pageable: staged, then copied out
    for wi, (start, ln) in enumerate(_windows(s, blob_len)):
        off = wi % 4
        block[:] = POISON
        got = C.c_size_t()
        assert lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, sl, start, ln,
                                          C.c_void_p(block.ctypes.data + GUARD + off), ln, C.byref(got)) == 0
        assert (block[GUARD + off:GUARD + off + ln] == data[start:start + ln]).all(), (start, ln)
        assert (block[:GUARD + off] == POISON).all() and (block[GUARD + off + ln:] == POISON).all(), (start, ln)
        rs = batch.range_launch_stats(s.coder)
        assert rs["stripes_decoded"] == 0 and rs["stripes_copied"] == rs["stripes_touched"] > 0, rs
        assert rs["bytes_staged"] == ln, rs  # a copy stripe stages only the bytes it reads
        st = s.coder.decode_launch_stats()
        assert st["class_stripes"] + st["table_stripes"] + st["generic_stripes"] + st["jit_stripes"] == 0, st
        assert sum(st["class_launches"].values()) + st["table_launches"] + st["generic_launches"] == 0, st


def test_copy_and_decode_stripes_in_one_call():
    """Only the 7 data slices: under rotation stripe 0's chunks are all present (copy) while
    stripes 1 and 2 keep theirs in missing slices (decode)."""
    n, blob_len = 20, 250_000
    s, data, enc, sl = _encoded((20, 7, 16), blob_len)
    avail = 0x7F
    cfg = s._cfg()
    ptrs = (C.c_void_p * n)()
    keep = [enc[i * sl:(i + 1) * sl].copy() for i in range(7)]
    for i, a in enumerate(keep):
        ptrs[i] = a.ctypes.data
    block = batch.host_empty(blob_len + 2 * GUARD + 3)
    for start, ln in ((0, blob_len), (99_990, 20), (14_399, 200_000), (5, 99_995)):
        plan = _py_plan(s, n, blob_len, avail, start, ln)
        block[:] = POISON
        got = C.c_size_t()
        assert lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, sl, start, ln,
                                          C.c_void_p(block.ctypes.data + GUARD + 1), ln, C.byref(got)) == 0
        assert (block[GUARD + 1:GUARD + 1 + ln] == data[start:start + ln]).all(), (start, ln)
        assert (block[:GUARD + 1] == POISON).all() and (block[GUARD + 1 + ln:] == POISON).all(), (start, ln)
        _check_stats(s, 7, plan, int(s.geometry(blob_len).chunk_size), 144, "class", (start, ln))
    assert [c for c, _, _ in _py_plan(s, n, blob_len, avail, 0, blob_len)] == [True, False, False]


def test_percall_more_than_64_stripes():
    """te_slicer_decode_range over more than 64 touched stripes leaves the zero-copy path: the
    staged pieces go to device memory, the decode runs there and the window's bytes are copied
    back.  A 67,000,000 B object is 67 stripes of 1 MB (the production row): two windows over 66 of them
    under 7-of-20 survivor sets (decode stripes, and the copy stripes the rotation leaves), one over all 67 with
    every slice present (copy only), into a pageable poisoned buffer."""
    n, blob_len = 20, 67_000_000
    s, data, enc, sl = _encoded((20, 7, 16), blob_len)
    g = s.geometry(blob_len)
    S, cs, sc = int(g.stripe_size), int(g.chunk_size), int(g.sub_chunk_size)
    assert (int(g.num_stripes), S, sc) == (67, 1_000_000, 1430)
    cfg = s._cfg()
    block = np.empty(blob_len + 2 * GUARD + 3, np.uint8)
    for survivors, start, ln, off in (([0, 2, 3, 8, 11, 16, 18], S + 4_321, 66 * S - 4_321 - 1_234, 3),
                                      (list(range(13, 20)), S - 1, 65 * S + 2, 1),
                                      (list(range(n)), 5, blob_len - 9, 2)):
        avail = sum(1 << i for i in survivors)
        ptrs = (C.c_void_p * n)()
        for i in survivors:
            ptrs[i] = enc.ctypes.data + i * sl
        plan = _py_plan(s, n, blob_len, avail, start, ln)
        assert len(plan) > 64
        block[:] = POISON
        got = C.c_size_t()
        r = lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, sl, start, ln,
                                       C.c_void_p(block.ctypes.data + GUARD + off), ln, C.byref(got))
        where = (survivors, start, ln)
        assert r == 0 and got.value == ln, (r, where)
        assert (block[GUARD + off:GUARD + off + ln] == data[start:start + ln]).all(), where
        assert (block[:GUARD + off] == POISON).all() and (block[GUARD + off + ln:] == POISON).all(), where
        ndec = sum(1 for c, _, _ in plan if not c)
        rs = batch.range_launch_stats(s.coder)
        assert (rs["stripes_touched"], rs["stripes_decoded"], rs["stripes_copied"]) == (len(plan), ndec, len(plan) - ndec), (rs, where)
        assert 0 < rs["bytes_staged"] <= 7 * len(plan) * cs, (rs, where)
        if len(survivors) == n:
            assert ndec == 0 and rs["bytes_staged"] == ln, (rs, where)
        else:
            assert ndec > 50, (ndec, where)
        st = s.coder.decode_launch_stats()
        assert st["direct_out"] == 0 and st["jit_stripes"] == st["generic_stripes"] == 0, (st, where)
        # more than 64 but fewer than 1,024 stripes in more class groups than streams: one
        # table-driven launch (the mid-size routing of the full decode); else the class kernels
        assert st["class_stripes"] + st["table_stripes"] == ndec, (st, where)
        if ndec > 64 and st["table_stripes"]:
            assert (st["table_launches"], st["table_stripes"], st["class_stripes"]) == (1, ndec, 0), (st, where)


def _a0(survivors, st, n=20):
    """Known column-0 nodes of stripe st under rotation: the stripe's decode class."""
    return sum(1 for sl in survivors if (sl - (st * 7) % n) % n < 10)


def test_batched_class_kernels_random_windows():
    """400 objects of 250,000 B in one te_decode_range_batch_device call, random 7-of-20 survivor
    sets and a different window each (single bytes, sub-word, whole objects, and windows with both
    ends inside a stripe), odd out_offs: at least 1,024 decode stripes, so the G = 2 class kernels
    run on forked streams.  Then the same call with whole-object windows against
    te_decode_batch_device, byte for byte."""
    import torch
    n, nobj, blob_len = 20, 400, 250_000
    # the objects share one encoded copy (slices_off 0): what differs is the survivor set, the
    # window and where it lands
    s, data, enc, sl = _encoded((20, 7, 16), blob_len)
    g = s.geometry(blob_len)
    S, cs = int(g.stripe_size), int(g.chunk_size)
    rng = random.Random(0xBA7C4)
    objs, plans, classes = [], [], set()
    stride = blob_len + 2 * GUARD + 4  # a multiple of 4: the alignment of out_off is the term added below
    assert stride % 4 == 0 and GUARD % 4 == 0
    for i in range(nobj):
        a0 = i % 8  # stripe 0's class; the rotation gives stripes 1 and 2 others
        surv = sorted(rng.sample(range(10), a0) + rng.sample(range(10, 20), 7 - a0))
        avail = sum(1 << x for x in surv)
        kind = i % 50
        if kind == 0:
            start, ln = rng.randrange(blob_len), 1
        elif kind == 1:
            start = rng.randrange(blob_len - 3)
            ln = rng.choice((2, 3))
        elif kind == 2:
            start, ln = 0, blob_len
        else:
            start = rng.randrange(0, S - 1)
            ln = rng.randrange(2 * S + 1, blob_len) - start + 1
        plan = _py_plan(s, n, blob_len, avail, start, ln)
        for j, (c, _, _) in enumerate(plan):
            if not c:
                classes.add(_a0(surv, start // S + j))
        objs.append((0, sl, avail, GUARD + i * stride + (1, 3, 2, 0)[i % 4], start, ln))
        plans.append(plan)
    ndec = sum(1 for p in plans for c, _, _ in p if not c)
    # odd out_offs, and every alignment mod 4, among the decode objects and among the copy stripes' objects
    assert sum(o[3] & 1 for o in objs) == nobj // 2 and {o[3] % 4 for o in objs} == {0, 1, 2, 3}
    assert {o[3] % 4 for o, p in zip(objs, plans) if any(c for c, _, _ in p)} == {0, 1, 2, 3}
    assert classes == set(range(8)), classes   # checked on the host, before anything runs
    assert ndec >= 1024, ndec                  # the batched class kernels' routing threshold
    metas = enc[sl - 48:sl].tobytes() * nobj
    d_sl = torch.from_numpy(enc).cuda()
    expect = np.full(nobj * stride + 2 * GUARD, POISON, np.uint8)
    for (_, _, _, off, start, ln) in objs:
        expect[off:off + ln] = data[start:start + ln]
    d_out = torch.full((expect.size,), POISON, dtype=torch.uint8, device="cuda")
    batch.decode_range_batch(s, d_sl, objs, metas, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (bad[:8], bad.size)
    rs = batch.range_launch_stats(s.coder)
    assert rs["stripes_touched"] == sum(len(p) for p in plans) and rs["stripes_decoded"] == ndec, rs
    assert rs["stripes_copied"] == rs["stripes_touched"] - ndec and rs["bytes_staged"] == 0, rs
    st = s.coder.decode_launch_stats()
    assert st["class_stripes"] == ndec and st["table_stripes"] == st["generic_stripes"] == st["jit_stripes"] == 0, st
    assert st["class_g"] == 2 and st["class_streams"] >= 2, st
    assert sorted(st["class_launches"]) == list(range(8)), st
    # whole-object windows == the full decode
    full_objs = [(0, sl, o[2], o[3], 0, blob_len) for o in objs]
    d_a = torch.full((expect.size,), POISON, dtype=torch.uint8, device="cuda")
    d_b = torch.full((expect.size,), POISON, dtype=torch.uint8, device="cuda")
    batch.decode_range_batch(s, d_sl, full_objs, metas, d_a)
    batch.decode_batch(s, d_sl, [(0, sl, o[2], o[3]) for o in objs], metas, d_b)
    torch.cuda.synchronize()
    assert torch.equal(d_a, d_b)
    a = d_a.cpu().numpy()
    for (_, _, _, off, _, _) in objs[:40]:
        assert (a[off:off + blob_len] == data).all()


def _table_child():
    """The windows of the per-call case on the table-driven kernel (class kernels off), and one
    Clay(20,10,19) object, whose decode always runs it."""
    assert os.environ.get("TEC_DEC_CLASS") == "0" and os.environ.get("TEC_DEBUG_KNOBS") == "1"
    _run_percall((20, 7, 16), 250_000, "table")
    _run_percall((20, 7, 16), 70_001, "table", nsets=1)
    _run_percall((20, 10, 19), 250_000, "table")
    print("table-kernel windows ok")


def test_table_kernel_windows():
    env = dict(os.environ, TEC_DEBUG_KNOBS="1", TEC_DEC_CLASS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "table"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "table-kernel windows ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_table_kernel_other_profile():
    """Clay(20,10,19) has no class kernels: its windows run the table-driven kernel in this process too."""
    _run_percall((20, 10, 19), 250_000, "table", nsets=1)


def test_generic_kernel_windows():
    """Clay(12,8,11) (q = 4, t = 3) decodes on the generic kernel: head straddle, sub-word, whole."""
    blob_len = 250_000
    s = _slicer((12, 8, 11))
    cs = int(s.geometry(blob_len).chunk_size)
    _run_percall((12, 8, 11), blob_len, "generic",
                 windows=[(100_000 + 2 * cs + 3, 4 * cs + 6), (100_000 + cs + 9, 2), (100_000 + cs + 10, 3), (0, blob_len)])


if __name__ == "__main__":
    assert sys.argv[1:] == ["table"]
    _table_child()
