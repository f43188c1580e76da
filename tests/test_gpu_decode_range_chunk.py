"""The chunk path of ranged reads (te_clay_set_range_chunk_path, TE_RANGE_CHUNK) on the device: a
window with exactly one erased data chunk rebuilds that chunk's piece on the windowed recover
class kernels (dec_class_<8 + 2 a0>_win[_small]) and gathers the present pieces.

Every output lands in a poisoned buffer with guard bytes on both sides.  The window's bytes must
equal data[start:start + len] and, bit for bit, the same call with the knob off; every byte outside
must come back unchanged.  Each case asserts its stripe counts (te_clay_range_launch_stats,
te_clay_range_chunk_launch_stats) and its kernel path (te_clay_decode_launch_stats).

Shapes, as in tests/test_gpu_decode_range.py (whose encoded objects are shared): 250,000 B (sub-chunk
144 B), 70,001 B (one stripe, sub-chunk 102 B = 2 mod 4: the aliased last word), 2,300,000 B (the
production row of 1,430 B, three stripes)."""
import ctypes as C
import random

import numpy as np
import pytest

from tape_amd import _lib, batch
from tape_amd._lib import lib

import test_gpu_decode_range as R

pytestmark = pytest.mark.gpu
GUARD, POISON = R.GUARD, R.POISON
N, K = 20, 7
ALL = (1 << N) - 1
CHUNK_CLASSES = set(range(8, 24, 2))


def _slice_of(rotated, st, x):
    return (x + (st * 7) % N) % N if rotated else x


def _geo(s, blob_len):
    g = s.geometry(blob_len)
    return int(g.stripe_size), int(g.chunk_size), int(g.sub_chunk_size), int(g.num_stripes)


def _ptrs(enc, sl, avail):
    """The present slices as te_slicer_decode_range takes them, each a private copy (kept alive)."""
    keep = {i: enc[i * sl:(i + 1) * sl].copy() for i in range(N) if avail >> i & 1}
    ptrs = (C.c_void_p * N)()
    for i, a in keep.items():
        ptrs[i] = a.ctypes.data
    return ptrs, keep


def _call(s, ptrs, sl, start, ln, block, off):
    block[:] = POISON
    got = C.c_size_t()
    cfg = s._cfg()
    r = lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, sl, start, ln,
                                   C.c_void_p(block.ctypes.data + GUARD + off), ln, C.byref(got))
    return r, got.value


def _read(s, data, ptrs, sl, start, ln, block, off, where):
    """One window with the knob on, checked against the object and the guards, then with the knob
    off, bit for bit.  Returns the knob-on call's (range stats, chunk stats, decode launch stats)."""
    batch.set_range_chunk_path(s.coder, True)
    try:
        r, got = _call(s, ptrs, sl, start, ln, block, off)
        assert r == 0 and got == ln, (r, got, where)
        on = block.copy()
        stats = (batch.range_launch_stats(s.coder), batch.range_chunk_launch_stats(s.coder), s.coder.decode_launch_stats())
    finally:
        batch.set_range_chunk_path(s.coder, False)
    assert (on[GUARD + off:GUARD + off + ln] == data[start:start + ln]).all(), ("window bytes", where)
    assert (on[:GUARD + off] == POISON).all(), ("bytes before the window were written", where)
    assert (on[GUARD + off + ln:] == POISON).all(), ("bytes after the window were written", where)
    r, got = _call(s, ptrs, sl, start, ln, block, off)
    assert r == 0 and got == ln, (r, got, where)
    assert (block == on).all(), ("knob on != knob off", where)
    assert batch.range_chunk_launch_stats(s.coder) == {"stripes_rebuilt": 0, "gather_jobs": 0, "bytes_stored": 0}, where
    return stats


def _assert_one_chunk(stats, ln, cs, where, cls=None, gathers=0, stored=None):
    rs, cst, st = stats
    assert cst == {"stripes_rebuilt": 1, "gather_jobs": gathers, "bytes_stored": ln if stored is None else stored}, (cst, where)
    assert (rs["stripes_touched"], rs["stripes_decoded"], rs["stripes_copied"], rs["gather_jobs"]) == (1, 0, 0, gathers), (rs, where)
    # the recover job's k chunks, plus at most the window's present pieces
    assert K * cs <= rs["bytes_staged"] <= K * cs + ln, (rs, where)
    assert len(st["class_launches"]) == 1 and sum(st["class_launches"].values()) == 1, (st, where)
    got = next(iter(st["class_launches"]))
    assert got in CHUNK_CLASSES and (cls is None or got == cls), (st, cls, where)
    assert st["class_g"] == 1 and st["class_stripes"] == 1 and st["direct_out"] == 1, (st, where)
    assert st["table_stripes"] == st["generic_stripes"] == st["jit_stripes"] == 0, (st, where)


def _inner_windows(B, cs, sc):
    """Windows inside the chunk at object byte B (start, len): the edges of the head and tail clip."""
    w = [(B + 401, 1), (B + 401, 2), (B + 400, 3), (B + 401, 3), (B + 403, 1)]      # inside one word
    w += [(B + 403, 2), (B + 402, 5)]                                                # across a word boundary
    w += [(B + 3 * sc - d, 9) for d in (1, 2, 3, 4, 5)]                              # lo in a row's last 5 bytes
    w += [(B + sc - d, 3) for d in (1, 2, 3, 4)]                                     # ... hi in the same tail word
    w += [(B + 7 * sc - 2, 2 * sc + 4)]                                              # whole rows between two clips
    w += [(B, 1), (B + cs - 1, 1), (B + cs - 3, 3), (B, cs)]                         # first byte, last byte(s), whole chunk
    return w


@pytest.mark.parametrize("blob_len", [250_000, 70_001, 2_300_000])
def test_percall_windows_inside_one_erased_chunk(blob_len):
    s, data, enc, sl = R._encoded((20, 7, 16), blob_len)
    S, cs, sc, ns = _geo(s, blob_len)
    assert sc == {250_000: 144, 70_001: 102, 2_300_000: 1430}[blob_len]
    assert batch.range_chunk_path(s.coder) is False  # off by default
    block = batch.host_empty(cs + 2 * GUARD + 3)
    st, x = (1, 2) if ns > 1 else (0, 2)
    gone = _slice_of(1, st, x)
    B = st * S + x * cs
    rng = random.Random(blob_len)
    # one slice missing (19 present: the gateway's degraded track), then 7 survivors without it
    sets = [ALL & ~(1 << gone), sum(1 << i for i in rng.sample([i for i in range(N) if i != gone], K))]
    for si, avail in enumerate(sets):
        ptrs, keep = _ptrs(enc, sl, avail)
        a0 = R._a0([i for i in range(N) if avail >> i & 1], st) if si else None
        wins = [(B + 5 * sc + 8 + a, 37, o) for a in range(4) for o in range(4)] if si == 0 else []  # start x out alignment
        wins += [(a, b, (wi + si) % 4) for wi, (a, b) in enumerate(_inner_windows(B, cs, sc))]
        for start, ln, off in wins:
            where = (blob_len, hex(avail), start, ln, off)
            stats = _read(s, data, ptrs, sl, start, ln, block, off, where)
            _assert_one_chunk(stats, ln, cs, where, cls=None if a0 is None else 8 + 2 * a0)
    # a window ending at blob_len, inside the short last stripe's last chunk
    last = ns - 1
    tail = blob_len - last * S
    x = (tail - 1) // cs
    ln = min(777, tail - x * cs)
    avail = ALL & ~(1 << _slice_of(1, last, x))
    ptrs, keep = _ptrs(enc, sl, avail)
    for off in (1, 2):
        where = (blob_len, "tail", ln, off)
        _assert_one_chunk(_read(s, data, ptrs, sl, blob_len - ln, ln, block, off, where), ln, cs, where)


def test_windows_touching_neighbouring_chunks():
    """Identity mapping, slice 3 absent: windows across 2 and 3 chunks and across every stripe
    rebuild shard 3 alone and gather the rest.  Under a parity-only survivor set the same windows
    hold two or more erased chunks and stay TE_RANGE_DECODE."""
    blob_len = 250_000
    s, data, enc, sl = R._encoded((20, 7, 16), blob_len, rotated=False)
    S, cs, sc, ns = _geo(s, blob_len)
    block = batch.host_empty(blob_len + 2 * GUARD + 3)
    wins = [(3 * cs - 10, 30, 1, 20), (3 * cs - 1, 2, 1, 1), (4 * cs - 2, 5, 1, 2), (2 * cs + 5, 2 * cs, 2, cs),
            (S + 3 * cs - 7, cs + 14, 2, cs)]  # (start, len, gather jobs, bytes rebuilt)
    ptrs, keep = _ptrs(enc, sl, ALL & ~(1 << 3))
    for wi, (start, ln, gathers, stored) in enumerate(wins):
        where = ("slice 3 absent", start, ln)
        _assert_one_chunk(_read(s, data, ptrs, sl, start, ln, block, wi % 4, where), ln, cs, where, gathers=gathers, stored=stored)
    # the whole object: three chunk stripes (the last one's window ends inside chunk 3)
    tail = blob_len - 2 * S
    assert 3 * cs < tail < 4 * cs
    rs, cst, st = _read(s, data, ptrs, sl, 0, blob_len, block, 3, "whole object")
    assert cst == {"stripes_rebuilt": 3, "gather_jobs": 6 + 6 + 3, "bytes_stored": 2 * cs + tail - 3 * cs}, cst
    assert (rs["stripes_touched"], rs["stripes_decoded"], rs["stripes_copied"], rs["gather_jobs"]) == (3, 0, 0, 15), rs
    assert set(st["class_launches"]) <= CHUNK_CLASSES and st["class_stripes"] == 3 and st["class_g"] == 1, st
    # parity only: two or more erased chunks per window
    par = sum(1 << i for i in range(13, 20))
    ptrs, keep = _ptrs(enc, sl, par)
    for wi, (start, ln, _, _) in enumerate(wins):
        rs, cst, st = _read(s, data, ptrs, sl, start, ln, block, wi % 4, ("parity only", start, ln))
        assert cst == {"stripes_rebuilt": 0, "gather_jobs": 0, "bytes_stored": 0}, (cst, start, ln)
        assert (rs["stripes_touched"], rs["stripes_decoded"], rs["stripes_copied"]) == (1, 1, 0), (rs, start, ln)
        assert st["class_launches"] == {0: 1} and st["class_stripes"] == 1, (st, start, ln)  # a0 = 0: the decode class


@pytest.mark.parametrize("a0", range(8))
def test_every_recover_class(a0):
    """Identity mapping, one 7-survivor set per class: a0 known column-0 nodes (1..a0) and 7 - a0
    column-1 nodes, data node 0 erased (a0 = 7: known {1..6, 7}, lost node 0); for a0 < 6 data node 6
    is erased too and is rebuilt as well.  The launch must be class 8 + 2 a0, per-call kernel."""
    blob_len = 70_001
    s, data, enc, sl = R._encoded((20, 7, 16), blob_len, rotated=False)
    S, cs, sc, ns = _geo(s, blob_len)
    surv = list(range(1, a0 + 1)) + list(range(10, 10 + K - a0))
    assert len(surv) == K and sum(1 for v in surv if v < 10) == a0 and 0 not in surv
    ptrs, keep = _ptrs(enc, sl, sum(1 << i for i in surv))
    block = batch.host_empty(cs + 2 * GUARD + 3)
    for x in (0, 6) if a0 < 6 else (0,):
        B = x * cs
        hi = min(cs, blob_len - B)  # chunk 6 ends at blob_len
        for wi, (start, ln) in enumerate(((B + sc - 3, 2 * sc + 5), (B + 1, 2), (B, hi))):
            where = (a0, x, start, ln)
            _assert_one_chunk(_read(s, data, ptrs, sl, start, ln, block, (wi + a0) % 4, where), ln, cs, where, cls=8 + 2 * a0)


def test_batch_mixes_chunk_copy_and_decode_stripes():
    """One te_decode_range_batch_device call: 96 objects each with a window that rebuilds one chunk
    (more than the per-call threshold of 64 stripes: the G = 2 kernels), 10 copy-only objects and 24
    full-decode objects, odd out_offs, against the object bytes and against the knob-off call."""
    import torch
    blob_len = 250_000
    s, data, enc, sl = R._encoded((20, 7, 16), blob_len)
    S, cs, sc, ns = _geo(s, blob_len)
    rng = random.Random(0xC40C)
    stride = 2 * cs + 2 * GUARD + 4
    objs, want_chunk_cls, want_dec_cls, gather_chunk, gather_copy, stored = [], set(), set(), 0, 0, 0
    nchunk, ncopy, ndec = 96, 10, 24
    for i in range(nchunk + ncopy + ndec):
        out_off = GUARD + i * stride + (1, 3, 2, 0)[i % 4]
        if i < nchunk:
            st, x = rng.randrange(2), rng.randrange(1, 6)
            gone = _slice_of(1, st, x)
            # keep the neighbours' slices so a window over two chunks has exactly one erased
            near = [_slice_of(1, st, x - 1), _slice_of(1, st, x + 1)]
            surv = sorted(near + rng.sample([v for v in range(N) if v != gone and v not in near], K - 2))
            B = st * S + x * cs
            kind = i % 4
            if kind == 0:
                start, ln, g = B + rng.randrange(cs - 64), rng.randrange(1, 64), 0
            elif kind == 1:
                start, ln, g = B, cs, 0
            elif kind == 2:
                start, ln, g = B - 9, 30, 1             # across the chunk's start
            else:
                start, ln, g = B + cs - 5, 11, 1        # across the chunk's end
            want_chunk_cls.add(8 + 2 * R._a0(surv, st))
            gather_chunk += g
            stored += min(start + ln, B + cs) - max(start, B)
        elif i < nchunk + ncopy:
            surv = list(range(N))
            start, ln = rng.randrange(S - 2 * cs), rng.randrange(1, 2 * cs)   # inside stripe 0
            gather_copy += (start + ln - 1) // cs - start // cs + 1
        else:
            a0 = i % 4   # stripe 0 (no rotation): column-0 parity nodes 7..9 and column 1 -- every data chunk erased
            surv = sorted([7, 8, 9][:a0] + rng.sample(range(10, 20), K - a0))
            start, ln = rng.randrange(cs), cs + rng.randrange(1, cs)   # two chunks of stripe 0, both erased
            want_dec_cls.add(a0)
        objs.append((0, sl, sum(1 << v for v in surv), out_off, start, ln))
    for o in objs[nchunk:]:
        assert o[4] + o[5] <= S and o[5] <= 2 * cs   # one stripe each
    assert all(o[5] <= 2 * cs for o in objs)
    metas = enc[sl - 48:sl].tobytes() * len(objs)
    d_sl = torch.from_numpy(enc).cuda()
    total = len(objs) * stride + 2 * GUARD
    expect = np.full(total, POISON, np.uint8)
    for (_, _, _, off, start, ln) in objs:
        expect[off:off + ln] = data[start:start + ln]
    d_on = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    d_off = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    batch.set_range_chunk_path(s.coder, True)
    try:
        batch.decode_range_batch(s, d_sl, objs, metas, d_on)
        torch.cuda.synchronize()
        rs, cst, st = batch.range_launch_stats(s.coder), batch.range_chunk_launch_stats(s.coder), s.coder.decode_launch_stats()
    finally:
        batch.set_range_chunk_path(s.coder, False)
    got = d_on.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (bad[:8], bad.size)
    assert cst == {"stripes_rebuilt": nchunk, "gather_jobs": gather_chunk, "bytes_stored": stored}, (cst, rs)
    assert (rs["stripes_touched"], rs["stripes_decoded"], rs["stripes_copied"]) == (len(objs), ndec, ncopy), rs
    assert rs["gather_jobs"] == gather_chunk + gather_copy and rs["bytes_staged"] == 0, rs
    assert st["class_g"] == 2 and st["class_stripes"] == nchunk + ndec, st
    assert st["table_stripes"] == st["generic_stripes"] == st["jit_stripes"] == 0, st
    assert {c for c in st["class_launches"] if c < 8} == want_dec_cls == {0, 1, 2, 3}, st    # the decode stripes only
    assert {c for c in st["class_launches"] if c >= 8} == want_chunk_cls, (st, want_chunk_cls)
    assert all(v == 1 for v in st["class_launches"].values()), st                            # one launch per class
    # knob off: bit-identical output, today's counts
    batch.decode_range_batch(s, d_sl, objs, metas, d_off)
    torch.cuda.synchronize()
    assert torch.equal(d_on, d_off)
    rs0 = batch.range_launch_stats(s.coder)
    assert (rs0["stripes_touched"], rs0["stripes_decoded"], rs0["stripes_copied"]) == (len(objs), ndec + nchunk, ncopy), rs0
    assert batch.range_chunk_launch_stats(s.coder) == {"stripes_rebuilt": 0, "gather_jobs": 0, "bytes_stored": 0}


def test_knob_and_edges():
    blob_len = 250_000
    s, data, enc, sl = R._encoded((20, 7, 16), blob_len)
    S, cs, sc, ns = _geo(s, blob_len)
    zero = {"stripes_rebuilt": 0, "gather_jobs": 0, "bytes_stored": 0}
    fresh = R._slicer()
    assert batch.range_chunk_path(fresh.coder) is False and batch.range_chunk_launch_stats(fresh.coder) == zero
    block = batch.host_empty(cs + 2 * GUARD + 3)
    avail = ALL & ~(1 << 2)  # stripe 0 (no rotation): shard 2 erased
    ptrs, keep = _ptrs(enc, sl, avail)
    start, ln = 2 * cs + 100, 50
    # off: the new stats are zero, the ranged stats and the kernel path are the decode's
    assert _call(s, ptrs, sl, start, ln, block, 1) == (0, ln)
    assert (block[GUARD + 1:GUARD + 1 + ln] == data[start:start + ln]).all()
    assert batch.range_chunk_launch_stats(s.coder) == zero
    rs = batch.range_launch_stats(s.coder)
    assert (rs["stripes_touched"], rs["stripes_decoded"], rs["stripes_copied"], rs["gather_jobs"]) == (1, 1, 0, 0), rs
    assert rs["bytes_staged"] == K * cs, rs
    st = s.coder.decode_launch_stats()
    assert set(st["class_launches"]) <= set(range(8)) and st["class_stripes"] == 1, st
    batch.set_range_chunk_path(s.coder, True)
    try:
        assert batch.range_chunk_path(s.coder) is True
        # len == 0 writes nothing and touches nothing
        assert _call(s, ptrs, sl, start, 0, block, 2) == (0, 0)
        assert (block == POISON).all()
        assert batch.range_chunk_launch_stats(s.coder) == zero and batch.range_launch_stats(s.coder)["stripes_touched"] == 0
        # fewer than k slices
        few, keep2 = _ptrs(enc, sl, 0b111111 << 8)
        assert _call(s, few, sl, start, ln, block, 0)[0] == _lib.TE_ERR_NOT_ENOUGH_SLICES
        assert (block == POISON).all()
        # the planner names what the call does
        assert s.range_plan_ex(blob_len, avail, start, ln) == (0, [(_lib.RANGE_CHUNK, start, start + ln, 2)])
        assert _call(s, ptrs, sl, start, ln, block, 3) == (0, ln)
        assert batch.range_chunk_launch_stats(s.coder) == {"stripes_rebuilt": 1, "gather_jobs": 0, "bytes_stored": ln}
    finally:
        batch.set_range_chunk_path(s.coder, False)
    # Clay(20,10,19) has no class kernels: the knob changes nothing there
    p = (20, 10, 19)
    s2, data2, enc2, sl2 = R._encoded(p, blob_len)
    cs2 = int(s2.geometry(blob_len).chunk_size)
    block2 = batch.host_empty(cs2 + 2 * GUARD + 3)
    ptrs2, keep3 = _ptrs(enc2, sl2, ALL & ~(1 << 2))
    stats = _read(s2, data2, ptrs2, sl2, 2 * cs2 + 100, 50, block2, 1, p)
    assert stats[1] == zero and stats[0]["stripes_decoded"] == 1, stats
    assert stats[2]["table_stripes"] + stats[2]["generic_stripes"] == 1 and stats[2]["class_stripes"] == 0, stats
    assert s2.range_plan_ex(blob_len, ALL & ~(1 << 2), 2 * cs2 + 100, 50)[1][0][0] == _lib.RANGE_DECODE
