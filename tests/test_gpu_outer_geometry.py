"""Every GF(2^16) outer-coder kernel (tape_amd/csrc/rs16.hip) at the edges of its selection rules,
asserted from te_outer_last_launch_stats: rs16_matrix_kernel<G, KB, PTRS, TV, TB> (encode by
strides, decode by pointer arguments), rs16_encode_low_kernel<C>, both rates of rs16_encode_kernel
and the rs16_decode_kernel<KB, TLDS> instances that can be reached.  kernels.hpp picks the kernel
from (k, m) or (k, missing) -- rs16_mat_supported, rs16_mat_tail_bytes -- and engine.cpp from
rs16::chunk / work_len; the paths asserted here were derived from those by hand and are literals.

Each case drives the device entry points (encode_device, decode_device, decode_device_batch) on 2
segments (unless stated) whose strides leave gaps between segments, into an output pre-filled with
0xA5 with 4 KiB of guard on both sides inside the same allocation, at three chunk sizes: 64 B (32
elements, under one wave), 1,088 B (544 elements: a partial 256-thread block and a partial
512-thread tile) and 2,112 B (1,056 elements: past the transform kernel's 1,024-thread block).  The
whole allocation is compared: every produced chunk bit-exact with the oracle (encode:
oracle.rs16.encode per segment; decode: the original data chunks, and once per (k, n)
oracle.rs16.decode), every guard and gap byte still 0xA5.  Inputs are seeded random bytes with two
elements of every shard forced to 0x0000 and 0xffff, so nibble indices 0 and 15 occur in every
table."""
import itertools
import random

import numpy as np
import pytest

from oracle import rs16
from tape_amd import _lib, outer
from tape_amd.slicer import EngineError

pytestmark = pytest.mark.gpu

GUARD = 4096
POISON = 0xA5
SIZES = (64, 1088, 2112)
LDS_MAX = 160 * 1024
NO_LAUNCH = {"matrix_launches": 0, "transform_launches": 0, "low_reg_launches": 0, "decode_launches": 0}


def _torch():
    import torch
    return torch


def _shards(rng, count, cb):
    """`count` random shards of cb bytes; in each, one element 0x0000 and the next 0xffff."""
    a = rng.integers(0, 256, (count, cb), dtype=np.uint8)
    for j in range(count):
        e = (2 * j) % 30
        a[j, e] = a[j, e + 32] = 0x00
        a[j, e + 1] = a[j, e + 33] = 0xFF
    return a


def _expect_stats(st, want):
    got = {f: st[f] for f in want}
    assert got == want, (got, want, st)


def _same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError("%s: %d bytes differ, first at %d (got %#x, want %#x)"
                             % (what, bad.size, bad[0], got[bad[0]], exp[bad[0]]))


def parity_of(k, m, data):
    """oracle.rs16.encode of one segment's k shards."""
    return np.frombuffer(b"".join(rs16.encode(k, m, [d.tobytes() for d in data])), np.uint8).reshape(m, -1)


def _status(call, *args):
    try:
        call(*args)
        return _lib.TE_OK
    except EngineError as e:
        return e.code


def run_encode(k, m, cb, segs=2, expect_status=_lib.TE_OK):
    """te_outer_encode_device of `segs` segments: inputs at stride k * cb + 128, outputs at stride
    m * cb + 192 inside a poisoned, guarded allocation.  Returns the launch stats."""
    torch = _torch()
    rng = np.random.default_rng((k << 20) ^ (m << 8) ^ cb ^ segs)
    seg_in, seg_out = k * cb + 128, m * cb + 192
    host_in = rng.integers(0, 256, segs * seg_in, dtype=np.uint8)
    datas = []
    for g in range(segs):
        d = _shards(rng, k, cb)
        host_in[g * seg_in:g * seg_in + k * cb] = d.reshape(-1)
        datas.append(d)
    d_in = torch.from_numpy(host_in).cuda()
    total = 2 * GUARD + segs * seg_out
    buf = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    exp = np.full(total, POISON, np.uint8)
    r = _status(outer.encode_device, k, m, d_in, cb, segs, seg_in, buf[GUARD:], seg_out)
    torch.cuda.synchronize()
    assert r == expect_status, _lib.strerror(r)
    if expect_status == _lib.TE_OK:
        for g in range(segs):
            at = GUARD + g * seg_out
            exp[at:at + m * cb] = parity_of(k, m, datas[g]).reshape(-1)
    _same(buf.cpu().numpy(), exp, "encode (%d, %d) cb %d" % (k, m, cb))
    assert torch.equal(d_in.cpu(), torch.from_numpy(host_in)), "inputs changed"
    return outer.launch_stats()


class Coded:
    """`segs` segments of OuterCoder(k, n) on the device: every chunk of a segment in one tensor at
    stride cb + 64, parity from the oracle."""

    def __init__(self, k, n, cb, segs, seed=0):
        torch = _torch()
        self.k, self.n, self.m, self.cb, self.segs = k, n, n - k, cb, segs
        rng = np.random.default_rng((k << 20) ^ (n << 8) ^ cb ^ (segs << 12) ^ seed)
        self.stride = cb + 64
        host = rng.integers(0, 256, segs * n * self.stride, dtype=np.uint8)
        self.data = []
        for g in range(segs):
            d = _shards(rng, k, cb)
            self.data.append(d)
            both = np.concatenate([d, parity_of(k, self.m, d)]) if self.m else d
            for i in range(n):
                at = (g * n + i) * self.stride
                host[at:at + cb] = both[i]
        self.host = host
        self.dev = torch.from_numpy(host).cuda()

    def addr(self, g, i):
        return self.dev.data_ptr() + (g * self.n + i) * self.stride

    def chunk(self, g, i):
        at = (g * self.n + i) * self.stride
        return self.host[at:at + self.cb].tobytes()

    def decode(self, keeps, segments=None, oracle=False, expect_status=_lib.TE_OK):
        """te_outer_decode_device (one segment) or _batch of the first `segments` segments, segment g
        from the chunks keeps[g % len(keeps)], into a poisoned, guarded allocation at stride
        k * cb + 192.  Returns the launch stats."""
        torch = _torch()
        k, n, cb = self.k, self.n, self.cb
        segs = self.segs if segments is None else segments
        seg_out = k * cb + 192
        total = 2 * GUARD + segs * seg_out
        buf = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
        exp = np.full(total, POISON, np.uint8)
        chunks = [[self.addr(g, i) if i in keeps[g % len(keeps)] else None for i in range(n)] for g in range(segs)]
        if segs == 1:
            status = _status(outer.decode_device, k, n, chunks[0], cb, buf[GUARD:])
        else:
            status = _status(outer.decode_device_batch, k, n, chunks, cb, buf[GUARD:], seg_out)
        torch.cuda.synchronize()
        assert status == expect_status, _lib.strerror(status)
        if expect_status == _lib.TE_OK:
            for g in range(segs):
                at = GUARD + g * seg_out
                exp[at:at + k * cb] = self.data[g].reshape(-1)
        _same(buf.cpu().numpy(), exp, "decode (%d, %d) cb %d keep %s" % (k, n, cb, keeps))
        assert torch.equal(self.dev.cpu(), torch.from_numpy(self.host)), "inputs changed"
        if oracle:  # the oracle's decoder agrees with the original data
            kp = keeps[0]
            want = rs16.decode(k, self.m, {i: self.chunk(0, i) for i in kp})
            assert b"".join(want) == self.data[0].tobytes()
        return outer.launch_stats()


def survivor_sets(k, n, missing):
    """Two sets of k survivors with `missing` data chunks absent: the first data chunks missing and
    the first parity chunks received; a seeded scatter of both.  All k missing: parity only, twice;
    fewer: data and parity mixed, twice (a parity-only set exists only when all k are missing)."""
    rnd = random.Random(k * 1000 + n * 10 + missing)
    a = list(range(missing, k)) + list(range(k, k + missing))
    b = sorted(rnd.sample(range(k), k - missing)) + sorted(rnd.sample(range(k, n), missing))
    return [a, b]


# ---- encode: rs16_matrix_kernel by strides ----
# (k, m) -> G (4-row groups), KB (input slots), tail entry bytes (0: even G)
MATRIX_ENCODE = [
    (1, 1, 1, 16, 2),
    (16, 2, 1, 16, 4),     # k at the KB = 16 edge
    (17, 3, 1, 32, 8),
    (32, 4, 1, 32, 8),     # k at its cap
    (3, 8, 2, 16, 0),
    (5, 9, 3, 16, 2),
    (9, 18, 5, 16, 4),
    (17, 33, 9, 32, 2),    # OuterCoder(17, 50)
    (16, 32, 8, 16, 0),
    (5, 64, 16, 16, 0),
    (10, 61, 16, 16, 0),   # image 81,920 B = kRs16MatLds exactly; rows 61..63 of the last group are not stored
]


@pytest.mark.parametrize("k,m,g,kb,tail", MATRIX_ENCODE)
def test_encode_matrix(k, m, g, kb, tail):
    for cb in SIZES:
        st = run_encode(k, m, cb)
        tiles = 2 * ((cb // 4 + 511) // 512)
        _expect_stats(st, {"matrix_launches": 1, "matrix_ptr_launches": 0, "matrix_segments": 2, "matrix_g": g,
                           "matrix_kb": kb, "matrix_tail_bytes": tail, "matrix_tailv": 0, "matrix_grid": tiles,
                           "matrix_tiles": tiles, "transform_launches": 0, "low_reg_launches": 0,
                           "decode_launches": 0})


# ---- encode: rs16_encode_low_kernel<C>, reached with no knob ----
LOW_ENCODE = [
    (1, 65, 1),
    (2, 66, 2),
    (3, 67, 4),      # k < C: zero-padded inputs, the k - 1 clamp of the loads
    (8, 65, 8),      # k = C
    (11, 61, 16),    # image 90,112 B, one step over the cap; last chunk of 13 rows
    (32, 40, 32),    # chunks of 32 + 8 rows
    (17, 100, 32),   # chunks of 32, 32, 32, 4 rows
]


@pytest.mark.parametrize("k,m,c", LOW_ENCODE)
def test_encode_low_register(k, m, c):
    for cb in SIZES:
        st = run_encode(k, m, cb)
        _expect_stats(st, {"low_reg_launches": 1, "low_reg_segments": 2, "low_reg_c": c, "matrix_launches": 0,
                           "transform_launches": 0, "decode_launches": 0})


@pytest.mark.parametrize("k,m,c", [(17, 33, 32), (5, 9, 8)])
def test_encode_low_register_by_knob(k, m, c, monkeypatch):
    """TEC_RS16_NO_MATRIX=1 (read on every call: tec_knob does not cache) sends matrix shapes to the
    low-register kernel."""
    monkeypatch.setenv("TEC_DEBUG_KNOBS", "1")
    monkeypatch.setenv("TEC_RS16_NO_MATRIX", "1")
    for cb in SIZES:
        st = run_encode(k, m, cb)
        _expect_stats(st, {"low_reg_launches": 1, "low_reg_segments": 2, "low_reg_c": c, "matrix_launches": 0,
                           "transform_launches": 0})
    monkeypatch.undo()
    _expect_stats(run_encode(k, m, 64), {"low_reg_launches": 0, "matrix_launches": 1})


# ---- encode: rs16_encode_kernel ----
def _pow2(x):
    p = 1
    while p < x:
        p *= 2
    return p


TRANSFORM_ENCODE = [
    (40, 9, 1, 16),     # chunks of 16, 16, 8 originals
    (50, 3, 1, 4),      # 13 folded chunks, the last of 2
    (33, 64, 1, 64),    # one partial chunk
    (64, 64, 1, 64),    # one full chunk
    (32, 32, 1, 32),
    (33, 100, 0, 64),   # low rate with k > 32: recovery chunks of 64 + 36
]


@pytest.mark.parametrize("k,m,high,c", TRANSFORM_ENCODE)
def test_encode_transform(k, m, high, c):
    assert c == (_pow2(m) if high else _pow2(k))
    # rs16.hpp work_len and skew_span: the LDS the launch needs at the block size it reports
    work = 2 * c if high else -(-m // c) * c
    span = -(-(k if high else m) // c) * c + 2 * c + 1
    for cb in SIZES:
        st = run_encode(k, m, cb)
        _expect_stats(st, {"transform_launches": 1, "transform_segments": 2, "transform_high": high,
                           "transform_c": c, "matrix_launches": 0, "low_reg_launches": 0, "decode_launches": 0})
        t = st["transform_threads"]
        assert t in (128, 256, 512, 1024)
        assert st["transform_lds"] == span * 128 + work * t * 2 <= LDS_MAX


def test_encode_refused_past_lds():
    """(33, 600): low rate, 10 recovery chunks of 64 = 640 u16 of work per column, more LDS than a
    128-thread block may have: TE_ERR_UNSUPPORTED, nothing launched, nothing written."""
    _expect_stats(run_encode(33, 100, 64), {"transform_launches": 1})
    st = run_encode(33, 600, 64, expect_status=_lib.TE_ERR_UNSUPPORTED)
    _expect_stats(st, NO_LAUNCH)


def test_encode_matrix_grid_stride():
    """(3, 5) at 2,112 B, 1,100 segments: 2 tiles per segment (the second partial), 2,200 tiles on a
    grid of 2,048 workgroups, so 152 workgroups take a second tile."""
    st = run_encode(3, 5, 2112, segs=1100)
    _expect_stats(st, {"matrix_launches": 1, "matrix_segments": 1100, "matrix_g": 2, "matrix_kb": 16,
                       "matrix_tail_bytes": 0, "matrix_grid": 2048, "matrix_tiles": 2200})
    assert st["matrix_tiles"] > st["matrix_grid"]


# ---- decode: rs16_matrix_kernel by pointer arguments ----
# (k, n, missing data chunks) -> G, KB, tail bytes
MATRIX_DECODE = [
    (17, 50, 17, 5, 32, 2),   # OuterCoder(17, 50), all data lost
    (17, 50, 1, 1, 32, 2),
    (16, 48, 16, 4, 16, 0),
    (16, 48, 10, 3, 16, 4),
    (32, 64, 20, 5, 32, 8),   # image 81,920 B = kRs16MatLds exactly
]


@pytest.mark.parametrize("k,n,missing,g,kb,tail", MATRIX_DECODE)
def test_decode_matrix_pointers(k, n, missing, g, kb, tail):
    sets = survivor_sets(k, n, missing)
    for cb in SIZES:
        c = Coded(k, n, cb, 2)
        for i, keep in enumerate(sets):
            st = c.decode([keep], oracle=(cb == SIZES[0] and i == 0))
            tiles = 2 * ((cb // 4 + 511) // 512)
            _expect_stats(st, {"matrix_launches": 1, "matrix_ptr_launches": 1, "matrix_segments": 2, "matrix_g": g,
                               "matrix_kb": kb, "matrix_tail_bytes": tail, "matrix_tailv": 0, "matrix_grid": tiles,
                               "matrix_tiles": tiles, "decode_launches": 0, "transform_launches": 0,
                               "low_reg_launches": 0})


# ---- decode: rs16_decode_kernel<KB, TLDS> ----
# (k, n, missing, segments) -> KB (0: any k), tables in LDS, launches
TABLE_DECODE = [
    (32, 64, 21, 2, 32, 0, 1),    # one missing chunk past the matrix image's cap
    (29, 58, 29, 2, 32, 0, 1),    # k < KB: the r >= k products read entry 0 of table k - 1
    (26, 52, 25, 2, 28, 0, 1),    # one data chunk received: copied, not restored
    (33, 40, 7, 2, 0, 1, 1),
    (48, 64, 16, 2, 0, 0, 1),
    (64, 128, 64, 3, 0, 0, 2),    # 128 pointers per segment: launches of 2 and 1 segments
]


@pytest.mark.parametrize("k,n,missing,segs,kb,lds,launches", TABLE_DECODE)
def test_decode_table_kernel(k, n, missing, segs, kb, lds, launches):
    sets = survivor_sets(k, n, missing)
    for cb in SIZES:
        c = Coded(k, n, cb, segs)
        for i, keep in enumerate(sets):
            st = c.decode([keep], oracle=(cb == SIZES[0] and i == 0))
            _expect_stats(st, {"decode_launches": launches, "decode_segments": segs, "decode_kb": kb,
                               "decode_lds": lds, "matrix_launches": 0, "transform_launches": 0,
                               "low_reg_launches": 0})


def test_decode_refused_past_max_k():
    """(65, 70) with a data chunk missing: more received shards than a decoding-matrix row holds --
    TE_ERR_UNSUPPORTED from the validation pass, before anything is enqueued: nothing written, not
    even the copies of the received data chunks."""
    c = Coded(65, 70, 64, 1)
    keep = [i for i in range(70) if i != 3][:65]
    c.decode([keep], expect_status=_lib.TE_ERR_UNSUPPORTED)
    c2 = Coded(65, 70, 64, 2)
    c2.decode([keep, list(range(65))], expect_status=_lib.TE_ERR_UNSUPPORTED)


def test_decode_matrix_grid_stride():
    """OuterCoder(1, 2), 130 segments of 32,832-byte chunks from parity alone: 2 pointers per
    segment, so launches of 128 and 2 segments; 17 tiles per segment, so the first launch has 2,176
    tiles on 2,048 workgroups.  The stats carry a call's last launch: the 128-segment launch is
    read from a second call over the first 128 segments."""
    c = Coded(1, 2, 32832, 130)
    st = c.decode([[1]])
    _expect_stats(st, {"matrix_launches": 2, "matrix_ptr_launches": 2, "matrix_segments": 130, "matrix_g": 1,
                       "matrix_kb": 16, "matrix_tail_bytes": 2, "matrix_grid": 34, "matrix_tiles": 34,
                       "decode_launches": 0})
    st = c.decode([[1]], segments=128)
    _expect_stats(st, {"matrix_launches": 1, "matrix_ptr_launches": 1, "matrix_segments": 128, "matrix_grid": 2048,
                       "matrix_tiles": 2176})
    assert st["matrix_tiles"] > st["matrix_grid"]


def test_pointer_array_full():
    """(17, 50) with 15 data chunks missing: 32 pointers per segment, 8 segments fill the 256 pointer
    arguments of one launch exactly; a ninth segment starts a second launch."""
    k, n, missing = 17, 50, 15
    keep = survivor_sets(k, n, missing)[1]
    c = Coded(k, n, 64, 9)
    _expect_stats(c.decode([keep], segments=8), {"matrix_launches": 1, "matrix_ptr_launches": 1, "matrix_segments": 8,
                                                 "matrix_g": 4, "matrix_kb": 32, "matrix_tail_bytes": 0})
    _expect_stats(c.decode([keep]), {"matrix_launches": 2, "matrix_ptr_launches": 2, "matrix_segments": 9})


def test_table_cache_eviction():
    """70 distinct survivor sets of (8, 16) through the 64-entry table cache, then the first again:
    every decode correct, at least one call evicts, and the first set -- the least recently used of
    the 70 -- is rebuilt (a miss) when it returns."""
    k, n = 8, 16
    rnd = random.Random(816)
    pool = [s for s in itertools.combinations(range(n), k) if any(i not in s for i in range(k))]
    sets = [list(s) for s in rnd.sample(pool, 70)]
    c = Coded(k, n, 64, 1)
    evictions = 0
    for i, keep in enumerate(sets):
        st = c.decode([keep])
        _expect_stats(st, {"matrix_launches": 1, "matrix_ptr_launches": 1, "lut_misses": 1})
        assert st["lut_evictions"] <= 1
        evictions += st["lut_evictions"]
    assert evictions >= 6  # 70 new tables into 64 places
    _expect_stats(c.decode([sets[-1]]), {"matrix_launches": 1, "lut_misses": 0, "lut_evictions": 0})
    _expect_stats(c.decode([sets[0]]), {"matrix_launches": 1, "lut_misses": 1, "lut_evictions": 1})
