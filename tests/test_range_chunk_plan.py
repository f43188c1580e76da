"""te_slicer_range_plan_ex against plain Python arithmetic (no GPU): the chunk path's routing rule.

A touched stripe is TE_RANGE_CHUNK when exactly one of the data chunks its window intersects is an
absent slice's (te_shard_to_slice under the call's rotation) and the object is one whose node
recover runs a class kernel: Clay(20,7,16), sub-chunks of at least 8 bytes, 31-bit offsets.  The
planner then names the data shard that is rebuilt.  Two or more absent chunks stay
TE_RANGE_DECODE, none is TE_RANGE_COPY, and with chunk_path = 0 the plan is te_slicer_range_plan's.

Windows and blob lengths are those of tests/test_range_plan.py."""
import ctypes as C
import random

import pytest

import tape_amd as T
from tape_amd import _lib
from tape_amd._lib import lib
from tape_amd.slicer import ClayParams, EncodingProfile

import test_range_plan as RP

N, K = RP.N, RP.K


def chunk_masks(rotated):
    """Parity only (two layouts), each data slice erased alone, and random 7-of-20 sets."""
    rng = random.Random(0xC4A2 + rotated)
    m = [sum(1 << i for i in range(13, 20)), sum(1 << i for i in range(K, 2 * K))]
    m += [((1 << N) - 1) & ~(1 << x) for x in range(K)]
    m += [sum(1 << i for i in rng.sample(range(N), K)) for _ in range(10)]
    return m


def eligible(g):
    """The object's node recover runs a class kernel (profile checked by the caller)."""
    return (int(g.sub_chunk_size) >= 8 and N * int(g.slice_len) < 0x7FFFFFFF and K * int(g.chunk_size) < 0x7FFFFFFF)


def py_plan_ex(rotated, g, blob_len, avail, start, length, chunk_path):
    S, cs = int(g.stripe_size), int(g.chunk_size)
    if length == 0:
        return 0, []
    s0, s1 = start // S, (start + length - 1) // S
    out = []
    for st in range(s0, s1 + 1):
        lo = start - st * S if st == s0 else 0
        hi = min(start + length, (st + 1) * S, blob_len) - st * S
        miss = [x for x in range(lo // cs, (hi - 1) // cs + 1) if not avail >> RP.shard_to_slice(rotated, st, x) & 1]
        if not miss:
            out.append((_lib.RANGE_COPY, lo, hi, None))
        elif len(miss) == 1 and chunk_path and eligible(g):
            out.append((_lib.RANGE_CHUNK, lo, hi, miss[0]))
        else:
            out.append((_lib.RANGE_DECODE, lo, hi, None))
    return s0, out


@pytest.mark.parametrize("rotated", [0, 1])
@pytest.mark.parametrize("blob_len", RP.OBJECTS)
def test_plan_ex_matches_python(blob_len, rotated):
    s = RP._slicer(rotated)
    g = s.geometry(blob_len)
    S, cs, sc = int(g.stripe_size), int(g.chunk_size), int(g.sub_chunk_size)
    assert eligible(g) == (blob_len != 1)  # the 1 B object's sub-chunk is below the class kernels' 8 bytes
    seen = set()
    for mi, avail in enumerate(chunk_masks(rotated)):
        rows = range(100) if mi == 0 else (0, 1, 2, 99)
        for start in RP.positions(blob_len, S, cs, sc, rows):
            lens = {0, 1, 2, 3, 4, 5, cs, cs + 1, 2 * cs + 1, blob_len - start}
            if start == 0:
                lens.add(blob_len)
            for ln in sorted(l for l in lens if start + l <= blob_len):
                want = py_plan_ex(rotated, g, blob_len, avail, start, ln, True)
                assert s.range_plan_ex(blob_len, avail, start, ln) == want, (hex(avail), start, ln)
                seen.update(c for c, _, _, _ in want[1])
                if mi < 9 or ln < 3:
                    # chunk_path = 0: te_slicer_range_plan's classes, lo and hi, no shard
                    first, plan = s.range_plan(blob_len, avail, start, ln)
                    assert s.range_plan_ex(blob_len, avail, start, ln, False) == \
                        (first, [(c, lo, hi, None) for c, lo, hi in plan]), (hex(avail), start, ln)
                    assert [(lo, hi) for _, lo, hi in plan] == [(lo, hi) for _, lo, hi, _ in want[1]]
    if blob_len != 1:
        assert seen == {_lib.RANGE_COPY, _lib.RANGE_DECODE, _lib.RANGE_CHUNK}, seen
    else:
        assert _lib.RANGE_CHUNK not in seen


def test_one_data_slice_erased():
    """Identity mapping, slice 3 absent: a window inside chunk 3 rebuilds shard 3, a window that
    also touches chunks 2 and 4 still rebuilds only shard 3, a window clear of chunk 3 copies.
    Parity only: every window of two or more chunks has two erased and decodes."""
    blob = 250_000
    s = RP._slicer(0)
    g = s.geometry(blob)
    cs = int(g.chunk_size)
    avail = ((1 << N) - 1) & ~(1 << 3)
    assert s.range_plan_ex(blob, avail, 3 * cs + 10, 100) == (0, [(_lib.RANGE_CHUNK, 3 * cs + 10, 3 * cs + 110, 3)])
    assert s.range_plan_ex(blob, avail, 2 * cs + 10, 2 * cs) == (0, [(_lib.RANGE_CHUNK, 2 * cs + 10, 4 * cs + 10, 3)])
    assert s.range_plan_ex(blob, avail, 4 * cs, cs) == (0, [(_lib.RANGE_COPY, 4 * cs, 5 * cs, None)])
    par = sum(1 << i for i in range(13, 20))
    assert s.range_plan_ex(blob, par, 3 * cs + 10, 100) == (0, [(_lib.RANGE_CHUNK, 3 * cs + 10, 3 * cs + 110, 3)])
    assert s.range_plan_ex(blob, par, 2 * cs + 10, 2 * cs) == (0, [(_lib.RANGE_DECODE, 2 * cs + 10, 4 * cs + 10, None)])
    # rotated: stripe 1's shard x is slice x + 7, so slice 10 absent erases shard 3 of stripe 1 only
    r = RP._slicer(1)
    S = int(g.stripe_size)
    avail = ((1 << N) - 1) & ~(1 << 10)
    assert r.range_plan_ex(blob, avail, 0, blob)[1][1] == (_lib.RANGE_CHUNK, 0, S, 3)
    assert [c for c, _, _, _ in r.range_plan_ex(blob, avail, 0, blob)[1]] == \
        [_lib.RANGE_COPY, _lib.RANGE_CHUNK, _lib.RANGE_COPY]


@pytest.mark.parametrize("params", [(20, 10, 19), (12, 8, 11)])
def test_other_profiles_never_report_chunk(params):
    n, k, d = params
    s = T.Slicer.with_rotation(T.ClayCoder(n, k, d))
    s.profile = EncodingProfile.clay(ClayParams(n | k << 8 | d << 16))
    blob = 250_000
    cs = int(s.geometry(blob).chunk_size)
    for x in range(k):
        avail = ((1 << n) - 1) & ~(1 << x)
        for start, ln in ((x * cs + 5, 10), (0, blob), (cs - 1, 2)):
            first, plan = s.range_plan(blob, avail, start, ln)
            assert s.range_plan_ex(blob, avail, start, ln) == (first, [(c, lo, hi, None) for c, lo, hi in plan])
    assert any(c == _lib.RANGE_DECODE for c, _, _ in s.range_plan(blob, ((1 << n) - 1) & ~1, 0, blob)[1])


def test_argument_rules_and_knob():
    s = RP._slicer(1)
    full = (1 << N) - 1
    cfg = s._cfg()
    first, cnt = C.c_uint64(), C.c_uint64()

    def raw(blob_len, avail, start, ln, chunk_path=1):
        return lib.te_slicer_range_plan_ex(s.coder.handle, C.byref(cfg), blob_len, avail, start, ln, chunk_path,
                                           C.byref(first), C.byref(cnt), None, None, None, None)

    assert raw(1000, full, 0, 1000) == 0 and (first.value, cnt.value) == (0, 1)  # every array may be NULL
    assert raw(1000, full, 999, 2) == _lib.TE_ERR_INVALID_ARG
    assert raw(1000, full, 500, 0) == 0 and cnt.value == 0
    assert raw(1000, 0x3F, 0, 10) == _lib.TE_ERR_NOT_ENOUGH_SLICES  # fewer than k: as te_slicer_range_plan
    assert lib.te_slicer_range_plan_ex(None, C.byref(cfg), 10, full, 0, 1, 1, None, None, None, None, None, None) == \
        _lib.TE_ERR_INVALID_ARG
    # the knob: off by default, 0 / 1 only, per handle; the planner does not read it
    assert s.range_chunk_path() is False
    assert lib.te_clay_set_range_chunk_path(s.coder.handle, 2) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_clay_set_range_chunk_path(None, 1) == _lib.TE_ERR_INVALID_ARG
    one = full & ~1
    before = s.range_plan_ex(250_000, one, 5, 10)
    s.set_range_chunk_path(True)
    assert s.range_chunk_path() is True and RP._slicer(1).range_chunk_path() is False
    assert s.range_plan_ex(250_000, one, 5, 10) == before == (0, [(_lib.RANGE_CHUNK, 5, 15, 0)])
    assert s.range_plan(250_000, one, 5, 10) == (0, [(_lib.RANGE_DECODE, 5, 15)])
    s.set_range_chunk_path(False)
    assert s.range_chunk_path() is False
    assert lib.te_clay_range_chunk_launch_stats(None, None) == _lib.TE_ERR_INVALID_ARG


def test_ctypes_mirror_matches_the_header():
    fields = RP._header_struct("te_range_chunk_stats")
    assert [f for f, _ in fields] == [f for f, _ in _lib.te_range_chunk_stats._fields_]
    assert all(t == "uint64_t" for _, t in fields) and C.sizeof(_lib.te_range_chunk_stats) == 24
    assert C.sizeof(_lib.te_range_launch_stats) == 40  # its layout is unchanged
    txt = open(_lib.HEADER_PATH).read()
    assert "#define TE_RANGE_CHUNK 2" in txt and _lib.RANGE_CHUNK == 2
