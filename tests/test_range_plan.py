"""te_slicer_range_plan against plain Python arithmetic, the argument rules of the ranged read entry
points, and their ctypes mirrors (no GPU).

A window [start, start + len) of an object touches stripes start // S .. (start + len - 1) // S; in
stripe s it is [lo, hi) in stripe bytes; data chunk x holds stripe bytes [x cs, (x + 1) cs); the
stripe is a copy stripe when every chunk the window intersects is a present slice's
(te_shard_to_slice under the call's rotation), else a decode stripe."""
import ctypes as C
import random
import re

import pytest

import tape_amd as T
from tape_amd import _lib
from tape_amd._lib import lib

N, K = 20, 7
OBJECTS = [250_000, 2_300_000, 70_001, 1]
U64 = (1 << 64) - 1


def _slicer(rotated):
    s = T.Slicer.clay_default()
    s.strategy = T.MappingStrategy.Rotated if rotated else T.MappingStrategy.Identity
    return s


def shard_to_slice(rotated, st, x):
    return (x + (st * 7) % N) % N if rotated else x


def py_plan(rotated, S, cs, blob_len, avail, start, length):
    if length == 0:
        return 0, []
    s0, s1 = start // S, (start + length - 1) // S
    out = []
    for st in range(s0, s1 + 1):
        lo = start - st * S if st == s0 else 0
        hi = min(start + length, (st + 1) * S, blob_len) - st * S
        chunks = range(lo // cs, (hi - 1) // cs + 1)
        copy = all(avail >> shard_to_slice(rotated, st, x) & 1 for x in chunks)
        out.append((_lib.RANGE_COPY if copy else _lib.RANGE_DECODE, lo, hi))
    return s0, out


def masks(rotated):
    rng = random.Random(0xC1A7 + rotated)
    # all present, the data slices only, parity slices only
    m = [(1 << N) - 1, (1 << K) - 1, sum(1 << i for i in range(K, 2 * K))]
    for _ in range(12):
        m.append(sum(1 << i for i in rng.sample(range(N), K)))
    return m


def positions(blob_len, S, cs, sc, rows):
    """Window starts: stripe boundaries, chunk boundaries, sub-chunk row boundaries (each +- 1),
    the first and the last byte."""
    p = {0, blob_len - 1}
    ns = (blob_len + S - 1) // S
    for st in range(ns):
        for x in range(K + 1):
            for z in rows:
                b = st * S + x * cs + z * sc
                p.update((b - 1, b, b + 1))
    return sorted(q for q in p if 0 <= q < blob_len)


@pytest.mark.parametrize("rotated", [0, 1])
@pytest.mark.parametrize("blob_len", OBJECTS)
def test_plan_matches_python(blob_len, rotated):
    s = _slicer(rotated)
    g = s.geometry(blob_len)
    S, cs, sc = int(g.stripe_size), int(g.chunk_size), int(g.sub_chunk_size)
    assert int(g.num_stripes) == {250_000: 3, 2_300_000: 3, 70_001: 1, 1: 1}[blob_len]
    for mi, avail in enumerate(masks(rotated)):
        # every sub-chunk row boundary under the first mask, a few rows under the others
        rows = range(100) if mi == 0 else (0, 1, 2, 99)
        for start in positions(blob_len, S, cs, sc, rows):
            lens = {0, 1, 2, 3, 4, 5, blob_len - start}
            if start == 0:
                lens.add(blob_len)
            for ln in sorted(l for l in lens if start + l <= blob_len):
                assert s.range_plan(blob_len, avail, start, ln) == py_plan(rotated, S, cs, blob_len, avail, start, ln), \
                    (hex(avail), start, ln)


def test_plan_classes_follow_the_mask_not_the_padded_set():
    """All 20 present: every window is copy-only although the decode would pad 13 erasures.  Only
    parity present: every window decodes.  Data slices only, identity: copy; rotated: stripe 1's
    chunks sit in slices 7..13, so it decodes."""
    blob = 250_000
    for rotated in (0, 1):
        s = _slicer(rotated)
        assert all(c == _lib.RANGE_COPY for c, _, _ in s.range_plan(blob, (1 << N) - 1, 0, blob)[1])
        par = sum(1 << i for i in range(13, 20))
        assert [c for c, _, _ in s.range_plan(blob, par, 0, 100_000)[1]] == [_lib.RANGE_DECODE]
    data_only = (1 << K) - 1
    assert [c for c, _, _ in _slicer(0).range_plan(blob, data_only, 0, blob)[1]] == [_lib.RANGE_COPY] * 3
    assert [c for c, _, _ in _slicer(1).range_plan(blob, data_only, 0, blob)[1]] == \
        [_lib.RANGE_COPY, _lib.RANGE_DECODE, _lib.RANGE_DECODE]


def _raw_plan(s, blob_len, avail, start, ln):
    first, cnt = C.c_uint64(), C.c_uint64()
    cfg = s._cfg()
    return lib.te_slicer_range_plan(s.coder.handle, C.byref(cfg), blob_len, avail, start, ln, C.byref(first),
                                    C.byref(cnt), None, None, None), first.value, cnt.value


def test_plan_argument_rules():
    s = _slicer(1)
    full = (1 << N) - 1
    assert _raw_plan(s, 1000, full, 0, 1000) == (0, 0, 1)
    assert _raw_plan(s, 1000, full, 999, 2)[0] == _lib.TE_ERR_INVALID_ARG      # past the end
    assert _raw_plan(s, 1000, full, 1001, 0)[0] == _lib.TE_ERR_INVALID_ARG
    assert _raw_plan(s, 1000, full, U64, 2)[0] == _lib.TE_ERR_INVALID_ARG      # start + len overflows
    assert _raw_plan(s, 1000, full, 2, U64)[0] == _lib.TE_ERR_INVALID_ARG
    assert _raw_plan(s, 1000, full, 1000, 0) == (0, 0, 0)                      # len 0: touches nothing
    assert _raw_plan(s, 1000, full, 500, 0) == (0, 0, 0)
    assert _raw_plan(s, 0, full, 0, 0) == (0, 0, 0)                            # the empty blob
    assert _raw_plan(s, 0, full, 0, 1)[0] == _lib.TE_ERR_INVALID_ARG
    assert _raw_plan(s, 0, full, 1, 0)[0] == _lib.TE_ERR_INVALID_ARG
    six = (1 << 6) - 1
    assert _raw_plan(s, 1000, six, 0, 10)[0] == _lib.TE_ERR_NOT_ENOUGH_SLICES  # even for a copy-only window
    assert _raw_plan(s, 1000, six | 1 << 25, 0, 10)[0] == _lib.TE_ERR_NOT_ENOUGH_SLICES  # bits past n do not count
    cfg = s._cfg()
    assert lib.te_slicer_range_plan(None, C.byref(cfg), 10, full, 0, 1, None, None, None, None, None) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_clay_range_launch_stats(None, None) == _lib.TE_ERR_INVALID_ARG


def _meta(s, blob_len):
    g = s.geometry(blob_len)
    m = _lib.te_slice_metadata(1, blob_len, int(g.stripe_size), s.profile.encoding, s.profile.params, 0)
    out = (C.c_uint8 * 48)()
    lib.te_slice_metadata_to_bytes(C.byref(m), out)
    return bytes(out), int(g.slice_len)


def test_compute_entry_points_validate_then_need_a_device():
    """Both compute entry points check their arguments (the window included) before they look for
    a device, and without one return TE_ERR_NO_DEVICE: there is no CPU fallback."""
    s = _slicer(1)
    blob = 250_000
    meta, sl = _meta(s, blob)
    cfg = s._cfg()
    mb = (C.c_uint8 * 48).from_buffer_copy(meta)
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below returns before device work

    def batch_call(avail, start, ln):
        obj = _lib.te_decode_range_object(0, sl, avail, 0, 0, start, ln)
        return lib.te_decode_range_batch_device(s.coder.handle, C.byref(cfg), fake, C.byref(obj), mb, 1, fake, None)

    full = (1 << N) - 1
    assert batch_call(full, blob - 1, 2) == _lib.TE_ERR_INVALID_ARG
    assert batch_call(full, U64, 2) == _lib.TE_ERR_INVALID_ARG
    assert batch_call(0x3F, 0, 1) == _lib.TE_ERR_NOT_ENOUGH_SLICES
    assert lib.te_decode_range_batch_device(s.coder.handle, C.byref(cfg), fake, None, mb, 1, fake, None) == _lib.TE_ERR_INVALID_ARG

    slice_ = bytes(sl - 48) + meta
    bufs = [(C.c_uint8 * sl).from_buffer_copy(slice_) for _ in range(K)]

    def call(nslices, start, ln, cap=None):
        ptrs = (C.c_void_p * N)()
        for i in range(nslices):
            ptrs[i] = C.cast(bufs[i], C.c_void_p)
        out = (C.c_uint8 * max(1, ln if ln < 1 << 20 else 1))()
        got = C.c_size_t(77)
        r = lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, sl, start, ln, out,
                                       len(out) if cap is None else cap, C.byref(got))
        return r, got.value

    assert call(K, blob, 1)[0] == _lib.TE_ERR_INVALID_ARG
    assert call(K, 5, U64)[0] == _lib.TE_ERR_INVALID_ARG
    assert call(K - 1, 0, 1)[0] == _lib.TE_ERR_NOT_ENOUGH_SLICES
    assert call(0, 0, 1)[0] == _lib.TE_ERR_NOT_ENOUGH_SLICES
    assert call(K, 0, 100, cap=99)[0] == _lib.TE_ERR_BUFFER_TOO_SMALL
    if _lib.device_count() == 0:
        assert batch_call(full, 0, blob) == _lib.TE_ERR_NO_DEVICE
        assert batch_call(full, 10, 0) == _lib.TE_ERR_NO_DEVICE
        assert call(K, 0, 100) == (_lib.TE_ERR_NO_DEVICE, 100)
        assert call(K, 100, 0) == (_lib.TE_ERR_NO_DEVICE, 0)
        with pytest.raises(T.NoDeviceError):
            s.decode_range([(i, slice_) for i in range(K)], 3, 5)


def _header_struct(name):
    txt = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        toks = decl.replace(",", " , ").split()
        if not toks:
            continue
        ctype = toks[0]
        fields += [(t, ctype) for t in toks[1:] if t != ","]
    return fields


def test_ctypes_mirrors_match_the_header():
    size = {"uint64_t": 8, "uint32_t": 4}
    for name, total in (("te_decode_range_object", 48), ("te_range_launch_stats", 40)):
        mirror = getattr(_lib, name)
        fields = _header_struct(name)
        assert [f for f, _ in fields] == [f for f, _ in mirror._fields_], name
        off = 0
        for f, ctype in fields:
            assert getattr(mirror, f).offset == off and getattr(mirror, f).size == size[ctype], (name, f)
            off += size[ctype]
        assert C.sizeof(mirror) == off == total, name
    # the window extends te_decode_object: same leading fields at the same offsets
    for f, _ in _lib.te_decode_object._fields_:
        assert getattr(_lib.te_decode_range_object, f).offset == getattr(_lib.te_decode_object, f).offset
    txt = open(_lib.HEADER_PATH).read()
    assert "#define TE_RANGE_COPY 0" in txt and "#define TE_RANGE_DECODE 1" in txt
    assert (_lib.RANGE_COPY, _lib.RANGE_DECODE) == (0, 1)
