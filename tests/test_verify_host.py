"""Host side of the verified reads (no GPU compute here): te_verify_slice against hashlib, the
argument checks of the device entry points (made before any device use), their NO_DEVICE answer on
a host without one, and the order in which the leaf-verify kernel walks a ragged item list."""
import ctypes as C
import hashlib
import random

import pytest

import tape_amd as T
from tape_amd import _lib, merkle

N = 20
lib = _lib.lib


def leaf(data: bytes) -> bytes:
    return hashlib.sha256(b"LEAF" + data).digest()


def blocks(ln: int) -> int:
    """SHA-256 blocks of "LEAF" || ln bytes || 0x80 || zeros || 8-byte length."""
    return (ln + 4 + 1 + 8 + 63) // 64


@pytest.mark.parametrize("ln", [0, 1, 3, 55, 56, 64, 100_001])
def test_verify_slice_matches_hashlib(ln):
    rng = random.Random(ln)
    data = rng.randbytes(ln)
    leaves = [leaf(rng.randbytes(9)) for _ in range(N)]
    pos = ln % N
    leaves[pos] = leaf(data)
    assert merkle.verify_slice(leaves, pos, data)
    assert not merkle.verify_slice(leaves, (pos + 1) % N, data)  # another slice's leaf
    assert not merkle.verify_slice(leaves, N, data)             # position >= n
    assert not merkle.verify_slice(leaves, N + 7, data)
    assert not merkle.verify_slice(leaves[:pos], pos, data)     # position >= a shorter n
    if ln:
        bad = bytearray(data)
        bad[rng.randrange(ln)] ^= 0x40
        assert not merkle.verify_slice(leaves, pos, bytes(bad))
    assert not merkle.verify_slice(leaves, pos, data + b"\0")


def _item(off, ln, e=0, ob=0, bit=1):
    return _lib.te_verify_item(off, ln, e, ob, bit, 0)


def _no_device(r):
    """A valid call's answer: NO_DEVICE on a host without one (there is no CPU fallback)."""
    if T.device_count() == 0:
        assert r == _lib.TE_ERR_NO_DEVICE


def test_verify_leaves_device_argument_checks():
    c = T.ClayCoder(20, 7, 16)
    p = C.c_void_p(4096)

    def call(items, digests=p):
        arr = (_lib.te_verify_item * len(items))(*items)
        return lib.te_verify_leaves_device(c.handle, p, arr, len(items), p, digests, None, None, None)

    assert call([_item(0, 64), _item(64, 6)]) == _lib.TE_ERR_INVALID_ARG   # len % 4
    assert call([_item(0, 64), _item(66, 8)]) == _lib.TE_ERR_INVALID_ARG   # offset % 4
    assert call([_item(0, 64)], digests=None) == _lib.TE_ERR_INVALID_ARG   # digests are required
    if T.device_count() == 0:
        assert call([_item(0, 64), _item(64, 0)]) == _lib.TE_ERR_NO_DEVICE


def _meta(blob_len, stripe):
    return T.SliceMetadata.new(blob_len, stripe).to_bytes()


def test_verified_batch_argument_checks():
    s = T.Slicer.clay_default()
    c = s.coder.handle
    cfg = s._cfg()
    g = s.geometry(20_000)
    p = C.c_void_p(4096)
    leaves = (C.c_uint8 * (N * 32))()
    meta = (C.c_uint8 * 48).from_buffer_copy(_meta(20_000, g.stripe_size))
    rej, ok, st = (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), (C.c_int * 1)()
    mask = (1 << 9) - 1

    def dec(off, slen):
        o = _lib.te_decode_object(off, slen, mask, 0, 0)
        return lib.te_decode_verified_batch_device(c, C.byref(cfg), p, C.byref(o), meta, leaves, 1, p, rej, st, None)

    def rec(off, slen, out_off=0):
        o = _lib.te_recover_object(off, slen, mask, 12, out_off)
        return lib.te_recover_verified_batch_device(c, C.byref(cfg), p, C.byref(o), meta, leaves, 1, p, rej, ok, st,
                                                    None)

    assert g.slice_len % 4 == 0
    for f in (dec, rec):
        assert f(0, g.slice_len + 2) == _lib.TE_ERR_INVALID_ARG
        assert f(6, g.slice_len) == _lib.TE_ERR_INVALID_ARG
        _no_device(f(8, g.slice_len))
    assert rec(0, g.slice_len, out_off=2) == _lib.TE_ERR_INVALID_ARG

    plan = s.repair_plan_from_params(3, [i for i in range(N) if i != 3], 20_000, g.stripe_size)
    from tape_amd import batch

    def rep(out_off):
        arr = batch.repair_descs([(plan, {i: 0 for i in range(N) if i != 3}, out_off, bytes(meta))])
        return lib.te_repair_verified_batch_device(c, p, arr, leaves, 1, p, ok, None)

    assert rep(2) == _lib.TE_ERR_INVALID_ARG
    _no_device(rep(0))


def test_slicer_decode_verified_rejects_on_the_host():
    """The per-call form hashes on the host by default: with too few slices that verify it answers
    NotEnoughSlices and names the rejected ones, device or not."""
    s = T.Slicer.clay_default()
    g = s.geometry(1000)
    rng = random.Random(5)
    sl = {i: rng.randbytes(g.slice_len) for i in range(8)}
    leaves = [leaf(sl[i]) if i in sl else bytes(32) for i in range(N)]
    leaves[2] = leaf(b"other")
    leaves[5] = leaf(b"other")
    ptrs = (C.c_void_p * N)()
    keep = {i: (C.c_uint8 * len(b)).from_buffer_copy(b) for i, b in sl.items()}
    for i, b in keep.items():
        ptrs[i] = C.cast(b, C.c_void_p)
    lb = (C.c_uint8 * (N * 32)).from_buffer_copy(b"".join(leaves))
    out = (C.c_uint8 * 4096)()
    got, rej = C.c_size_t(), C.c_uint32()
    cfg = s._cfg()
    r = lib.te_slicer_decode_verified(s.coder.handle, C.byref(cfg), ptrs, g.slice_len, lb, out, len(out), C.byref(got),
                                      C.byref(rej))
    assert r == _lib.TE_ERR_NOT_ENOUGH_SLICES
    assert rej.value == (1 << 2) | (1 << 5)
    with pytest.raises(T.DecodeError) as e:
        s.decode_verified(list(sl.items()), leaves)
    assert e.value.variant == "NotEnoughSlices"


def test_item_order_is_a_sorted_bijection():
    rng = random.Random(11)
    lens = [0, 4, 48, 52, 56, 60, 64, 116, 120, 124, 128, 6140, 98_296, 98_300, 98_304, 196_612]
    lens += [4 * rng.randrange(0, 60_000) for _ in range(200)] + [715_048] * 7 + [48] * 9
    rng.shuffle(lens)
    items = [(4 * i, ln, i, i // 20, 1 << (i % 20)) for i, ln in enumerate(lens)]
    order = merkle.verify_order(items)
    assert sorted(order) == list(range(len(items)))               # a bijection
    walked = [blocks(lens[i]) for i in order]
    assert walked == sorted(walked, reverse=True)                 # by block count, descending
    for a, b in zip(order, order[1:]):                            # equal counts keep the caller's order
        if blocks(lens[a]) == blocks(lens[b]):
            assert a < b
    assert merkle.verify_order([]) == []


def test_block_count_examples():
    """The padding cases the GPU test walks: the block count steps where "LEAF" + data + 0x80 + the
    8-byte length no longer fit."""
    assert [blocks(x) for x in (0, 48, 52, 56, 112, 116, 120)] == [1, 1, 2, 2, 2, 3, 3]
    order = merkle.verify_order([(0, 48, 0, 0, 1), (0, 52, 0, 0, 1), (0, 116, 0, 0, 1), (0, 112, 0, 0, 1)])
    assert order == [2, 1, 3, 0]
