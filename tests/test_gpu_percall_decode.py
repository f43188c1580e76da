"""Per-call decode (te_slicer_decode / te_clay_decode) through each host-buffer path of
upload_slices (engine.cpp): pageable slices gathered into pinned staging (slices <= 2 MiB),
page-locked slices copied directly (te_host_alloc), a mix of the two (gathered), and long
pageable slices handed to the driver.  Every decoded blob must equal the original bytes
(Slicer::decode's contract, slicer.rs:298-364); the survivor sets include the worst case (13..19)
and random ones.  The encode under them is checked against the oracle in test_gpu_parity.py."""
import ctypes as C
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import batch
from tape_amd._lib import lib

pytestmark = pytest.mark.gpu
N = 20
MiB = 1024 * 1024


def _encode(s, data):
    cfg, hdl = s._cfg(), s.coder.handle
    g = s.geometry(len(data))
    out = np.empty(N * g.slice_len, np.uint8)
    src = np.frombuffer(data, np.uint8)
    assert lib.te_slicer_encode(hdl, C.byref(cfg), C.c_void_p(src.ctypes.data), len(data),
                                C.c_void_p(out.ctypes.data), out.size) == 0
    return out, g.slice_len


def _decode(s, slices, sl, n):
    cfg, hdl = s._cfg(), s.coder.handle
    ptrs = (C.c_void_p * N)()
    for i, a in slices.items():
        ptrs[i] = a.ctypes.data
    dec = np.empty(max(1, n), np.uint8)
    got = C.c_size_t()
    assert lib.te_slicer_decode(hdl, C.byref(cfg), ptrs, sl, C.c_void_p(dec.ctypes.data), dec.size, C.byref(got)) == 0
    assert got.value == n
    return dec[:n].tobytes()


@pytest.mark.parametrize("ln", [1, 4096, 1_000_000, 4 * MiB, 16 * MiB + 77])
@pytest.mark.parametrize("kind", ["pageable", "pinned", "mixed"])
def test_slicer_decode_host_paths(ln, kind):
    rng = random.Random(ln * 7 + len(kind))
    data = bytes(rng.getrandbits(8) for _ in range(min(ln, 4096))) * (ln // 4096 + 1)
    data = data[:ln]
    s = T.Slicer.clay_default()
    out, sl = _encode(s, data)
    for survivors in (list(range(13, 20)), sorted(rng.sample(range(N), 7)), sorted(rng.sample(range(N), 11))):
        slices = {}
        for j, i in enumerate(survivors):
            pin = kind == "pinned" or (kind == "mixed" and j % 2 == 0)
            a = batch.host_empty(sl) if pin else np.empty(sl, np.uint8)
            a[:] = out[i * sl:(i + 1) * sl]
            slices[i] = a
        assert _decode(s, slices, sl, ln) == data, (kind, survivors)


class _PageLocked:
    """A page-locked host block: from te_host_alloc, or a numpy array pinned in place with
    te_host_register (unregistered on exit)."""

    def __init__(self, kind, nbytes):
        self.kind = kind
        self.a = batch.host_empty(nbytes) if kind == "alloc" else np.empty(nbytes, np.uint8)

    def __enter__(self):
        if self.kind == "registered":
            batch.host_register(self.a)
        return self.a

    def __exit__(self, *exc):
        if self.kind == "registered":
            batch.host_unregister(self.a)


GUARD = 16


def _into_block(block, off, n, call):
    """Run call(dst) with dst the n bytes at GUARD + off of the 0xA5-filled block: the bytes before
    and after dst must come back untouched."""
    block[:] = 0xA5
    dst = block[GUARD + off:GUARD + off + n]
    call(dst)
    assert (block[:GUARD + off] == 0xA5).all(), "bytes before the output were written"
    assert (block[GUARD + off + n:] == 0xA5).all(), "bytes after the output were written"
    return dst


@pytest.mark.parametrize("ln", [1, 4096, 1_000_001, 4 * MiB])
@pytest.mark.parametrize("kind", ["alloc", "registered"])
def test_slicer_decode_page_locked_output(ln, kind):
    """te_slicer_decode into a page-locked `out`: the kernels store straight into it (the zero-copy
    branch, at the buffer's device address), at every byte alignment of `out`.  The class kernels'
    and the table kernel's stores are buffer stores of 1, 2, 4 or 16 bytes at `out` + offset with
    the range check on the blob length -- they already run at 2-aligned addresses (sub-chunks of
    2 mod 4 bytes) and rely on gfx9's unaligned buffer access, which holds for odd addresses alike;
    the generic kernel picks dword, half-word or byte stores from the address (dev_io.hpp)."""
    rng = random.Random(ln * 11 + len(kind))
    data = (bytes(rng.getrandbits(8) for _ in range(min(ln, 4099))) * (ln // 4099 + 1))[:ln]
    s = T.Slicer.clay_default()
    out, sl = _encode(s, data)
    cfg, hdl = s._cfg(), s.coder.handle
    with _PageLocked(kind, ln + 2 * GUARD + 3) as block:
        for survivors in (list(range(13, 20)), sorted(rng.sample(range(N), 7))):
            ptrs = (C.c_void_p * N)()
            keep = {i: out[i * sl:(i + 1) * sl].copy() for i in survivors}
            for i, a in keep.items():
                ptrs[i] = a.ctypes.data
            for off in (0, 1, 2, 3):
                def call(dst):
                    got = C.c_size_t()
                    assert lib.te_slicer_decode(hdl, C.byref(cfg), ptrs, sl, C.c_void_p(dst.ctypes.data), dst.size,
                                                C.byref(got)) == 0
                    assert got.value == ln
                dst = _into_block(block, off, ln, call)
                assert dst.tobytes() == data, (kind, survivors, off)
                st = s.coder.decode_launch_stats()
                # stored in place, no staging copy: also for memory the caller registered, whose
                # device address the engine asks HIP for
                assert st["direct_out"] == 1, st
                assert st["class_stripes"] + st["table_stripes"] + st["generic_stripes"] == int(s.geometry(ln).num_stripes)
                assert st["class_g"] in (0, 1), st  # a per-call decode: the one-wave class kernels


@pytest.mark.parametrize("ln", [1, 4096, 300_001, 1_000_001, 4 * MiB])
@pytest.mark.parametrize("kind", ["alloc", "registered"])
def test_clay_decode_page_locked_output(ln, kind):
    """te_clay_decode (always one stripe of k * chunk bytes: the chunk follows the length) into a
    page-locked `out` at every alignment.  Sub-chunk sizes 2 and 6 (the generic kernel), 430
    (2 mod 4), 1430, and 5992 for 4 MiB in one stripe: 1,498 words, 24 column groups, the widest
    per-call geometry."""
    c = T.ClayCoder(20, 7, 16)
    rng = random.Random(ln * 13 + len(kind))
    data = (bytes(rng.getrandbits(8) for _ in range(min(ln, 4099))) * (ln // 4099 + 1))[:ln]
    chunks = c.encode(data)
    cs = len(chunks[0])
    assert cs // 100 == {1: 2, 4096: 6, 300_001: 430, 1_000_001: 1430, 4 * MiB: 5992}[ln]
    with _PageLocked(kind, 7 * cs + 2 * GUARD + 3) as block:
        for survivors in (list(range(13, 20)), sorted(rng.sample(range(N), 7))):
            ptrs = (C.c_void_p * N)()
            keep = {i: np.frombuffer(chunks[i], np.uint8).copy() for i in survivors}
            for i, a in keep.items():
                ptrs[i] = a.ctypes.data
            for off in (0, 1, 2, 3):
                def call(dst):
                    assert lib.te_clay_decode(c.handle, ptrs, cs, C.c_void_p(dst.ctypes.data), dst.size) == 0
                dst = _into_block(block, off, 7 * cs, call)
                assert dst[:ln].tobytes() == data, (kind, ln, survivors, off)
                assert not dst[ln:].any()  # the padding decodes to zeros
                st = c.decode_launch_stats()
                assert st["direct_out"] == 1, st  # stored in place, no staging copy
                assert st["class_stripes"] + st["table_stripes"] + st["generic_stripes"] == 1, st
                assert st["generic_stripes"] == (1 if cs // 100 < 8 else 0), st


@pytest.mark.parametrize("kind", ["pageable", "pinned"])
def test_clay_decode_host_paths(kind):
    c = T.ClayCoder(20, 7, 16)
    data = bytes(random.Random(5).getrandbits(8) for _ in range(300_001))
    chunks = c.encode(data)
    cs = len(chunks[0])
    ptrs = (C.c_void_p * N)()
    keep = []
    for i in range(6, 13):
        a = batch.host_empty(cs) if kind == "pinned" else np.empty(cs, np.uint8)
        a[:] = np.frombuffer(chunks[i], np.uint8)
        keep.append(a)
        ptrs[i] = a.ctypes.data
    out = np.empty(7 * cs, np.uint8)
    assert lib.te_clay_decode(c.handle, ptrs, cs, C.c_void_p(out.ctypes.data), out.size) == 0
    assert out.tobytes()[:len(data)] == data
