"""The data-verify entry points without a device: argument validation (every check runs before
any device call, so it answers the same with and without a GPU), the work-buffer size against
te_slicer_geometry, and the new symbols in the header and the generated Rust binding."""
import ctypes as C
import os
import re

import pytest

import tape_amd as T
from tape_amd import _lib, batch
from tape_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20
MiB = 1 << 20
INVALID, FULL, SMALL = _lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_MERKLE_TREE_FULL, _lib.TE_ERR_BUFFER_TOO_SMALL
SYMBOLS = ("te_roots_check_device", "te_verify_data_work_bytes", "te_verify_data_batch_device",
           "te_verify_data_batch_host", "te_slicer_verify_data", "te_clay_verify_data_launch_stats")
P = C.c_void_p(0x1000)  # a non-NULL, aligned pointer no check dereferences


@pytest.fixture(scope="module")
def slicer():
    return T.Slicer.clay_default()


def test_roots_check_arguments():
    def call(n=20, nobj=1, height=5, leaf=P, xroot=P, xleaf=None, roots=None, ok=P, mask=None):
        return lib.te_roots_check_device(leaf, n, nobj, height, xroot, xleaf, roots, ok, mask, None)
    assert call(n=0) == INVALID
    assert call(n=65) == INVALID
    assert call(height=33) == INVALID
    assert call(n=33, height=5) == INVALID      # n > 2^height
    assert call(n=2, height=0) == INVALID
    assert call(leaf=None) == INVALID
    assert call(xroot=None) == INVALID
    assert call(ok=None) == INVALID
    assert call(leaf=C.c_void_p(0x1002)) == INVALID
    assert call(mask=C.c_void_p(0x1004)) == INVALID
    # the optional pointers may be NULL: with no object there is nothing to launch
    assert call(nobj=0) == _lib.TE_OK
    assert call(n=64, height=6, nobj=0) == _lib.TE_OK and call(n=1, height=32, nobj=0) == _lib.TE_OK


def test_batch_device_arguments(slicer):
    h, cfg = slicer.coder.handle, slicer._cfg()
    objs = batch.encode_descs([(0, 1000, 0, 0)])
    need = batch.verify_data_work_bytes(slicer, objs)

    def call(c=h, cf=C.byref(cfg), data=P, ob=objs, nobj=1, height=5, xroot=P, work=P, wb=need, ok=P):
        return lib.te_verify_data_batch_device(c, cf, data, ob, nobj, height, xroot, None, work, wb, None, ok, None, None)
    assert call(c=None) == INVALID
    assert call(cf=None) == INVALID
    assert call(ob=None) == INVALID
    assert call(data=None) == INVALID
    assert call(xroot=None) == INVALID
    assert call(work=None) == INVALID
    assert call(ok=None) == INVALID
    assert call(height=0) == INVALID and call(height=33) == INVALID
    assert call(height=4) == FULL               # 20 slices, 16 leaves
    assert call(work=C.c_void_p(0x1004)) == INVALID
    assert call(wb=need - 1) == SMALL
    assert call(wb=0) == SMALL


def test_batch_host_arguments(slicer):
    h, cfg = slicer.coder.handle, slicer._cfg()
    objs = batch.encode_descs([(0, 1000, 0, 0)])

    def call(c=h, cf=C.byref(cfg), data=P, ob=objs, nobj=1, height=5, xroot=P, ok=P):
        return lib.te_verify_data_batch_host(c, cf, data, ob, nobj, height, xroot, None, None, ok, None, 0)
    assert call(c=None) == INVALID
    assert call(cf=None) == INVALID
    assert call(ob=None) == INVALID
    assert call(data=None) == INVALID
    assert call(xroot=None) == INVALID
    assert call(ok=None) == INVALID
    assert call(height=0) == INVALID and call(height=33) == INVALID
    assert call(height=4) == FULL


def test_per_call_arguments(slicer):
    h, cfg = slicer.coder.handle, slicer._cfg()
    ok = C.c_int(7)
    root = (C.c_uint8 * 32)()
    data = (C.c_uint8 * 8)()

    def call(c=h, cf=C.byref(cfg), d=data, ln=8, height=5, x=root, okp=C.byref(ok)):
        return lib.te_slicer_verify_data(c, cf, d, ln, height, x, None, okp)
    assert call(c=None) == INVALID
    assert call(cf=None) == INVALID
    assert call(d=None) == INVALID
    assert call(x=None) == INVALID
    assert call(okp=None) == INVALID
    assert call(height=0) == INVALID and call(height=33) == INVALID
    assert call(height=4) == FULL
    assert ok.value == 7  # no failed call wrote a verdict
    with pytest.raises(ValueError):
        slicer.verify_data(b"abc", b"short")


@pytest.mark.parametrize("blob_len", [0, 1, 1_000_001, 4 * MiB])
def test_work_bytes_from_geometry(slicer, blob_len):
    g = slicer.geometry(blob_len)
    slices = N * int(g.slice_len)
    assert int(g.slice_len) % 4 == 0
    one = batch.verify_data_work_bytes(slicer, [(0, blob_len, 0, 0)])
    assert one == (slices + 31) // 32 * 32 + N * 32
    # out_off and chunk_index do not enter; a batch packs the slices back to back, then every leaf
    assert batch.verify_data_work_bytes(slicer, [(5, blob_len, 12345, 9)]) == one
    three = batch.verify_data_work_bytes(slicer, [(0, blob_len, 0, 0), (0, 1_000, 0, 0), (0, blob_len, 0, 0)])
    small = N * int(slicer.geometry(1_000).slice_len)
    assert three == (2 * slices + small + 31) // 32 * 32 + 3 * N * 32
    assert batch.verify_data_work_bytes(slicer, []) == 0


def test_stats_start_at_zero():
    st = T.Slicer.clay_default().verify_data_launch_stats()
    assert set(st) == {"objects", "windows", "groups", "leaf_launches", "root_check_launches", "h2d_bytes",
                       "h2d_expected_bytes", "d2h_bytes"}
    assert not any(st.values())
    assert lib.te_clay_verify_data_launch_stats(None, None) == INVALID


def test_symbols_in_header_and_rust():
    declared = set(_lib.declared_symbols())
    rs = open(os.path.join(ROOT, "rust", "tapeec-sys", "src", "lib.rs")).read()
    rust = set(re.findall(r"pub fn (te_\w+)", rs))
    so = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in declared and name in rust and hasattr(so, name), name
    body = re.search(r"pub struct te_verify_data_stats \{(.*?)\n\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == [f for f, _ in _lib.te_verify_data_stats._fields_]
    hdr = open(_lib.HEADER_PATH).read()
    for name in SYMBOLS[:5]:  # each declaration's comment cites the reference's verify and encode_with_root
        doc = hdr[:hdr.index("int " + name if name != "te_verify_data_work_bytes" else "size_t " + name)]
        doc = doc[doc.rindex("/*"):]
        if name == "te_verify_data_work_bytes":
            continue  # declared under te_verify_data_batch_device's comment
        assert "read.rs:174-185" in doc and "encoder.rs:166-193" in doc, name
    shim = open(os.path.join(ROOT, "rust", "tape-slicer-gpu", "src", "slicer_hook.rs")).read()
    assert "pub fn verify_data(" in shim and "ffi::te_slicer_verify_data(" in shim
