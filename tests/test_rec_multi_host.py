"""The multi-output rebuild's host side, checked on the host (no GPU):
tests/native/rec_multi_check.cpp runs tape_amd/csrc/rec_multi_plan.hpp for Clay(20,7,16) -- 512
seeded (survivor set, lost subset) pairs over every a0 = 0..7, lost sets of 2, 3, 7 and 13 slices
in either column and across both, identity and rotated layouts: each sub-mask's program interpreted
value by value, every output row through the job's node -> slot table, must rebuild exactly the lost
slices' chunks of an oracle-encoded stripe; the split rule over every lost-set size for one
survivor set per a0 (a partition, every part compiles and fits, a set that fits whole stays whole);
the mask rules and the routing rule at their edges.  Then the argument errors through the C ABI."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rec_multi_plan(tmp_path):
    exe = str(tmp_path / "rec_multi_check")
    ora = os.path.join(ROOT, "oracle")
    if not os.path.exists(os.path.join(ora, "libclay_oracle.so")):
        subprocess.run(["make", "-s", "-C", ora], check=True)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++20", "-Wall", "-I", os.path.join(ROOT, "tape_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "rec_multi_check.cpp"), "-L", ora, "-lclay_oracle",
                        "-Wl,-rpath," + ora, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]  # the exit status is the number of failed checks
    assert "rec_multi pairs 512" in r.stdout and r.stdout.rstrip().endswith("bad 0")


# ---- argument validation through the C ABI: every error below is decided before any device use ----
TE_OK, NOT_ENOUGH, INVALID_LAYOUT, INVALID_ARG = 0, 3, 5, 20


@pytest.fixture(scope="module")
def abi():
    import tape_amd as T
    from tape_amd import _lib
    sl = T.Slicer.with_rotation(T.ClayCoder(20, 7, 16))
    slen = int(sl.geometry(20000).slice_len)
    meta = T.SliceMetadata.new(20000, sl.stripe_size).to_bytes()
    yield _lib, _lib.lib, sl.coder.handle, sl._cfg(), slen, meta


def _call(abi, avail, lost, slice_len=None, meta=None):
    _lib, lib, h, cfg, slen, m = abi
    o = _lib.te_recover_multi_object(0, slen if slice_len is None else slice_len, avail, lost, 0)
    mb = (C.c_uint8 * 48).from_buffer_copy(m if meta is None else meta)
    # device pointers that are never dereferenced: every case returns before the device is touched
    return lib.te_recover_multi_batch_device(h, C.byref(cfg), C.c_void_p(0x1000), C.byref(o), mb, 1, C.c_void_p(0x2000), None)


@pytest.mark.parametrize("avail,lost", [(0x7f, 0), (0x7f, 1 << 20), (0x7f, 1 << 31), (0x7f, 0x40), (0x7f, 0x7f),
                                        (0x3f, 0xfffc0)])
def test_abi_invalid_lost_mask(abi, avail, lost):
    assert _call(abi, avail, lost) == INVALID_ARG


def test_abi_not_enough_slices(abi):
    assert _call(abi, 0x3f, 0x80) == NOT_ENOUGH
    assert _call(abi, 0, 0x80) == NOT_ENOUGH


def test_abi_layout_errors(abi):
    _lib, lib, h, cfg, slen, m = abi
    assert _call(abi, 0x7f, 0x180, slice_len=slen + 200) == INVALID_LAYOUT  # not this object's slice length
    assert _call(abi, 0x7f, 0x180, slice_len=40) == INVALID_LAYOUT          # shorter than the suffix's chunks
    import tape_amd as T
    bad = T.SliceMetadata.new(20000, 999).to_bytes()  # no stripe size: the suffix does not parse -- the single-slice path's error
    mb = (C.c_uint8 * 48).from_buffer_copy(bad)
    md = _lib.te_slice_metadata()
    want = lib.te_slice_metadata_from_slice(mb, 48, C.byref(md))
    assert want not in (TE_OK, 21)
    assert _call(abi, 0x7f, 0x180, meta=bad) == want


def test_abi_null_arguments(abi):
    _lib, lib, h, cfg, slen, m = abi
    o = _lib.te_recover_multi_object(0, slen, 0x7f, 0x180, 0)
    mb = (C.c_uint8 * 48).from_buffer_copy(m)
    assert lib.te_recover_multi_batch_device(None, C.byref(cfg), None, C.byref(o), mb, 1, None, None) == INVALID_ARG
    assert lib.te_recover_multi_batch_device(h, None, None, C.byref(o), mb, 1, None, None) == INVALID_ARG
    assert lib.te_recover_multi_batch_device(h, C.byref(cfg), None, None, mb, 1, None, None) == INVALID_ARG
    assert lib.te_recover_multi_batch_device(h, C.byref(cfg), None, C.byref(o), None, 1, None, None) == INVALID_ARG
    assert lib.te_recover_multi_batch_device(h, C.byref(cfg), None, None, None, 0, None, None) == TE_OK
    st = _lib.te_recover_multi_stats()
    assert lib.te_clay_recover_multi_launch_stats(h, C.byref(st)) == TE_OK
    assert lib.te_clay_recover_multi_launch_stats(None, C.byref(st)) == INVALID_ARG
    assert (st.multi_launches, st.passes, st.jobs) == (0, 0, 0)


def test_abi_host_form_arguments(abi):
    """te_slicer_recover_multi: a lost bit whose slice is present, an empty lost mask, a missing
    output pointer, too few slices -- decided from the pointers alone."""
    _lib, lib, h, cfg, slen, m = abi
    buf = bytes(slen - 48) + m
    keep = [C.create_string_buffer(buf, slen) for _ in range(7)]
    ptrs = (C.c_void_p * 20)(*([C.addressof(k) for k in keep] + [None] * 13))
    outs = (C.c_void_p * 2)(C.addressof(keep[0]), C.addressof(keep[1]))
    f = lib.te_slicer_recover_multi
    assert f(h, C.byref(cfg), ptrs, slen, 0, outs) == INVALID_ARG
    assert f(h, C.byref(cfg), ptrs, slen, 0x41, outs) == INVALID_ARG        # slice 6 is present
    assert f(h, C.byref(cfg), ptrs, slen, 1 << 20, outs) == INVALID_ARG
    assert f(h, C.byref(cfg), ptrs, slen, 0x180, (C.c_void_p * 2)(C.addressof(keep[0]), None)) == INVALID_ARG
    few = (C.c_void_p * 20)(*([C.addressof(k) for k in keep[:6]] + [None] * 14))
    assert f(h, C.byref(cfg), few, slen, 0x180, outs) == NOT_ENOUGH
    assert f(h, C.byref(cfg), ptrs, 40, 0x180, outs) == INVALID_LAYOUT
