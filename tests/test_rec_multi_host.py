"""The multi-output rebuild's host side, checked on the host (no GPU):
tests/native/rec_multi_check.cpp (built once) runs tape_amd/csrc/rec_multi_plan.hpp for Clay(20,7,16) -- 512
seeded (survivor set, lost subset) pairs over every a0 = 0..7, lost sets of 2, 3, 7 and 13 slices
in either column and across both, identity and rotated layouts: each sub-mask's program interpreted
value by value, every output row through the job's node -> slot table, must rebuild exactly the lost
slices' chunks of an oracle-encoded stripe; the split rule over every lost-set size for one
survivor set per a0 (a partition, every part compiles and fits, a set that fits whole stays whole);
the mask rules and the routing rule at their edges.  The same values and split parts run for
Clay(20,8,17), (20,9,18) and (20,10,19) (`rec_multi_check <k>`), whose programs have other matrix
tables, 12, 11 and 10 padded erasures and slot tables of their own; its report mode is what
tests/test_recover_multi_geometry_cases.py reads.  Then the argument errors through the C ABI."""
import ctypes as C
import subprocess

import pytest

import rec_multi_native as native


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/native/rec_multi_check.cpp, built once for every run of the session."""
    return native.build(tmp_path_factory)


def test_rec_multi_plan(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]  # the exit status is the number of failed checks
    assert "rec_multi pairs 512" in r.stdout and r.stdout.rstrip().endswith("bad 0")
    assert r.stdout.rstrip() == ("rec_multi pairs 512 passes 758 split 198 rows 320000 split_sets 2312 "
                                 "(split 1081 whole 1231) bad 0")  # the run is seeded: the line as it has always been


@pytest.mark.parametrize("k", [8, 9, 10])
def test_rec_multi_plan_other_profiles(check_exe, k):
    """Clay(20,k,k+9): the values and split parts and the rec_route edges.  64 pairs per a0 (16 of
    each lost-set size), a0 = 0..min(k, 10); a run takes about two seconds."""
    r = subprocess.run([check_exe, str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    a0s = min(k, 10) - max(0, k - 10) + 1
    assert f"rec_multi k {k} pairs {64 * a0s} " in r.stdout and r.stdout.rstrip().endswith("bad 0")
    # every pair stores alpha rows per lost slice exactly once: 16 pairs of 2, 3, ceil(m / 2) and m slices per a0
    m = 20 - k
    assert f" rows {a0s * 16 * (2 + 3 + (m + 1) // 2 + m) * 100} " in r.stdout


def test_rec_multi_report(check_exe):
    """The report mode on a case whose figures are known: two lost nodes of column 0 of
    Clay(20,7,16) are one pass, a pair that is finished together; a malformed case is refused."""
    r = subprocess.run([check_exe, "report", "7:3c0d:12:0:0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split()[:4] == ["case", "7:3c0d:12:0:0", "passes", "1"] and len(lines) == 2
    f = dict(zip(lines[1].split()[1::2], lines[1].split()[2::2]))
    assert f["sub"] == "00012" and int(f["rows"]) == int(f["nslots"]) + 2 and int(f["finish_both"]) > 0 and f["noslot"] == "0"
    assert subprocess.run([check_exe, "report", "7:3c0d:1:0:0"], capture_output=True).returncode == 2  # slice 0 is present


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
