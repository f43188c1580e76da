"""The ranged read entry points on the Rust side: the generated tapeec-sys declarations are in step
with include/tape_ec.h and the ctypes mirror, and the tape-slicer-gpu shim's Slicer hook offers
decode_range over te_slicer_decode_range.  Checked textually, like tests/test_rust_binding.py (no
Rust toolchain in the image)."""
import os
import re
import subprocess
import sys

from tape_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = os.path.join(ROOT, "rust", "tapeec-sys", "src", "lib.rs")
HOOK = os.path.join(ROOT, "rust", "tape-slicer-gpu", "src", "slicer_hook.rs")
ENTRY_POINTS = ("te_slicer_range_plan", "te_decode_range_batch_device", "te_slicer_decode_range",
                "te_clay_range_launch_stats")


def test_generated_binding_is_current_and_has_the_ranged_calls():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_rust_sys.py"), "--check"])
    assert r.returncode == 0, "rust/tapeec-sys/src/lib.rs is stale: run scripts/gen_rust_sys.py"
    rs = open(RS).read()
    declared = set(re.findall(r"pub fn (te_\w+)", rs))
    assert set(ENTRY_POINTS) <= declared
    assert set(ENTRY_POINTS) <= set(_lib.declared_symbols())
    assert ("pub fn te_slicer_decode_range(c: *mut te_clay, cfg: *const te_slicer_cfg, slices: *const *const u8, "
            "slice_len: usize, start: u64, len: u64, out: *mut u8, cap: usize, out_len: *mut usize) -> c_int;") in rs
    assert "pub fn te_slicer_range_plan(c: *const te_clay," in rs  # host only: a const handle
    assert re.search(r"TE_RANGE_COPY\b.*= 0;", rs)
    assert re.search(r"TE_RANGE_DECODE\b.*= 1;", rs)


def test_struct_fields_match_ctypes_mirror():
    rs = open(RS).read()
    for name in ("te_decode_range_object", "te_range_launch_stats"):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, rs, flags=re.S).group(1)
        fields = re.findall(r"pub (\w+):\s*(\w+)", body)
        mirror = getattr(_lib, name)._fields_
        assert [f for f, _ in fields] == [f[0] for f in mirror], (name, fields)
        width = {"u64": 8, "u32": 4}
        import ctypes as C
        assert [width[t] for _, t in fields] == [C.sizeof(f[1]) for f in mirror], (name, fields)


def test_shim_offers_decode_range():
    hook = open(HOOK).read()
    m = re.search(r"pub fn decode_range\(&mut self, cfg: &ObjectCfg, slices: &\[\(usize, &\[u8\]\)\], start: u64, len: u64\)"
                  r"\s*-> Result<Vec<u8>, DecodeError> \{(.*?)\n    \}", hook, flags=re.S)
    assert m, "ClayCoder::decode_range is missing from the Slicer hook"
    body = m.group(1)
    assert "ffi::te_slicer_decode_range(self.raw.as_ptr(), &c, ptrs.as_ptr(), slen, start, len," in body
    assert "decode_status(r)" in body and "out.truncate(got)" in body
    assert "vec![0u8; len as usize]" in body  # exactly the window, not the object
    called = set(re.findall(r"ffi::(te_\w+)\(", hook))
    assert {"te_slicer_decode_range", "te_slicer_range_plan", "te_clay_range_launch_stats"} <= called
    # the stats struct literal names every field of the header's struct
    lit = re.search(r"= ffi::te_range_launch_stats \{(.*?)\}", hook, flags=re.S).group(1)
    assert re.findall(r"(\w+): 0", lit) == [f[0] for f in _lib.te_range_launch_stats._fields_]
