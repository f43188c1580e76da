"""The decode call's host side, checked on the host (no GPU): tests/native/dec_plan_check.cpp runs
tape_amd/csrc/dec_plan.hpp -- the one stripe walk, pattern key, group key, staged-geometry rule
and class routing decode_enqueue, range_chunk_ok and recover_batch share -- for Clay(20,7,16) over
seeded random inputs and their edges: one job per stripe of a full or raw decode, the last clipped
to the object; a ranged call's copies and job windows tiling the window exactly once, each copy
from the slice that holds its data chunk, a stripe copied exactly when its touched chunks are
present; the chunk path's lone erased chunk as a windowed job of that shard; node recover's output
node under rotation; distinct keys in first-seen order; the group key ordered like the integer key
it replaces; each bound of the geometry rule from both sides; the fold-back rule at each edge, the
class groups' order, and TE_ERR_UNSUPPORTED for a chunk stripe without a windowed kernel."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dec_plan(tmp_path):
    exe = str(tmp_path / "dec_plan_check")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++20", "-Wall", "-I", os.path.join(ROOT, "tape_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "dec_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]  # the exit status is the number of failed checks
    assert "dec_plan bad 0" in r.stdout
