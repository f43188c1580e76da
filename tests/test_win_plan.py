"""The host pipelines' window planning, checked on the host (no GPU): tests/native/win_plan_check.cpp
runs tape_amd/csrc/win_plan.hpp -- the one window_cuts, add_run and VerLayout the read and rebuild
pipelines share -- over seeded random inputs and their edge cases: cuts that start at 0, end at n,
increase, fit the window or hold a single object and are greedy; coalesced copy runs that map the
same bytes as the raw pieces, skip zero lengths and merge only what is contiguous on both sides; a
verify workspace laid out expected | digests | masks, 4-byte aligned, whose read shape equals the
offsets verify_wait used."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_win_plan(tmp_path):
    exe = str(tmp_path / "win_plan_check")
    r = subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", "-I", os.path.join(ROOT, "tape_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "win_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "win_plan bad 0" in r.stdout
