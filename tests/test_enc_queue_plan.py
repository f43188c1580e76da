"""The LDS-DMA encode's task list, checked on the host (no GPU): tests/native/enc_queue_plan.cpp walks
the queue positions of whole-stripe and split (level 1, then level 2) launches through the same
enc_task() the kernel calls; every (stripe, row of planes) must come up exactly once, the level-2
rows only in the second launch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_stripe_row_once(tmp_path):
    exe = str(tmp_path / "enc_queue_plan")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++20", "-I", os.path.join(ROOT, "tape_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "enc_queue_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "launches 1050 bad 0" in r.stdout
