"""tests/native/rec_multi_check.cpp for the tests that run it (tests/test_rec_multi_host.py,
tests/test_recover_multi_geometry_cases.py): one build recipe, one build per session, and the
parser of its report mode.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_exe = {}


def build(tmp_path_factory):
    """The check as a program, built on first use."""
    if "exe" not in _exe:
        exe = str(tmp_path_factory.mktemp("native") / "rec_multi_check")
        ora = os.path.join(ROOT, "oracle")
        if not os.path.exists(os.path.join(ora, "libclay_oracle.so")):
            subprocess.run(["make", "-s", "-C", ora], check=True)
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++20", "-Wall", "-I", os.path.join(ROOT, "tape_amd", "csrc"),
                            os.path.join(ROOT, "tests", "native", "rec_multi_check.cpp"), "-L", ora, "-lclay_oracle",
                            "-Wl,-rpath," + ora, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _exe["exe"] = exe
    return _exe["exe"]


def report(exe, cases):
    """cases: [(k, available mask, lost mask, rotated, stripe)] -> per case the list of its passes,
    each a dict of the report's figures as ints (`sub` is a node mask)."""
    args = [f"{k}:{a:x}:{lo:x}:{int(rot)}:{st}" for k, a, lo, rot, st in cases]
    out = []
    for at in range(0, len(args), 400):  # a command line of bounded length
        r = subprocess.run([exe, "report"] + args[at:at + 400], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
        for ln in r.stdout.splitlines():
            f = ln.split()
            if f[0] == "case":
                assert f[1] == args[len(out)]
                out.append([])
                npass = int(f[3])
            else:
                out[-1].append({f[i]: int(f[i + 1], 16 if f[i] == "sub" else 10) for i in range(1, len(f), 2)})
                assert len(out[-1]) <= npass
    assert len(out) == len(cases)
    return out
