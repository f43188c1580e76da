"""A/B of the full-object decode across the ranged-read change (the decode kernels' output stores
gained a head clip): bench.py --mode decode --pattern random and --mode recover, the parent
commit's library and this tree's alternated over ROUNDS rounds in one GPU visit (the procedure of
DESIGN 4.1).  Writes profiles/range_decode_ab.json: per mode both medians, the parent's own
max - min spread, and whether the new median lies within it.

usage: python scripts/range_decode_ab.py PARENT_TREE [ROUNDS]   (a built checkout of the parent: its
bench.py runs with its own package and library)
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(tree, mode):
    cmd = [sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--mode", mode]
    if mode == "decode":
        cmd += ["--pattern", "random"]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=280)
    if r.returncode:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(r.returncode)  # a failed run ends the visit: nothing more is started
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def main():
    parent = os.path.abspath(sys.argv[1])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    out = {"rounds": rounds, "steps": 10, "warmup": 3, "modes": {}}
    for mode in ("decode", "recover"):
        ms = {"parent": [], "new": []}
        for _ in range(rounds):
            ms["parent"].append(run(parent, mode))
            ms["new"].append(run(ROOT, mode))
        p, n = statistics.median(ms["parent"]), statistics.median(ms["new"])
        spread = max(ms["parent"]) - min(ms["parent"])
        out["modes"][mode] = {"ms_per_step": ms, "parent_median": p, "new_median": n, "parent_spread": spread,
                              "neutral": abs(n - p) <= spread or n <= p}
        print(mode, out["modes"][mode], flush=True)
    path = os.path.join(ROOT, "profiles", "range_decode_ab.json")
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
