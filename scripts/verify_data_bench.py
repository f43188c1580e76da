"""Data verify against the only way to the same answer that existed before it:
te_encode_commit_batch_host into a page-locked scratch output, the roots compared on the host.

  --shape a4m     1024 x 4 MiB objects in page-locked host memory, three legs over the same input:
                    baseline   te_encode_commit_batch_host (hashing AUTO) + the compare of the roots;
                    verify     te_verify_data_batch_host;
                    h2d_only   the input's H2D copy alone: what the verify leg approaches.
  --shape b64m    32 x 64 MiB objects (9.7 MB slices), the same legs: a leaf launch is one slice's
                  serial SHA-256, ~0.4 s per group, so the baseline's host hashing may win here.
  --shape dev4m   1024 x 4 MiB objects resident in HBM, kernel times from te_kernel_timing:
                    device_verify   te_verify_data_batch_device;
                    device_commit   te_encode_batch_device + te_commit_batch_device with roots;
                    root_check / tree   the new root kernel against tree_kernel alone (a
                                        te_commit_batch_device with and without roots differ by it).

One shape per process, each under its own time limit, chained:

  timeout -k 10 900 python scripts/verify_data_bench.py --shape a4m --out profiles/verify_data_bench.json && \\
  timeout -k 10 600 python scripts/verify_data_bench.py --shape b64m --out profiles/verify_data_bench.json && \\
  timeout -k 10 600 python scripts/verify_data_bench.py --shape dev4m --out profiles/verify_data_bench.json

The legs alternate round by round after one untimed round of each.  Host-shape times are a host
clock around calls that return only when the results are in host memory.  Done when the verify
leg's median is below the baseline's by more than the baseline's own round-to-round spread
(`verify_beats_baseline`).  --out merges the shape into the JSON file.  Needs a gfx950 device.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tape_amd as T  # noqa: E402
from tape_amd import batch, merkle  # noqa: E402
from tape_amd._lib import lib  # noqa: E402

SHAPES = {"a4m": (1024, 4 << 20), "b64m": (32, 64 << 20), "dev4m": (1024, 4 << 20)}
H = T.SLICE_TREE_HEIGHT


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "runs": v}


def fill(dev, nbytes, seed):
    """Seeded bytes on the device, generated in pieces."""
    torch.manual_seed(seed)
    t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    step = 256 << 20
    for at in range(0, nbytes, step):
        ln = min(step, nbytes - at)
        t[at:at + ln] = torch.randint(0, 256, (ln,), dtype=torch.uint8, device=dev)
    return t


def host_shape(a, s, nobj, size, dev):
    n = s.n()
    slen = int(s.geometry(size).slice_len)
    per = n * slen
    d_in = fill(dev, nobj * size, a.seed)
    h_in = batch.host_empty(nobj * size)
    t_in = torch.from_numpy(h_in)
    t_in.copy_(d_in)
    torch.cuda.synchronize()
    h_out = batch.host_empty(nobj * per)  # the baseline's scratch: slices nobody reads
    leaf = batch.host_empty(nobj * n * 32)
    roots = batch.host_empty(nobj * 32)
    enc = batch.encode_descs([(o * size, size, o * per, o) for o in range(nobj)])
    batch.set_commit_hashing("auto")
    batch.encode_commit_batch_host(s, h_in, enc, h_out, leaf, roots, height=H, window_bytes=a.window)
    want_roots, want_leaf = roots.copy(), leaf.copy()
    xr = (C.c_uint8 * (nobj * 32)).from_buffer_copy(want_roots.tobytes())
    xl = (C.c_uint8 * (nobj * n * 32)).from_buffer_copy(want_leaf.tobytes())
    got_roots = (C.c_uint8 * (nobj * 32))()
    ok = (C.c_uint32 * nobj)()
    mask = (C.c_uint64 * nobj)()
    h, cfg = s.coder.handle, s._cfg()
    vstats = {}

    def run_baseline():
        roots[:] = 0
        batch.encode_commit_batch_host(s, h_in, enc, h_out, leaf, roots, height=H, window_bytes=a.window)
        assert np.array_equal(roots, want_roots)  # the compare a caller makes, 32 bytes per object

    def run_verify():
        r = lib.te_verify_data_batch_host(h, C.byref(cfg), C.c_void_p(h_in.ctypes.data), enc, nobj, H, xr,
                                          xl if a.leaves else None, got_roots, ok, mask if a.leaves else None, a.window)
        assert r == 0, r
        assert all(ok[:nobj]) and bytes(got_roots) == want_roots.tobytes()
        vstats.update(batch.verify_data_launch_stats(s.coder))

    def run_h2d():
        d_in.copy_(t_in, non_blocking=True)
        torch.cuda.synchronize()

    legs = {"baseline": run_baseline, "verify": run_verify, "h2d_only": run_h2d}
    times = {name: [] for name in legs}
    for r in range(a.rounds + 1):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            if r:  # round 0 warms every leg up
                times[name].append(ms)
        print(f"round {r}: " + ", ".join(f"{name} {times[name][-1]:.1f} ms" for name in legs if times[name]), flush=True)
    # one flipped byte is caught, in the object it belongs to
    victim = nobj // 3
    h_in[victim * size + size // 2] ^= 1
    r = lib.te_verify_data_batch_host(h, C.byref(cfg), C.c_void_p(h_in.ctypes.data), enc, nobj, H, xr, None, None, ok,
                                      None, a.window)
    assert r == 0 and [int(x) for x in ok[:nobj]] == [int(o != victim) for o in range(nobj)]
    out = {"nobj": nobj, "size": size, "slice_len": slen, "window_bytes": a.window, "rounds": a.rounds,
           "expected_leaves": bool(a.leaves), "hash_threads": batch.host_hash_threads(), "bytes_in": nobj * size,
           "baseline_bytes_out": nobj * per, "verify_stats": vstats}
    for name in legs:
        out[name + "_ms"] = stats(times[name])
    b = out["baseline_ms"]
    out["verify_beats_baseline"] = out["verify_ms"]["median"] < b["median"] - b["spread"]
    out["verify_over_baseline"] = out["verify_ms"]["median"] / b["median"]
    out["verify_over_h2d_only"] = out["verify_ms"]["median"] / out["h2d_only_ms"]["median"]
    out["verify_GiBps"] = nobj * size / 2**30 / (out["verify_ms"]["median"] / 1e3)
    out["baseline_GiBps"] = nobj * size / 2**30 / (b["median"] / 1e3)
    return out


def device_shape(a, s, nobj, size, dev):
    n = s.n()
    slen = int(s.geometry(size).slice_len)
    per = n * slen
    d_in = fill(dev, nobj * size, a.seed)
    objs = batch.encode_descs([(o * size, size, o * per, o) for o in range(nobj)])
    d_sl = torch.empty(nobj * per, dtype=torch.uint8, device=dev)
    d_leaf = torch.empty(nobj * n * 32, dtype=torch.uint8, device=dev)
    d_roots = torch.empty(nobj * 32, dtype=torch.uint8, device=dev)
    work = torch.empty(batch.verify_data_work_bytes(s, objs), dtype=torch.uint8, device=dev)
    d_got = torch.empty(nobj * 32, dtype=torch.uint8, device=dev)
    d_ok = torch.zeros(nobj, dtype=torch.int32, device=dev)
    d_mask = torch.zeros(nobj, dtype=torch.int64, device=dev)

    def commit(with_roots=True, encode=True):
        if encode:
            batch.encode_batch(s, d_in, objs, d_sl)
        merkle.commit_batch(d_sl, per, slen, n, nobj, d_leaf, d_roots if with_roots else None, height=H)

    def verify():
        batch.verify_data_batch(s, d_in, objs, d_roots, expected_leaves=d_leaf, roots=d_got, ok=d_ok,
                                bad_leaf_mask=d_mask, work=work, height=H)

    def root_check():
        merkle.roots_check_device(d_leaf, n, nobj, d_roots, d_ok, expected_leaves=d_leaf, roots=d_got,
                                  bad_leaf_mask=d_mask, height=H)

    commit()
    torch.cuda.synchronize()
    legs = {"device_commit": commit, "device_verify": verify, "leaves_and_tree": lambda: commit(True, False),
            "leaves_only": lambda: commit(False, False), "root_check": root_check}
    times = {name: [] for name in legs}
    batch.kernel_timing(True)
    for r in range(a.rounds + 1):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            batch.kernel_time_ms()
            fn()
            torch.cuda.synchronize()
            ms, _ = batch.kernel_time_ms()
            if r:
                times[name].append(ms)
        assert bool(d_ok.all()) and torch.equal(d_got, d_roots) and not bool(d_mask.any())
        print(f"round {r}: " + ", ".join(f"{name} {times[name][-1]:.2f} ms" for name in legs if times[name]), flush=True)
    batch.kernel_timing(False)
    out = {"nobj": nobj, "size": size, "slice_len": slen, "rounds": a.rounds}
    for name in legs:
        out[name + "_kernel_ms"] = stats(times[name])
    out["tree_kernel_ms"] = out["leaves_and_tree_kernel_ms"]["median"] - out["leaves_only_kernel_ms"]["median"]
    out["verify_over_commit"] = out["device_verify_kernel_ms"]["median"] / out["device_commit_kernel_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="a4m")
    ap.add_argument("--nobj", type=int, default=0, help="override the shape's object count")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=0, help="window_bytes of both host calls (0 = each call's default: 4 GiB groups / 8 GiB)")
    ap.add_argument("--leaves", type=int, default=1, help="1: expected leaves given, masks returned")
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("verify_data_bench needs a gfx950 device: nothing is measured without one")
    nobj, size = SHAPES[a.shape]
    nobj = a.nobj or nobj
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    out = (device_shape if a.shape == "dev4m" else host_shape)(a, s, nobj, size, dev)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.shape] = out
        open(a.out, "w").write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
