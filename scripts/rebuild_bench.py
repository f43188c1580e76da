"""Node rebuild pipeline against the per-object ways that existed before it: verified
repair and verified recover of objects whose fragments / peer slices lie in page-locked host memory,
three legs over the same buffers:

  parent     repair: a loop of te_slicer_repair + te_verify_slice, one call per object;
             recover: per object the H2D copies of its peer slices, a one-object
             te_recover_verified_batch_device and the D2H copy of the rebuilt slice;
  batch      te_repair_batch_host / te_recover_batch_host with leaves;
  copy_only  the batch call's H2D and D2H copies with no hashing and no kernels
             (TEC_DEBUG_KNOBS=1 TEC_REBUILD_COPY_ONLY=1): the ceiling of the pipeline on the box.

Shapes: `repair4m` / `recover4m` = 1024 x 4 MiB objects, `repair64m` / `recover64m` = 32 x 64 MiB;
a repair has all 19 other slices up, a recover random 7-of-20 peers.  One shape per process; each GPU
step under its own time limit, chained:

  timeout -k 10 600 python scripts/rebuild_bench.py --shape repair4m --out profiles/rebuild_bench.json && \\
  timeout -k 10 600 python scripts/rebuild_bench.py --shape recover4m --out profiles/rebuild_bench.json

The legs run alternately, round by round, after one untimed round of each; times are a host clock
around calls that return only when the bytes are in host memory.  Acceptance: the batch call's
median is below the parent's by more than the parent's own round-to-round spread
(`batch_beats_parent`).  --out merges the shape into the JSON file.  Needs a gfx950 device.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

os.environ["TEC_DEBUG_KNOBS"] = "1"  # the copy-only leg's switch is read per call
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tape_amd as T  # noqa: E402
from tape_amd import _lib, batch, merkle  # noqa: E402
from tape_amd._lib import lib  # noqa: E402

SHAPES = {"repair4m": (1024, 4 << 20), "recover4m": (1024, 4 << 20), "repair64m": (32, 64 << 20),
          "recover64m": (32, 64 << 20)}


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="repair4m")
    ap.add_argument("--nobj", type=int, default=0, help="override the shape's object count")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=0, help="window_bytes (0 = 128 MiB)")
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("rebuild_bench needs a gfx950 device: nothing is measured without one")
    nobj, size = SHAPES[a.shape]
    nobj = a.nobj or nobj
    repair = a.shape.startswith("repair")
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n, k = s.n(), s.k()
    g = s.geometry(size)
    slen = int(g.slice_len)
    per = n * slen
    # objects encoded and committed on the device, then every slice copied to host memory
    torch.manual_seed(a.seed)
    d_in = torch.randint(0, 256, (nobj * size,), dtype=torch.uint8, device=dev)
    d_sl = torch.empty(nobj * per, dtype=torch.uint8, device=dev)
    batch.encode_batch(s, d_in, [(i * size, size, i * per, i) for i in range(nobj)], d_sl)
    d_leaf = torch.empty(nobj * n * 32, dtype=torch.uint8, device=dev)
    merkle.commit_batch(d_sl, per, slen, n, nobj, d_leaf)
    torch.cuda.synchronize()
    h_sl = batch.host_empty(nobj * per)
    torch.from_numpy(h_sl).copy_(d_sl)
    leaves = d_leaf.cpu().numpy().tobytes()
    del d_in, d_sl, d_leaf
    torch.cuda.empty_cache()
    rng = random.Random(a.seed)
    lost = [rng.randrange(n) for _ in range(nobj)]
    h_out = batch.host_empty(nobj * slen)
    want = np.concatenate([h_sl[o * per + lost[o] * slen:o * per + (lost[o] + 1) * slen] for o in range(nobj)])
    lb = (C.c_uint8 * len(leaves)).from_buffer_copy(leaves)
    base_out, base_lb = h_out.ctypes.data, C.addressof(lb)
    ok = (C.c_uint32 * nobj)()
    h = s.coder.handle
    cfg = s._cfg()

    if repair:
        plans = {}
        for lo in set(lost):
            plans[lo] = s.repair_plan_from_params(lo, [j for j in range(n) if j != lo], size, int(g.stripe_size))
        need = {lo: [int(lib.te_extract_repair_data_size(p.handle, j)) for j in range(n)] for lo, p in plans.items()}
        total = sum(sum(need[lo]) for lo in lost)
        h_in = batch.host_empty(total)
        base_in = h_in.ctypes.data
        objs, cur, got = [], 0, C.c_size_t()
        for o in range(nobj):
            offs = {}
            for j in range(n):
                ln = need[lost[o]][j]
                if not ln:
                    continue
                r = lib.te_extract_repair_data(plans[lost[o]].handle, C.c_void_p(h_sl.ctypes.data + o * per + j * slen), slen,
                                               j, C.c_void_p(base_in + cur), ln, C.byref(got))
                assert r == 0 and got.value == ln
                offs[j] = cur
                cur += ln
            objs.append((plans[lost[o]], offs, o * slen, h_sl[o * per + slen - 48:o * per + slen].tobytes()))
        descs = batch.repair_descs(objs)
        cuts = batch.repair_window_plan(s.coder, descs, a.window)
        moved_in = total
        pp, pl = [], []
        for o in range(nobj):
            p, ln = (C.c_void_p * n)(), (C.c_size_t * n)()
            for j, off in objs[o][1].items():
                p[j] = base_in + off
                ln[j] = need[lost[o]][j]
            pp.append(p)
            pl.append(ln)
        metas = [(C.c_uint8 * 48).from_buffer_copy(ob[3]) for ob in objs]

        def run_parent():
            for o in range(nobj):
                r = lib.te_slicer_repair(h, plans[lost[o]].handle, pp[o], pl[o], metas[o], C.c_void_p(base_out + o * slen), slen)
                assert r == 0, (o, r)
                assert lib.te_verify_slice(C.c_void_p(base_lb + o * n * 32), n, lost[o], C.c_void_p(base_out + o * slen), slen) == 1

        def call_batch():
            return lib.te_repair_batch_host(h, C.c_void_p(base_in), descs, lb, nobj, C.c_void_p(base_out), ok, a.window)
    else:
        sets = [sorted(rng.sample([j for j in range(n) if j != lost[o]], k)) for o in range(nobj)]
        masks = [sum(1 << j for j in p) for p in sets]
        metas = b"".join(h_sl[o * per + slen - 48:o * per + slen].tobytes() for o in range(nobj))
        mb = (C.c_uint8 * len(metas)).from_buffer_copy(metas)
        descs = batch.recover_descs([(o * per, slen, masks[o], lost[o], o * slen) for o in range(nobj)])
        cuts = batch.recover_window_plan(s.coder, descs, a.window)
        moved_in = k * slen * nobj
        rej, st = (C.c_uint32 * nobj)(), (C.c_int * nobj)()
        d_one = torch.empty(per, dtype=torch.uint8, device=dev)
        d_rec = torch.empty(slen, dtype=torch.uint8, device=dev)
        t_sl, t_out = torch.from_numpy(h_sl), torch.from_numpy(h_out)
        one = [batch.recover_descs([(0, slen, masks[o], lost[o], 0)]) for o in range(nobj)]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        r1, o1, s1 = (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), (C.c_int * 1)()

        def run_parent():
            for o in range(nobj):
                for j in sets[o]:
                    d_one[j * slen:(j + 1) * slen].copy_(t_sl[o * per + j * slen:o * per + (j + 1) * slen], non_blocking=True)
                r = lib.te_recover_verified_batch_device(h, C.byref(cfg), C.c_void_p(d_one.data_ptr()), one[o],
                                                         C.c_void_p(C.addressof(mb) + o * 48), C.c_void_p(base_lb + o * n * 32),
                                                         1, C.c_void_p(d_rec.data_ptr()), r1, o1, s1, stream)
                assert r == 0 and s1[0] == 0 and o1[0] == 1 and r1[0] == 0, (o, r)
                t_out[o * slen:(o + 1) * slen].copy_(d_rec)

        def call_batch():
            return lib.te_recover_batch_host(h, C.byref(cfg), C.c_void_p(h_sl.ctypes.data), descs, mb, lb, nobj,
                                             C.c_void_p(base_out), rej, ok, st, a.window)

    def run_batch():
        assert call_batch() == 0 and all(ok[:nobj])

    def run_copy_only():
        os.environ["TEC_REBUILD_COPY_ONLY"] = "1"
        try:
            r = call_batch()
        finally:
            os.environ["TEC_REBUILD_COPY_ONLY"] = "0"
        assert r == 0, r

    legs = {"parent": run_parent, "batch": run_batch, "copy_only": run_copy_only}
    times = {name: [] for name in legs}
    rb_stats = {}
    for r in range(a.rounds + 1):
        for name, fn in legs.items():
            if name != "copy_only":
                h_out[:] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            if name != "copy_only":
                assert np.array_equal(h_out, want), name
            else:
                rb_stats[name] = batch.rebuild_launch_stats(s.coder)
            if name == "batch":
                rb_stats[name] = batch.rebuild_launch_stats(s.coder)
            if r:  # round 0 warms every leg up
                times[name].append(ms)
        print(f"round {r}: " + ", ".join(f"{name} {times[name][-1]:.1f} ms" for name in legs if times[name]), flush=True)
    out = {"nobj": nobj, "size": size, "slice_len": slen, "windows": len(cuts) - 1, "window_bytes": a.window or 128 << 20,
           "rounds": a.rounds, "hash_threads": batch.host_hash_threads(), "bytes_in": moved_in, "bytes_out": nobj * slen,
           "rebuild_stats": rb_stats}
    for name in legs:
        out[name + "_ms"] = stats(times[name])
    p = out["parent_ms"]
    out["batch_beats_parent"] = out["batch_ms"]["median"] < p["median"] - p["spread"]
    out["batch_over_parent"] = out["batch_ms"]["median"] / p["median"]
    out["batch_over_copy_only"] = out["batch_ms"]["median"] / out["copy_only_ms"]["median"]
    out["rebuilt_GiBps"] = nobj * slen / 2**30 / (out["batch_ms"]["median"] / 1e3)
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.shape] = out
        open(a.out, "w").write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
