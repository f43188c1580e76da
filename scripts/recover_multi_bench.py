"""Multi-slice node recover against the route that existed before it: L lost slices
of each object rebuilt by one te_recover_multi_batch_device call, or by L te_recover_batch_device
calls over the same resident peer slices (the parent route, in the same process).

  device   --nobj x --size objects on the device, random 7-of-20 survivors per object, L lost slices
           drawn from the other 13; both legs' kernel time (te_kernel_timing: event pairs around the
           call's launches) and wall time (host clock, stream synchronised), per L;
  percall  one object in pageable host memory: te_slicer_recover_multi against L times (H2D of the
           7 peer slices, a one-object te_recover_batch_device, D2H of the rebuilt slice).

The legs alternate round by round after one untimed round of each (the first call of a leg also
compiles its stripes' programs on the host); figures are medians with the runs kept.  Every leg's
output is compared with the encoded slices.  L = 1 measures the routing rule: the multi call
delegates to the single-slice path.

  timeout -k 10 900 python scripts/recover_multi_bench.py --out profiles/recover_multi_bench.json

Needs a gfx950 device.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tape_amd as T  # noqa: E402
from tape_amd import _lib, batch  # noqa: E402
from tape_amd._lib import lib  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "runs": v}


def kernel_ms():
    tot, cnt = C.c_double(), C.c_uint32()
    assert lib.te_kernel_time_ms(C.byref(tot), C.byref(cnt)) == 0
    return tot.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nobj", type=int, default=1024)
    ap.add_argument("--size", type=int, default=4 << 20)
    ap.add_argument("--lost", default="1,2,4,13")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("recover_multi_bench needs a gfx950 device: nothing is measured without one")
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n, k = s.n(), s.k()
    nobj, size = a.nobj, a.size
    slen = int(s.geometry(size).slice_len)
    per = n * slen
    torch.manual_seed(a.seed)
    d_in = torch.randint(0, 256, (nobj * size,), dtype=torch.uint8, device=dev)
    d_sl = torch.empty(nobj * per, dtype=torch.uint8, device=dev)
    batch.encode_batch(s, d_in, [(i * size, size, i * per, i) for i in range(nobj)], d_sl)
    torch.cuda.synchronize()
    del d_in
    torch.cuda.empty_cache()
    metas = b"".join(d_sl[o * per + slen - 48:o * per + slen].cpu().numpy().tobytes() for o in range(nobj))
    rng = random.Random(a.seed)
    surv = [sorted(rng.sample(range(n), k)) for _ in range(nobj)]
    masks = [sum(1 << j for j in p) for p in surv]
    order = [rng.sample([j for j in range(n) if j not in p], n - k) for p in surv]  # lost slices: a prefix of it
    sl3 = d_sl.view(nobj, n, slen)
    res = {"nobj": nobj, "size": size, "slice_len": slen, "rounds": a.rounds, "device": {}, "percall": {}}
    lib.te_kernel_timing(1)
    for L in [int(x) for x in a.lost.split(",")]:
        lost = [sorted(o[:L]) for o in order]
        d_out = torch.empty(nobj * L * slen, dtype=torch.uint8, device=dev)
        idx = torch.tensor(lost, device=dev)
        want = sl3[torch.arange(nobj, device=dev)[:, None], idx].reshape(-1)
        multi = [(o * per, slen, masks[o], sum(1 << j for j in lost[o]), o * L * slen) for o in range(nobj)]
        single = [[(o * per, slen, masks[o], lost[o][j], (o * L + j) * slen) for o in range(nobj)] for j in range(L)]

        def run_multi():
            batch.recover_multi_batch(s, d_sl, multi, metas, d_out)

        def run_parent():
            for j in range(L):
                batch.recover_batch(s, d_sl, single[j], metas, d_out)

        legs = {"parent": run_parent, "multi": run_multi}
        wall = {x: [] for x in legs}
        kern = {x: [] for x in legs}
        for r in range(a.rounds + 1):
            for name, fn in legs.items():
                d_out.zero_()
                torch.cuda.synchronize()
                kernel_ms()  # drain the pairs of the setup
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                km = kernel_ms()
                assert torch.equal(d_out, want), (name, L)
                if r:
                    wall[name].append(ms)
                    kern[name].append(km)
                if name == "multi":
                    st = batch.recover_multi_launch_stats(s.coder)
            print(f"L={L} round {r}: " + ", ".join(f"{x} kernel {kern[x][-1]:.2f} wall {wall[x][-1]:.1f} ms"
                                                   for x in legs if wall[x]), flush=True)
        e = {"multi_stats": st}
        for name in legs:
            e[name + "_kernel_ms"] = stats(kern[name])
            e[name + "_wall_ms"] = stats(wall[name])
        p = e["parent_kernel_ms"]
        e["multi_over_parent_kernel"] = e["multi_kernel_ms"]["median"] / p["median"]
        e["multi_beats_parent_kernel"] = e["multi_kernel_ms"]["median"] < p["median"] - p["spread"]
        e["multi_over_parent_wall"] = e["multi_wall_ms"]["median"] / e["parent_wall_ms"]["median"]
        res["device"][str(L)] = e
        del d_out, want
        torch.cuda.empty_cache()
    lib.te_kernel_timing(0)

    # per call, host to host, pageable memory: object 0
    h_sl = d_sl[:per].cpu().numpy().reshape(n, slen).copy()
    d_one = torch.empty(per, dtype=torch.uint8, device=dev)
    d_rec = torch.empty(slen, dtype=torch.uint8, device=dev)
    cfg = s._cfg()
    keep = {j: np.ascontiguousarray(h_sl[j]).copy() for j in surv[0]}
    ptrs = (C.c_void_p * n)(*[keep[j].ctypes.data if j in keep else None for j in range(n)])
    mb = (C.c_uint8 * 48).from_buffer_copy(metas[:48])
    for L in [int(x) for x in a.lost.split(",")]:
        lost = sorted(order[0][:L])
        outs = [np.zeros(slen, np.uint8) for _ in lost]
        optrs = (C.c_void_p * L)(*[o.ctypes.data for o in outs])
        lm = sum(1 << j for j in lost)
        one = [batch.recover_descs([(0, slen, masks[0], j, 0)]) for j in lost]

        def run_multi():
            assert lib.te_slicer_recover_multi(s.coder.handle, C.byref(cfg), ptrs, slen, lm, optrs) == 0

        def run_parent():
            for i, j in enumerate(lost):
                for p in surv[0]:
                    d_one[p * slen:(p + 1) * slen].copy_(torch.from_numpy(keep[p]), non_blocking=True)
                assert lib.te_recover_batch_device(s.coder.handle, C.byref(cfg), C.c_void_p(d_one.data_ptr()), one[i], mb, 1,
                                                   C.c_void_p(d_rec.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
                torch.from_numpy(outs[i]).copy_(d_rec)

        legs = {"parent": run_parent, "multi": run_multi}
        wall = {x: [] for x in legs}
        for r in range(2 * a.rounds + 1):
            for name, fn in legs.items():
                for o in outs:
                    o[:] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ms = (time.perf_counter() - t0) * 1e3
                for o, j in zip(outs, lost):
                    assert np.array_equal(o, h_sl[j]), (name, L, j)
                if r:
                    wall[name].append(ms)
        e = {name + "_ms": stats(wall[name]) for name in legs}
        e["multi_over_parent"] = e["multi_ms"]["median"] / e["parent_ms"]["median"]
        res["percall"][str(L)] = e
        print(f"percall L={L}: parent {e['parent_ms']['median']:.2f} ms, multi {e['multi_ms']['median']:.2f} ms", flush=True)
    print(json.dumps({k: v for k, v in res.items() if k not in ("device", "percall")}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
