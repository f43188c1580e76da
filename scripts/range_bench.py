"""Ranged reads against the full decode: device time should follow the stripes a window
touches, not the object's size.

usage: python scripts/range_bench.py [--nobj 32] [--size 67108864] [--rounds 7] [--out profiles/range_bench.json]

Device lines: nobj objects resident in HBM, Clay(20,7,16) rotated, random 7-of-20 survivor sets;
the full te_decode_batch_device (what any range costs without this feature), then
te_decode_range_batch_device with one window per object of 64 KiB, 1 MiB and 8 MiB at seeded
random offsets, and the 1 MiB window again with all 20 slices present (copy stripes only).  Times
are HIP event pairs around the launches (te_kernel_timing), medians of `rounds` rounds after one
untimed round, with min and max.  Every line's bytes are checked against the objects once.
Per-call host lines: one object's slices on the host, te_slicer_decode against
te_slicer_decode_range of a 64 KiB and a 1 MiB window, wall time, pageable and page-locked buffers.
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
from tape_amd import batch  # noqa: E402
from tape_amd._lib import lib  # noqa: E402

KiB, MiB = 1 << 10, 1 << 20


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nobj", type=int, default=32)
    ap.add_argument("--size", type=int, default=64 * MiB)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=33)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("range_bench needs a gfx950 device: nothing is measured without one")
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n, k = s.n(), s.k()
    g = s.geometry(a.size)
    slen, per, ns, S = int(g.slice_len), n * int(g.slice_len), int(g.num_stripes), int(g.stripe_size)
    torch.manual_seed(a.seed)
    d_in = torch.randint(0, 256, (a.nobj * a.size,), dtype=torch.uint8, device=dev)
    d_sl = torch.empty(a.nobj * per, dtype=torch.uint8, device=dev)
    batch.encode_batch(s, d_in, [(i * a.size, a.size, i * per, i) for i in range(a.nobj)], d_sl)
    torch.cuda.synchronize()
    rng = random.Random(a.seed)
    masks = [sum(1 << i for i in rng.sample(range(n), k)) for _ in range(a.nobj)]
    metas = b"".join(d_sl[i * per + slen - 48:i * per + slen].cpu().numpy().tobytes() for i in range(a.nobj))
    d_out = torch.empty(a.nobj * a.size, dtype=torch.uint8, device=dev)

    def kernel_ms(fn):
        batch.kernel_timing(True)
        fn()
        ms, _ = batch.kernel_time_ms()
        batch.kernel_timing(False)
        return ms

    def timed(fn):
        fn()  # untimed round
        torch.cuda.synchronize()
        return stats([kernel_ms(fn) for _ in range(a.rounds)])

    lines = {}
    full_descs = batch.decode_descs([(o * per, slen, masks[o], o * a.size) for o in range(a.nobj)])
    d_out.zero_()
    lines["full"] = {"ms": timed(lambda: batch.decode_batch(s, d_sl, full_descs, metas, d_out)),
                     "stripes_decoded": a.nobj * ns, "stripes_copied": 0, "window": a.size}
    assert torch.equal(d_out, d_in)
    full_med = lines["full"]["ms"]["median"]
    lines["full"]["ms_per_decode_stripe"] = full_med / (a.nobj * ns)

    def ranged(name, win, avail):
        starts = [rng.randrange(0, a.size - win + 1) for _ in range(a.nobj)]
        descs = batch.decode_range_descs([(o * per, slen, avail[o], o * win, starts[o], win) for o in range(a.nobj)])
        d_out.zero_()
        ms = timed(lambda: batch.decode_range_batch(s, d_sl, descs, metas, d_out))
        for o in range(a.nobj):
            assert torch.equal(d_out[o * win:(o + 1) * win], d_in[o * a.size + starts[o]:o * a.size + starts[o] + win]), (name, o)
        rs = batch.range_launch_stats(s.coder)
        st = s.coder.decode_launch_stats()
        nd = rs["stripes_decoded"]
        lines[name] = {"ms": ms, "window": win, "stripes_touched": rs["stripes_touched"], "stripes_decoded": nd,
                       "stripes_copied": rs["stripes_copied"], "gather_jobs": rs["gather_jobs"],
                       "class_stripes": st["class_stripes"], "table_stripes": st["table_stripes"], "class_g": st["class_g"],
                       "ratio_to_full": ms["median"] / full_med, "full_over_ranged": full_med / ms["median"],
                       "stripe_fraction": rs["stripes_touched"] / (a.nobj * ns),
                       "ms_per_decode_stripe": ms["median"] / nd if nd else None}

    ranged("range_64KiB", 64 * KiB, masks)
    ranged("range_1MiB", MiB, masks)
    ranged("range_8MiB", 8 * MiB, masks)
    ranged("range_1MiB_all_present", MiB, [(1 << n) - 1] * a.nobj)

    # ---- per-call host form: one object ----
    host_sl = d_sl[:per].cpu().numpy()
    obj = d_in[:a.size].cpu().numpy()
    surv = sorted(i for i in range(n) if masks[0] >> i & 1)
    cfg = s._cfg()
    percall = {}
    for kind in ("pageable", "pinned"):
        alloc = batch.host_empty if kind == "pinned" else (lambda nbytes: np.empty(nbytes, np.uint8))
        keep = {}
        ptrs = (C.c_void_p * n)()
        for i in surv:
            keep[i] = alloc(slen)
            keep[i][:] = host_sl[i * slen:(i + 1) * slen]
            ptrs[i] = keep[i].ctypes.data
        out = alloc(a.size)
        got = C.c_size_t()

        def wall(fn):
            fn()
            v = []
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                fn()
                v.append((time.perf_counter() - t0) * 1e3)
            return stats(v)

        def full_call():
            assert lib.te_slicer_decode(s.coder.handle, C.byref(cfg), ptrs, slen, C.c_void_p(out.ctypes.data), out.size,
                                        C.byref(got)) == 0

        res = {"full": {"ms": wall(full_call)}}
        assert (out == obj).all()
        for name, win in (("range_64KiB", 64 * KiB), ("range_1MiB", MiB)):
            start = rng.randrange(0, a.size - win + 1)

            def range_call():
                assert lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, slen, start, win,
                                                  C.c_void_p(out.ctypes.data), out.size, C.byref(got)) == 0

            ms = wall(range_call)
            assert got.value == win and (out[:win] == obj[start:start + win]).all()
            rs = batch.range_launch_stats(s.coder)
            res[name] = {"ms": ms, "window": win, "stripes_touched": rs["stripes_touched"],
                         "stripes_decoded": rs["stripes_decoded"], "bytes_staged": rs["bytes_staged"],
                         "full_over_ranged": res["full"]["ms"]["median"] / ms["median"]}
        percall[kind] = res

    out = {"nobj": a.nobj, "size": a.size, "stripes_per_object": ns, "stripe_size": S, "slice_len": slen, "rounds": a.rounds,
           "device_kernel_ms": lines, "percall_wall_ms": percall}
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
