"""The chunk path of ranged reads against the full decode of the stripe: a 64 KiB window
inside one data chunk whose slice is lost, the gateway's small Range read under a degraded track.

usage: python scripts/range_chunk_bench.py [--nobj 32] [--size 67108864] [--rounds 15] [--label new]
                                           [--modes off,on] [--out profiles/range_chunk_bench.json]

The shapes of scripts/range_bench.py: nobj objects resident in HBM, Clay(20,7,16) rotated, one
64 KiB window per object at a seeded random offset inside one data chunk, that chunk's slice absent
and the other 19 present (te_decode_range_batch_device, HIP event pairs around the launches:
te_kernel_timing); and the per-call host form, one object's slices in page-locked memory
(te_slicer_decode_range into a page-locked buffer: kernel time and wall time).  Each shape runs with
the knob off and on in alternating rounds after an untimed round of each; medians with min, max and
every run.  A library without the knob (the parent commit's build, TAPE_EC_LIB) runs the knob-off
rounds only: the baseline the knob-off line must sit inside.  Compare it with a --modes off run
of this build: rounds that alternate with the other path's kernels measured 3-5 % longer than the
same call timed alone.  Every line's bytes are checked against the objects.  Appends one JSON line
per run to --out.  Needs a gfx950 device.
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
    ap.add_argument("--window", type=int, default=64 * KiB)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--seed", type=int, default=33)
    ap.add_argument("--label", default="new")
    ap.add_argument("--modes", default="off,on", help="knob settings to time, alternating (off alone: as the parent runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("range_chunk_bench needs a gfx950 device: nothing is measured without one")
    have_knob = hasattr(batch, "set_range_chunk_path")
    modes = tuple(m for m in a.modes.split(",") if m == "off" or (m == "on" and have_knob))
    assert modes, "nothing to time"
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n = s.n()
    g = s.geometry(a.size)
    slen, per, ns, S, cs = int(g.slice_len), n * int(g.slice_len), int(g.num_stripes), int(g.stripe_size), int(g.chunk_size)
    assert a.window <= cs, "the window must fit one data chunk"
    torch.manual_seed(a.seed)
    d_in = torch.randint(0, 256, (a.nobj * a.size,), dtype=torch.uint8, device=dev)
    d_sl = torch.empty(a.nobj * per, dtype=torch.uint8, device=dev)
    batch.encode_batch(s, d_in, [(i * a.size, a.size, i * per, i) for i in range(a.nobj)], d_sl)
    torch.cuda.synchronize()
    metas = b"".join(d_sl[i * per + slen - 48:i * per + slen].cpu().numpy().tobytes() for i in range(a.nobj))
    rng = random.Random(a.seed)

    def window():
        """(start, absent slice): a window inside one data chunk of a full stripe, that chunk's slice."""
        st, x = rng.randrange(ns - 1), rng.randrange(6)  # chunks 0..5 lie wholly inside the stripe's S bytes
        start = st * S + x * cs + rng.randrange(cs - a.window + 1)
        return start, (x + (st * 7) % n) % n

    def knob(mode):
        if have_knob:
            batch.set_range_chunk_path(s.coder, mode == "on")

    def kernel_ms(fn):
        batch.kernel_timing(True)
        fn()
        ms, _ = batch.kernel_time_ms()
        batch.kernel_timing(False)
        return ms

    def path():
        rs, st = batch.range_launch_stats(s.coder), s.coder.decode_launch_stats()
        d = {"stripes_touched": rs["stripes_touched"], "stripes_decoded": rs["stripes_decoded"],
             "gather_jobs": rs["gather_jobs"], "bytes_staged": rs["bytes_staged"], "class_launches": st["class_launches"],
             "class_stripes": st["class_stripes"], "table_stripes": st["table_stripes"], "class_g": st["class_g"]}
        if have_knob:
            d.update(batch.range_chunk_launch_stats(s.coder))
        return d

    # ---- device form: one window in each of nobj resident objects ----
    wins = [window() for _ in range(a.nobj)]
    full = (1 << n) - 1
    descs = batch.decode_range_descs([(o * per, slen, full & ~(1 << wins[o][1]), o * a.window, wins[o][0], a.window)
                                      for o in range(a.nobj)])
    d_out = torch.empty(a.nobj * a.window, dtype=torch.uint8, device=dev)
    device = {m: {"runs": []} for m in modes}
    for m in modes:  # untimed round, checked
        knob(m)
        d_out.zero_()
        batch.decode_range_batch(s, d_sl, descs, metas, d_out)
        torch.cuda.synchronize()
        for o in range(a.nobj):
            assert torch.equal(d_out[o * a.window:(o + 1) * a.window],
                               d_in[o * a.size + wins[o][0]:o * a.size + wins[o][0] + a.window]), (m, o)
        device[m].update(path())
    for _ in range(a.rounds):
        for m in modes:
            knob(m)
            device[m]["runs"].append(kernel_ms(lambda: batch.decode_range_batch(s, d_sl, descs, metas, d_out)))
    for m in modes:
        device[m]["ms"] = stats(device[m].pop("runs"))

    # ---- per-call host form: one object, page-locked slices and output ----
    host_sl = d_sl[:per].cpu().numpy()
    obj = d_in[:a.size].cpu().numpy()
    start, gone = window()
    keep = {}
    ptrs = (C.c_void_p * n)()
    for i in range(n):
        if i == gone:
            continue
        keep[i] = batch.host_empty(slen)
        keep[i][:] = host_sl[i * slen:(i + 1) * slen]
        ptrs[i] = keep[i].ctypes.data
    out = batch.host_empty(a.window)
    got = C.c_size_t()
    cfg = s._cfg()

    def call():
        assert lib.te_slicer_decode_range(s.coder.handle, C.byref(cfg), ptrs, slen, start, a.window,
                                          C.c_void_p(out.ctypes.data), out.size, C.byref(got)) == 0

    percall = {m: {"kernel": [], "wall": []} for m in modes}
    for m in modes:
        knob(m)
        out[:] = 0
        call()
        assert got.value == a.window and (out == obj[start:start + a.window]).all(), m
        percall[m].update(path())
    for _ in range(a.rounds):
        for m in modes:
            knob(m)
            percall[m]["kernel"].append(kernel_ms(call))
            t0 = time.perf_counter()
            call()
            percall[m]["wall"].append((time.perf_counter() - t0) * 1e3)
    for m in modes:
        percall[m]["kernel_ms"] = stats(percall[m].pop("kernel"))
        percall[m]["wall_ms"] = stats(percall[m].pop("wall"))
    knob("off")

    line = {"label": a.label, "nobj": a.nobj, "size": a.size, "window": a.window, "rounds": a.rounds, "chunk_size": cs,
            "stripes_per_object": ns, "device_kernel_ms": device, "percall": percall}
    if len(modes) == 2:
        line["device_on_over_off"] = device["on"]["ms"]["median"] / device["off"]["ms"]["median"]
        line["percall_kernel_on_over_off"] = percall["on"]["kernel_ms"]["median"] / percall["off"]["kernel_ms"]["median"]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a").write(txt + "\n")


if __name__ == "__main__":
    main()
