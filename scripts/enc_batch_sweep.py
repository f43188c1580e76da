#!/usr/bin/env python3
"""enc_batch_sweep.py -- kernel time of the batched device encode against the batch size.

One process, one set of buffers, the same calls as bench.py's headline (tape_amd.batch.encode_batch
of N x 4 MiB objects, Clay(20,7,16), rotated 1 MB stripes).  The object counts are interleaved
round-robin (every round runs every size once), so a change of box state hits every size; per size
and round the kernel milliseconds come from te_kernel_timing.  Prints one JSON line per round, then
one with the least-squares fit  ms = a + b * objects  over the per-size medians and its residuals:
`a` is the fixed cost of a launch (drain, fill), `a / ms(1024)` the most a scheduling change can
gain on the headline.

    python scripts/enc_batch_sweep.py [--rounds 5] [--reps 3] [--out profiles/enc_batch_sweep_X.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MiB = 1024 * 1024
SIZES = (256, 512, 1024, 1536, 2048, 4096)


def fit_line(xs, ys):
    """Least squares y = a + b x; returns a, b and the residuals."""
    n = len(xs)
    mx, my = sum(xs) / n, sum(ys) / n
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    a = my - b * mx
    return a, b, [y - (a + b * x) for x, y in zip(xs, ys)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls per size per round (their mean is the round's figure)")
    ap.add_argument("--sizes", type=str, default=",".join(map(str, SIZES)))
    ap.add_argument("--out", type=str, default=None, help="also write the lines to this file")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

    import torch
    import tape_amd as T
    from tape_amd import batch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    T.lib.te_set_device(0)
    L, nmax = 4 * MiB, max(sizes)
    slicer = T.Slicer.clay_default()
    g = slicer.geometry(L)
    per = 20 * g.slice_len
    d_in = torch.empty(nmax * L, dtype=torch.uint8, device=dev)
    for o in range(0, nmax * L, 1 << 30):  # any bytes do: the kernel's time does not depend on them
        e = min(nmax * L, o + (1 << 30))
        d_in[o:e] = torch.randint(0, 256, (e - o,), dtype=torch.uint8, device=dev)
    d_out = torch.empty(nmax * per, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()
    descs = {n: batch.encode_descs([(i * L, L, i * per, 0) for i in range(n)]) for n in sizes}

    lines = []

    def emit(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    for n in sizes:  # warm-up: every size once (descriptor upload, workspace growth)
        batch.encode_batch(slicer, d_in, descs[n], d_out, stream)
    torch.cuda.synchronize()
    per_size = {n: [] for n in sizes}
    for r in range(args.rounds):
        row = {}
        for n in sizes:
            batch.kernel_time_ms()
            batch.kernel_timing(True)
            for _ in range(args.reps):
                batch.encode_batch(slicer, d_in, descs[n], d_out, stream)
            torch.cuda.synchronize()
            batch.kernel_timing(False)
            ms, calls = batch.kernel_time_ms()
            row[str(n)] = round(ms / max(1, calls), 4)
            per_size[n].append(ms / max(1, calls))
        emit({"round": r, "reps": args.reps, "kernel_ms": row})
    med = {n: statistics.median(v) for n, v in per_size.items()}
    a, b, res = fit_line(sizes, [med[n] for n in sizes])
    p = torch.cuda.get_device_properties(dev)
    emit({"fit": "ms = a + b * objects (least squares over the per-size medians)",
          "a_ms": round(a, 4), "b_ms_per_object": round(b, 7),
          "median_ms": {str(n): round(med[n], 4) for n in sizes},
          "spread_ms": {str(n): round(max(per_size[n]) - min(per_size[n]), 4) for n in sizes},
          "residual_ms": {str(n): round(x, 4) for n, x in zip(sizes, res)},
          "a_over_ms_1024": round(a / med[1024], 4) if 1024 in med else None,
          "lib": os.path.basename(T._lib.LIB_PATH) if hasattr(T, "_lib") else None,
          "gpu": {"name": p.name, "cus": p.multi_processor_count,
                  "pci": f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}"}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
