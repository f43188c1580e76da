"""Host read pipeline against the only host read that existed before it: verified
reads of objects whose slices lie in page-locked host memory, three legs over the same buffers:

  parent     a loop of te_slicer_decode_verified, one call per object (each call synchronises);
  batch      te_decode_verified_batch_host;
  stream     te_stream_reader_*: the batch's windows submitted back to back, then one wait;
  copy_only  the batch call's H2D and D2H copies with no hashing and no kernels
             (TEC_DEBUG_KNOBS=1 TEC_READ_COPY_ONLY=1): the ceiling of the pipeline on the box.

Shapes: `4m` = 1024 x 4 MiB objects with random 7-of-20 survivor sets, `64m` = 32 x 64 MiB objects
(the SDK's track size), worst-case survivors.  One shape per process; each GPU step under its own
time limit, chained:

  timeout -k 10 600 python scripts/read_pipeline_bench.py --shape 4m --out profiles/read_pipeline_bench.json && \\
  timeout -k 10 600 python scripts/read_pipeline_bench.py --shape 64m --out profiles/read_pipeline_bench.json

The legs run alternately, round by round, after one untimed round of each; times are a host clock
around calls that return only when the bytes are in host memory.  The acceptance rule is against
the parent: the pipelined read may take no longer than the parent loop beyond the parent's own
run-to-run spread (`batch_within_parent_spread`).  --out merges the shape into the JSON file.
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

os.environ["TEC_DEBUG_KNOBS"] = "1"  # the copy-only leg's switch is read per call
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import tape_amd as T  # noqa: E402
from tape_amd import _lib, batch, merkle  # noqa: E402
from tape_amd._lib import lib  # noqa: E402

SHAPES = {"4m": (1024, 4 << 20, "random"), "64m": (32, 64 << 20, "worst")}


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="4m")
    ap.add_argument("--nobj", type=int, default=0, help="override the shape's object count")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=0, help="window_bytes (0 = 128 MiB)")
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("read_pipeline_bench needs a gfx950 device: nothing is measured without one")
    nobj, size, sets_kind = SHAPES[a.shape]
    nobj = a.nobj or nobj
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n, k = s.n(), s.k()
    slen = int(s.geometry(size).slice_len)
    per = n * slen
    # objects encoded and committed on the device, then every slice copied to page-locked host memory
    torch.manual_seed(a.seed)
    d_in = torch.randint(0, 256, (nobj * size,), dtype=torch.uint8, device=dev)
    d_sl = torch.empty(nobj * per, dtype=torch.uint8, device=dev)
    batch.encode_batch(s, d_in, [(i * size, size, i * per, i) for i in range(nobj)], d_sl)
    d_leaf = torch.empty(nobj * n * 32, dtype=torch.uint8, device=dev)
    merkle.commit_batch(d_sl, per, slen, n, nobj, d_leaf)
    torch.cuda.synchronize()
    h_sl = batch.host_empty(nobj * per)
    h_out = batch.host_empty(nobj * size)
    torch.from_numpy(h_sl).copy_(d_sl)
    want = d_in.cpu().numpy()
    leaves = d_leaf.cpu().numpy().tobytes()
    del d_in, d_sl, d_leaf
    torch.cuda.empty_cache()
    rng = random.Random(a.seed)
    sets = [sorted(rng.sample(range(n), k)) if sets_kind == "random" else list(range(n - k, n)) for _ in range(nobj)]
    masks = [sum(1 << i for i in p) for p in sets]
    metas = b"".join(h_sl[o * per + slen - 48:o * per + slen].tobytes() for o in range(nobj))
    descs = batch.decode_descs([(o * per, slen, masks[o], o * size) for o in range(nobj)])
    cuts = batch.decode_window_plan(s.coder, descs, metas, a.window)
    cfg = s._cfg()
    mb = (C.c_uint8 * len(metas)).from_buffer_copy(metas)
    lb = (C.c_uint8 * len(leaves)).from_buffer_copy(leaves)
    rej = (C.c_uint32 * nobj)()
    st = (C.c_int * nobj)()
    base_sl, base_out, base_lb = h_sl.ctypes.data, h_out.ctypes.data, C.addressof(lb)
    ptrs = []
    for o in range(nobj):
        p = (C.c_void_p * n)()
        for i in sets[o]:
            p[i] = base_sl + o * per + i * slen
        ptrs.append(p)

    def run_parent():
        got, r1 = C.c_size_t(), C.c_uint32()
        for o in range(nobj):
            r = lib.te_slicer_decode_verified(s.coder.handle, C.byref(cfg), ptrs[o], slen, C.c_void_p(base_lb + o * n * 32),
                                              C.c_void_p(base_out + o * size), size, C.byref(got), C.byref(r1))
            assert r == 0 and got.value == size and r1.value == 0, (o, r)

    def run_batch():
        r = lib.te_decode_verified_batch_host(s.coder.handle, C.byref(cfg), C.c_void_p(base_sl), descs, mb, lb, nobj,
                                              C.c_void_p(base_out), rej, st, a.window)
        assert r == 0 and not any(st) and not any(rej), r

    reader = batch.StreamReader([s])
    win_args = [((_lib.te_decode_object * (q - p))(*descs[p:q]), metas[p * 48:q * 48], leaves[p * n * 32:q * n * 32])
                for p, q in zip(cuts, cuts[1:])]

    def run_stream():
        t = 0
        for d, m, lv in win_args:
            t = reader.submit(h_sl, d, m, h_out, leaves=lv)
        for status, rejected in reader.wait(t).values():
            assert not any(status) and not any(rejected)

    def run_copy_only():
        os.environ["TEC_READ_COPY_ONLY"] = "1"
        try:
            r = lib.te_decode_verified_batch_host(s.coder.handle, C.byref(cfg), C.c_void_p(base_sl), descs, mb, lb, nobj,
                                                  C.c_void_p(base_out), rej, st, a.window)
        finally:
            os.environ["TEC_READ_COPY_ONLY"] = "0"
        assert r == 0, r

    legs = {"parent": run_parent, "batch": run_batch, "stream": run_stream, "copy_only": run_copy_only}
    times = {name: [] for name in legs}
    read_stats = {}
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
            if name in ("batch", "copy_only"):
                read_stats[name] = batch.read_launch_stats(s.coder)
            if r:  # round 0 warms every leg up
                times[name].append(ms)
    reader.close()
    out = {"nobj": nobj, "size": size, "slice_len": slen, "survivors": sets_kind, "windows": len(cuts) - 1,
           "window_bytes": a.window or 128 << 20, "rounds": a.rounds, "hash_threads": batch.host_hash_threads(),
           "read_stats": read_stats}
    for name in legs:
        out[name + "_ms"] = stats(times[name])
    gib = nobj * size / 2**30
    for name in legs:
        out[name + "_GiBps"] = gib / (out[name + "_ms"]["median"] / 1e3)
    p = out["parent_ms"]
    for name in ("batch", "stream"):
        out[name + "_within_parent_spread"] = out[name + "_ms"]["median"] <= p["median"] + p["spread"]
        out[name + "_over_parent"] = out[name + "_ms"]["median"] / p["median"]
        out[name + "_over_copy_only"] = out[name + "_ms"]["median"] / out["copy_only_ms"]["median"]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[a.shape] = out
        open(a.out, "w").write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
