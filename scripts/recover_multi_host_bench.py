"""The node's multi-spool rebuild from host memory: L lost slices of each object by
one te_recover_multi_batch_host call, against the route that existed before it -- L calls of
te_recover_batch_host, each uploading the same k peer slices -- and against the copies alone.

  --nobj x --size objects in pinned host memory, random 7-of-20 survivors per object, L lost slices
  drawn from the other 13; per L, verified (leaves given) and unverified:
    parent     L te_recover_batch_host calls.  With --parent-lib (a libtapeec.so built from the parent
               commit, loaded beside this tree's) they run on that build; without it on this tree's,
               whose single-slice entry point is the parent's code;
    multi      one te_recover_multi_batch_host call;
    copy_only  the multi call with TEC_DEBUG_KNOBS=1 TEC_REBUILD_COPY_ONLY=1: its windows' copies
               with no hashing and no kernels, the ceiling of the pipeline (7 + L slice lengths).
  The legs alternate round by round in one process; round 0 of every (L, form) is kept apart as the
  first call (the multi leg's includes compiling its stripes' programs, which runs on the host
  pool); the others give medians with min and max.  Every parent and multi leg's bytes are compared
  with the encoded slices, every verified leg's masks with the lost masks.

  TEC_DEBUG_KNOBS=1 timeout -k 10 1100 python scripts/recover_multi_host_bench.py \
      --out profiles/recover_multi_host_bench.json

Needs a gfx950 device and nobj * 20 slice lengths of page-locked memory (1024 x 4 MiB: 12.3 GB).
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


def parent_entry(path):
    """te_recover_batch_host of another build, on a handle of that build."""
    L = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    L.te_clay_new.restype = C.c_int
    L.te_clay_new.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.te_recover_batch_host.restype = C.c_int
    L.te_recover_batch_host.argtypes = [vp, C.POINTER(_lib.te_slicer_cfg), vp, C.POINTER(_lib.te_recover_object), vp, vp, sz,
                                        vp, vp, vp, vp, sz]
    h = vp()
    assert L.te_clay_new(20, 7, 16, C.byref(h)) == 0
    return L, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nobj", type=int, default=1024)
    ap.add_argument("--size", type=int, default=4 << 20)
    ap.add_argument("--lost", default="1,2,4,13")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--unchanged", default="", help="a JSON file of bench.py runs to record beside the legs")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("recover_multi_host_bench needs a gfx950 device: nothing is measured without one")
    knobs = os.environ.get("TEC_DEBUG_KNOBS") == "1"
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n, k = s.n(), s.k()
    nobj, size = a.nobj, a.size
    slen = int(s.geometry(size).slice_len)
    per = n * slen
    # the slices: encoded on the device in groups, brought to one pinned buffer
    h_sl = batch.host_empty(nobj * per)
    torch.manual_seed(a.seed)
    grp = 64
    for g0 in range(0, nobj, grp):
        g = min(grp, nobj - g0)
        d_in = torch.randint(0, 256, (g * size,), dtype=torch.uint8, device=dev)
        d_sl = torch.empty(g * per, dtype=torch.uint8, device=dev)
        batch.encode_batch(s, d_in, [(i * size, size, i * per, g0 + i) for i in range(g)], d_sl)
        torch.cuda.synchronize()
        h_sl[g0 * per:(g0 + g) * per] = d_sl.cpu().numpy()
    del d_in, d_sl
    torch.cuda.empty_cache()
    sl3 = h_sl.reshape(nobj, n, slen)
    metas = b"".join(sl3[o, 0, slen - 48:].tobytes() for o in range(nobj))
    from tape_amd import merkle
    leaves = b"".join(b"".join(merkle.hash_leaf(sl3[o, j].tobytes()) for j in range(n)) for o in range(nobj))
    rng = random.Random(a.seed)
    surv = [sorted(rng.sample(range(n), k)) for _ in range(nobj)]
    masks = [sum(1 << j for j in p) for p in surv]
    order = [rng.sample([j for j in range(n) if j not in p], n - k) for p in surv]
    cfg = s._cfg()
    mb = batch._meta_bytes(metas)
    lb = (C.c_uint8 * len(leaves)).from_buffer_copy(leaves)
    plib, ph = parent_entry(a.parent_lib) if a.parent_lib else (lib, s.coder.handle)
    rej, ok, st = (C.c_uint32 * nobj)(), (C.c_uint32 * nobj)(), (C.c_int * nobj)()
    res = {"nobj": nobj, "size": size, "slice_len": slen, "rounds": a.rounds, "parent_lib": bool(a.parent_lib),
           "copy_only_leg": knobs, "runs": {}}
    for L in [int(x) for x in a.lost.split(",")]:
        lost = [sorted(o[:L]) for o in order]
        lm = [sum(1 << j for j in x) for x in lost]
        h_out = batch.host_empty(nobj * L * slen)
        multi = batch.recover_multi_descs([(o * per, slen, masks[o], lm[o], o * L * slen) for o in range(nobj)])
        single = [batch.recover_descs([(o * per, slen, masks[o], lost[o][j], (o * L + j) * slen) for o in range(nobj)])
                  for j in range(L)]
        for verified in (True, False):
            lv = lb if verified else None
            args = (rej, ok, st) if verified else (None, None, None)

            def run_multi():
                r = lib.te_recover_multi_batch_host(s.coder.handle, C.byref(cfg), C.c_void_p(h_sl.ctypes.data), multi, mb, lv,
                                                    nobj, C.c_void_p(h_out.ctypes.data), *args, 0)
                assert r == 0, r
                assert not verified or list(ok) == lm

            def run_parent():
                for j in range(L):
                    r = plib.te_recover_batch_host(ph, C.byref(cfg), C.c_void_p(h_sl.ctypes.data), single[j], mb, lv, nobj,
                                                   C.c_void_p(h_out.ctypes.data), *args, 0)
                    assert r == 0, r
                    assert not verified or all(ok)

            def run_copy():
                os.environ["TEC_REBUILD_COPY_ONLY"] = "1"
                try:
                    run_multi_unchecked()
                finally:
                    os.environ["TEC_REBUILD_COPY_ONLY"] = "0"

            def run_multi_unchecked():
                r = lib.te_recover_multi_batch_host(s.coder.handle, C.byref(cfg), C.c_void_p(h_sl.ctypes.data), multi, mb, lv,
                                                    nobj, C.c_void_p(h_out.ctypes.data), *args, 0)
                assert r == 0, r

            legs = {"parent": run_parent, "multi": run_multi}
            if knobs:
                legs["copy_only"] = run_copy
            wall = {x: [] for x in legs}
            first = {}
            for r in range(a.rounds + 1):
                for name, fn in legs.items():
                    h_out[:] = 0
                    t0 = time.perf_counter()
                    fn()
                    ms = (time.perf_counter() - t0) * 1e3
                    if name != "copy_only":
                        for o in range(0, nobj, max(1, nobj // 64)):  # every leg's bytes, a sample of objects in full
                            for j, i in enumerate(lost[o]):
                                assert np.array_equal(h_out[(o * L + j) * slen:(o * L + j + 1) * slen], sl3[o, i]), (name, L, o, i)
                    (wall[name].append(ms) if r else first.__setitem__(name, ms))
                    if name == "multi":  # the multi leg's own counters, not the copy-only leg's after it
                        rb, rm = batch.rebuild_launch_stats(s.coder), batch.recover_multi_launch_stats(s.coder)
                print(f"L={L} {'verified' if verified else 'unverified'} round {r}: " +
                      ", ".join(f"{x} {(wall[x][-1] if r else first[x]):.1f} ms" for x in legs), flush=True)
            e = {"first_call_ms": first, "rebuild_stats": rb, "multi_stats": rm}
            for name in legs:
                e[name + "_ms"] = stats(wall[name])
            p, m = e["parent_ms"], e["multi_ms"]
            e["multi_over_parent"] = m["median"] / p["median"]
            e["multi_beats_parent"] = m["median"] < p["median"] - p["spread"]
            if knobs:
                e["multi_over_copy_only"] = m["median"] / e["copy_only_ms"]["median"]
            e["multi_first_over_steady"] = first["multi"] / m["median"]
            res["runs"][f"L{L}_{'verified' if verified else 'unverified'}"] = e
        del h_out
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if a.unchanged:  # bench.py result lines of the paths this change leaves alone, parent against new
        res["unchanged_paths"] = json.load(open(a.unchanged))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
