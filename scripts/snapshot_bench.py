"""Snapshot codec against the only route a caller had before it, at OuterCoder(17, 50)
for full segments (68 MiB of compressed log each):

  device  te_snapshot_encode_device / te_snapshot_decode_device on device buffers: kernel time
          (te_kernel_timing) and a host clock around call + stream wait;
  host    te_snapshot_encode_host / te_snapshot_decode_host, page-locked host buffers;
  parts   INTEGRATION §5d's recipe: a te_outer_encode per segment, a te_slicer_encode per symbol and
          te_hash_leaves on the host (decode: a te_slicer_decode per track, a te_outer_decode per
          segment).  Every entry point of this leg exists unchanged in the parent commit.

One segment count per process, each GPU step under its own time limit, chained:

  timeout -k 10 500 python scripts/snapshot_bench.py --segments 1 --out profiles/snapshot_bench.json && \\
  timeout -k 10 900 python scripts/snapshot_bench.py --segments 16 --rounds 1 --out profiles/snapshot_bench.json

The decode reads every track's first 7 slices.  Needs a gfx950 device.
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
from tape_amd import _lib, batch, snapshot  # noqa: E402
from tape_amd._lib import lib  # noqa: E402

N, NI = 50, 20


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def ktime():
    ms, cnt = C.c_double(), C.c_uint32()
    assert lib.te_kernel_time_ms(C.byref(ms), C.byref(cnt)) == 0
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-parts", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("snapshot_bench needs a gfx950 device: nothing is measured without one")
    s = T.Slicer.clay_default()
    c = s.coder
    k = snapshot.snapshot_outer_k(N)
    length = a.segments * snapshot.snapshot_max_segment_bytes(N)
    P = snapshot.plan(length, N, c)
    assert P["segments"] == a.segments
    total, nch = P["total_slice_bytes"], P["chunks"]
    sl = P["segs"][0]["slice_len"]
    sym = P["segs"][0]["symbol_bytes"]
    torch.manual_seed(5)
    d_src = torch.randint(0, 256, (length + 8,), dtype=torch.uint8, device="cuda")
    d_sl = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_leaf = torch.empty(nch * NI * 32, dtype=torch.uint8, device="cuda")
    d_root = torch.empty(nch * 32, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(snapshot.work_bytes(length, N, c), dtype=torch.uint8, device="cuda")
    h_src = batch.host_empty(length)
    torch.from_numpy(h_src).copy_(d_src[:length])
    h_sl = batch.host_empty(total)
    h_leaf = np.zeros(nch * NI * 32, np.uint8)
    h_root = np.zeros(nch * 32, np.uint8)
    res = {"segments": a.segments, "compressed_bytes": length, "slice_bytes": total, "chunks": nch, "rounds": a.rounds}
    enc = {"device_kernel_ms": [], "device_wall_ms": [], "host_wall_ms": [], "parts_wall_ms": []}
    dec = {"device_kernel_ms": [], "device_wall_ms": [], "host_wall_ms": [], "parts_wall_ms": []}

    # ---- encode ----
    def enc_device():
        snapshot.encode_device(d_src, length, N, d_sl, d_leaf, d_root, d_work, c)
        torch.cuda.synchronize()

    def enc_host():
        r = lib.te_snapshot_encode_host(c.handle, C.c_void_p(h_src.ctypes.data), length, N, C.c_void_p(h_sl.ctypes.data),
                                        total, C.c_void_p(h_leaf.ctypes.data), C.c_void_p(h_root.ctypes.data))
        assert r == 0, r

    cfg = s._cfg()
    p_out = batch.host_empty(N * sym)
    p_pay = batch.host_empty(8 + sym)
    p_sl = batch.host_empty(NI * sl)
    p_leaf = np.zeros(NI * 32, np.uint8)

    def enc_parts():
        mx = snapshot.snapshot_max_segment_bytes(N)
        cb = C.c_size_t()
        packed = np.empty(4 + mx, np.uint8)
        for g in range(a.segments):
            packed[:4] = np.frombuffer(mx.to_bytes(4, "little"), np.uint8)
            packed[4:] = h_src[g * mx:(g + 1) * mx]
            r = lib.te_outer_encode(k, N, C.c_void_p(packed.ctypes.data), packed.size, C.c_void_p(p_out.ctypes.data),
                                    p_out.size, C.byref(cb))
            assert r == 0 and cb.value == sym, r
            for grp in range(N):
                p_pay[:8] = np.frombuffer(g.to_bytes(8, "little"), np.uint8)
                p_pay[8:] = p_out[grp * sym:(grp + 1) * sym]
                r = lib.te_slicer_encode(c.handle, C.byref(cfg), C.c_void_p(p_pay.ctypes.data), p_pay.size,
                                         C.c_void_p(p_sl.ctypes.data), p_sl.size)
                assert r == 0, r
                assert lib.te_hash_leaves(C.c_void_p(p_sl.ctypes.data), sl, NI, 0, C.c_void_p(p_leaf.ctypes.data)) == 0
                t = g * N + grp
                if t in (0, nch - 1):  # spot check against the pipeline's output
                    assert np.array_equal(p_sl, h_sl[t * NI * sl:(t + 1) * NI * sl]), t
                    assert np.array_equal(p_leaf, h_leaf[t * NI * 32:(t + 1) * NI * 32]), t

    lib.te_kernel_timing(1)
    for r in range(a.rounds + 1):
        ktime()
        t0 = time.perf_counter()
        enc_device()
        w = (time.perf_counter() - t0) * 1e3
        kms = ktime()
        if r:
            enc["device_wall_ms"].append(w)
            enc["device_kernel_ms"].append(kms)
    lib.te_kernel_timing(0)
    for r in range(a.rounds + 1):
        t0 = time.perf_counter()
        enc_host()
        if r:
            enc["host_wall_ms"].append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(h_sl[:NI * sl], d_sl[:NI * sl].cpu().numpy())
    res["encode_stats"] = snapshot.launch_stats(c)
    if not a.skip_parts:
        for r in range(2 if a.rounds > 1 else 1):
            t0 = time.perf_counter()
            enc_parts()
            enc["parts_wall_ms"].append((time.perf_counter() - t0) * 1e3)

    # ---- decode: every track, its first 7 slices ----
    descs = [(t % N, P["segs"][t // N]["slices_off"] + (t % N) * NI * sl, sl, 0x7F) for t in range(nch)]
    metas = b"".join(h_sl[d[1] + sl - 48:d[1] + sl].tobytes() for d in descs)
    d_out = torch.empty(length + 64, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(2, dtype=torch.int64, device="cuda")
    d_dwork = torch.empty(snapshot.decode_work_bytes(descs, metas, N, c), dtype=torch.uint8, device="cuda")
    h_out = batch.host_empty(length)
    arr = snapshot.track_descs(descs)
    st, rej, seg, got = (C.c_int * nch)(), (C.c_uint32 * nch)(), (C.c_uint64 * nch)(), C.c_uint64()

    def dec_device():
        rep = snapshot.decode_device(d_sl, descs, metas, N, d_out, length, d_dwork, d_res, None, c)
        torch.cuda.synchronize()
        assert rep["code"] == 0, rep["code"]

    def dec_host():
        r = lib.te_snapshot_decode_host(c.handle, N, C.c_void_p(h_sl.ctypes.data), arr, metas, None, nch,
                                        C.c_void_p(h_out.ctypes.data), length, C.byref(got), st, rej, seg)
        assert r == 0 and got.value == length, r

    def dec_parts():
        pay = batch.host_empty(8 + sym)
        syms = batch.host_empty(N * sym)
        outp = batch.host_empty(k * sym)
        n_out = C.c_size_t()
        for g in range(a.segments):
            for grp in range(N):
                base = h_sl.ctypes.data + descs[g * N + grp][1]
                ptrs = (C.c_void_p * NI)(*[base + i * sl if i < 7 else None for i in range(NI)])
                r = lib.te_slicer_decode(c.handle, C.byref(cfg), ptrs, sl, C.c_void_p(pay.ctypes.data), pay.size, C.byref(n_out))
                assert r == 0 and n_out.value == 8 + sym, r
                syms[grp * sym:(grp + 1) * sym] = pay[8:]
            ch = (C.c_void_p * N)(*[syms.ctypes.data + i * sym for i in range(N)])
            assert lib.te_outer_decode(k, N, ch, sym, C.c_void_p(outp.ctypes.data), outp.size) == 0
            mx = int.from_bytes(outp[:4].tobytes(), "little")
            h_out[g * mx:(g + 1) * mx] = outp[4:4 + mx]

    lib.te_kernel_timing(1)
    for r in range(a.rounds + 1):
        ktime()
        t0 = time.perf_counter()
        dec_device()
        w = (time.perf_counter() - t0) * 1e3
        kms = ktime()
        if r:
            dec["device_wall_ms"].append(w)
            dec["device_kernel_ms"].append(kms)
    lib.te_kernel_timing(0)
    assert d_res.cpu().tolist() == [0, length] and torch.equal(d_out[:length], d_src[:length])
    for r in range(a.rounds + 1):
        h_out[:] = 0
        t0 = time.perf_counter()
        dec_host()
        if r:
            dec["host_wall_ms"].append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(h_out, h_src)
    res["decode_stats"] = snapshot.launch_stats(c)
    if not a.skip_parts:
        for r in range(2 if a.rounds > 1 else 1):
            h_out[:] = 0
            t0 = time.perf_counter()
            dec_parts()
            dec["parts_wall_ms"].append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(h_out, h_src)

    gib = length / 2**30
    for name, legs in (("encode", enc), ("decode", dec)):
        res[name] = {leg: med(v) for leg, v in legs.items() if v}
        res[name + "_GiBps_of_compressed"] = {leg: gib / (m["median"] / 1e3) for leg, m in res[name].items()}
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = json.load(open(a.out)) if os.path.exists(a.out) else {}
        allres[f"segments_{a.segments}"] = res
        open(a.out, "w").write(json.dumps(allres, indent=1) + "\n")


if __name__ == "__main__":
    main()
