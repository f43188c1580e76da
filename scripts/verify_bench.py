"""Cost of the verified reads on the device: the ragged leaf-verify kernel against
commit.hip's leaf_kernel at equal stream count and slice length, and a verified batch decode
against the plain one, for objects read from random k-of-n survivor sets.

usage: python scripts/verify_bench.py [--nobj 1024] [--size 4194304] [--rounds 7] [--out FILE.json]

Kernel times are HIP event pairs around the launches (te_kernel_timing); call times are a host
clock around the call and a device synchronise.  The two kernels are timed alternately, round by
round, after one untimed round of each; the spread of the leaf_kernel rounds is the margin the
comparison allows and is printed beside it.  Needs a gfx950 device.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import tape_amd as T  # noqa: E402
from tape_amd import batch, merkle  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nobj", type=int, default=1024)
    ap.add_argument("--size", type=int, default=4 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if T.device_count() < 1:
        raise SystemExit("verify_bench needs a gfx950 device: nothing is measured without one")
    dev = torch.device("cuda:0")
    s = T.Slicer.clay_default()
    n, k = s.n(), s.k()
    g = s.geometry(a.size)
    slen, per = g.slice_len, n * g.slice_len
    torch.manual_seed(a.seed)
    d_in = torch.randint(0, 256, (a.nobj * a.size,), dtype=torch.uint8, device=dev)
    d_sl = torch.empty(a.nobj * per, dtype=torch.uint8, device=dev)
    batch.encode_batch(s, d_in, [(i * a.size, a.size, i * per, i) for i in range(a.nobj)], d_sl)
    # expected hashes from the write side's kernel, which the verify kernel must agree with
    d_leaf = torch.empty(a.nobj * n * 32, dtype=torch.uint8, device=dev)
    merkle.commit_batch(d_sl, per, slen, n, a.nobj, d_leaf)
    torch.cuda.synchronize()
    rng = random.Random(a.seed)
    sets = [sorted(rng.sample(range(n), k)) for _ in range(a.nobj)]
    masks = [sum(1 << i for i in p) for p in sets]
    items = merkle.verify_items([(o * per + i * slen, slen, o * n + i, o, 1 << i) for o in range(a.nobj) for i in sets[o]])
    nstreams = len(items)
    d_dig = torch.empty(nstreams * 32, dtype=torch.uint8, device=dev)
    d_ok = torch.empty(nstreams, dtype=torch.int32, device=dev)
    d_mask = torch.zeros(a.nobj, dtype=torch.int32, device=dev)
    d_leaf_k = torch.empty(a.nobj * k * 32, dtype=torch.uint8, device=dev)

    def kernel_ms(fn):
        batch.kernel_timing(True)
        fn()
        ms, _ = batch.kernel_time_ms()
        batch.kernel_timing(False)
        return ms

    def run_verify():
        d_mask.zero_()
        merkle.verify_leaves_device(s.coder, d_sl, items, d_leaf, d_dig, d_ok, d_mask)

    def run_leaf():  # leaf_kernel alone (no tree): k slices of every object, the same stream count
        merkle.commit_batch(d_sl, per, slen, k, a.nobj, d_leaf_k)

    t_verify, t_leaf = [], []
    for r in range(a.rounds + 1):
        tv, tl = kernel_ms(run_verify), kernel_ms(run_leaf)
        if r:  # round 0 warms both up
            t_verify.append(tv)
            t_leaf.append(tl)
    torch.cuda.synchronize()
    assert bool((d_ok == 1).all()), "verify kernel disagrees with leaf_kernel"
    assert [m & 0xFFFFFFFF for m in d_mask.cpu().tolist()] == masks

    metas = b"".join(d_sl[i * per + slen - 48:i * per + slen].cpu().numpy().tobytes() for i in range(a.nobj))
    descs = batch.decode_descs([(o * per, slen, masks[o], o * a.size) for o in range(a.nobj)])
    leaves = d_leaf.cpu().numpy().tobytes()
    d_out = torch.empty(a.nobj * a.size, dtype=torch.uint8, device=dev)

    def call_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    res = {}

    def run_plain():
        batch.decode_batch(s, d_sl, descs, metas, d_out)

    def run_verified():
        res["status"], res["rejected"] = batch.decode_verified_batch(s, d_sl, descs, metas, leaves, d_out)

    t_plain, t_verified, k_plain = [], [], []
    for r in range(a.rounds + 1):
        d_out.zero_()
        tp = call_ms(run_plain)
        kp = kernel_ms(run_plain)
        assert torch.equal(d_out, d_in)
        d_out.zero_()
        tv = call_ms(run_verified)
        assert torch.equal(d_out, d_in) and not any(res["status"]) and not any(res["rejected"])
        if r:
            t_plain.append(tp)
            k_plain.append(kp)
            t_verified.append(tv)

    out = {
        "nobj": a.nobj, "size": a.size, "slice_len": slen, "survivors": k, "streams": nstreams, "rounds": a.rounds,
        "verify_kernel_ms": stats(t_verify), "leaf_kernel_ms": stats(t_leaf),
        "decode_call_ms": stats(t_plain), "decode_kernel_ms": stats(k_plain), "verified_decode_call_ms": stats(t_verified),
    }
    v, lf = out["verify_kernel_ms"], out["leaf_kernel_ms"]
    out["verify_minus_leaf_ms"] = v["median"] - lf["median"]
    out["verify_within_leaf_spread"] = v["median"] <= lf["median"] + lf["spread"]
    out["verified_minus_plain_call_ms"] = out["verified_decode_call_ms"]["median"] - out["decode_call_ms"]["median"]
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
