"""Repair at the geometry edges of its three kernels, with the kernel that ran asserted from
te_clay_repair_launch_stats (repair_enqueue in tape_amd/csrc/engine.cpp picks rep_fold_kernel<G>,
rep_stage_kernel<G> or the generic kernel per stripe).  The repaired chunk or slice is compared,
bit-exact, with the ORACLE's encoded one; helper fragments are cut from the oracle's encode, so no
GPU result enters a comparison.  Outputs are poisoned with 0xA5 and guarded.

Which kernel a stripe takes (kernels.hpp, repair_enqueue): Clay(20,7,16) (nu = 0, n = 2q) with
minimum_to_repair's helper set when the other column's known nodes are its first 7, or its first 8
less one of the first 7, runs the folded kernel; any other set with a plane program
(repair_stage_supported: q = 10, beta = 10, at most 13 erased, 10 known and 4 aloof nodes) the staged
kernel; both need sub-chunks of at least 8 bytes, below which the generic kernel runs -- as it does
for a layout without a plane program, (12,8,11).  Both fast kernels give a workgroup g = min(groups,
kMaxG) waves of 64 four-byte words and a stripe ceil(groups / g) workgroups.

Per-call te_clay_repair goes through the handle's page-locked staging, which earlier calls wrote
too: consecutive calls here repair different lost nodes, so a word the kernel never stores holds
another chunk's bytes, not the right ones.  The batch case writes straight into a poisoned device
buffer."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib

pytestmark = pytest.mark.gpu
N = 20
POISON = 0xA5
RAW_GUARD, GUARD = 64, 16
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tape_amd")
STAGE_MAX_ALOOF = 4  # repair_stage.hip kMaxAloof


def _maxg(name, src):
    """The build's waves-per-workgroup cap: -D<name>=g in the Makefile, else the source's default."""
    m = re.search(r"-D%s=(\d+)" % name, open(os.path.join(CSRC, "Makefile")).read()) or \
        re.search(r"#define %s (\d+)" % name, open(os.path.join(CSRC, "csrc", src)).read())
    return int(m.group(1))


FOLD_MAXG = _maxg("TEC_RFOLD_MAXG", "repair_fold.hip")
STAGE_MAXG = _maxg("TEC_REP_MAXG", "repair_stage.hip")
# ceil(sc / 4) crossing 64 g for g = 1 .. kMaxG of either kernel, one size beyond each that needs
# two workgroups per stripe, and the smallest staged sizes
EDGE_SC = sorted({8, 10, 14} | {256 * g + e for m in (FOLD_MAXG, STAGE_MAXG) for g in range(1, m + 1) for e in (0, 2)} |
                 {256 * (m + 1) + 2 for m in (FOLD_MAXG, STAGE_MAXG)})
SMALL_SC = [2, 4, 6]
LOST = [0, 6, 9, 10, 19]


def _geom(sc, maxg):
    wps = (sc + 3) // 4 if sc >= 4 else 1
    groups = (wps + 63) // 64
    g = min(groups, maxg)
    return g, (groups + g - 1) // g


def _is_fold_set(known):
    return known == set(range(7)) or any(known == set(range(8)) - {p} for p in range(7))


def _expected_path(o, sc, lost_shard, helper_shards):
    """The kernel of one stripe, from the layout and the helper set alone."""
    beta = o.alpha // o.q
    if o.nu == 0 and o.n == 2 * o.q and (o.q, o.t, o.k) == (10, 2, 7) and sc >= 8:
        col = lost_shard // o.q
        if _is_fold_set({h % o.q for h in helper_shards if h // o.q != col}):
            return "fold"
    aloof = o.n - 1 - len(helper_shards)
    nerased, nknown = o.q + aloof, o.k
    stage_ok = o.q == 10 and beta == 10 and sc >= 8 and nerased <= 13 and nknown <= 10 and aloof <= STAGE_MAX_ALOOF
    return "stage" if stage_ok else "generic"


def _want(path, sc, stripes=1):
    want = dict.fromkeys(("fold_launches", "stage_launches", "generic_launches", "fold_g", "fold_wgs", "stage_g",
                          "stage_wgs", "fold_stripes", "stage_stripes", "generic_stripes"), 0)
    want[path + "_launches"], want[path + "_stripes"] = 1, stripes
    if path != "generic":
        want[path + "_g"], want[path + "_wgs"] = _geom(sc, FOLD_MAXG if path == "fold" else STAGE_MAXG)
    return want


@functools.lru_cache(None)
def _coder(params):
    return T.ClayCoder(*params)


@functools.lru_cache(None)
def _oracle_clay(params):
    from oracle import oracle as O
    return O.OracleClay(*params)


@functools.lru_cache(None)
def _chunks(params, sc):
    """The oracle's n chunks of one stripe at sub-chunk sc: computed once, shared, left unchanged."""
    from oracle import oracle as O
    o = _oracle_clay(params)
    data = O.splitmix64_bytes(0x4E9A ^ sc << 8 ^ params[1], o.k * o.alpha * sc).tobytes()
    ch = o.encode(data)
    assert len(ch[0]) == o.alpha * sc
    return ch


def _raw_repair(params, sc, lost, avail):
    """te_clay_repair of chunk `lost` from the nodes in avail into a poisoned, guarded block; the
    plan is checked against the oracle's minimum_to_repair.  Returns (stats, helper ids)."""
    c, o, ch = _coder(params), _oracle_clay(params), _chunks(params, sc)
    cs = o.alpha * sc
    plan = c.plan_repair(lost, avail)
    assert plan == o.minimum_to_repair(lost, avail), (lost, avail)
    ids = [h for h, _ in plan]
    frags = [np.frombuffer(b"".join(ch[h][z * sc:(z + 1) * sc] for z in planes), np.uint8) for h, planes in plan]
    hs = (C.c_uint32 * len(ids))(*ids)
    ptrs = (C.c_void_p * len(ids))(*[f.ctypes.data for f in frags])
    block = np.full(cs + 2 * RAW_GUARD, POISON, np.uint8)
    r = _lib.lib.te_clay_repair(c.handle, lost, hs, ptrs, len(ids), cs, block.ctypes.data + RAW_GUARD)
    assert r == 0, (r, _lib.lib.te_last_error_detail())
    assert (block[:RAW_GUARD] == POISON).all() and (block[RAW_GUARD + cs:] == POISON).all(), "guard bytes written"
    got, exp = block[RAW_GUARD:RAW_GUARD + cs], np.frombuffer(ch[lost], np.uint8)
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        pytest.fail(f"sc {sc} lost {lost} helpers {ids}: first mismatch at plane {at // sc} column {at % sc}: "
                    f"got {got[at]:#x}, expected {exp[at]:#x}")
    return c.repair_launch_stats(), ids


def _helper_sets(lost):
    """(name, available nodes, kernel at sc >= 8) for Clay(20,7,16): all 19 others; one of the other
    column's first 7 down; two of them down."""
    ob = 10 if lost < 10 else 0
    p1, p2 = lost % 7, (lost + 3) % 7
    others = [i for i in range(N) if i != lost]
    return [("all", others, "fold"),
            ("one-down", [i for i in others if i != ob + p1], "fold"),
            ("two-down", [i for i in others if i not in (ob + p1, ob + p2)], "stage")]


def test_edge_sizes():
    """EDGE_SC holds, for each fast kernel, every g = 1 .. kMaxG at one workgroup per stripe on both
    sides of its 64 g-word edge, and a size of two workgroups."""
    for maxg in (FOLD_MAXG, STAGE_MAXG):
        geoms = {_geom(sc, maxg) for sc in EDGE_SC}
        assert {(g, 1) for g in range(1, maxg + 1)} <= geoms and (maxg, 2) in geoms, geoms
        for g in range(1, maxg + 1):
            assert _geom(256 * g, maxg) == (g, 1) and _geom(256 * g + 2, maxg) != (g, 1)


@pytest.mark.parametrize("sc", EDGE_SC + SMALL_SC)
def test_raw_repair_716(sc):
    params = (20, 7, 16)
    o = _oracle_clay(params)
    for s in range(3):
        for lost in LOST:
            name, avail, path = _helper_sets(lost)[s]
            if sc < 8:
                path = "generic"
            st, ids = _raw_repair(params, sc, lost, avail)
            assert _expected_path(o, sc, lost, ids) == path, (name, lost, ids)
            assert st == _want(path, sc), (sc, name, lost, st)


@pytest.mark.parametrize("params,sc", [((20, 10, 19), 6), ((20, 10, 19), 258), ((12, 8, 11), 6), ((12, 8, 11), 258)],
                         ids=["10-6", "10-258", "12.8-6", "12.8-258"])
def test_raw_repair_other_profiles(params, sc):
    """d = n - 1: every other node helps.  (20,10,19) has no folded kernel (k = 10) and a plane
    program, so the staged kernel from 8-byte sub-chunks; (12,8,11) (q = 4) the generic one."""
    o = _oracle_clay(params)
    n = params[0]
    for lost in (0, params[1], n - 1):
        st, ids = _raw_repair(params, sc, lost, [i for i in range(n) if i != lost])
        path = _expected_path(o, sc, lost, ids)
        assert path == ("generic" if params[0] == 12 or sc < 8 else "stage")
        assert st == _want(path, sc), (params, sc, lost, st)


# ---------------------------------------------------------------- device batch ----------------
def _shard(st, sl):
    return T.slice_to_shard(T.MappingStrategy.Rotated, N, st, sl)


def _two_down(lost, ns):
    """Two slices that sit in the other column than the lost one on every stripe (a column-mate
    down cannot be repaired), the first pair in a fixed order that leaves a stripe without a folded
    helper set."""
    def other_column(d):
        return all(_shard(st, d) // 10 != _shard(st, lost) // 10 for st in range(ns))
    cand = [d for d in ((lost + 10 + a) % N for a in (0, 1, -1, 2, -2, 3, -3, 4, -4)) if other_column(d)]
    for i, a in enumerate(cand):
        for b in cand[i + 1:]:
            if any(not _is_fold_set(_known(st, (a, b))) for st in range(ns)):
                return a, b
    raise AssertionError(f"no pair for lost {lost}")


def _known(st, downs):
    """Positions of the other column's helpers on stripe st: its first 7 available nodes."""
    gone = {_shard(st, d) % 10 for d in downs}
    return set([p for p in range(10) if p not in gone][:7])


def test_repair_batch_geometry(oracle):
    """te_repair_batch_device over 24 objects of 3,000 B (sc = 6), 50,000 B, 300,000 B (3 stripes at
    sc = 144) and 2,000,000 B (2 stripes at sc = 1430: 6 word groups, 3 workgroups per stripe); a third
    with every other slice up, a third with slice (lost + 10) % 20 down, a third with two of the other
    column down.  Every repaired slice, metadata suffix included, equals the oracle's; the stats show
    the stripes each kernel got, computed here per stripe from the rotation."""
    import torch
    from tape_amd import batch
    s = T.Slicer.clay_default()
    o716 = _oracle_clay((20, 7, 16))
    sizes = [3_000, 50_000, 300_000, 2_000_000]
    objs, blobs, exp, keep = [], [], [np.full(GUARD, POISON, np.uint8)], []
    cur, oat = 0, GUARD
    n = {"fold": 0, "stage": 0, "generic": 0}
    launch = {"fold": set(), "stage": set(), "generic": set()}
    big = set()  # kernels of the 2,000,000 B objects' stripes
    for i in range(24):
        L, pattern, lost = sizes[i % 4], (i // 4) % 3, (i * 7 + 3) % N
        g = s.geometry(L)
        ns, sc, slen = int(g.num_stripes), int(g.sub_chunk_size), int(g.slice_len)
        assert (ns, sc) == {3_000: (1, 6), 50_000: (1, 72), 300_000: (3, 144), 2_000_000: (2, 1430)}[L]
        downs = [(), ((lost + 10) % N,), _two_down(lost, ns)][pattern]
        avail = [j for j in range(N) if j != lost and j not in downs]
        sl = oracle.slicer_encode_np(o716, oracle.splitmix64_bytes(0x9E0 + i, L), rotated=True)
        assert sl.shape == (N, slen)
        p = s.repair_plan_from_params(lost, avail, L, int(g.stripe_size))
        offs = {}
        for h in avail:
            b = T.extract_repair_data(sl[h].tobytes(), p, h)
            if b:
                offs[h] = cur
                blobs.append(b)
                cur += len(b)
        keep.append(p)
        objs.append((p, offs, oat, sl[0][-48:].tobytes()))
        exp += [sl[lost], np.full(GUARD, POISON, np.uint8)]
        oat += slen + GUARD
        for st in range(ns):
            path = "generic" if sc < 8 else "fold" if _is_fold_set(_known(st, downs)) else "stage"
            n[path] += 1
            launch[path].add(int(g.chunk_size))  # one launch per chunk size for the folded kernel, one for the rest
            if L == 2_000_000:
                big.add(path)
    assert min(n.values()) > 0, n
    d_help = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    d_exp = torch.from_numpy(np.concatenate(exp)).cuda()
    d_rep = torch.full((d_exp.numel(),), POISON, dtype=torch.uint8, device="cuda")
    batch.repair_batch(s.coder, d_help, objs, d_rep)
    torch.cuda.synchronize()
    if not torch.equal(d_rep, d_exp):
        at = int((d_rep != d_exp).nonzero()[0])
        i = max(j for j in range(24) if objs[j][2] - GUARD <= at)
        pytest.fail(f"first mismatch at byte {at}: object {i} ({sizes[i % 4]} B) + {at - objs[i][2]}: "
                    f"got {int(d_rep[at]):#x}, expected {int(d_exp[at]):#x}")
    st = s.coder.repair_launch_stats()
    assert {k: st[k + "_stripes"] for k in n} == n, st
    assert {k: st[k + "_launches"] for k in n} == {k: len(v) for k, v in launch.items()}, st
    # chunk sizes are launched in first-seen order: the last folded and the last staged launch are
    # the 2,000,000 B objects'
    assert big == {"fold", "stage"}
    assert (st["fold_g"], st["fold_wgs"]) == _geom(1430, FOLD_MAXG), st
    assert (st["stage_g"], st["stage_wgs"]) == _geom(1430, STAGE_MAXG), st
