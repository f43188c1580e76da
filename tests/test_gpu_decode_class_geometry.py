"""The decode / recover class kernels (tape_amd/csrc/decode_class.hip, dec_class.hpp) in the shape the
read figures come from: the batch kernels (two waves of 64 column words per workgroup, a stripe
spread over several workgroups, scratch rows in global memory, class groups side by side on forked
streams) on 1 MB stripes (sub-chunk sc = 1430: 358 words, 6 column groups, 3 workgroups), and at the
column-count edges of that kernel.  Every comparison is bit-exact: decode against the original
bytes, recover against the slice the GPU encode wrote (pinned to the oracle by test_gpu_parity.py and
test_gpu_encode_queue.py) and, for one object per call, against the oracle's slice.  Outputs are
poisoned with 0xA5, laid back to back (so offsets are odd after an odd length) and compared whole on
the device, guard bytes included.  Which kernels ran is asserted from te_clay_decode_launch_stats.

Two facts of the layout shape the cases.  (1) All stripes of an object share one chunk size
(Slicer::encode takes chunk_size_for(min(stripe, blob)); te_slicer_geometry), so a short last
stripe of a 1 MB-stripe object still has sc = 1430 and only a shorter output (out_len); other
sub-chunk sizes reach the batch kernel through one-stripe objects, whose chunk size the decoder
takes from the slice length (Slicer::decode, validate_layout).  The column-edge cases are therefore
one-stripe objects of 66 per call, their slices made by ClayCoder::encode on the GPU plus the
metadata suffix.  (2) Under the default rotated mapping a stripe's class follows its shards, and
stripe 1 is rotated by 7 against stripe 0: a survivor set of class a0 at stripe 0 is of another
class at stripe 1 (classes 0 and 1 on both stripes of one object is impossible), so the two-class
calls use the pairs {a0, a0 + 4} under rotation and the pairs (0,1) .. (6,7) under the identity
mapping; the expected class ids of every call are computed here per stripe, from the shard map."""
import bisect
import functools
import itertools
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import batch

pytestmark = pytest.mark.gpu
N, K = 20, 7
POISON, GUARD = 0xA5, 16
FULL = 2_000_000  # two full 1 MB stripes


def _slicer(rotated):
    return T.Slicer.clay_default() if rotated else T.Slicer.new(T.ClayCoder(20, 7, 16))


@functools.lru_cache(None)
def _shard_map(rotated):
    strat = T.MappingStrategy.Rotated if rotated else T.MappingStrategy.Identity
    return [[T.slice_to_shard(strat, N, st, sl) for sl in range(N)] for st in range(4)]


def _a0(rotated, st, keep):  # known column-0 nodes of stripe st
    m = _shard_map(rotated)[st]
    return sum(m[i] < 10 for i in keep)


def _dec_ids(rotated, ns, keep):
    return [_a0(rotated, st, keep) for st in range(ns)]


def _rec_ids(rotated, ns, keep, lost):
    return [8 + 2 * _a0(rotated, st, keep) + _shard_map(rotated)[st][lost] // 10 for st in range(ns)]


def _survivors(rnd, a0):
    return tuple(sorted(rnd.sample(range(10), a0) + rnd.sample(range(10, 20), K - a0)))


def _mask(keep):
    return sum(1 << j for j in keep)


@functools.lru_cache(None)
def _rotated_pool():
    """Survivor sets by (class at stripe 0, class at stripe 1) under the rotated mapping, up to 64
    of each, spread over the 77,520 sets."""
    pool = {}
    for j, keep in enumerate(itertools.combinations(range(N), K)):
        lst = pool.setdefault((_a0(True, 0, keep), _a0(True, 1, keep)), [])
        if len(lst) < 64 and (j % 7 == 0 or len(lst) < 8):
            lst.append(keep)
    return pool


class _Set:
    pass


_sets = {}


def _encoded(rotated, lens, seed):
    """Objects of the given lengths, every byte from one seeded device generator, encoded once by
    the batched GPU encode; shared by the tests and left unchanged."""
    import torch
    key = (rotated, tuple(lens), seed)
    if key in _sets:
        return _sets[key]
    e = _Set()
    e.s = _slicer(rotated)
    e.lens = list(lens)
    e.geo = [e.s.geometry(L) for L in lens]
    e.slen = [int(g.slice_len) for g in e.geo]
    e.in_off, e.sl_off = [], []
    a = b = 0
    for L, sl in zip(lens, e.slen):
        e.in_off.append(a)
        e.sl_off.append(b)
        a += (L + 15) & ~15
        b += N * sl
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    e.d_in = torch.randint(0, 256, (a,), dtype=torch.uint8, device="cuda", generator=gen)
    e.d_sl = torch.empty(b, dtype=torch.uint8, device="cuda")
    batch.encode_batch(e.s, e.d_in, [(e.in_off[i], lens[i], e.sl_off[i], 0) for i in range(len(lens))], e.d_sl)
    torch.cuda.synchronize()
    e.metas = [T.SliceMetadata.new(L, int(g.stripe_size)).to_bytes() for L, g in zip(lens, e.geo)]
    for i in (0, len(lens) - 1):  # the suffix built here is the one the encoder wrote
        at = e.sl_off[i] + e.slen[i]
        assert e.d_sl[at - 48:at].cpu().numpy().tobytes() == e.metas[i]
    _sets[key] = e
    return e


@pytest.fixture(scope="module", autouse=True)
def _release_sets():
    yield
    _sets.clear()


def _guarded(pieces):
    import torch
    g = torch.full((GUARD,), POISON, dtype=torch.uint8, device="cuda")
    return torch.cat([g] + pieces + [g])


def _same(got, exp, starts, what):
    """Whole-buffer comparison on the device; the first mismatch goes to the host for the report."""
    import torch
    if torch.equal(got, exp):
        return
    at = int((got != exp).nonzero()[0])
    obj = bisect.bisect_right(starts, at) - 1
    where = f"object {obj} + {at - starts[obj]}" if obj >= 0 else "front guard"
    pytest.fail(f"{what}: first mismatch at byte {at} ({where}): got {int(got[at]):#x}, expected {int(exp[at]):#x}")


def _decode(e, idx, keeps, what, repeat=1):
    """One decode call of objects idx of set e with survivor sets keeps, outputs back to back
    between guards; returns the launch stats."""
    import torch
    objs, pieces, starts = [], [], []
    at = GUARD
    for i, keep in zip(idx, keeps):
        objs.append((e.sl_off[i], e.slen[i], _mask(keep), at))
        pieces.append(e.d_in[e.in_off[i]:e.in_off[i] + e.lens[i]])
        starts.append(at)
        at += e.lens[i]
    exp = _guarded(pieces)
    out = torch.empty(at + GUARD, dtype=torch.uint8, device="cuda")
    metas = b"".join(e.metas[i] for i in idx)
    for r in range(repeat):
        out.fill_(POISON)
        batch.decode_batch(e.s, e.d_sl, objs, metas, out)
        torch.cuda.synchronize()
        _same(out, exp, starts, f"{what} (call {r})")
    return e.s.coder.decode_launch_stats()


def _recover(e, idx, keeps, losts, what, oracle=None, rotated=True, repeat=1):
    """One recover call; the lost slices back to back between guards, against the encoded ones
    and (object idx[0]) against the oracle's."""
    import torch
    objs, pieces, starts = [], [], []
    at = GUARD
    for i, keep, lost in zip(idx, keeps, losts):
        assert lost not in keep
        objs.append((e.sl_off[i], e.slen[i], _mask(keep), lost, at))
        pieces.append(e.d_sl[e.sl_off[i] + lost * e.slen[i]:e.sl_off[i] + (lost + 1) * e.slen[i]])
        starts.append(at)
        at += e.slen[i]
    exp = _guarded(pieces)
    out = torch.empty(at + GUARD, dtype=torch.uint8, device="cuda")
    metas = b"".join(e.metas[i] for i in idx)
    for r in range(repeat):
        out.fill_(POISON)
        batch.recover_batch(e.s, e.d_sl, objs, metas, out)
        torch.cuda.synchronize()
        _same(out, exp, starts, f"{what} (call {r})")
    if oracle is not None:
        i = idx[0]
        data = e.d_in[e.in_off[i]:e.in_off[i] + e.lens[i]].cpu().numpy()
        ref = oracle.slicer_encode_np(oracle.OracleClay(20, 7, 16), data, rotated=rotated)[losts[0]]
        got = out[starts[0]:starts[0] + e.slen[i]].cpu().numpy()
        assert np.array_equal(got, ref), f"{what}: object {i}'s recovered slice differs from the oracle's"
    return e.s.coder.decode_launch_stats()


def _only_classes(st, launches, stripes, streams):
    assert st["class_g"] == 2, st
    assert st["class_launches"] == launches, st
    assert st["class_stripes"] == stripes, st
    assert st["class_streams"] == streams, st
    assert (st["table_launches"], st["generic_launches"], st["jit_launches"]) == (0, 0, 0), st
    assert (st["table_stripes"], st["generic_stripes"], st["jit_stripes"]) == (0, 0, 0), st


# ---- a. G = 2 at sc = 1430, two class groups: 35 objects of two full stripes, 70 stripes --------
PAIRS = [(False, (0, 1)), (False, (2, 3)), (False, (4, 5)), (False, (6, 7)),
         (True, (0, 4)), (True, (1, 5)), (True, (2, 6)), (True, (3, 7))]


@pytest.mark.parametrize("rotated,pair", PAIRS, ids=[f"{'rot' if r else 'id'}-{p[0]}{p[1]}" for r, p in PAIRS])
def test_decode_two_classes_full_stripes(rotated, pair):
    e = _encoded(rotated, [FULL] * 35, 0xA0 + rotated)
    assert all(int(g.sub_chunk_size) == 1430 and int(g.num_stripes) == 2 for g in e.geo)
    rnd = random.Random(pair[0] * 10 + rotated)
    keeps = []
    for i in range(35):
        if rotated:  # class p on one stripe, q on the other
            p, q = pair if i % 2 == 0 else pair[::-1]
            keeps.append(rnd.choice(_rotated_pool()[(p, q)]))
        else:
            keeps.append(_survivors(rnd, pair[i % 2]))
    ids = [c for k in keeps for c in _dec_ids(rotated, 2, k)]
    assert set(ids) == set(pair) and len(ids) == 70
    st = _decode(e, range(35), keeps, f"decode classes {pair}")
    _only_classes(st, {pair[0]: 1, pair[1]: 1}, 70, 2)


@pytest.mark.parametrize("first", [8, 12, 16, 20])
def test_recover_four_classes_full_stripes(oracle, first):
    """The 16 recover classes, four per call (identity mapping: a class holds on both stripes)."""
    e = _encoded(False, [FULL] * 35, 0xA0)
    rnd = random.Random(first)
    keeps, losts = [], []
    for i in range(35):
        cid = first + i % 4
        a0, yl = (cid - 8) // 2, (cid - 8) % 2
        keep = _survivors(rnd, a0)
        keeps.append(keep)
        losts.append(rnd.choice([j for j in range(10 * yl, 10 * yl + 10) if j not in keep]))
    ids = [c for k, l in zip(keeps, losts) for c in _rec_ids(False, 2, k, l)]
    assert set(ids) == set(range(first, first + 4))
    st = _recover(e, range(35), keeps, losts, f"recover classes {first}..{first + 3}", oracle, rotated=False)
    _only_classes(st, {c: 1 for c in range(first, first + 4)}, 70, 4)


# ---- d. worst case (slices 0..12 erased) in shape a, and mixed with random sets ------------------
def test_decode_worst_case_full_stripes():
    e = _encoded(True, [FULL] * 35, 0xA1)
    worst = tuple(range(13, 20))
    assert _dec_ids(True, 2, worst) == [0, 4]  # shards 13..19, then 6..12
    st = _decode(e, range(35), [worst] * 35, "worst-case decode")
    _only_classes(st, {0: 1, 4: 1}, 70, 2)


def test_decode_worst_case_mixed_with_random_sets():
    """Half worst case (classes 0 and 4 on the two stripes), half sets drawn at random from those
    whose two stripes fall in classes {0, 1, 4, 5}: four class groups, so the call of 70 stripes
    runs on the batch class kernels, one group per stream."""
    e = _encoded(True, [FULL] * 35, 0xA1)
    rnd = random.Random(0xD)
    allowed = {0, 1, 4, 5}
    sets = sorted(k for cc, ks in _rotated_pool().items() if set(cc) <= allowed for k in ks)
    assert len(sets) > 100
    keeps = [tuple(range(13, 20)) if i % 2 == 0 else rnd.choice(sets) for i in range(35)]
    assert len(set(keeps)) > 12  # the random half is not a few sets over and over
    assert {c for k in keeps for c in _dec_ids(True, 2, k)} == allowed
    st = _decode(e, range(35), keeps, "worst case + class-bound random sets")
    _only_classes(st, {c: 1 for c in allowed}, 70, 4)


def test_decode_worst_case_mixed_with_any_sets_table_path():
    """Half worst case, half unrestricted random 7-of-20 sets: more than 4 class groups in a call
    of fewer than 1,024 stripes, which the engine runs in one table-driven launch instead."""
    e = _encoded(True, [FULL] * 35, 0xA1)
    rnd = random.Random(0xD)
    keeps = [tuple(range(13, 20)) if i % 2 == 0 else tuple(sorted(rnd.sample(range(N), K))) for i in range(35)]
    assert len({c for k in keeps for c in _dec_ids(True, 2, k)}) > 4
    st = _decode(e, range(35), keeps, "worst case + random sets")
    assert (st["table_launches"], st["table_stripes"]) == (1, 70), st
    assert st["class_launches"] == {} and st["class_stripes"] == 0, st
    assert (st["generic_stripes"], st["jit_stripes"]) == (0, 0), st


def test_recover_split_call_sums_launch_stats(oracle):
    """A recover batch with an object the fused path does not take (sub-chunk 6) is run in two
    parts; the launch stats cover the whole call: 70 stripes on four batch class kernels and the
    small object's one stripe on the generic kernel."""
    e = _encoded(False, [FULL] * 35 + [4200], 0xA2)
    assert int(e.geo[-1].sub_chunk_size) == 6
    rnd = random.Random(0xE)
    keeps, losts = [], []
    for i in range(36):
        cid = 8 + i % 4
        a0, yl = (cid - 8) // 2, (cid - 8) % 2
        keep = _survivors(rnd, a0)
        keeps.append(keep)
        losts.append(rnd.choice([j for j in range(10 * yl, 10 * yl + 10) if j not in keep]))
    order = list(range(17)) + [35] + list(range(17, 35))  # the small object in the middle of the call
    st = _recover(e, order, [keeps[i] for i in order], [losts[i] for i in order], "split recover", oracle, rotated=False)
    assert st["class_g"] == 2 and st["class_streams"] == 4, st
    assert st["class_launches"] == {8: 1, 9: 1, 10: 1, 11: 1} and st["class_stripes"] == 70, st
    assert (st["generic_launches"], st["generic_stripes"]) == (1, 1), st
    assert (st["table_stripes"], st["jit_stripes"]) == (0, 0), st


# ---- b. column-group and tail edges: one-stripe objects of a chosen sub-chunk size --------------
EDGES = [8, 10, 254, 256, 258, 510, 512, 514, 768, 770, 1024, 1026]
WITH_SC6 = {8, 512, 1026}  # these calls also carry two sc = 6 objects, which stay on the generic kernel


@pytest.mark.parametrize("sc", EDGES)
def test_decode_column_edges(oracle, sc):
    """66 one-stripe objects of sub-chunk size sc (words: sc/4 rounded up; 64-word groups, two per
    workgroup), four classes, blob lengths r over the whole range of that sc: r = 7 * chunk (every
    row whole), r ending on a word boundary and inside a word (the byte stores of a word across
    the end of the output), and the smallest r of the sc."""
    import torch
    case = EDGES.index(sc)
    coder = T.ClayCoder(20, 7, 16)
    s = T.Slicer.clay_default()
    cs, hi, lo = sc * 100, (sc // 2) * 1400, (sc // 2 - 1) * 1400
    rnd = random.Random(sc)
    rs = [hi, hi - 1, hi - 2, hi - 3, hi - 4, hi - 5, lo + 1, lo + 2, lo + 3, lo + 4]
    rs += [rnd.randrange(lo + 1, hi + 1) for _ in range(66 - len(rs))]
    classes = [(2 * case + j) % 8 for j in range(4)]
    slen = cs + 48
    small = [4200, 4197] if sc in WITH_SC6 else []
    g6 = s.geometry(4200)
    assert int(g6.sub_chunk_size) == 6
    host = np.empty(len(rs) * N * slen + len(small) * N * int(g6.slice_len), np.uint8)
    objs, pieces, starts, metas, keeps = [], [], [], b"", []
    at, sl_at = GUARD, 0
    for i, r in enumerate(rs + small):
        data = oracle.splitmix64_bytes((sc << 16) ^ i, r)
        keep = _survivors(rnd, classes[i % 4])
        if i < len(rs):
            assert coder.chunk_size_for(r) == cs
            chunks = coder.encode(data.tobytes())  # stripe 0 is not rotated: slice j holds chunk j
            meta = T.SliceMetadata.new(r, 100_000 if r <= 100_000 else 1_000_000).to_bytes()
            this = slen
            for j in range(N):
                host[sl_at + j * slen:sl_at + j * slen + cs] = np.frombuffer(chunks[j], np.uint8)
                host[sl_at + j * slen + cs:sl_at + (j + 1) * slen] = np.frombuffer(meta, np.uint8)
        else:
            slices = s.encode(data.tobytes())
            meta, this = slices[0][-48:], len(slices[0])
            host[sl_at:sl_at + N * this] = np.frombuffer(b"".join(slices), np.uint8)
        objs.append((sl_at, this, _mask(keep), at))
        keeps.append(keep)
        metas += meta
        pieces.append(torch.from_numpy(data))
        starts.append(at)
        at += r
        sl_at += N * this
    exp = _guarded([torch.cat(pieces).cuda()])
    d_sl = torch.from_numpy(host).cuda()
    out = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert {o[3] % 4 for o in objs} == {0, 1, 2, 3}  # output offsets of every alignment
    batch.decode_batch(s, d_sl, objs, metas, out)
    torch.cuda.synchronize()
    _same(out, exp, starts, f"sc {sc}")
    st = s.coder.decode_launch_stats()
    assert st["class_g"] == 2 and st["class_streams"] == 4, st
    assert st["class_launches"] == {c: 1 for c in classes} and st["class_stripes"] == len(rs), st
    assert (st["table_stripes"], st["jit_stripes"]) == (0, 0), st
    assert (st["generic_launches"], st["generic_stripes"]) == ((1, 2) if small else (0, 0)), st


# ---- c. every class in one call of 1,024 stripes, on forked streams, twice on one handle --------
def _many():
    rnd = random.Random(512)
    lens = [rnd.randrange(1_200_000, 1_300_001) for _ in range(512)]
    return _encoded(True, lens, 0xC0)


def test_decode_all_classes_1024_stripes():
    e = _many()
    rnd = random.Random(0xC1)
    pool = {a0: [_survivors(rnd, a0) for _ in range(4)] for a0 in range(8)}
    keeps = [pool[i % 8][(i // 8) % 4] for i in range(512)]  # class i % 8 at stripe 0
    ids = [c for k in keeps for c in _dec_ids(True, 2, k)]
    assert set(ids) == set(range(8)) and len(ids) == 1024
    assert len(set(e.slen)) == 1  # one chunk size and slice length: one class group per class
    st = _decode(e, range(512), keeps, "all decode classes", repeat=2)
    _only_classes(st, {c: 1 for c in range(8)}, 1024, 4)


def test_recover_all_classes_1024_stripes(oracle):
    e = _many()
    rnd = random.Random(0xC2)
    pool = {}
    for cid in range(8, 24):
        a0, yl = (cid - 8) // 2, (cid - 8) % 2
        pool[cid] = []
        for _ in range(2):
            keep = _survivors(rnd, a0)
            pool[cid].append((keep, rnd.choice([j for j in range(10 * yl, 10 * yl + 10) if j not in keep])))
    picks = [pool[8 + i % 16][(i // 16) % 2] for i in range(512)]  # class 8 + i % 16 at stripe 0
    keeps, losts = [p[0] for p in picks], [p[1] for p in picks]
    ids = [c for k, l in zip(keeps, losts) for c in _rec_ids(True, 2, k, l)]
    assert set(ids) == set(range(8, 24)) and len(ids) == 1024
    st = _recover(e, range(512), keeps, losts, "all recover classes", oracle, rotated=True, repeat=2)
    _only_classes(st, {c: 1 for c in range(8, 24)}, 1024, 4)
