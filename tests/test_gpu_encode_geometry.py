"""Encode at the geometry edges of its three kernels, with the kernel that ran asserted from
te_clay_encode_launch_stats (encode_enqueue in tape_amd/csrc/engine.cpp picks enc_dma_kernel,
enc_stage_kernel<K, G, MASKED> or the generic gpe_kernel per launch group).  Every comparison is
bit-exact against the oracle (OracleClay.encode, slicer_encode_np), never against a GPU result.

Per-call raw encode (te_clay_encode, one stripe of k * alpha * sc bytes -- the only way to an
arbitrary sub-chunk size sc) writes into a numpy block filled with 0xA5 with 64 guard bytes on each
side.  The call copies n * cs bytes out of the handle's device buffer, which earlier calls wrote
too, so every call has data of its own seed: a word the kernel never stores then holds another
call's bytes, not the right ones.  The device batch cases get a 0xA5-filled device buffer with 16
guard bytes between objects, compared whole on the device.

Row stores of the staged kernel (encode_stage.hip).  A workgroup of G waves owns a segment of
RS = 256 G bytes of every row of sc bytes; lseg = min(RS, sc - seg * RS).  It stores lseg >> 4
16-byte blocks, then either one more lane rewriting the row's last 16 bytes (the "wide tail", when
lseg & 15 != 0 and lseg >= 16) or, for lseg < 16, 16-bit stores; every other lane stores at an
out-of-range offset.  One workgroup per stripe up to sc = 1536 (lseg = sc, the whole row); beyond,
every workgroup but the last has lseg = RS = 1536 and the last sc - 1536 (wgs - 1), so lseg & 15 =
sc & 15 in both.  The Clay(20,7,16) sub-chunk sizes below give, as (sc & 15: sc):
  whole row, wide tail   0: 16 256 512 768 1024 1280 1536   2: 18 258 514 770 1026 1442   4: 260
                         6: 518   8: 776   10: 1034   12: 1276   14: 254 510 1278
  whole row, lseg < 16   2 4 6 8 10 12 14 (sc itself)
  last workgroup, wide   0: 3072 (lseg 1536)   2: 1794   4: 1796   6: 1798   8: 2056   10: 2314
                         12: 2572   14: 2830
  last workgroup, < 16   2: 1538 3074   4: 1540   14: 3086
260, 518, 776, 1034, 1276, 10, 12 and the eight between 1540 and 3086 supply the tails the other
sizes leave out (test_tail_coverage checks this table against the lists).  The largest inputs are
2.2 MB (K = 7, sc = 3086) and 1.5 MB (K = 10, sc = 1538).

Row stores of the LDS-DMA kernel (encode_dma.hip): one workgroup stores whole rows, nb = sc >> 4
16-byte blocks on lanes 0..63 and, as a second store, 64..nb - 1, then for tail = sc & 15 != 0 the
lane with lane + 64 == nb rewriting the row's last 16 bytes.  Its sizes, at both ends of its range
1282..1440, as (sc & 15: sc); nb = 80 up to 1294, 89 from 1428 and 90 at 1440:
  LDS-DMA, whole row     0: 1440   2: 1282   4: 1284 1428   6: 1430   8: 1288 1432   10: 1290 1434
                         12: 1292 1436   14: 1294 1438"""
import ctypes as C
import functools

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib

pytestmark = pytest.mark.gpu
N = 20
POISON = 0xA5
RAW_GUARD, GUARD = 64, 16

# sc -> (waves per workgroup, workgroups per stripe): 64 four-byte words per wave, at most 6 waves
STAGE_7 = {2: (1, 1), 4: (1, 1), 6: (1, 1), 8: (1, 1), 10: (1, 1), 12: (1, 1), 14: (1, 1), 16: (1, 1), 18: (1, 1),
           254: (1, 1), 256: (1, 1), 258: (2, 1), 260: (2, 1), 510: (2, 1), 512: (2, 1), 514: (3, 1), 518: (3, 1),
           768: (3, 1), 770: (4, 1), 776: (4, 1), 1024: (4, 1), 1026: (5, 1), 1034: (5, 1), 1276: (5, 1),
           1278: (5, 1), 1280: (5, 1), 1442: (6, 1), 1536: (6, 1), 1538: (6, 2), 1540: (6, 2), 1794: (6, 2),
           1796: (6, 2), 1798: (6, 2), 2056: (6, 2), 2314: (6, 2), 2572: (6, 2), 2830: (6, 2), 3072: (6, 2),
           3074: (6, 3), 3086: (6, 3)}
STAGE_10 = {8: (1, 1), 256: (1, 1), 258: (2, 1), 770: (4, 1), 1026: (5, 1), 1282: (6, 1), 1430: (6, 1), 1538: (6, 2)}
DMA_7 = (1282, 1284, 1288, 1290, 1292, 1294, 1428, 1430, 1432, 1434, 1436, 1438, 1440)
GENERIC = (((20, 8, 17), 64), ((12, 8, 11), 64))
SHORTEN = (0, 1, 4, 1399)  # data end dword aligned, unaligned, aligned, unaligned and inside an earlier row

RAW_CASES = [((20, 7, 16), sc, "stage") for sc in STAGE_7] + [((20, 7, 16), sc, "dma") for sc in DMA_7] + \
            [((20, 10, 19), sc, "stage") for sc in STAGE_10] + [(p, sc, "generic") for p, sc in GENERIC]


def test_tail_coverage():
    """The docstring's table: every even lseg & 15 on a whole-row segment and on a last-workgroup
    segment, as a wide tail; the short rows; the (G, workgroups) column of STAGE_7 / STAGE_10; and
    every even sc & 15 on the LDS-DMA kernel's rows, with the fewest and the most 16-byte blocks."""
    whole = {sc for sc in STAGE_7 if sc <= 1536}
    last = {sc: sc - 1536 * (STAGE_7[sc][1] - 1) for sc in STAGE_7 if sc > 1536}
    assert {sc & 15 for sc in whole if sc >= 16} == set(range(0, 16, 2))
    assert {sc for sc in whole if sc < 16} == {2, 4, 6, 8, 10, 12, 14}
    assert {lseg & 15 for lseg in last.values() if lseg >= 16} == set(range(0, 16, 2))
    assert {lseg for lseg in last.values() if lseg < 16} == {2, 4, 14}
    assert all(0 < lseg <= 1536 for lseg in last.values())
    for table in (STAGE_7, STAGE_10):
        for sc, (g, wgs) in table.items():
            groups = -(-(-(-sc // 4)) // 64)
            assert g == min(groups, 6) and wgs == -(-groups // g), sc
    assert {g for g, _ in STAGE_7.values()} == {1, 2, 3, 4, 5, 6}
    assert all(1280 < sc <= 1440 and sc % 2 == 0 for sc in DMA_7)
    assert {sc & 15 for sc in DMA_7} == set(range(0, 16, 2))
    assert {80, 90} <= {sc >> 4 for sc in DMA_7}
    assert {sc % 4 for sc in DMA_7} == {0, 2}


@functools.lru_cache(None)
def _coder(params):
    return T.ClayCoder(*params)


@functools.lru_cache(None)
def _oracle_clay(params):
    from oracle import oracle as O
    return O.OracleClay(*params)


def _raw_encode(c, data):
    """te_clay_encode of a numpy array into a poisoned, guarded block: (chunks n * cs, cs)."""
    cs = c.chunk_size_for(data.size)
    total = c.n() * cs
    block = np.full(total + 2 * RAW_GUARD, POISON, np.uint8)
    got = C.c_size_t()
    r = _lib.lib.te_clay_encode(c.handle, data.ctypes.data, data.size, block.ctypes.data + RAW_GUARD, total, C.byref(got))
    assert r == 0, (r, _lib.lib.te_last_error_detail())
    assert got.value == cs
    assert (block[:RAW_GUARD] == POISON).all() and (block[RAW_GUARD + total:] == POISON).all(), "guard bytes written"
    return block[RAW_GUARD:RAW_GUARD + total], cs


@pytest.mark.parametrize("params,sc,path", RAW_CASES, ids=[f"{p[1]}-{sc}-{path}" for p, sc, path in RAW_CASES])
def test_raw_encode(oracle, params, sc, path):
    """One stripe at sub-chunk sc, shortened by 0, 1, 4 and 1,399 bytes: the chunks equal the oracle's
    and the stats show the expected kernel, its geometry and whether the launch was masked.  (With
    (12,8,11), alpha = 64, 1,399 bytes fewer is one sub-chunk step less; the kernel is the same.)"""
    c, o = _coder(params), _oracle_clay(params)
    k, alpha = params[1], c.alpha()
    for r in SHORTEN:
        ln = k * alpha * sc - r
        cs = c.chunk_size_for(ln)
        if alpha == 100:
            assert cs == sc * alpha, (ln, cs)
        data = oracle.splitmix64_bytes((sc << 16 | r << 4 | k) + 1, ln)
        got, _ = _raw_encode(c, data)
        exp = np.frombuffer(b"".join(o.encode(data.tobytes())), np.uint8)
        assert got.size == exp.size
        if not np.array_equal(got, exp):
            at = int(np.flatnonzero(got != exp)[0])
            pytest.fail(f"sc {sc} r {r}: first mismatch at chunk {at // cs} plane {at % cs // (cs // alpha)} "
                        f"column {at % (cs // alpha)}: got {got[at]:#x}, expected {exp[at]:#x}")
        st = c.encode_launch_stats()
        masked = 1 if ln % 4 else 0
        zero = dict.fromkeys(st, 0)
        if path == "stage":
            g, wgs = (STAGE_7 if k == 7 else STAGE_10)[sc]
            want = dict(zero, stage_launches=1, stage_stripes=1, stage_masked_launches=masked, stage_g=g, stage_wgs=wgs)
        elif path == "dma":  # a per-call encode splits: the level-1 rows, then the level-2 chain
            want = dict(zero, dma_launches=2, dma_level1_launches=1, dma_level2_launches=1, dma_stripes=1)
        else:
            want = dict(zero, generic_launches=1, generic_stripes=1)
        assert st == want, (sc, r, st)


# ---------------------------------------------------------------- device batch ----------------
class _Batch:
    """Objects of the given lengths at the given source offsets, expected slices from the oracle;
    one 0xA5-filled output with GUARD bytes before, between and after the objects."""

    def __init__(self, oracle, rotated, lens, aligns, seed):
        import torch
        self.s = T.Slicer.clay_default() if rotated else T.Slicer.new(T.ClayCoder(20, 7, 16))
        o716 = _oracle_clay((20, 7, 16))
        self.lens, self.in_off, self.out_off, self.stripes, self.geo = list(lens), [], [], [], []
        at = 0
        for ln, al in zip(lens, aligns):
            at = (at + 3 & ~3) + al  # the source offset's two low bits
            self.in_off.append(at)
            at += ln
        host = oracle.splitmix64_bytes(seed, at + 16)
        exp = [np.full(GUARD, POISON, np.uint8)]
        oat = GUARD
        for ln, off in zip(lens, self.in_off):
            g = self.s.geometry(ln)
            sl = oracle.slicer_encode_np(o716, host[off:off + ln], rotated=rotated)
            assert sl.shape == (N, g.slice_len)
            self.geo.append(g)
            self.stripes.append(int(g.num_stripes))
            self.out_off.append(oat)
            exp += [sl.reshape(-1), np.full(GUARD, POISON, np.uint8)]
            oat += sl.size + GUARD
        self.d_in = torch.from_numpy(host).cuda()
        assert self.d_in.data_ptr() % 4 == 0
        self.d_exp = torch.from_numpy(np.concatenate(exp)).cuda()
        self.objs = [(self.in_off[i], lens[i], self.out_off[i], 0) for i in range(len(lens))]

    def run(self, what):
        import torch
        from tape_amd import batch
        out = torch.full((self.d_exp.numel(),), POISON, dtype=torch.uint8, device="cuda")
        batch.encode_batch(self.s, self.d_in, self.objs, out)
        torch.cuda.synchronize()
        if not torch.equal(out, self.d_exp):
            at = int((out != self.d_exp).nonzero()[0])
            i = max(j for j in range(len(self.lens)) if self.out_off[j] - GUARD <= at)
            rel, sl = at - self.out_off[i], int(self.geo[i].slice_len)
            pytest.fail(f"{what}: first mismatch at byte {at}: object {i} ({self.lens[i]} B at source offset "
                        f"{self.in_off[i]}) slice {rel // sl} + {rel % sl}" if 0 <= rel < N * sl else
                        f"{what}: guard byte {at} after object {i} written")
        return self.s.coder.encode_launch_stats()

    def expected_stats(self):
        """Launch groups of encode_enqueue, from the offsets: (chunk size, slice length, data end
        not dword aligned, source address odd); odd addresses run the generic kernel, sub-chunks of
        1282..1440 bytes the LDS-DMA kernel (unsplit in a batch), the rest the staged one."""
        keys = {"stage": set(), "generic": set(), "dma": set()}
        n = dict.fromkeys(keys, 0)
        masked = set()
        for ln, off, g in zip(self.lens, self.in_off, self.geo):
            S, sc = int(g.stripe_size), int(g.sub_chunk_size)
            for st in range(int(g.num_stripes)):
                a, src_len = off + st * S, min(S, ln - st * S)
                key = (int(g.chunk_size), int(g.slice_len), (a % 4 + src_len) % 4 != 0, a % 2 == 1)
                path = "generic" if a % 2 else "dma" if 1280 < sc <= 1440 else "stage"
                keys[path].add(key)
                n[path] += 1
                if path == "stage" and key[2]:
                    masked.add(key)
        return {"dma_launches": len(keys["dma"]), "dma_level1_launches": 0, "dma_level2_launches": 0,
                "stage_launches": len(keys["stage"]), "stage_masked_launches": len(masked),
                "generic_launches": len(keys["generic"]), "dma_stripes": n["dma"], "stage_stripes": n["stage"],
                "generic_stripes": n["generic"]}


def _check_stats(st, want):
    assert {f: st[f] for f in want} == want, st
    assert (st["stage_g"] > 0) == (st["stage_launches"] > 0) == (st["stage_wgs"] > 0), st


# 64 one-stripe objects of 1 .. 100,000 bytes (sc = 2 .. 144), object i at a source offset = i mod 4
SMALL_LENS = [1, 2, 3, 4, 5, 1399, 1400, 1401, 1402, 2799, 2800, 2801, 99_999, 100_000, 99_998, 99_997] + \
             [1 + (i * 2_654_435_761) % 100_000 for i in range(48)]
SMALL_ALIGN = [i % 4 for i in range(64)]
MULTI_LENS = [100_001, 250_003, 1_000_000]  # 2, 3 and 10 stripes of 100 kB at sc = 144


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "identity"])
def test_batch_one_stripe_objects(oracle, rotated):
    """(a) even source addresses count as staged stripes, odd ones as generic stripes."""
    assert len(SMALL_LENS) == 64 and max(SMALL_LENS) == 100_000 and min(SMALL_LENS) == 1
    b = _Batch(oracle, rotated, SMALL_LENS, SMALL_ALIGN, 0xE0C0DE)
    assert set(b.stripes) == {1}
    scs = {int(g.sub_chunk_size) for g in b.geo}
    assert min(scs) == 2 and max(scs) == 144
    want = b.expected_stats()
    assert want["stage_stripes"] == 32 and want["generic_stripes"] == 32 and want["dma_stripes"] == 0
    assert want["stage_masked_launches"] > 0 and want["stage_masked_launches"] < want["stage_launches"]
    _check_stats(b.run("one-stripe objects"), want)


def test_batch_short_last_stripe(oracle):
    """(b) 100 kB stripes with a short last one: its padding rows are written over the poison."""
    b = _Batch(oracle, True, MULTI_LENS, [0, 2, 0], 0xE0C0DF)
    assert b.stripes == [2, 3, 10] and {int(g.sub_chunk_size) for g in b.geo} == {144}
    want = b.expected_stats()
    assert want["stage_stripes"] == 15 and want["generic_stripes"] == want["dma_stripes"] == 0
    st = b.run("short last stripe")
    _check_stats(st, want)
    assert (st["stage_g"], st["stage_wgs"]) == (1, 1)


def test_batch_mixed_call_twice(oracle):
    """(c) one call with staged, generic and LDS-DMA launches, stripe counts summing to the call's;
    (d) the same call again on the handle: the same stats, not doubled."""
    lens = SMALL_LENS + MULTI_LENS + [2_000_003]
    b = _Batch(oracle, True, lens, SMALL_ALIGN + [0, 2, 1, 0], 0xE0C0E0)
    assert b.stripes[-1] == 3 and int(b.geo[-1].sub_chunk_size) == 1430
    want = b.expected_stats()
    assert want["dma_stripes"] == 3 and want["dma_launches"] == 2  # the 3-byte last stripe ends unaligned
    assert want["stage_stripes"] == 32 + 5 and want["generic_stripes"] == 32 + 10
    assert want["dma_stripes"] + want["stage_stripes"] + want["generic_stripes"] == sum(b.stripes)
    first = b.run("mixed call")
    _check_stats(first, want)
    assert b.run("mixed call, again") == first
