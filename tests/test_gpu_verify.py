"""Verified reads on the device: the ragged leaf-verify kernel (verify.hip) against hashlib, and
the verified decode / recover / repair calls built on it.  Expected hashes come from
hashlib.sha256(b"LEAF" + data), never from the library."""
import hashlib
import random

import numpy as np
import pytest

import tape_amd as T
from tape_amd import _lib, batch, merkle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, K = 20, 7
# every padding case (the terminator and the length in the data's last block, in the next, the
# length alone in the next), a launch boundary of 1,536 blocks straddled, and three launches
EDGE = [0, 4, 48, 52, 56, 60, 64, 116, 120, 124, 128, 6140, 98_296, 98_300, 98_304, 196_612]
NITEMS = 130  # two full waves and a partial one


def leaf(data) -> bytes:
    return hashlib.sha256(b"LEAF" + bytes(data)).digest()


class Ragged:
    """130 slices of mixed lengths in shuffled order in one buffer, and hashlib's leaves of them."""

    def __init__(self):
        rng = random.Random(0x5EED)
        self.lens = EDGE + [4 * rng.randrange(0, 700) for _ in range(NITEMS - len(EDGE))]
        rng.shuffle(self.lens)
        self.offs, cur = [], 0
        for ln in self.lens:
            self.offs.append(cur)
            cur += ln + 4 * rng.randrange(0, 3)  # gaps: nothing assumes the slices are adjacent
        self.data = np.frombuffer(rng.randbytes(cur + 4), np.uint8).copy()
        self.leaves = [leaf(self.bytes_of(self.data, i)) for i in range(NITEMS)]
        # item i answers to expected hash i and sets bit i % 20 of object i // 20
        self.items = [(self.offs[i], self.lens[i], i, i // N, 1 << (i % N)) for i in range(NITEMS)]
        self.nobj = (NITEMS + N - 1) // N

    def bytes_of(self, data, i):
        return data[self.offs[i]:self.offs[i] + self.lens[i]].tobytes()

    def at(self, ln):
        return self.lens.index(ln)

    def run(self, coder, data, expected):
        dev = torch.device("cuda:0")
        d_data = torch.from_numpy(data).to(dev)
        d_exp = torch.from_numpy(np.frombuffer(b"".join(expected), np.uint8).copy()).to(dev)
        d_dig = torch.full((NITEMS * 32,), 0xEE, dtype=torch.uint8, device=dev)
        d_ok = torch.full((NITEMS,), 7, dtype=torch.int32, device=dev)
        d_mask = torch.zeros(self.nobj, dtype=torch.int32, device=dev)
        merkle.verify_leaves_device(coder, d_data, self.items, d_exp, d_dig, d_ok, d_mask)
        torch.cuda.synchronize()
        dig = d_dig.cpu().numpy().tobytes()
        return ([dig[32 * i:32 * i + 32] for i in range(NITEMS)], d_ok.cpu().tolist(),
                [m & 0xFFFFFFFF for m in d_mask.cpu().tolist()])


@pytest.fixture(scope="module")
def ragged():
    return Ragged()


@pytest.fixture(scope="module")
def slicer():
    return T.Slicer.clay_default()


def test_ragged_digests(ragged, slicer):
    dig, ok, mask = ragged.run(slicer.coder, ragged.data, ragged.leaves)
    bad = [(i, ragged.lens[i]) for i in range(NITEMS) if dig[i] != ragged.leaves[i]]
    assert not bad, bad
    assert ok == [1] * NITEMS
    want = [sum(1 << (i % N) for i in range(NITEMS) if i // N == o) for o in range(ragged.nobj)]
    assert mask == want


def test_ragged_digests_only(ragged, slicer):
    """No expected hashes: digests alone, ok and the masks untouched."""
    dev = torch.device("cuda:0")
    d_dig = torch.zeros(NITEMS * 32, dtype=torch.uint8, device=dev)
    d_ok = torch.full((NITEMS,), 7, dtype=torch.int32, device=dev)
    merkle.verify_leaves_device(slicer.coder, torch.from_numpy(ragged.data).to(dev), ragged.items, None, d_dig, d_ok,
                                None)
    torch.cuda.synchronize()
    assert d_dig.cpu().numpy().tobytes() == b"".join(ragged.leaves)
    assert d_ok.cpu().tolist() == [7] * NITEMS


def test_mismatch(ragged, slicer):
    data = ragged.data.copy()
    expected = list(ragged.leaves)
    first, last, suffix, wrong = ragged.at(6140), ragged.at(98_300), ragged.at(196_612), ragged.at(124)
    data[ragged.offs[first]:ragged.offs[first] + 4] ^= 0xFF                                  # its first word
    data[ragged.offs[last] + 98_300 - 4:ragged.offs[last] + 98_300] ^= 0xFF                  # its last data word
    data[ragged.offs[suffix] + 196_612 - 48 + 17] ^= 0x01                                    # a byte of its metadata suffix
    expected[wrong] = leaf(b"not this slice")
    dig, ok, mask = ragged.run(slicer.coder, data, expected)
    assert dig == [leaf(ragged.bytes_of(data, i)) for i in range(NITEMS)]  # of the bytes given
    failed = {first, last, suffix, wrong}
    assert len(failed) == 4
    assert [i for i in range(NITEMS) if ok[i] == 0] == sorted(failed)
    assert all(v in (0, 1) for v in ok)
    want = [sum(1 << (i % N) for i in range(NITEMS) if i // N == o and i not in failed) for o in range(ragged.nobj)]
    assert mask == want


class Encoded:
    """Objects encoded by encode_batch, their slices on the host and hashlib's leaves of them."""

    def __init__(self, slicer, oracle, sizes, seed):
        dev = torch.device("cuda:0")
        self.sizes = sizes
        self.blobs = [oracle.splitmix64_bytes(seed ^ (i * 0x9E37), ln) for i, ln in enumerate(sizes)]
        self.geo = [slicer.geometry(ln) for ln in sizes]
        self.in_off, self.sl_off, a, b = [], [], 0, 0
        for ln, g in zip(sizes, self.geo):
            self.in_off.append(a)
            self.sl_off.append(b)
            a += (ln + 15) & ~15
            b += N * g.slice_len
        host = np.zeros(a, np.uint8)
        for o, blob in zip(self.in_off, self.blobs):
            host[o:o + len(blob)] = blob
        d_sl = torch.zeros(b, dtype=torch.uint8, device=dev)
        batch.encode_batch(slicer, torch.from_numpy(host).to(dev),
                           [(self.in_off[i], sizes[i], self.sl_off[i], i) for i in range(len(sizes))], d_sl)
        torch.cuda.synchronize()
        self.slices = d_sl.cpu().numpy()
        self.leaves = [[leaf(self.slice(o, i)) for i in range(N)] for o in range(len(sizes))]
        self.metas = b"".join(self.slice(o, 0)[-48:].tobytes() for o in range(len(sizes)))

    def slice(self, o, i, src=None):
        src = self.slices if src is None else src
        ln = self.geo[o].slice_len
        return src[self.sl_off[o] + i * ln:self.sl_off[o] + (i + 1) * ln]


def _mask(ids):
    return sum(1 << i for i in ids)


def test_verified_decode(slicer, oracle):
    o716 = oracle.OracleClay(20, 7, 16)
    dev = torch.device("cuda:0")
    sizes = [20_000] * 48 + [2_500_000] * 4 + [20_000] * 2
    nobj, short = len(sizes), (52, 53)
    e = Encoded(slicer, oracle, sizes, 0xD0C0DE)
    assert e.geo[48].num_stripes == 3 and merkle_blocks(e.geo[48].slice_len) > 2 * 1536  # several launches
    rng = random.Random(77)
    bad = e.slices.copy()
    present, corrupt = [], []
    for o in range(nobj):
        p = sorted(rng.sample(range(N), K if o in short else 9))
        c = sorted(rng.sample(p, 1 if o in short else o % 3))
        for i in c:  # anywhere in the slice: its data, or its metadata suffix
            sl = e.slice(o, i, bad)
            sl[rng.randrange(len(sl))] ^= 1 << rng.randrange(8)
        present.append(p)
        corrupt.append(c)
    out_off, cur = [], 0
    for ln in sizes:
        out_off.append(cur)
        cur += (ln + 15) & ~15
    d_out = torch.full((cur,), 0xA5, dtype=torch.uint8, device=dev)
    objs = [(e.sl_off[o], e.geo[o].slice_len, _mask(present[o]), out_off[o]) for o in range(nobj)]
    status, rejected = batch.decode_verified_batch(slicer, torch.from_numpy(bad).to(dev), objs, e.metas, e.leaves, d_out)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    stats = slicer.coder.decode_launch_stats()  # the decode part of the verified call
    assert stats["class_stripes"] + stats["table_stripes"] + stats["generic_stripes"] + stats["jit_stripes"] > 0
    assert rejected == [_mask(c) for c in corrupt]
    for o in range(nobj):
        got = out[out_off[o]:out_off[o] + sizes[o]]
        if o in short:  # 6 verified slices: refused, and its output range untouched
            assert status[o] == _lib.TE_ERR_NOT_ENOUGH_SLICES, o
            assert (got == 0xA5).all(), o
            continue
        assert status[o] == _lib.TE_OK, o
        good = [i for i in present[o] if i not in corrupt[o]]
        assert len(good) >= K
        if o < 48 or o == 48:  # the CPU oracle's decode of the verified slices (one of the large objects)
            assert oracle.slicer_decode(o716, {i: e.slice(o, i).tobytes() for i in good}) == e.blobs[o].tobytes(), o
        assert np.array_equal(got, e.blobs[o]), o
    pad = [out[out_off[o] + sizes[o]:out_off[o] + ((sizes[o] + 15) & ~15)] for o in range(nobj)]
    assert all((p == 0xA5).all() for p in pad)  # nothing past an object's bytes


def merkle_blocks(ln: int) -> int:
    return (ln + 4 + 1 + 8 + 63) // 64


@pytest.fixture(scope="module")
def small(slicer, oracle):
    return Encoded(slicer, oracle, [20_000] * 6, 0xBEEF)


def test_verified_recover(slicer, small):
    dev = torch.device("cuda:0")
    e, nobj = small, 6
    slen = e.geo[0].slice_len
    rng = random.Random(3)
    bad = e.slices.copy()
    lost, present, corrupt = [], [], []
    for o in range(nobj):
        lo = (7 * o + 3) % N
        p = sorted(rng.sample([i for i in range(N) if i != lo], 8))
        c = [p[o % 8]] if o % 2 else []  # a corrupted peer among the 8 present
        for i in c:
            e.slice(o, i, bad)[rng.randrange(slen)] ^= 0x10
        lost.append(lo)
        present.append(p)
        corrupt.append(c)
    objs = [(e.sl_off[o], slen, _mask(present[o]), lost[o], o * slen) for o in range(nobj)]
    d_bad = torch.from_numpy(bad).to(dev)
    truth = np.concatenate([e.slice(o, lost[o]) for o in range(nobj)])
    for altered in (False, True):
        leaves = [list(x) for x in e.leaves]
        if altered:  # objects 1 and 4: leaves[lost] is another slice's
            for o in (1, 4):
                leaves[o][lost[o]] = leaves[o][(lost[o] + 1) % N]
        d_rec = torch.full((nobj * slen,), 0xA5, dtype=torch.uint8, device=dev)
        status, rejected, ok = batch.recover_verified_batch(slicer, d_bad, objs, e.metas, leaves, d_rec)
        assert status == [_lib.TE_OK] * nobj
        assert rejected == [_mask(c) for c in corrupt]
        assert ok == [0 if altered and o in (1, 4) else 1 for o in range(nobj)]
        assert np.array_equal(d_rec.cpu().numpy(), truth)  # rebuilt either way, corrupted peers left out


def test_verified_repair(slicer, small):
    dev = torch.device("cuda:0")
    e, nobj = small, 6
    slen = e.geo[0].slice_len
    plans, offs, blobs, cur, lost = [], [], [], 0, []
    for o in range(nobj):
        lo = (5 * o + 1) % N
        avail = [j for j in range(N) if j != lo]
        p = slicer.repair_plan_from_params(lo, avail, e.sizes[o], e.geo[o].stripe_size)
        m = {}
        for h in avail:
            b = T.extract_repair_data(e.slice(o, h).tobytes(), p, h)
            if b:
                m[h] = cur
                blobs.append(b)
                cur += len(b)
        plans.append(p)
        offs.append(m)
        lost.append(lo)
    d_help = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).to(dev)
    objs = [(plans[o], offs[o], o * slen, e.metas[48 * o:48 * o + 48]) for o in range(nobj)]
    truth = np.concatenate([e.slice(o, lost[o]) for o in range(nobj)])
    for altered in (False, True):
        leaves = [list(x) for x in e.leaves]
        if altered:
            for o in (0, 5):
                leaves[o][lost[o]] = hashlib.sha256(b"other").digest()
        d_rep = torch.full((nobj * slen,), 0xA5, dtype=torch.uint8, device=dev)
        ok = batch.repair_verified_batch(slicer.coder, d_help, objs, leaves, d_rep)
        assert ok == [0 if altered and o in (0, 5) else 1 for o in range(nobj)]
        assert np.array_equal(d_rep.cpu().numpy(), truth)


def test_per_call_host_and_device_hashing(slicer, oracle):
    blob = oracle.splitmix64_bytes(0xCA11, 300_000).tobytes()
    sl = slicer.encode(blob)
    assert len(sl[0]) % 4 == 0
    leaves = [leaf(x) for x in sl]
    chunks = [(i, sl[i]) for i in (0, 2, 3, 7, 8, 11, 14, 17, 19)]
    hit = bytearray(chunks[4][1])
    hit[1234] ^= 0x80
    chunks[4] = (8, bytes(hit))
    got = {}
    try:
        for mode in ("host", "device"):
            batch.set_commit_hashing(mode)
            got[mode] = slicer.decode_verified(chunks, leaves)
    finally:
        batch.set_commit_hashing("auto")
    assert got["host"] == got["device"] == (blob, [8])
