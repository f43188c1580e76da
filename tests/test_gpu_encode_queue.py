"""The LDS-DMA encode's stripe queue (tape_amd/csrc/encode_dma.hip): persistent workgroups that draw
stripes from a counter and prefetch the next stripe's first planes during the current one's last.

Every case goes through batch.encode_batch (the device batch path) unless it says otherwise, and
compares all 20 slices, metadata suffix included, byte for byte with the oracle.  The objects are
1 MB-stripe objects (sub-chunk 1,430 B), so every stripe runs the LDS-DMA kernel.  With
TEC_DEBUG_KNOBS=1 TEC_ENC_GRID=g a launch has g workgroups, so a handful of stripes already loops.
"""
import numpy as np
import pytest

import tape_amd as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
N = 20
MiB = 1024 * 1024
_expected = {}


@pytest.fixture(scope="module")
def o716(oracle):
    return oracle.OracleClay(20, 7, 16)


def _data(oracle, seed, ln):
    return oracle.splitmix64_bytes(0xE9C0DE ^ seed, ln)


def _expect(oracle, o716, seed, ln):
    """Oracle slices [20, slice_len] of object (seed, ln), chunk_index 0: computed once, shared."""
    if (seed, ln) not in _expected:
        _expected[(seed, ln)] = oracle.slicer_encode_np(o716, _data(oracle, seed, ln))
    return _expected[(seed, ln)]


def _grid(monkeypatch, g):
    monkeypatch.setenv("TEC_DEBUG_KNOBS", "1")  # measurement knobs are read only with this set
    monkeypatch.setenv("TEC_ENC_GRID", str(g))


def _encode_check(oracle, o716, sizes, gap=0, repeat=1):
    """encode_batch of objects (seed i, sizes[i]) laid gap bytes apart; every slice against the oracle,
    and every stripe of the call on the LDS-DMA kernel (te_clay_encode_launch_stats): one unsplit
    launch per (slice length, data end dword aligned or not).  Returns those launch groups."""
    from tape_amd import batch
    s = T.Slicer.clay_default()
    offs, outs, cur, ocur = [], [], 0, 0
    for ln in sizes:
        offs.append(cur)
        cur += ln + gap
        cur += cur & 1  # even addresses only: a stripe at an odd one runs the generic kernel
        outs.append(ocur)
        ocur += N * s.geometry(ln).slice_len
    host = np.zeros(cur, np.uint8)
    for i, ln in enumerate(sizes):
        host[offs[i]:offs[i] + ln] = _data(oracle, i, ln)
    d_in = torch.from_numpy(host).to("cuda:0")
    d_out = torch.empty(ocur, dtype=torch.uint8, device="cuda:0")
    assert d_in.data_ptr() % 4 == 0
    groups, stripes = set(), 0
    for i, ln in enumerate(sizes):
        g = s.geometry(ln)
        for st in range(g.num_stripes):
            a, src_len = offs[i] + st * g.stripe_size, min(g.stripe_size, ln - st * g.stripe_size)
            assert a % 2 == 0
            groups.add((g.slice_len, (a % 4 + src_len) % 4 != 0))
            stripes += 1
    for _ in range(repeat):
        d_out.fill_(0xA5)
        batch.encode_batch(s, d_in, [(offs[i], sizes[i], outs[i], 0) for i in range(len(sizes))], d_out)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        for i, ln in enumerate(sizes):
            exp = _expect(oracle, o716, i, ln)
            assert np.array_equal(out[outs[i]:outs[i] + exp.size].reshape(N, -1), exp), (i, ln)
        st = s.coder.encode_launch_stats()
        assert st["dma_stripes"] == stripes and st["dma_launches"] == len(groups), st
        assert st["dma_level1_launches"] == st["dma_level2_launches"] == 0, st
        assert st["stage_launches"] == st["generic_launches"] == st["stage_stripes"] == st["generic_stripes"] == 0, st
    return groups


@pytest.mark.parametrize("sizes", [
    [4_000_000] * 3,   # 12 stripes on 3 workgroups: 4 tasks each
    [3_000_000],       # 3 stripes: tasks == workgroups
    [4_000_000],       # 4 stripes: one more than the workgroups
    [MiB],             # 2 stripes: fewer tasks than workgroups
], ids=["12", "3", "4", "2"])
def test_grid3(oracle, o716, monkeypatch, sizes):
    _grid(monkeypatch, 3)
    _encode_check(oracle, o716, sizes)


@pytest.mark.parametrize("g", [1, 2])
def test_full_and_short_stripes_alternate(oracle, o716, monkeypatch, g):
    """1 MiB objects: stripes of 1,000,000 B and 48,576 B (the two-stripe shape that hung the r04
    row-piece kernel).  One workgroup walks full, short, full, ...: a prefetch from a full stripe
    into a short one and from a short one into a full one; two workgroups split them by kind."""
    _grid(monkeypatch, g)
    _encode_check(oracle, o716, [MiB] * 3)


@pytest.mark.parametrize("g", [1, 3])
def test_masked_and_unmasked_launches(oracle, o716, monkeypatch, g):
    """Dword-aligned and unaligned data ends get a launch (and a queue counter) each in one call.
    The 2-byte gap (3 after an odd length) leaves later objects 2-aligned only (odd offsets do not run
    the LDS-DMA kernel)."""
    _grid(monkeypatch, g)
    groups = _encode_check(oracle, o716, [4 * MiB, MiB, 1_000_001, 2_000_003, 1_999_998], gap=2)
    # the two-stripe objects share a slice length and have stripes ending dword aligned and not: a
    # launch of each kind
    two = T.Slicer.clay_default().geometry(MiB).slice_len
    assert {m for sl, m in groups if sl == two} == {False, True}


def test_last_task_without_successor(oracle, o716, monkeypatch):
    """One workgroup runs an object's five stripes in order; after the fifth the queue is empty."""
    _grid(monkeypatch, 1)
    _encode_check(oracle, o716, [4 * MiB])


def test_keep_filter(oracle, o716, monkeypatch):
    """te_recover_batch_device re-encodes the stripes whose lost shard is a parity chunk with a keep
    filter (store_mask), the others not at all: with the default rotation an object's stripes are a
    mix of both.  The recovered slice equals the oracle's."""
    from tape_amd import batch
    _grid(monkeypatch, 2)
    s = T.Slicer.clay_default()
    sizes = [4 * MiB, MiB, 4_000_000]
    lost = [9, 17, 12]
    parts, objs, metas, exp, cur, ocur = [], [], b"", [], 0, 0
    for i, ln in enumerate(sizes):
        e = _expect(oracle, o716, i, ln)
        slen = e.shape[1]
        parts.append(e.reshape(-1))
        avail = [(lost[i] + j) % N for j in range(1, 8)]
        objs.append((cur, slen, sum(1 << a for a in avail), lost[i], ocur))
        exp.append(e[lost[i]])
        metas += e[0][-48:].tobytes()
        cur += e.size
        ocur += slen
    d_sl = torch.from_numpy(np.concatenate(parts)).to("cuda:0")
    d_rec = torch.full((ocur,), 0xA5, dtype=torch.uint8, device="cuda:0")
    batch.recover_batch(s, d_sl, objs, metas, d_rec)
    torch.cuda.synchronize()
    assert np.array_equal(d_rec.cpu().numpy(), np.concatenate(exp))


@pytest.mark.parametrize("g", [None, "cu", "64"])
def test_counter_rezeroed_every_call(oracle, o716, monkeypatch, g):
    """300 x 1 MiB objects are 600 stripes, more than the resident workgroups of any gfx950 part;
    three calls on one handle over a poisoned output.  With no knobs, and with "cu", a launch has two
    workgroups per CU and draws the other stripes from its counter; with 64 workgroups it draws
    most of them.  A counter left over from the call before would hand out no stripe."""
    if g is not None:
        _grid(monkeypatch, g)
    from tape_amd import batch
    nobj = 300
    s = T.Slicer.clay_default()
    exp = _expect(oracle, o716, 0, MiB)
    per = exp.size
    d_in = torch.from_numpy(np.tile(_data(oracle, 0, MiB), nobj)).to("cuda:0")
    d_exp = torch.from_numpy(exp.reshape(-1)).to("cuda:0")
    d_out = torch.empty(nobj * per, dtype=torch.uint8, device="cuda:0")
    descs = batch.encode_descs([(i * MiB, MiB, i * per, 0) for i in range(nobj)])
    for _ in range(3):
        d_out.fill_(0xA5)
        batch.encode_batch(s, d_in, descs, d_out)
        torch.cuda.synchronize()
        assert bool((d_out.view(nobj, per) == d_exp[None, :]).all())


@pytest.mark.parametrize("g", [None, 2])
def test_per_call_path(oracle, o716, monkeypatch, g):
    """te_slicer_encode (at most 512 stripes: seven level-1 tasks per stripe, then the level-2
    launch), as it runs by default and with two workgroups per launch."""
    if g is not None:
        _grid(monkeypatch, g)
    s = T.Slicer.clay_default()
    for seed, ln in ((0, MiB), (1, 1_000_001)):
        got = s.encode(_data(oracle, seed, ln).tobytes())
        exp = _expect(oracle, o716, seed, ln)
        assert [bytes(x) for x in got] == [e.tobytes() for e in exp], ln
