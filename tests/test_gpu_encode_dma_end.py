"""The LDS-DMA encode (tape_amd/csrc/encode_dma.hip, enc_dma_kernel) with the data end at every
position the kernel treats differently: the table of tests/encode_end_cases.py (checked on the CPU
by tests/test_encode_end_cases.py), in every launch form.

An object is two 1 MB stripes, 1,000,000 + r bytes of its own seed, at a source offset with the low
bits src_al; the bytes between the objects are non-zero, so a data-end word that is not masked, or
a later word that is not dropped, shows.  Every comparison is bit-exact against the CPU oracle
(slicer_encode_np, computed once per object and shared by the forms), all 20 slices with the
metadata suffix.  The batch forms write one 0xA5-filled device buffer with 16 guard bytes before,
between and after the objects and compare it whole; the per-call form, whose device output buffer
belongs to the handle, encodes an object of another seed before each case instead.  Every form
asserts from encode_launch_stats() that every stripe ran the LDS-DMA kernel, in a masked and in an
unmasked launch.

The launch form TEC_ENC_SPLIT_BATCH is read once when the library loads: run as a program
(`python tests/test_gpu_encode_dma_end.py child`) this file is the child process of
test_split_batch_in_child and runs the whole table once."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import encode_end_cases as E  # noqa: E402
import tape_amd as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tape_amd import batch  # noqa: E402

pytestmark = pytest.mark.gpu
N = 20
POISON, GUARD = 0xA5, 16
GAP = 0xC3  # the source bytes around the objects
SLICE_LEN = 2 * E.CS + 48
_expected, _o716 = {}, []


def _chunk_index(i):
    return (0, 5, (1 << 40) + 3)[i % 3]


def _data(i, r):
    return O.splitmix64_bytes(0xDA7AE9D ^ (i << 24), E.STRIPE + r)


def _expect(i, r):
    """Oracle slices [20, slice_len] of table object i: computed once, shared, left unchanged."""
    if not _o716:
        _o716.append(O.OracleClay(20, 7, 16))
    if (i, r) not in _expected:
        sl = O.slicer_encode_np(_o716[0], _data(i, r), chunk_index=_chunk_index(i))
        assert sl.shape == (N, SLICE_LEN)
        sl.setflags(write=False)
        _expected[(i, r)] = sl
    return _expected[(i, r)]


class _Table:
    """The whole table as one device batch: source, object descriptors and the expected output."""

    def __init__(self):
        import torch
        self.s = T.Slicer.clay_default()
        self.in_off, at = [], 8
        for r, al in E.CASES:
            at = (at + 3 & ~3) + al
            self.in_off.append(at)
            at += E.STRIPE + r + 8
        host = np.full(at + 16, GAP, np.uint8)
        exp = [np.full(GUARD, POISON, np.uint8)]
        self.out_off, oat = [], GUARD
        for i, (r, al) in enumerate(E.CASES):
            assert int(self.s.geometry(E.STRIPE + r).slice_len) == SLICE_LEN
            host[self.in_off[i]:self.in_off[i] + E.STRIPE + r] = _data(i, r)
            self.out_off.append(oat)
            exp += [_expect(i, r).reshape(-1), np.full(GUARD, POISON, np.uint8)]
            oat += N * SLICE_LEN + GUARD
        self.d_in = torch.from_numpy(host).cuda()
        assert self.d_in.data_ptr() % 4 == 0
        self.d_exp = torch.from_numpy(np.concatenate(exp)).cuda()
        self.objs = batch.encode_descs([(self.in_off[i], E.STRIPE + r, self.out_off[i], _chunk_index(i))
                                        for i, (r, al) in enumerate(E.CASES)])
        # the launch groups, from the addresses: (data end not dword aligned) per stripe
        self.masked = [((self.in_off[i] + st * E.STRIPE) % 4 + ln) % 4 != 0 for i, st, ln, _ in E.stripes()]
        assert self.masked == [m for _, _, _, m in E.stripes()]
        assert all(off % 4 == al for off, (_, al) in zip(self.in_off, E.CASES))

    def run(self, what):
        import torch
        out = torch.full((self.d_exp.numel(),), POISON, dtype=torch.uint8, device="cuda")
        batch.encode_batch(self.s, self.d_in, self.objs, out)
        torch.cuda.synchronize()
        if not torch.equal(out, self.d_exp):
            bad = (out != self.d_exp).nonzero().flatten()
            at = int(bad[0])
            i = max(j for j in range(len(E.CASES)) if self.out_off[j] - GUARD <= at)
            rel = at - self.out_off[i]
            where = "a guard byte" if not 0 <= rel < N * SLICE_LEN else _where(rel)
            pytest.fail(f"{what}: {bad.numel()} wrong bytes, the first at {at}: object {i} {E.end(*E.CASES[i])}: {where}")
        return self.s.coder.encode_launch_stats()


def _where(rel):
    sl, b = divmod(rel, SLICE_LEN)
    if b >= 2 * E.CS:
        return f"slice {sl}, metadata byte {b - 2 * E.CS}"
    st, c = divmod(b, E.CS)
    return f"slice {sl}, stripe {st}, plane {c // E.SC}, column {c % E.SC}"


def _check_stats(st, groups, split):
    """Every stripe on the LDS-DMA kernel: one launch per group (slice length, masked), or a
    level-1 and a level-2 launch per group in the split form."""
    want = dict.fromkeys(st, 0)
    want.update(dma_stripes=2 * len(E.CASES), dma_launches=groups * (2 if split else 1),
                dma_level1_launches=groups if split else 0, dma_level2_launches=groups if split else 0)
    assert st == want, st


@pytest.fixture(scope="module")
def table():
    t = _Table()
    yield t
    _expected.clear()


def test_unsplit_batch(table):
    """One encode_batch of the whole table on the default grid: a workgroup per stripe."""
    assert set(table.masked) == {False, True}
    _check_stats(table.run("unsplit batch"), 2, False)


def test_unsplit_batch_one_workgroup(table, monkeypatch):
    """TEC_ENC_GRID=1: one workgroup walks every task of a launch, so each task's mailbox (wi, ez,
    ex, fix word) follows another task's and every short stripe's first planes are prefetched
    during the task before it (test_one_workgroup_order has the order)."""
    monkeypatch.setenv("TEC_DEBUG_KNOBS", "1")  # measurement knobs are read only with this set
    monkeypatch.setenv("TEC_ENC_GRID", "1")
    _check_stats(table.run("one workgroup"), 2, False)


def test_per_call():
    """Slicer.encode's path (te_slicer_encode) splits a call: seven level-1 workgroups per stripe,
    then the level-2 launch, so the partner word (row ex) and the own word (row ez // 10) are
    substituted by different workgroups.  A launch of each kind per group: the full first stripe
    ends dword aligned, so an object whose last stripe does not has two groups.  The handle's
    device output buffer keeps the call before; an object of another seed is encoded in between, so
    a word the kernel never stores holds that object's bytes."""
    s = T.Slicer.clay_default()
    scrub = (O.splitmix64_bytes(0x5C12B, 2 * E.STRIPE) | 1).tobytes()  # non-zero behind every data end
    seen = set()
    for r, al in E.per_call_cases():
        i = E.CASES.index((r, al))
        s.set_chunk_index(0)
        s.encode(scrub)
        data, exp = _data(i, r), _expect(i, r)
        s.set_chunk_index(_chunk_index(i))
        got = np.frombuffer(b"".join(s.encode(data.tobytes())), np.uint8)
        assert got.size == exp.size
        if not np.array_equal(got, exp.reshape(-1)):
            bad = np.flatnonzero(got != exp.reshape(-1))
            pytest.fail(f"per call: {bad.size} wrong bytes, {E.end(r, al)}: the first in {_where(int(bad[0]))}")
        groups = 1 if r % 4 == 0 else 2
        seen.add(groups)
        st = s.coder.encode_launch_stats()
        want = dict(dict.fromkeys(st, 0), dma_stripes=2, dma_launches=2 * groups, dma_level1_launches=groups,
                    dma_level2_launches=groups)
        assert st == want, (r, st)
    assert seen == {1, 2}


def _child():
    per = int(os.environ.get("TEC_ENC_SPLIT_BATCH", "0"))
    assert per in (2, 3) and os.environ.get("TEC_DEBUG_KNOBS") == "1"
    st = _Table().run(f"split batch, {per} level-1 rows per workgroup")
    assert st["dma_level1_launches"] > 0, st
    _check_stats(st, 2, True)
    print(f"data ends, split batch {per} ok")


@pytest.mark.parametrize("per", [2, 3])
def test_split_batch_in_child(per):
    """TEC_ENC_SPLIT_BATCH=2: level-1 parts of 2, 2, 2 and 1 rows; =3: 3, 3 and 1; z0_limit = 7 cuts
    the last part, and the level-2 rows run in a second launch."""
    env = dict(os.environ, TEC_DEBUG_KNOBS="1", TEC_ENC_SPLIT_BATCH=str(per))
    env.pop("TEC_ENC_GRID", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and f"data ends, split batch {per} ok" in r.stdout, \
        (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    assert sys.argv[1:] == ["child"]
    _child()
