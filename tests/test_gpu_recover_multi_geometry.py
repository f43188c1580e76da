"""The multi-output rebuild kernel (tape_amd/csrc/recover_multi.hip, recover_multi_kernel<NK, G>) at
the edges of its geometry: every instance NK = 7..10, G = 1, 2, at every kind of row the recover
entry points can give it (2 and 3 words, the widest one-stripe rows with and without a tail word,
three stripes with a short last one, the production row of each profile in small and large calls),
every named lost set of every profile in both layouts, and output offsets of every alignment.  The
cases, with the waves per workgroup, workgroups per stripe, launches, jobs and passes each call
must run, are in tests/recover_multi_geometry_cases.py (checked on the CPU by
tests/test_recover_multi_geometry_cases.py, which also shows why rows of 64 to 129 words cannot
reach this kernel).

The expected bytes are the CPU oracle's Slicer::encode of the object, never the library's.  Inputs
are made once per (profile, row, layout) and left unchanged; the slices a call may not read are
poisoned in the copy it is given.  Every call writes into a buffer pre-filled with 0xA5, guard
bands between the objects, and the whole buffer is compared bit for bit with the expected image: a
byte stored outside a rebuilt slice, or left unwritten inside one, fails with the first
mismatching offset.  Every call asserts its path, launches, stripes, rows, passes and jobs from
te_clay_recover_multi_launch_stats (jobs <= 64 pins G = 1, more pins G = min(2, waves)), and from
te_clay_decode_launch_stats that no table, generic or class kernel ran."""
import numpy as np
import pytest

import recover_multi_geometry_cases as R
import tape_amd as T
from tape_amd import batch
from tape_amd.slicer import ClayParams, EncodingProfile

pytestmark = pytest.mark.gpu
N, POISON, ABSENT, GUARD = R.N, 0xA5, 0x3C, R.GUARD
IDS = [f"{k}of20" for _, k, _ in R.PROFILES]
LAYOUTS = pytest.mark.parametrize("rotated", [False, True], ids=["identity", "rotated"])

_slicers, _slices, _inputs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d in (_slicers, _slices, _inputs):
        d.clear()


def _slicer(params, rotated):
    key = (params, rotated)
    if key not in _slicers:
        n, k, d = params
        s = T.Slicer.with_rotation(T.ClayCoder(n, k, d)) if rotated else T.Slicer(T.ClayCoder(n, k, d))
        s.profile = EncodingProfile.clay(ClayParams.new(n, k, d))
        _slicers[key] = s
    return _slicers[key]


def _oracle_slices(oracle, params, row, rotated):
    """(n, slice_len) of the oracle's encode of the row's object; made once, never written."""
    key = (params, row, rotated)
    if key not in _slices:
        n, k, d = params
        sc, length, ns, _ = R.rows(k)[row]
        s = _slicer(params, rotated)
        g = s.geometry(length)
        assert (int(g.sub_chunk_size), int(g.num_stripes)) == (sc, ns)  # once more, before anything runs
        data = oracle.splitmix64_bytes(0x726D67 ^ (k << 24) ^ length ^ int(rotated), length)
        sl = oracle.slicer_encode(oracle.OracleClay(n, k, d), data.tobytes(), rotated=rotated, params=s.profile.params)
        arr = np.stack([np.frombuffer(x, np.uint8) for x in sl])
        assert arr.shape == (n, int(g.slice_len)) == (n, ns * sc * R.ALPHA + R.META)
        arr.setflags(write=False)
        _slices[key] = arr
    return _slices[key]


def _input(oracle, params, row, rotated, name):
    """The object's slices on the device with every slice the set does not list as available
    poisoned; one resident copy per (object, set), shared by the descriptors that name it."""
    import torch
    key = (params, row, rotated, name)
    if key not in _inputs:
        sl = _oracle_slices(oracle, params, row, rotated)
        avail = R.lost_sets(params[1])[name][0]
        img = np.full_like(sl, ABSENT)
        img[avail] = sl[avail]
        _inputs[key] = torch.from_numpy(img.reshape(-1)).cuda()
    return _inputs[key]


def _same(got, exp, starts, what):
    import torch
    if torch.equal(got, exp):
        return
    at = int((got != exp).nonzero()[0])
    obj = max([i for i, s in enumerate(starts) if s <= at], default=-1)
    where = f"object {obj} + {at - starts[obj]}" if obj >= 0 else "front guard"
    raise AssertionError(f"{what}: first mismatch at byte {at} of {exp.numel()} ({where}): got {int(got[at]):#x}, "
                         f"expected {int(exp[at]):#x}")


def _run(oracle, params, call, rotated, what, misalign=0):
    """One te_recover_multi_batch_device call over call = [(row, lost set)]; asserts the bytes and
    the launch stats the case table gives."""
    import torch
    n, k, d = params
    s = _slicer(params, rotated)
    sets = R.lost_sets(k)
    bufs, base = {}, {}
    for row, name in call:  # one resident copy per distinct (row, set)
        if (row, name) not in bufs:
            base[(row, name)] = sum(b.numel() for b in bufs.values())
            bufs[(row, name)] = _input(oracle, params, row, rotated, name)
    d_in = torch.cat(list(bufs.values())) if len(bufs) > 1 else next(iter(bufs.values()))
    descs, metas, pieces, starts = [], b"", [np.full(GUARD + misalign, POISON, np.uint8)], []
    at = GUARD + misalign
    for i, (row, name) in enumerate(call):
        sl = _oracle_slices(oracle, params, row, rotated)
        avail, lost, _ = sets[name]
        slen = sl.shape[1]
        descs.append((base[(row, name)], slen, R.mask(avail), R.mask(lost), at))
        metas += sl[avail[0]][-48:].tobytes()
        starts.append(at)
        gap = GUARD + (1 if misalign else 0)  # the next object's offset moves on by one modulo 4
        pieces += [sl[j] for j in sorted(lost)] + [np.full(gap, POISON, np.uint8)]
        at += len(lost) * slen + gap
    if misalign:
        assert len({o[4] % 4 for o in descs}) == min(4, len(descs)) and descs[0][4] % 4 == misalign
    exp = torch.from_numpy(np.concatenate(pieces)).cuda()
    assert exp.numel() == at
    out = torch.full((at,), POISON, dtype=torch.uint8, device="cuda")
    batch.recover_multi_batch(s, d_in, descs, metas, out)
    torch.cuda.synchronize()
    _same(out, exp, starts, what)
    st = batch.recover_multi_launch_stats(s.coder)
    want = R.call_stats(k, call, rotated)
    for key, v in want.items():
        assert st[key] == v, (what, key, st, want)
    dl = s.coder.decode_launch_stats()
    assert dl["table_launches"] == 0 and dl["generic_launches"] == 0 and not dl["class_launches"], (what, dl)
    assert dl["table_stripes"] == dl["generic_stripes"] == dl["class_stripes"] == 0, (what, dl)
    return st


ROWS = ["smallest", "tail3", "widest_tail", "widest_whole", "stripe3", "production"]


@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("params", R.PROFILES, ids=IDS)
def test_instance_and_row(oracle, params, row, large):
    """Every (NK, G, row): the one-pass pairs, the across-columns pair first, rotated layout (the
    production and three-stripe objects' later stripes hold other nodes in the lost slices)."""
    k = params[1]
    call = R.geometry_call(k, row, large)
    sc = R.rows(k)[row][0]
    g, wgs = R.GEOMETRY[k][row][large]
    what = f"Clay{params} {row} (sc {sc}) {'large' if large else 'small'} call: G = {g}, {wgs} workgroups per stripe"
    st = _run(oracle, params, call, True, what)
    assert (st["jobs"] > R.SMALL_JOBS) == large, (what, st)  # pins G: the stats do not carry it
    assert R.launch(sc, st["jobs"]) == (g, wgs) and st["multi_launches"] == 1


@LAYOUTS
@pytest.mark.parametrize("params,name", [(p, nm) for p in R.PROFILES for nm in R.lost_sets(p[1])],
                         ids=lambda v: f"{v[1]}of20" if isinstance(v, tuple) else v)
def test_lost_set(oracle, params, name, rotated):
    """Every named lost set at sc = 10 and at the widest tail row in one call (two chunk sizes: two
    launches); rotated, the three-stripe object with a short last stripe as well."""
    call = [(row, name) for row in R.lost_set_call(rotated)]
    st = _run(oracle, params, call, rotated, f"Clay{params} {name} {'rotated' if rotated else 'identity'}")
    assert st["jobs"] <= R.SMALL_JOBS and st["multi_launches"] == len(call) >= 2, st
    assert (st["split_stripes"] > 0) == (st["passes"] > 1), st


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
@pytest.mark.parametrize("params", R.PROFILES, ids=IDS)
def test_output_offsets(oracle, params, misalign):
    """Output offsets of every alignment at sc = 10 and the widest rows with and without a tail
    word: a slice length is a multiple of 4, so the gaps move each object on by one."""
    call = [(row, nm) for nm in ("data_and_parity_across", "column0_pair") for row in R.OFFSET_ROWS]
    _run(oracle, params, call, True, f"Clay{params} out_off % 4 == {misalign}", misalign=misalign)
