"""The table-driven decode kernel (tape_amd/csrc/decode_stage.hip, dec_stage_kernel<NK, G>) at the
edges of its geometry: every instance NK = 7..10, G = 1, 2, at sub-chunk sizes of 2, 3, 64, 65,
128, 129, 257 and 358 words with and without a tail word, output shares that end inside a word at
the kernel's column edges, and its node-recover programs.  The cases, with the waves per workgroup
and workgroups per stripe each call runs, are in tests/decode_geometry_cases.py (checked on the
CPU by tests/test_decode_geometry_cases.py).

Objects are one stripe; their slices are ClayCoder.encode's chunks (on the GPU, pinned to the
oracle by test_gpu_parity.py) plus the metadata suffix, made once per (profile, sc) and left
unchanged; the decoder takes the chunk size from the slice length.  Outputs are poisoned with
0xA5, laid back to back between guard bytes (offsets are odd after odd lengths) and compared
whole, bit for bit: decode against the original bytes and, for the first object of a call, the
CPU oracle's decode; recover against the encoded slice and, for the first object, the oracle's
encode.  Every call asserts the kernel that ran from te_clay_decode_launch_stats.

Clay(20,8,17), (20,9,18) and (20,10,19) reach the kernel in this process.  Clay(20,7,16) reaches it
only with the class kernels switched off by the engine's measurement knob, which is read once per
process: run as a program (`python tests/test_gpu_decode_table_geometry.py child`) this file is
the child process of test_clay_20_7_16_in_child and runs all of that profile's cases."""
import bisect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import decode_geometry_cases as G  # noqa: E402
import tape_amd as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tape_amd import batch  # noqa: E402
from tape_amd.slicer import ClayParams, EncodingProfile  # noqa: E402

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xA5, 16
N = G.N


def _slicer(params, rotated=True):
    n, k, d = params
    s = T.Slicer.with_rotation(T.ClayCoder(n, k, d)) if rotated else T.Slicer(T.ClayCoder(n, k, d))
    s.profile = EncodingProfile.clay(ClayParams.new(n, k, d))
    return s


_slicers, _objects, _recover_sets = {}, {}, {}


def slicer_of(params):
    if params not in _slicers:
        _slicers[params] = _slicer(params)
        _slicers[params].coder.set_decode_jit("off")  # the hipRTC pattern kernels never take over
    return _slicers[params]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d in (_slicers, _objects, _recover_sets):
        d.clear()


class _Set:
    pass


def _one_stripe_objects(params, sc):
    """The six objects of (profile, sc): seeded bytes, zero-padded to k * cs, encoded by
    ClayCoder.encode, the metadata suffix appended; on the device, shared and left unchanged."""
    import torch
    key = (params, sc)
    if key in _objects:
        return _objects[key]
    n, k, d = params
    s = slicer_of(params)
    coder = s.coder
    alpha = coder.alpha()
    cs = sc * alpha
    assert coder.chunk_size_for(k * cs) == cs and cs // alpha == sc  # checked on the host, before anything runs
    e = _Set()
    e.s, e.cs, e.slen = s, cs, cs + 48
    e.lens = [L for L, _ in G.lengths(k, alpha, sc)]
    for L, natural in G.lengths(k, alpha, sc):
        assert (coder.chunk_size_for(L) == cs) == natural
    e.data, e.metas, e.sl_off = [], [], []
    host = np.empty(len(e.lens) * n * e.slen, np.uint8)
    for i, L in enumerate(e.lens):
        data = O.splitmix64_bytes((sc << 20) ^ (k << 8) ^ i, L)
        padded = np.zeros(k * cs, np.uint8)
        padded[:L] = data
        chunks = coder.encode(padded.tobytes())  # stripe 0 is not rotated: slice j holds chunk j
        meta = T.SliceMetadata.with_profile(L, G.meta_stripe(L), s.profile).to_bytes()
        base = i * n * e.slen
        for j in range(n):
            host[base + j * e.slen:base + j * e.slen + cs] = np.frombuffer(chunks[j], np.uint8)
            host[base + j * e.slen + cs:base + (j + 1) * e.slen] = np.frombuffer(meta, np.uint8)
        e.data.append(data)
        e.metas.append(meta)
        e.sl_off.append(base)
    e.host = host
    e.d_sl = torch.from_numpy(host).cuda()
    e.d_data = [torch.from_numpy(x).cuda() for x in e.data]
    _objects[key] = e
    return e


def _mask(keep):
    return sum(1 << j for j in keep)


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
    raise AssertionError(f"{what}: first mismatch at byte {at} ({where}): got {int(got[at]):#x}, expected {int(exp[at]):#x}")


def _decode_call(params, sc, call, what):
    """One decode_batch call of (object index, survivor set) pairs; returns the launch stats."""
    import torch
    e = _one_stripe_objects(params, sc)
    objs, pieces, starts = [], [], []
    at = GUARD
    for i, keep in call:
        objs.append((e.sl_off[i], e.slen, _mask(keep), at))
        pieces.append(e.d_data[i])
        starts.append(at)
        at += e.lens[i]
    assert {o[3] % 4 for o in objs} == {0, 1, 2, 3}  # output offsets of every alignment
    exp = _guarded(pieces)
    out = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    batch.decode_batch(e.s, e.d_sl, objs, b"".join(e.metas[i] for i, _ in call), out)
    torch.cuda.synchronize()
    _same(out, exp, starts, what)
    # one object (a truncated length under the call's second survivor set) against the CPU
    # oracle's decode of the same chunks
    o = min(7, len(call) - 1)
    i, keep = call[o]
    base = e.sl_off[i]
    ref = O.OracleClay(*params).decode({j: e.host[base + j * e.slen:base + j * e.slen + e.cs].tobytes() for j in keep})
    got = out[starts[o]:starts[o] + e.lens[i]].cpu().numpy().tobytes()
    assert got == ref[:e.lens[i]], f"{what}: object {o} differs from the oracle's decode"
    return e.s.coder.decode_launch_stats()


def _only_table(st, stripes, what):
    assert st["table_stripes"] == stripes and st["table_launches"] == 1, (what, st)
    assert st["class_stripes"] == st["generic_stripes"] == st["jit_launches"] == 0, (what, st)
    assert st["class_launches"] == {} and st["jit_stripes"] == 0, (what, st)


def _only_generic(st, stripes, what):
    assert st["generic_stripes"] == stripes and st["generic_launches"] == 1, (what, st)
    assert st["class_stripes"] == st["table_stripes"] == st["jit_launches"] == 0, (what, st)


def run_decode_case(params, sc, large):
    nw, small_geo, large_geo, _ = G.TABLE_SC[sc]
    assert nw == (sc + 3) // 4
    call = G.table_call(params, sc, large)
    assert (len(call) > G.SMALL_STRIPES) == large
    g, wgs = large_geo if large else small_geo
    what = f"Clay{params} sc {sc} {'large' if large else 'small'} call (G = {g}, {wgs} workgroups per stripe)"
    _only_table(_decode_call(params, sc, call, what), len(call), what)


def run_no_plane_program_case(params, sc):
    """A survivor set without a plane program: the generic kernel, and still the right bytes."""
    for keep in G.NO_PLANE_PROGRAM[params]:
        call = [(i, keep) for i in range(6)]
        what = f"Clay{params} sc {sc} survivors {keep[0]}..{keep[-1]}"
        _only_generic(_decode_call(params, sc, call, what), len(call), what)


# ---- node recover: objects of the slicer's own geometry, encoded by the batched GPU encode -------
def _recover_objects(params, want):
    import torch
    key = (params, want)
    if key in _recover_sets:
        return _recover_sets[key]
    n, k, d = params
    s = slicer_of(params)
    sc, L = G.RECOVER_SC[k][want]
    g = s.geometry(L)
    assert int(g.sub_chunk_size) == sc and (int(g.stripe_size), int(g.num_stripes), sc) == G.slicer_geometry(k, L)
    e = _Set()
    e.s, e.L, e.ns, e.slen, e.sc = s, L, int(g.num_stripes), int(g.slice_len), sc
    gen = torch.Generator(device="cuda")
    gen.manual_seed((want << 8) ^ k)
    e.nobj = 3
    stride = (L + 15) & ~15
    e.d_in = torch.randint(0, 256, (e.nobj * stride,), dtype=torch.uint8, device="cuda", generator=gen)
    e.d_sl = torch.empty(e.nobj * n * e.slen, dtype=torch.uint8, device="cuda")
    batch.encode_batch(s, e.d_in, [(i * stride, L, i * n * e.slen, 0) for i in range(e.nobj)], e.d_sl)
    torch.cuda.synchronize()
    e.meta = T.SliceMetadata.with_profile(L, int(g.stripe_size), s.profile).to_bytes()
    assert e.d_sl[e.slen - 48:e.slen].cpu().numpy().tobytes() == e.meta  # the suffix the encoder wrote
    e.data0 = e.d_in[:L].cpu().numpy()
    _recover_sets[key] = e
    return e


def run_recover_case(params, want, large):
    import torch
    n, k, d = params
    e = _recover_objects(params, want)
    cases = G.recover_cases(params)
    count = -(-G.RECOVER_LARGE_STRIPES // e.ns) if large else len(cases)
    assert (count * e.ns > G.SMALL_STRIPES) == large
    objs, pieces, starts = [], [], []
    at = GUARD
    for j in range(count):
        lost, peers = cases[j % len(cases)]
        i = (j // len(cases)) % e.nobj if j else 0
        base = i * n * e.slen
        objs.append((base, e.slen, _mask(peers), lost, at))
        pieces.append(e.d_sl[base + lost * e.slen:base + (lost + 1) * e.slen])
        starts.append(at)
        at += e.slen
    exp = _guarded(pieces)
    out = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    what = f"Clay{params} recover sc {e.sc} (for {want}), {count * e.ns} stripes"
    batch.recover_batch(e.s, e.d_sl, objs, e.meta * count, out)
    torch.cuda.synchronize()
    _same(out, exp, starts, what)
    ref = O.slicer_encode(O.OracleClay(n, k, d), e.data0.tobytes(), rotated=True, params=e.s.profile.params)[cases[0][0]]
    assert out[starts[0]:starts[0] + e.slen].cpu().numpy().tobytes() == ref, f"{what}: slice differs from the oracle's encode"
    _only_table(e.s.coder.decode_launch_stats(), count * e.ns, what)


IDS = [f"{k}of20" for _, k, _ in G.TABLE_IN_PROCESS]


@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("sc", list(G.TABLE_SC))
@pytest.mark.parametrize("params", G.TABLE_IN_PROCESS, ids=IDS)
def test_decode(params, sc, large):
    run_decode_case(params, sc, large)


@pytest.mark.parametrize("sc", [8, 258, 514, 1430])
@pytest.mark.parametrize("params", sorted(G.NO_PLANE_PROGRAM), ids=["9of20", "10of20"])
def test_decode_set_without_plane_program(params, sc):
    """Clay(20,10,19) from one whole column (slices 10..19), Clay(20,9,18) from slices 11..19."""
    run_no_plane_program_case(params, sc)


@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("want", [10, 258, 514, 1430])
@pytest.mark.parametrize("params", G.TABLE_IN_PROCESS, ids=IDS)
def test_recover(params, want, large):
    run_recover_case(params, want, large)


def _child():
    assert os.environ.get("TEC_DEC_CLASS") == "0" and os.environ.get("TEC_DEBUG_KNOBS") == "1"
    params = G.TABLE_CHILD
    for sc in G.TABLE_SC:
        for large in (False, True):
            run_decode_case(params, sc, large)
    for want in (10, 258, 514, 1430):
        for large in (False, True):
            run_recover_case(params, want, large)
    print("table-kernel geometry of Clay(20,7,16) ok")


def test_clay_20_7_16_in_child():
    env = dict(os.environ, TEC_DEBUG_KNOBS="1", TEC_DEC_CLASS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "table-kernel geometry of Clay(20,7,16) ok" in r.stdout, \
        (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    assert sys.argv[1:] == ["child"]
    _child()
