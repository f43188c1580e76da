"""The generic decode kernel (tape_amd/csrc/gpe.hip, gpe_kernel<MAXE>) at the edges of its geometry:
every instance MAXE = 4, 8, 13, 20 and both LDS launch branches (Clay(20,7,19) needs more than
64 KiB of LDS, Clay(20,5,14) 64,216 B), at sub-chunk sizes of one word, a tail word, exactly one
4-word block, a second block holding one live word, and more; output shares that end inside a
word; Clay(20,7,16) below the 8-byte sub-chunks where the plane-program kernels take over.  The
cases are in tests/decode_geometry_cases.py (checked on the CPU by tests/test_decode_geometry_cases.py).

Objects are one stripe, their slices ClayCoder.encode's chunks (on the GPU, pinned to the oracle
by test_gpu_parity.py) plus the metadata suffix, made once per (profile, sc) and left unchanged.
Both paths into the kernel run: raw ClayCoder.decode and the batched decode_batch, the latter
under the rotated and the identity mapping (the kernel applies the input rotation itself).  One
stripe is never rotated, so objects of three stripes through the Slicer run as well, where the two
mappings differ.  Outputs are poisoned with 0xA5, laid back to back between guard bytes and
compared whole, bit for bit, against the original bytes and, for one object per call, the CPU
oracle's decode.  Every call asserts the kernel that ran from te_clay_decode_launch_stats."""
import bisect
import os
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

_slicers, _objects = {}, {}


def slicers_of(params):
    """(rotated, identity) slicers over one coder."""
    if params not in _slicers:
        n, k, d = params
        coder = T.ClayCoder(n, k, d)
        coder.set_decode_jit("off")
        pair = (T.Slicer.with_rotation(coder), T.Slicer(coder))
        for s in pair:
            s.profile = EncodingProfile.clay(ClayParams.new(n, k, d))
        _slicers[params] = pair
    return _slicers[params]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _slicers.clear()
    _objects.clear()


class _Set:
    pass


def _one_stripe_objects(params, sc):
    import torch
    key = (params, sc)
    if key in _objects:
        return _objects[key]
    n, k, d = params
    s = slicers_of(params)[0]
    coder = s.coder
    alpha = coder.alpha()
    cs = sc * alpha
    assert alpha == G.clay_layout(n, k, d)[3] and coder.chunk_size_for(k * cs) == cs  # on the host, before anything runs
    e = _Set()
    e.cs, e.slen = cs, cs + 48
    e.lens = [L for L, _ in G.lengths(k, alpha, sc)]
    for L, natural in G.lengths(k, alpha, sc):
        assert (coder.chunk_size_for(L) == cs) == natural
    e.data, e.padded, e.metas, e.sl_off = [], [], [], []
    host = np.empty(len(e.lens) * n * e.slen, np.uint8)
    for i, L in enumerate(e.lens):
        data = O.splitmix64_bytes((sc << 20) ^ (n << 12) ^ (k << 6) ^ i, L)
        padded = np.zeros(k * cs, np.uint8)
        padded[:L] = data
        chunks = coder.encode(padded.tobytes())  # stripe 0 is not rotated: slice j holds chunk j
        meta = T.SliceMetadata.with_profile(L, G.meta_stripe(L), s.profile).to_bytes()
        base = i * n * e.slen
        for j in range(n):
            host[base + j * e.slen:base + j * e.slen + cs] = np.frombuffer(chunks[j], np.uint8)
            host[base + j * e.slen + cs:base + (j + 1) * e.slen] = np.frombuffer(meta, np.uint8)
        e.data.append(data)
        e.padded.append(padded)
        e.metas.append(meta)
        e.sl_off.append(base)
    e.host = host
    e.d_sl = torch.from_numpy(host).cuda()
    e.d_data = [torch.from_numpy(x).cuda() for x in e.data]
    _objects[key] = e
    return e


def _mask(keep):
    return sum(1 << j for j in keep)


def _same(got, exp, starts, what):
    import torch
    if torch.equal(got, exp):
        return
    at = int((got != exp).nonzero()[0])
    obj = bisect.bisect_right(starts, at) - 1
    where = f"object {obj} + {at - starts[obj]}" if obj >= 0 else "front guard"
    pytest.fail(f"{what}: first mismatch at byte {at} ({where}): got {int(got[at]):#x}, expected {int(exp[at]):#x}")


def _path(st, what, generic=0, klass=0):
    assert st["generic_stripes"] == generic and st["generic_launches"] == (1 if generic else 0), (what, st)
    assert st["class_stripes"] == klass, (what, st)
    assert st["table_stripes"] == st["jit_launches"] == st["jit_stripes"] == 0, (what, st)


def _batched(s, d_sl, objs, pieces, metas, what):
    """One decode_batch call, outputs back to back between guards; returns (out, starts, stats)."""
    import torch
    starts, at = [], GUARD
    call = []
    for (sl_off, slen, mask), piece in zip(objs, pieces):
        call.append((sl_off, slen, mask, at))
        starts.append(at)
        at += piece.numel()
    g = torch.full((GUARD,), POISON, dtype=torch.uint8, device="cuda")
    exp = torch.cat([g] + pieces + [g])
    out = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    batch.decode_batch(s, d_sl, call, metas, out)
    torch.cuda.synchronize()
    _same(out, exp, starts, what)
    return out, starts, s.coder.decode_launch_stats()


CASES = [(p, sc) for p, (_, _, _, scs) in G.GENERIC.items() for sc in scs]


@pytest.mark.parametrize("params,sc", CASES, ids=[f"{p[0]}-{p[1]}-{p[2]}-sc{sc}" for p, sc in CASES])
def test_generic_kernel(params, sc):
    n, k, d = params
    maxe, lds, over, _ = G.GENERIC[params]
    e = _one_stripe_objects(params, sc)
    call = G.generic_call(params, sc)
    what = f"Clay{params} sc {sc} (gpe_kernel<{maxe}>, {lds} B of LDS)"
    # raw ClayCoder.decode: the full object and a truncated one (its padding decodes as zeros)
    coder = slicers_of(params)[0].coder
    for i, keep in [c for c in call if c[0] < 2]:
        base = e.sl_off[i]
        got = coder.decode([(j, e.host[base + j * e.slen:base + j * e.slen + e.cs].tobytes()) for j in keep])
        assert got == e.padded[i].tobytes(), (what, "raw decode", i, keep)
        _path(coder.decode_launch_stats(), (what, "raw decode", keep), generic=1)
    # decode_batch: every length under every survivor set, rotated and identity mapping
    for s in slicers_of(params):
        objs = [(e.sl_off[i], e.slen, _mask(keep)) for i, keep in call]
        out, starts, st = _batched(s, e.d_sl, objs, [e.d_data[i] for i, _ in call], b"".join(e.metas[i] for i, _ in call),
                                   f"{what} {s.strategy.name}")
        assert {x % 4 for x in starts} == {0, 1, 2, 3}
        _path(st, (what, s.strategy.name), generic=len(call))
    o = 7  # a truncated length under the second (parity-heavy) survivor set, against the oracle
    i, keep = call[o]
    base = e.sl_off[i]
    ref = O.OracleClay(n, k, d).decode({j: e.host[base + j * e.slen:base + j * e.slen + e.cs].tobytes() for j in keep})
    assert out[starts[o]:starts[o] + e.lens[i]].cpu().numpy().tobytes() == ref[:e.lens[i]], (what, "oracle")


def test_clay_20_7_16_leaves_the_generic_kernel_at_sc_8():
    """From 8-byte sub-chunks on, Clay(20,7,16) runs its class kernels (a call of at most 64
    stripes: the per-call ones), not the generic kernel."""
    params = (20, 7, 16)
    e = _one_stripe_objects(params, 8)
    call = G.generic_call(params, 8)
    s = slicers_of(params)[0]
    objs = [(e.sl_off[i], e.slen, _mask(keep)) for i, keep in call]
    _, _, st = _batched(s, e.d_sl, objs, [e.d_data[i] for i, _ in call], b"".join(e.metas[i] for i, _ in call),
                        "Clay(20,7,16) sc 8")
    assert st["generic_stripes"] == st["generic_launches"] == st["jit_launches"] == 0, st
    assert st["class_stripes"] + st["table_stripes"] == len(call), st
    i, keep = call[6]
    base = e.sl_off[i]
    got = s.coder.decode([(j, e.host[base + j * e.slen:base + j * e.slen + e.cs].tobytes()) for j in keep])
    assert got == e.padded[i].tobytes()
    st = s.coder.decode_launch_stats()
    assert st["generic_stripes"] == st["generic_launches"] == st["jit_launches"] == 0, st
    assert st["class_stripes"] + st["table_stripes"] == 1, st


@pytest.mark.parametrize("params", list(G.GENERIC_ROTATED_SC), ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def test_generic_kernel_rotated_stripes(params):
    """Objects of three stripes through the Slicer: stripes 1 and 2 are rotated by 7 and 14 slices
    under the rotated mapping, which the kernel undoes from the job's rotation."""
    import torch
    n, k, d = params
    L = G.GENERIC_ROTATED_LEN
    data = O.splitmix64_bytes(0x707 ^ (n << 12) ^ k, L)
    sets = G.survivor_sets(n, k)
    for s in slicers_of(params):
        rotated = s.strategy == T.MappingStrategy.Rotated
        g = s.geometry(L)
        assert (int(g.num_stripes), int(g.sub_chunk_size)) == (3, G.GENERIC_ROTATED_SC[params])
        slices = s.encode(data.tobytes())
        slen = len(slices[0])
        assert slen == int(g.slice_len)
        d_sl = torch.from_numpy(np.frombuffer(b"".join(slices), np.uint8).copy()).cuda()
        d_data = torch.from_numpy(data).cuda()
        what = f"Clay{params} three stripes {s.strategy.name}"
        out, starts, st = _batched(s, d_sl, [(0, slen, _mask(keep)) for keep in sets], [d_data] * len(sets),
                                   slices[0][-48:] * len(sets), what)
        _path(st, what, generic=3 * len(sets))
        ref = O.slicer_decode(O.OracleClay(n, k, d), {j: slices[j] for j in sets[1]}, rotated=rotated)
        assert out[starts[1]:starts[1] + L].cpu().numpy().tobytes() == ref, (what, "oracle")
