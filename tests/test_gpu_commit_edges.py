"""te_commit_batch_device alone (tape_amd/csrc/commit.hip: leaf_kernel, tree_kernel) at every shape
edge of tests/commit_edge_cases.py, against hashlib and oracle/merkle_oracle.py: leaf hashes, roots
and proofs, bit-exact.

Every run hashes random bytes that start at a non-zero 4-aligned offset of their tensor, with the
objects tight or separated by bytes that belong to no slice; leaf, root and proof each lie between
two poisoned guard bands, which must be intact afterwards, and the input must be unchanged.
A mismatch is reported by position: (slice length, object, slice) for a leaf, (object, slice, level)
for a proof."""
import ctypes as C
import hashlib
from functools import lru_cache

import numpy as np
import pytest
import torch

import commit_edge_cases as E
from oracle import merkle_oracle as MO
from tape_amd import _lib, merkle

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = 0xA5
LEAD = 12  # the slices' offset inside their tensor (torch aligns the tensor itself to 256 bytes)


class Guarded:
    """A device output between two poisoned guard bands."""

    def __init__(self, nbytes):
        self.raw = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.view = self.raw[GUARD:GUARD + nbytes]

    def intact(self):
        r = self.raw.cpu().numpy()
        return bool((r[:GUARD] == POISON).all() and (r[-GUARD:] == POISON).all())

    def untouched(self):
        return bool((self.raw.cpu().numpy() == POISON).all())

    def host(self):
        return self.view.cpu().numpy().tobytes()


@lru_cache(maxsize=None)
def _case(n, nobj, slice_len, height, gap):
    """Random input and its commitments from hashlib and the oracle's hash_pair, built once per shape
    and left unchanged: (tensor bytes, obj_stride, leaves, roots, proofs), the last three as the
    device lays them out."""
    stride = n * slice_len + (8 if gap else 0)
    rng = np.random.default_rng([n, nobj, slice_len, height, int(gap)])
    host = rng.integers(0, 256, LEAD + nobj * stride + 8, dtype=np.uint8)
    raw = host.tobytes()
    leaves, roots, proofs = [], [], []
    for o in range(nobj):
        at = LEAD + o * stride
        lv = [hashlib.sha256(b"LEAF" + raw[at + i * slice_len:at + (i + 1) * slice_len]).digest() for i in range(n)]
        layers = E.tree_layers(lv, height)  # once per object, not once per proof
        leaves += lv
        roots.append(layers[height][0])
        proofs += [b"".join(E.proof_from_layers(layers, i)) for i in range(n)]
    return host, stride, b"".join(leaves), b"".join(roots), b"".join(proofs)


def _first_diff(got, want, unit=32):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    assert g.size == w.size
    bad = np.flatnonzero(g != w)
    return None if bad.size == 0 else int(bad[0]) // unit


def _run(n, nobj, slice_len, height, gap, want_roots=True, want_proofs=True):
    """One commit_batch call over _case's input; checks the guards and the input, returns the three
    guarded outputs (all three are allocated whether or not they are passed)."""
    host, stride = _case(n, nobj, slice_len, height, gap)[:2]
    dev = torch.from_numpy(host.copy()).cuda()
    leaf, root, proof = Guarded(nobj * n * 32), Guarded(nobj * 32), Guarded(nobj * n * max(height, 1) * 32)
    assert dev.data_ptr() % 4 == 0 and LEAD % 4 == 0 and LEAD
    merkle.commit_batch(dev[LEAD:], stride, slice_len, n, nobj, leaf.view, root.view if want_roots else None,
                        proof.view if want_proofs else None, height)
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == host.tobytes(), "the input changed"
    for name, g in (("leaf", leaf), ("root", root), ("proof", proof)):
        assert g.intact(), f"a store outside the {name} buffer"
    return leaf, root, proof


def _check_all(n, nobj, slice_len, height, gap):
    """Leaves, roots and proofs of one full call against the reference, first mismatch by position."""
    _, _, leaves, roots, proofs = _case(n, nobj, slice_len, height, gap)
    leaf, root, proof = _run(n, nobj, slice_len, height, gap)
    bad = _first_diff(leaf.host(), leaves)
    assert bad is None, f"leaf hash differs: length {slice_len}, object {bad // n}, slice {bad % n}"
    bad = _first_diff(root.host(), roots)
    assert bad is None, f"root differs: n {n}, height {height}, object {bad}"
    bad = _first_diff(proof.host(), proofs)
    assert bad is None, (f"proof differs: n {n}, height {height}, object {bad // (n * height)}, "
                         f"slice {bad // height % n}, level {bad % height}")
    return leaf, root, proof


# ---- leaf_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_len", E.SHORT)
def test_short_lengths(slice_len):
    n, nobj = E.LEAF_SHAPE
    _check_all(n, nobj, slice_len, E.tree_height(n), gap=E.gapped(slice_len // 4))


@pytest.mark.parametrize("slice_len", [L for below in sorted(E.SPLIT) for L in E.SPLIT[below]])
def test_lengths_around_the_launch_split(slice_len):
    n, nobj = E.LEAF_SHAPE
    _check_all(n, nobj, slice_len, E.tree_height(n), gap=E.gapped(slice_len // 4))


@pytest.mark.parametrize("slice_len", E.STREAM_LENGTHS)
@pytest.mark.parametrize("index", range(len(E.STREAMS)), ids=[f"{n}x{nobj}" for n, nobj in E.STREAMS])
def test_stream_counts(index, slice_len):
    n, nobj = E.STREAMS[index]
    _check_all(n, nobj, slice_len, E.tree_height(n), gap=E.gapped(index))


# ---- tree_kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nobj", E.TREE_NOBJ)
@pytest.mark.parametrize("n,height", E.TREE)
def test_tree_shapes(n, height, nobj):
    gap = E.gapped(n + nobj)
    leaf, root, proof = _check_all(n, nobj, E.TREE_SLICE_LEN, height, gap)
    # every proof the device wrote walks from its leaf to the device's root
    lb, rb, pb = leaf.host(), root.host(), proof.host()
    for o in range(nobj):
        r = rb[o * 32:(o + 1) * 32]
        for i in range(n):
            at = (o * n + i) * height * 32
            p = [pb[at + l * 32:at + (l + 1) * 32] for l in range(height)]
            assert MO.verify_leaf_hash(lb[(o * n + i) * 32:(o * n + i + 1) * 32], r, p, i, height), (o, i)


@pytest.mark.parametrize("nobj", E.TREE_NOBJ)
@pytest.mark.parametrize("n,height", E.TREE)
def test_root_check_kernel_accepts_the_commitments(n, height, nobj):
    """The leaves and roots this call wrote, fed to te_roots_check_device as leaves and expected
    roots: the two tree walks, which share no code, agree on every object."""
    leaf, root, _ = _run(n, nobj, E.TREE_SLICE_LEN, height, E.gapped(n + nobj), want_proofs=False)
    ok = torch.full((nobj,), -1, dtype=torch.int32, device="cuda")
    merkle.roots_check_device(leaf.view, n, nobj, root.view, ok, expected_leaves=leaf.view, height=height)
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1] * nobj


@pytest.mark.parametrize("n,height,nobj", E.OPTIONAL)
def test_optional_outputs(n, height, nobj):
    gap = E.gapped(n + nobj)
    _, _, leaves, roots, _ = _case(n, nobj, E.TREE_SLICE_LEN, height, gap)
    # roots without proofs (the snapshot codec's call)
    leaf, root, proof = _run(n, nobj, E.TREE_SLICE_LEN, height, gap, want_proofs=False)
    assert leaf.host() == leaves and root.host() == roots
    assert proof.untouched()
    # leaves only: the height is not looked at
    for h in (height, 0, 33):
        host, stride = _case(n, nobj, E.TREE_SLICE_LEN, height, gap)[:2]
        dev = torch.from_numpy(host.copy()).cuda()
        leaf, root, proof = Guarded(nobj * n * 32), Guarded(nobj * 32), Guarded(nobj * n * 33 * 32)
        merkle.commit_batch(dev[LEAD:], stride, E.TREE_SLICE_LEN, n, nobj, leaf.view, None, None, h)
        torch.cuda.synchronize()
        assert leaf.intact() and leaf.host() == leaves, h
        assert root.untouched() and proof.untouched(), h


# ---- argument checks ------------------------------------------------------------------------------
def _call(a, dev, leaf, root, proof):
    p = lambda on, t: C.c_void_p(t.data_ptr()) if on else None  # noqa: E731
    return _lib.lib.te_commit_batch_device(C.c_void_p(dev.data_ptr() + LEAD + a["base_shift"]), a["obj_stride"],
                                           a["slice_len"], a["n"], a["nobj"], a["height"], p(a["leaf"], leaf.view),
                                           p(a["roots"], root.view), p(a["proofs"], proof.view), None)


def _error_buffers(a):
    n, nobj, h = max(a["n"], 1), max(a["nobj"], 1), max(a["height"], 1)
    dev = torch.from_numpy(np.random.default_rng(7).integers(0, 256, LEAD + nobj * a["obj_stride"] + 16, dtype=np.uint8)).cuda()
    return dev, Guarded(nobj * n * 32), Guarded(nobj * 32), Guarded(nobj * n * h * 32)


@pytest.mark.parametrize("name,over,code", E.ERRORS, ids=[e[0] for e in E.ERRORS])
def test_argument_errors_write_nothing(name, over, code):
    a = E.error_case(over)
    dev, leaf, root, proof = _error_buffers(a)
    assert _call(a, dev, leaf, root, proof) == code
    torch.cuda.synchronize()
    assert leaf.untouched() and root.untouched() and proof.untouched()
    if code == E.INVALID_ARG:
        from tape_amd.slicer import EngineError
        with pytest.raises(EngineError) as e:  # the Python mirror raises what the engine's calls raise
            merkle.commit_batch(dev[LEAD + a["base_shift"]:], a["obj_stride"], a["slice_len"], a["n"], a["nobj"],
                                leaf.view if a["leaf"] else None, root.view if a["roots"] else None,
                                proof.view if a["proofs"] else None, a["height"])
        assert e.value.code == E.INVALID_ARG
    else:
        with pytest.raises(merkle.MerkleError) as e:
            merkle.commit_batch(dev[LEAD:], a["obj_stride"], a["slice_len"], a["n"], a["nobj"], leaf.view,
                                root.view if a["roots"] else None, proof.view if a["proofs"] else None, a["height"])
        assert e.value.variant == "TreeFull"
    torch.cuda.synchronize()
    assert leaf.untouched() and root.untouched() and proof.untouched()


def test_no_objects_is_ok_and_writes_nothing():
    a = E.error_case(dict(nobj=0))
    dev, leaf, root, proof = _error_buffers(a)
    assert _call(a, dev, leaf, root, proof) == E.OK
    torch.cuda.synchronize()
    assert leaf.untouched() and root.untouched() and proof.untouched()
