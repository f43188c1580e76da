"""te_roots_check_device alone, on random leaf hashes, against oracle/merkle_oracle.py: the
observed roots, the verdicts and the leaf masks, bit-exact.

Shapes: no pair at the leaf level (n = 1), an odd layer at each level (3, 20, 33), a full wave (64),
the 32-lane crossing (32, 33), the long empty-root chain (height 32); 65 objects leave the grid's
last workgroup ragged whatever the objects-per-workgroup choice."""
import numpy as np
import pytest
import torch

from tape_amd import merkle

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 5), (2, 1), (3, 5), (20, 5), (32, 5), (33, 6), (64, 6), (20, 32)]
NOBJ = [1, 3, 65]
GUARD = 64
POISON = 0xA5
_CACHE = {}


def _case(n, height, nobj):
    """Random leaves and the oracle's roots, built once per shape and left unchanged."""
    key = (n, height, nobj)
    if key not in _CACHE:
        from oracle import merkle_oracle as MO
        rng = np.random.default_rng(n * 1000 + height * 100 + nobj)
        leaves = rng.integers(0, 256, nobj * n * 32, dtype=np.uint8)
        lb = leaves.tobytes()
        roots = b"".join(MO.root_from_leaf_hashes([lb[(o * n + i) * 32:(o * n + i + 1) * 32] for i in range(n)], height)
                         for o in range(nobj))
        _CACHE[key] = (leaves, np.frombuffer(roots, np.uint8))
    return _CACHE[key]


class Guarded:
    """A device output between two poisoned guard bands."""

    def __init__(self, nbytes, dtype):
        self.raw = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.view = self.raw[GUARD:GUARD + nbytes].view(dtype)

    def intact(self):
        r = self.raw.cpu().numpy()
        return bool((r[:GUARD] == POISON).all() and (r[-GUARD:] == POISON).all())

    def host(self):
        return self.view.cpu().numpy()


def _run(n, height, nobj, leaves, xroots, xleaves=None, want_roots=True, want_mask=True):
    d_leaf = torch.from_numpy(leaves.copy()).cuda()
    d_xroot = torch.from_numpy(xroots.copy()).cuda()
    d_xleaf = torch.from_numpy(xleaves.copy()).cuda() if xleaves is not None else None
    roots = Guarded(nobj * 32, torch.uint8) if want_roots else None
    ok = Guarded(nobj * 4, torch.int32)
    mask = Guarded(nobj * 8, torch.int64) if want_mask else None
    merkle.roots_check_device(d_leaf, n, nobj, d_xroot, ok.view, expected_leaves=d_xleaf,
                              roots=roots.view if roots else None, bad_leaf_mask=mask.view if mask else None,
                              height=height)
    torch.cuda.synchronize()
    assert d_leaf.cpu().numpy().tobytes() == leaves.tobytes()  # inputs untouched
    for g in (roots, ok, mask):
        assert g is None or g.intact()
    return roots, ok, mask


@pytest.mark.parametrize("nobj", NOBJ)
@pytest.mark.parametrize("n,height", SHAPES)
def test_roots_match_oracle(n, height, nobj):
    leaves, want = _case(n, height, nobj)
    roots, ok, mask = _run(n, height, nobj, leaves, want, xleaves=leaves)
    assert roots.host().tobytes() == want.tobytes()
    assert ok.host().tolist() == [1] * nobj
    assert mask.host().tolist() == [0] * nobj


@pytest.mark.parametrize("nobj", NOBJ)
@pytest.mark.parametrize("n,height", SHAPES)
def test_one_expected_leaf_altered(n, height, nobj):
    leaves, want = _case(n, height, nobj)
    obj, leaf = nobj - 1 - (nobj // 3), n - 1 - (n // 3)
    xleaves = leaves.copy()
    xleaves[(obj * n + leaf) * 32 + 31 - (leaf % 32)] ^= 0x10
    roots, ok, mask = _run(n, height, nobj, leaves, want, xleaves=xleaves)
    assert roots.host().tobytes() == want.tobytes()
    assert ok.host().tolist() == [1] * nobj  # the expected roots were left true
    got = [int(m) & (2 ** 64 - 1) for m in mask.host().tolist()]
    assert got == [(1 << leaf) if o == obj else 0 for o in range(nobj)]


@pytest.mark.parametrize("nobj", NOBJ)
@pytest.mark.parametrize("n,height", SHAPES)
def test_one_expected_root_altered(n, height, nobj):
    leaves, want = _case(n, height, nobj)
    obj = nobj // 2
    xroots = want.copy()
    xroots[obj * 32 + 17] ^= 0x01
    roots, ok, mask = _run(n, height, nobj, leaves, xroots, xleaves=leaves)
    assert roots.host().tobytes() == want.tobytes()  # the observed root, not the expected one
    assert ok.host().tolist() == [0 if o == obj else 1 for o in range(nobj)]
    assert mask.host().tolist() == [0] * nobj


@pytest.mark.parametrize("n,height,nobj", [(20, 5, 65), (64, 6, 3), (1, 1, 1)])
def test_optional_outputs_null(n, height, nobj):
    leaves, want = _case(n, height, nobj)
    # no roots, no expected leaves, no mask
    roots, ok, mask = _run(n, height, nobj, leaves, want, want_roots=False, want_mask=False)
    assert ok.host().tolist() == [1] * nobj
    # a mask buffer without expected leaves is not written
    roots, ok, mask = _run(n, height, nobj, leaves, want, want_roots=False, want_mask=True)
    assert ok.host().tolist() == [1] * nobj
    assert (mask.raw.cpu().numpy() == POISON).all()
    # expected leaves without a mask buffer
    roots, ok, mask = _run(n, height, nobj, leaves, want, xleaves=leaves, want_mask=False)
    assert roots.host().tobytes() == want.tobytes() and ok.host().tolist() == [1] * nobj
