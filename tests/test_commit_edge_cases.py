"""The case tables of the commit kernels' edge tests (tests/commit_edge_cases.py) hold what their GPU
tests rely on, checked by enumeration against the constants in the source text; the layer walk the
GPU test uses as its reference agrees with oracle/merkle_oracle.py on every tree shape; and the
argument checks of te_commit_batch_device that are decided before any device call.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import commit_edge_cases as E
from oracle import merkle_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDUES = set(range(0, 64, 4))


def _src(name):
    with open(os.path.join(ROOT, "tape_amd", "csrc", name)) as f:
        return f.read()


# ---- the constants the tables are built on ----------------------------------------------------------
def test_launch_constant_matches_the_source():
    m = re.search(r"constexpr\s+uint64_t\s+kLeafBlocksPerLaunch\s*=\s*(\d+)\s*;", _src("commit.hip"))
    assert m and int(m.group(1)) == E.LEAF_BLOCKS_PER_LAUNCH == 1536
    # commit_leaf_launches (kernels.hpp) restates the split with the constant written out
    body = re.search(r"inline uint64_t commit_leaf_launches\(uint64_t slice_len\) \{(.*?)\n\}", _src("kernels.hpp"), re.S)
    assert body
    m = re.search(r"nl = \(T \+ (\d+)u\) / (\d+)u", body.group(1))
    assert m and (int(m.group(1)), int(m.group(2))) == (E.LEAF_BLOCKS_PER_LAUNCH - 1, E.LEAF_BLOCKS_PER_LAUNCH)
    m = re.search(r"constexpr\s+int\s+kCommitMaxLeaves\s*=\s*(\d+)\s*;", _src("kernels.hpp"))
    assert m and int(m.group(1)) == E.MAX_LEAVES == 64
    assert "__launch_bounds__(64) leaf_kernel" in _src("commit.hip") and E.LANES == 64


def test_block_formulas_against_sha256_padding():
    """blocks() is the padded message length of "LEAF" || slice; nfull() the blocks wholly inside it."""
    for L in range(0, 1024, 4):
        M = L + 4
        padded = M + 1 + 8
        assert E.blocks(L) == -(-padded // 64)
        assert E.nfull(L) == M // 64
        tail = E.blocks(L) - E.nfull(L)
        assert tail == {"own": 1, "shared": 1, "spill": 2}[E.last_block_case(L)]


# ---- SHORT ----------------------------------------------------------------------------------------
def test_short_is_every_multiple_of_4_below_324():
    assert E.SHORT == list(range(0, 324, 4)) and E.SHORT[0] == 0
    assert all(len(E.launches(L)) == 1 for L in E.SHORT)


@pytest.mark.parametrize("nf", [0, 1, 2, 3, 4])
def test_short_every_residue_at_every_pipeline_depth(nf):
    """Every terminator position with nf blocks through the prefetch pipeline: the prologue loads
    min(nf, 2) blocks and the loop refills max(nf - 2, 0) times."""
    got = {(L + 4) % 64 for L in E.SHORT if E.nfull(L) == nf}
    # (with no full block the message is under 64 bytes: the terminator cannot open a block)
    assert got == (RESIDUES if nf else RESIDUES - {0})
    assert {E.last_block_case(L) for L in E.SHORT if E.nfull(L) == nf} == \
        ({"own", "shared", "spill"} if nf else {"shared", "spill"})


# ---- SPLIT ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("below", sorted(E.SPLIT))
def test_split_edge_figures(below):
    last, first = E.SPLIT_EDGES[below]
    assert first == last + 4
    assert E.blocks(last) == below * E.LEAF_BLOCKS_PER_LAUNCH and E.blocks(first) == below * E.LEAF_BLOCKS_PER_LAUNCH + 1
    assert len(E.launches(last)) == below and len(E.launches(first)) == below + 1
    # the largest with T blocks, the smallest with T + 1
    around = range(last - 256, first + 256, 4)
    assert max(L for L in around if E.blocks(L) == E.blocks(last)) == last
    assert min(L for L in around if E.blocks(L) == E.blocks(first)) == first
    assert {1: (98_288, 98_292), 2: (196_592, 196_596)}[below] == (last, first)


@pytest.mark.parametrize("below", sorted(E.SPLIT))
def test_split_run_straddles_the_change(below):
    run = E.SPLIT[below]
    last, first = E.SPLIT_EDGES[below]
    assert len(run) == 16 and run == list(range(run[0], run[0] + 64, 4))
    assert {L % 64 for L in run} == RESIDUES
    counts = [len(E.launches(L)) for L in run]
    assert counts == [below] * 8 + [below + 1] * 8
    assert run[7] == last and run[8] == first
    assert max(max(E.SPLIT[b]) for b in E.SPLIT) == 196_624


@pytest.mark.parametrize("below", sorted(E.SPLIT))
def test_split_last_block_cases_under_a_resumed_launch(below):
    """All three last-block cases occur with below + 1 launches (2 and 3): the final blocks are
    assembled by a launch that loaded a parked state.  (The eight lengths under an edge end at
    (L + 4) % 64 = 24 .. 52: the terminator and the length share the data's last block.)"""
    run = E.SPLIT[below]
    assert {E.last_block_case(L) for L in run if len(E.launches(L)) == below + 1} == {"own", "shared", "spill"}
    assert [(L + 4) % 64 for L in run[:8]] == list(range(24, 56, 4))
    assert [(L + 4) % 64 for L in run[8:]] == [56, 60, 0, 4, 8, 12, 16, 20]


def test_multi_launch_cases_cut_inside_the_pipeline():
    """In every multi-launch case each launch but the last ends before nfull (so the pipeline is cut
    by b1, not by the data's end, and resumes at b0 > 0), the last launch still runs the pipeline
    before it assembles the final blocks, and the launches tile [0, T)."""
    multi = [L for run in E.SPLIT.values() for L in run] + list(E.STREAM_LENGTHS)
    seen = 0
    for L in multi:
        ls = E.launches(L)
        assert ls[0][0] == 0 and ls[-1][1] == E.blocks(L)
        assert all(a[1] == b[0] for a, b in zip(ls, ls[1:]))
        assert all(b1 - b0 <= E.LEAF_BLOCKS_PER_LAUNCH for b0, b1 in ls)
        if len(ls) > 1:
            seen += 1
            assert all(b1 < E.nfull(L) for _, b1 in ls[:-1])
            assert ls[-1][0] + 2 < E.nfull(L)
    assert seen == 8 + 16 + 1


# ---- STREAMS --------------------------------------------------------------------------------------
def test_stream_counts():
    assert [n * nobj for n, nobj in E.STREAMS] == [1, 63, 64, 65, 128, 129, 130]
    assert len({n for n, _ in E.STREAMS}) >= 5 and all(1 <= n <= E.MAX_LEAVES for n, _ in E.STREAMS)
    # a lone lane, a wave one short, full waves, and one and two lanes into the next wave
    assert [(n * nobj) % E.LANES for n, nobj in E.STREAMS] == [1, 63, 0, 1, 0, 1, 2]
    assert [len(E.launches(L)) for L in E.STREAM_LENGTHS] == [1, 2]
    n, nobj = E.LEAF_SHAPE
    assert n * nobj == 66 and (n * nobj) % E.LANES == 2 and n <= E.MAX_LEAVES
    assert {E.gapped(i) for i in range(len(E.STREAMS))} == {False, True}
    assert n * nobj * max(E.SPLIT[2]) < 14 << 20  # the largest input


def test_tree_height():
    assert [E.tree_height(n) for n in (1, 2, 3, 4, 5, 7, 13, 22, 64)] == [1, 1, 2, 2, 3, 3, 4, 5, 6]
    assert all(n <= 1 << E.tree_height(n) for n in range(1, 65))


# ---- TREE -----------------------------------------------------------------------------------------
def test_tree_shapes_claims():
    assert E.TREE == [(1, 1), (1, 5), (2, 1), (3, 2), (3, 5), (7, 3), (20, 5), (32, 5), (33, 6), (63, 6), (64, 6),
                      (20, 32), (64, 32)]
    assert E.TREE_NOBJ == [1, 3, 65, 130]
    assert all(1 <= n <= min(E.MAX_LEAVES, 1 << h) and 1 <= h <= MO.MAX_MERKLE_TREE_HEIGHT for n, h in E.TREE)

    def odd_levels(n, h):
        out, c = set(), n
        for l in range(h):
            if c & 1:
                out.add(l)
                c += 1
            c //= 2
        return out
    # a padded layer at every level: 0..4 among the shapes of production height and below, all 32 overall
    assert set().union(*(odd_levels(n, h) for n, h in E.TREE if h <= 6)) >= {0, 1, 2, 3, 4}
    assert set().union(*(odd_levels(n, h) for n, h in E.TREE)) == set(range(32))
    assert odd_levels(1, 1) == {0} and odd_levels(2, 1) == set()
    assert 0 in odd_levels(63, 6) and odd_levels(64, 6) == set()  # layer[63] as padding; rows 0..63 as leaves
    assert odd_levels(20, 32) == {2, 3} | set(range(5, 32))  # one node against empty roots 5..31
    assert odd_levels(64, 32) == set(range(6, 32))
    assert (E.TREE_NOBJ[2] - 1) // E.LANES == 1 and (E.TREE_NOBJ[3] - 1) // E.LANES == 2
    assert all(nobj % E.LANES for nobj in E.TREE_NOBJ)  # every grid's last workgroup is ragged
    assert set(E.OPTIONAL) <= {(n, h, nobj) for n, h in E.TREE for nobj in E.TREE_NOBJ}
    assert E.TREE_SLICE_LEN == 8


@pytest.mark.parametrize("n,height", E.TREE)
def test_layer_walk_agrees_with_the_oracle(n, height):
    """tree_layers / proof_from_layers (one walk per object) give the oracle's root and proofs, and the
    oracle's proofs verify under its own verify_leaf_hash: the GPU test's reference is consistent."""
    rng = np.random.default_rng(n * 100 + height)
    leaves = [rng.bytes(32) for _ in range(n)]
    layers = E.tree_layers(leaves, height)
    root = MO.root_from_leaf_hashes(leaves, height)
    assert layers[height] == [root]
    for i in range(n):
        proof = MO.create_proof_from_leaf_hashes(leaves, i, height)
        assert len(proof) == height and E.proof_from_layers(layers, i) == proof
        assert MO.verify_leaf_hash(leaves[i], root, proof, i, height)
        assert not MO.verify_leaf_hash(leaves[i], root, proof, i ^ 1, height)
    assert not MO.verify_leaf_hash(MO.hash_leaf(b"x"), root, E.proof_from_layers(layers, 0), 0, height)


# ---- ERRORS ---------------------------------------------------------------------------------------
def test_error_table_shape():
    names = [name for name, _, _ in E.ERRORS]
    assert len(set(names)) == len(names)
    assert {"n_zero", "n_65", "slice_len_6", "height_0_with_roots", "height_33_with_roots", "proofs_without_roots",
            "tree_full", "obj_stride_plus_2", "slices_base_plus_2"} <= set(names)
    for name, over, code in E.ERRORS:
        assert set(over) <= set(E.ERROR_BASE) and code in (E.INVALID_ARG, E.TREE_FULL), name
    a = E.error_case(dict(n=3, height=1))
    assert (a["n"], a["height"], a["obj_stride"]) == (3, 1, 3 * 64)
    base = E.error_case({})
    assert base["obj_stride"] % 4 == 0 and base["slice_len"] % 4 == 0 and base["base_shift"] == 0
    from tape_amd import _lib
    assert (E.INVALID_ARG, E.TREE_FULL, E.OK) == (_lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_MERKLE_TREE_FULL, _lib.TE_OK)


def _call_with_dummy_pointers(a):
    """te_commit_batch_device over pointers that are never followed: every case here is decided
    before the library looks for a device."""
    from tape_amd import _lib
    p = lambda on: C.c_void_p(4096) if on else None  # noqa: E731
    return _lib.lib.te_commit_batch_device(C.c_void_p(4096 + a["base_shift"]), a["obj_stride"], a["slice_len"], a["n"],
                                           a["nobj"], a["height"], p(a["leaf"]), p(a["roots"]), p(a["proofs"]), None)


@pytest.mark.parametrize("name,over,code", E.ERRORS, ids=[e[0] for e in E.ERRORS])
def test_argument_errors_come_before_the_device(name, over, code):
    assert _call_with_dummy_pointers(E.error_case(over)) == code


def test_no_objects_is_ok_without_a_device():
    assert _call_with_dummy_pointers(E.error_case(dict(nobj=0))) == E.OK
    # nobj == 0 comes first: nothing else is looked at
    assert _call_with_dummy_pointers(E.error_case(dict(nobj=0, slice_len=6, base_shift=1))) == E.OK


def test_header_states_the_alignment_contract():
    with open(os.path.join(ROOT, "include", "tape_ec.h")) as f:
        h = f.read()
    doc = h[h.index("/* Batched commitments on the device"):h.index("int te_commit_batch_device(")]
    assert "4-byte aligned" in doc and "obj_stride" in doc and "TE_ERR_INVALID_ARG" in doc
