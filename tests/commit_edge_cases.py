"""Case tables of tests/test_gpu_commit_edges.py: the shape edges of the two commitment kernels
(tape_amd/csrc/commit.hip), in plain Python (no device, no library).
tests/test_commit_edge_cases.py checks every property claimed here by enumeration.

leaf_kernel: one lane per slice stream, SHA-256 of "LEAF" || slice in 64-byte blocks.  What picks
its path is the slice length L (always a multiple of 4):
    blocks(L)   T = (M + 8) / 64 + 1 with M = L + 4                      commit.hip:43-44
    nfull(L)    the blocks that hold data only, read through the two-blocks-ahead pipeline;
                the rest are assembled word by word                      commit.hip:45
    (L + 4) % 64  where the 0x80 terminator falls: 0 = it opens a block of its own, 4..52 = it and
                the bit length share the data's last block, 56..60 = the length needs one more
    launches(L) launch_commit cuts a stream's T blocks into nl = ceil(T / 1536) launches of
                per = ceil(T / nl) blocks; between launches a stream's state is parked in its
                leaf-hash slot                                            commit.hip:151-154
and the stream count n * nobj against the 64 lanes of a workgroup: the idle lanes of the last,
partial wave redo the last stream without storing.

tree_kernel: one lane per object, its own layer walk over (n, height); 64 objects per workgroup."""
from oracle import merkle_oracle as MO

LEAF_BLOCKS_PER_LAUNCH = 1536  # kLeafBlocksPerLaunch, commit.hip:19
MAX_LEAVES = 64                # kCommitMaxLeaves, kernels.hpp
LANES = 64                     # __launch_bounds__(64): streams (objects) per workgroup


def blocks(L):
    return (L + 12) // 64 + 1


def nfull(L):
    return (L - 60) // 64 + 1 if L >= 60 else 0


def launches(L, per_launch=LEAF_BLOCKS_PER_LAUNCH):
    """[(b0, b1)] of launch_commit's leaf launches, b1 clipped to T as the kernel clips it."""
    T = blocks(L)
    nl = -(-T // per_launch)
    per = -(-T // nl)
    return [(b0, min(b0 + per, T)) for b0 in range(0, T, per)]


def last_block_case(L):
    """Where the terminator and the bit length fall: 'own', 'shared' or 'spill'."""
    r = (L + 4) % 64
    return "own" if r == 0 else ("shared" if r <= 52 else "spill")


def tree_height(n):
    """The smallest height that holds n leaves, at least 1."""
    return max(1, (n - 1).bit_length())


# ---- leaf_kernel ----------------------------------------------------------------------------------
LEAF_SHAPE = (22, 3)  # (n, nobj) of SHORT and SPLIT: 66 streams, one full wave and a partial one

# every (L + 4) % 64 at nfull = 0 .. 4 (and 5): the pipeline's prologue with 0, 1, 2, 3 and more
# blocks to load; L = 0 is hash_leaf(&[])
SHORT = list(range(0, 324, 4))

# The largest L with T blocks and the smallest with T + 1, for T = 1536 and 3072: the launch count
# goes 1 -> 2 and 2 -> 3 between them.  Eight multiples of 4 on either side: every L % 64 once.
SPLIT_EDGES = {1: (98_288, 98_292), 2: (196_592, 196_596)}  # launches below the edge: (last, first)
SPLIT = {nl: list(range(lo - 28, hi + 32, 4)) for nl, (lo, hi) in SPLIT_EDGES.items()}

# (n, nobj): 1, 63, 64, 65, 128, 129 and 130 streams, with differing n
STREAMS = [(1, 1), (7, 9), (64, 1), (5, 13), (64, 2), (3, 43), (13, 10)]
STREAM_LENGTHS = (124, 98_292)  # one launch, (L + 4) % 64 == 0; two launches


def gapped(index):
    """Every other case separates its objects by 8 bytes that belong to no slice."""
    return index % 2 == 1


# ---- tree_kernel ----------------------------------------------------------------------------------
# no pair at the leaf level (n = 1), an odd layer at each level (3, 7, 20, 33, 63), the last scratch
# row (63 pads into layer[63]; 64 fills rows 0..63), the chain of one node against growing empty
# roots (height above ceil(log2 n), up to 32)
TREE = [(1, 1), (1, 5), (2, 1), (3, 2), (3, 5), (7, 3), (20, 5), (32, 5), (33, 6), (63, 6), (64, 6), (20, 32), (64, 32)]
TREE_NOBJ = [1, 3, 65, 130]  # a partial workgroup, one full and a ragged one, two full and a ragged one
TREE_SLICE_LEN = 8
OPTIONAL = [(20, 5, 65), (64, 6, 3), (1, 1, 1)]  # (n, height, nobj) of the optional-output test


def tree_layers(leaves, height):
    """create_merkle_proof_hashes' layers (tree.rs:430-440; oracle/merkle_oracle.py), built once for
    an object: layers[l] is level l padded to an even count with EMPTY_ROOTS[l]; layers[height] is
    [root]."""
    empty = MO.empty_roots(height)
    layers, cur = [], list(leaves)
    for l in range(height):
        if len(cur) % 2:
            cur.append(empty[l])
        layers.append(cur)
        cur = [MO.hash_pair(cur[2 * j], cur[2 * j + 1]) for j in range(len(cur) // 2)]
    assert len(cur) == 1
    layers.append(cur)
    return layers


def proof_from_layers(layers, index):
    """tree.rs:442-455: the sibling of index's node at every level."""
    return [layers[l][(index >> l) ^ 1] for l in range(len(layers) - 1)]


# ---- te_commit_batch_device's argument checks -------------------------------------------------------
INVALID_ARG, TREE_FULL, OK = 20, 10, 0  # TE_ERR_INVALID_ARG, TE_ERR_MERKLE_TREE_FULL, TE_OK
ERROR_BASE = dict(n=20, nobj=2, slice_len=64, height=5, roots=True, proofs=True, leaf=True,
                  stride_extra=0,  # obj_stride = n * slice_len + stride_extra
                  base_shift=0)    # d_slices = a 4-aligned address + base_shift
ERRORS = [
    ("n_zero", dict(n=0), INVALID_ARG),
    ("n_65", dict(n=65, height=7), INVALID_ARG),
    ("slice_len_6", dict(slice_len=6), INVALID_ARG),
    ("height_0_with_roots", dict(height=0, proofs=False), INVALID_ARG),
    ("height_33_with_roots", dict(height=33, proofs=False), INVALID_ARG),
    ("height_33_with_proofs", dict(height=33), INVALID_ARG),
    ("proofs_without_roots", dict(roots=False), INVALID_ARG),
    ("no_leaf_buffer", dict(leaf=False), INVALID_ARG),
    ("tree_full", dict(n=3, height=1), TREE_FULL),
    ("tree_full_roots_only", dict(n=33, height=5, proofs=False), TREE_FULL),
    ("obj_stride_plus_2", dict(stride_extra=2), INVALID_ARG),
    ("obj_stride_plus_1", dict(stride_extra=1, roots=False, proofs=False), INVALID_ARG),
    ("slices_base_plus_2", dict(base_shift=2), INVALID_ARG),
    ("slices_base_plus_3", dict(base_shift=3, roots=False, proofs=False), INVALID_ARG),
]
NOBJ_ZERO = dict(ERROR_BASE, nobj=0)  # TE_OK, nothing written


def error_case(overrides):
    a = dict(ERROR_BASE, **overrides)
    a["obj_stride"] = a["n"] * a["slice_len"] + a["stride_extra"]
    return a
