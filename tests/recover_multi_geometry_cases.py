"""Case table of tests/test_gpu_recover_multi_geometry.py, in plain Python (no device, no library):
the profiles, sub-chunk sizes, call sizes, lost sets, layouts and output offsets at which the
multi-output rebuild kernel (tape_amd/csrc/recover_multi.hip, recover_multi_kernel<NK, G>) runs,
and what the launch rule (recover_multi_g / wgs_per_stripe = decode_geometry_cases.stage_g /
stage_wgs) and the split rule (rec_multi_plan.hpp) make of each.  tests/test_recover_multi_geometry_cases.py
checks all of it on the CPU, the claims about lost sets through the report mode of
tests/native/rec_multi_check.cpp.

Which rows the kernel can be given.  Every recover entry point takes only objects of the slicer's
own geometry (rec_validate: slice_len == te_slicer_geometry(blob_len).slice_len), and that geometry
cuts objects of up to 1 MB into stripes of 100,000 bytes, larger ones into stripes of 1 MB.  So the
sub-chunk sizes this kernel ever sees are, per profile,
  * the even sizes up to sc(100,000): 144, 126, 112 and 100 bytes for k = 7, 8, 9, 10 -- at most 36
    words, a part of one wave, G = 1 at any call size;
  * sc(1,000,000): 1430, 1250, 1112 and 1000 bytes (358, 313, 278 and 250 words) in objects of two
    stripes or more -- G = 1 in a small call, G = 2 in a large one;
  * sc(10,000,000) in objects above 100 MB, which is out of reach of a quick test.
The rows of 64, 65, 128 and 129 words (sc = 254 .. 514) that decode_geometry_cases.TABLE_SC lists
for the decode kernel cannot be produced for this kernel by any host code: REQUESTED records what
each of them becomes here and reachable_sc() is the rule, checked against Slicer.geometry."""
import random

import decode_geometry_cases as G
from decode_geometry_cases import TABLE_PROFILES, TABLE_SC, chunk_size_for, stage_g, stage_wgs, words

N, Q, ALPHA = G.N, G.Q, G.ALPHA
PROFILES = sorted(TABLE_PROFILES)  # NK = 7 runs in-process too: no class kernel takes an object with several lost slices
META = 48
SMALL_JOBS = G.SMALL_STRIPES       # recover_multi_enqueue: a call of at most this many jobs runs G = 1
LARGE_JOBS = 66


def reachable_sc(k):
    """Sub-chunk sizes of one-stripe objects, of objects up to 1 MB, of objects up to 100 MB."""
    top = chunk_size_for(k, ALPHA, G.STRIPES[0]) // ALPHA
    return list(range(2, top + 1, 2)), top, chunk_size_for(k, ALPHA, G.STRIPES[1]) // ALPHA


def _largest(k, rem):
    return max(sc for sc in reachable_sc(k)[0] if sc % 4 == rem)


def rows(k):
    """name: (sc, object length, stripes, what it exercises).  Lengths are the slicer's own."""
    tail, whole = _largest(k, 2), _largest(k, 0)
    assert G.RECOVER_SC[k][258][0] == tail
    return {
        "smallest": (8, 800 * k, 1, "2 words: 62 lanes alias word 1"),
        "tail3": (10, G.RECOVER_SC[k][10][1], 1, "3 words, the last a 2-byte tail word loaded 2 bytes early"),
        "widest_tail": (tail, G.RECOVER_SC[k][258][1], 1, "widest one-stripe row that ends in a tail word"),
        "widest_whole": (whole, min(k * whole * ALPHA, G.STRIPES[0]) - 1, 1, "widest one-stripe row without a tail word"),
        "stripe3": (reachable_sc(k)[1], 250_001, 3, "three stripes, a short last one: the slot table differs per stripe"),
        "production": (reachable_sc(k)[2], 1_000_003, 2, "production row, the only one with more than one wave"),
    }


# decode_geometry_cases.TABLE_SC row -> the row used here, and why
REQUESTED = {
    8: ("smallest", "as requested"),
    10: ("tail3", "as requested"),
    254: ("widest_tail", "not reachable: the widest one-stripe row with a tail word instead"),
    256: ("widest_whole", "not reachable: the widest one-stripe row without a tail word instead"),
    258: ("widest_tail", "not reachable: no row of this kernel puts a lone tail word into a second wave below the production row"),
    512: ("production", "not reachable: the production row is the only one of two waves or more"),
    514: ("production", "not reachable: the all-alias second wave of the last G = 2 workgroup occurs at the production rows of k = 8 and 9"),
    1430: ("production", "sc(1,000,000) of each profile: 1430, 1250, 1112, 1000"),
}
assert set(REQUESTED) <= set(TABLE_SC)


def launch(sc, jobs):
    """(G, workgroups per stripe) of a launch of `jobs` jobs at this sub-chunk size."""
    gmax = 1 if jobs <= SMALL_JOBS else 0  # D.small_dec -> DecArgs::gmax
    return stage_g(words(sc), gmax), stage_wgs(words(sc), gmax)


# (G, workgroups per stripe) of a small and of a large call, per profile and row
GEOMETRY = {
    7: {"smallest": ((1, 1), (1, 1)), "tail3": ((1, 1), (1, 1)), "widest_tail": ((1, 1), (1, 1)),
        "widest_whole": ((1, 1), (1, 1)), "stripe3": ((1, 1), (1, 1)), "production": ((1, 6), (2, 3))},
    8: {"smallest": ((1, 1), (1, 1)), "tail3": ((1, 1), (1, 1)), "widest_tail": ((1, 1), (1, 1)),
        "widest_whole": ((1, 1), (1, 1)), "stripe3": ((1, 1), (1, 1)), "production": ((1, 5), (2, 3))},
    9: {"smallest": ((1, 1), (1, 1)), "tail3": ((1, 1), (1, 1)), "widest_tail": ((1, 1), (1, 1)),
        "widest_whole": ((1, 1), (1, 1)), "stripe3": ((1, 1), (1, 1)), "production": ((1, 5), (2, 3))},
    10: {"smallest": ((1, 1), (1, 1)), "tail3": ((1, 1), (1, 1)), "widest_tail": ((1, 1), (1, 1)),
         "widest_whole": ((1, 1), (1, 1)), "stripe3": ((1, 1), (1, 1)), "production": ((1, 4), (2, 2))},
}


def bits(m):
    return [i for i in range(N) if (m >> i) & 1]


def mask(xs):
    return sum(1 << i for i in xs)


# Sets found by a seeded search over the report mode, as (available, lost) slice masks: a single
# pass that fills the 16 flush items of a step; one that parks the most values in scratch rows; one
# at the most LDS rows any pass of the profile was seen to need (27 = zero + trash + 25 slots).
# tests/test_recover_multi_geometry_cases.py repeats a search of this kind as a check: no pass of its
# sample exceeds these sets in LDS rows, flush items or scratch rows.
_SEARCHED = {
    7: {"item_limit": (0x80b43, 0x0b49c), "scratch": (0x1474c, 0x23093), "lds_rows": (0xc2186, 0x2d429)},
    8: {"item_limit": (0x80c9e, 0x79120), "scratch": (0x5d889, 0x00026), "lds_rows": (0xc6a44, 0x09082)},
    9: {"item_limit": (0xa2758, 0x5c825), "scratch": (0xa7917, 0x406a8), "lds_rows": (0x324c7, 0x01100)},
    10: {"item_limit": (0x5a7b3, 0xa584c), "scratch": (0x26cf8, 0xc8004), "lds_rows": (0xb3e94, 0x0c06b)},
}
THREE_PASSES = (0x51c03, 0xac3fc)  # Clay(20,7,16) only: 12 of the 13 erased nodes


def lost_sets(k):
    """name: (available slices, lost slices, why).  By slice = node in stripe 0 and in every stripe
    of an identity layout; nodes 0..9 are column 0 (0..k-1 the data), 10..19 column 1."""
    col1 = list(range(10, 20))
    rnd = random.Random(2000 + k)
    s = {}
    s["column0_pair"] = ([0, 2, 3] + col1[:k - 3], [1, 4], "two data nodes of column 0")
    s["column1_pair"] = ([0, 1, 2, 3, 4, 10, 11] + [13, 14, 15][:k - 7], [12, 17], "two parity nodes of column 1")
    s["data_and_parity_across"] = ([0, 1, 3, 4, 5, 10, 11] + [12, 13, 14][:k - 7], [2, 15], "a data node and a parity node, one per column")
    s["pair_both_lost"] = ([1, 2, 3] + col1[:k - 3], [0, 9], "a coupled pair (same column) both lost: the finish step stores both rows")
    s["pair_one_lost"] = ([1, 2, 3] + col1[:k - 3], [0, 19], "every pair of a lost node has an erased partner that is not lost: its row is not stored")
    surv = sorted(rnd.sample(range(N), k))
    s["all_lost"] = (surv, [i for i in range(N) if i not in surv], "all n - k slices: always split, every job's table has lost nodes without a slot")
    for extra, nl in ((1, 3), (2, 2)):
        av = sorted(rnd.sample(range(N), k + extra))
        s[f"k_plus_{extra}_available"] = (av, sorted(rnd.sample([i for i in range(N) if i not in av], nl)),
                                         f"{k + extra} available slices: the padding erases parity nodes that are present")
    s["n_minus_2_available"] = ([i for i in range(N) if i not in (6, 13)], [6, 13], "18 available slices: all but two erasures are padding")
    for name, why in (("item_limit", "one pass with a step of 16 flush items (kDecMaxOut)"),
                      ("scratch", "values parked in scratch rows across plane rows"),
                      ("lds_rows", "the most LDS rows a pass of this profile needs")):
        av, lo = _SEARCHED[k][name]
        s[name] = (bits(av), bits(lo), why)
    if k == 7 and THREE_PASSES:
        s["three_passes"] = (bits(THREE_PASSES[0]), bits(THREE_PASSES[1]), "a set the split rule deals into three parts")
    return s


ONE_PASS_PAIRS = ("data_and_parity_across", "column0_pair", "column1_pair")  # the sets of the geometry calls

# Passes of each set on stripes 0, 1, 2 of a rotated layout (stripe 0 is not rotated: the figure of
# every stripe of an identity layout), as the report mode of tests/native/rec_multi_check.cpp gives them
_ONE = (1, 1, 1)
_COMMON = {name: _ONE for name in ("column0_pair", "column1_pair", "data_and_parity_across", "pair_both_lost", "pair_one_lost",
                                   "k_plus_1_available", "k_plus_2_available", "n_minus_2_available")}
PASSES = {
    7: dict(_COMMON, all_lost=(2, 2, 3), item_limit=(1, 2, 2), scratch=(1, 1, 2), lds_rows=(2, 2, 2), three_passes=(3, 2, 2)),
    8: dict(_COMMON, all_lost=(2, 2, 2), item_limit=_ONE, scratch=_ONE, lds_rows=_ONE),
    9: dict(_COMMON, all_lost=(2, 2, 2), item_limit=(1, 2, 1), scratch=_ONE, lds_rows=_ONE),
    10: dict(_COMMON, all_lost=(2, 2, 2), item_limit=_ONE, scratch=_ONE, lds_rows=_ONE),
}


def passes(k, name, rotated, stripes):
    p = PASSES[k][name]
    return [p[st] if rotated else p[0] for st in range(stripes)]


def out_len_holds(sc, slice_len, nlost):
    """put_out's whole-word branch: off + sc <= out_len for the last plane of the last slot of a job
    (out_len = (nlost - 1) * slice_len + cs, rows at slot * slice_len + plane * sc)."""
    cs = sc * ALPHA
    return (nlost - 1) * slice_len + (ALPHA - 1) * sc + sc <= (nlost - 1) * slice_len + cs


# ---- the calls ------------------------------------------------------------------------------------
# A call is a list of (row, lost set) objects.  One job per (stripe, pass); the call's total decides
# G for every launch of it, and objects of one (chunk size, slice length) share a launch.
def lost_set_call(rotated):
    """Rows of the call every named lost set runs in: sc = 10 and the widest tail row (two chunk
    sizes: two launches), in a rotated layout the three-stripe object as well (a third)."""
    return ["tail3", "widest_tail"] + (["stripe3"] if rotated else [])


def geometry_call(k, row, large):
    """The one-pass pairs in turn, the across-columns pair first: three objects (small), or as many
    as make LARGE_JOBS jobs (large; the GPU test lets them share one resident copy of the slices)."""
    stripes = rows(k)[row][2]
    count = -(-LARGE_JOBS // stripes) if large else len(ONE_PASS_PAIRS)
    return [(row, ONE_PASS_PAIRS[i % len(ONE_PASS_PAIRS)]) for i in range(count)]


OFFSET_ROWS = ("tail3", "widest_whole", "widest_tail")  # output offsets of 0..3 mod 4 run on these
GUARD = 64


def call_stats(k, call, rotated):
    """What te_clay_recover_multi_launch_stats must say after the call."""
    r = rows(k)
    st = {"multi_objects": len(call), "single_objects": 0, "generic_objects": 0, "stripes": 0, "jobs": 0, "out_rows": 0,
          "passes": 0, "split_stripes": 0}
    for row, name in call:
        per = passes(k, name, rotated, r[row][2])
        st["stripes"] += len(per)
        st["jobs"] += sum(per)
        st["out_rows"] += len(per) * len(lost_sets(k)[name][1]) * ALPHA
        st["passes"] = max(st["passes"], max(per))
        st["split_stripes"] += sum(p > 1 for p in per)
    st["multi_launches"] = len({(r[row][0], r[row][2]) for row, _ in call})
    return st


def call_instances(k, call, rotated):
    """{(NK, G, sc)} of the call's launches."""
    jobs = call_stats(k, call, rotated)["jobs"]
    return {(k, launch(rows(k)[row][0], jobs)[0], rows(k)[row][0]) for row, _ in call}
