"""Case tables of tests/test_gpu_decode_table_geometry.py and tests/test_gpu_decode_generic_geometry.py,
in plain Python (no device, no library): the sub-chunk sizes, the object lengths of each, the
survivor sets with the kernel each must run, and what the launch rules of decode_stage.hip
(decode_stage_g / decode_stage_wgs) and gpe.hip (launch_gpe / launch_gpe_t) make of them.
tests/test_decode_geometry_cases.py checks this arithmetic on the CPU; the GPU files assert the
sizes once more against ClayCoder / Slicer.geometry before anything runs.

An object here is one stripe of k chunks of cs = sc * alpha bytes.  ClayCoder.chunk_size_for(L)
rounds L up to a multiple of 2 * alpha * k, so sc is even and the lengths with that sc are
(k * cs - 2 * alpha * k, k * cs]: `natural` lengths.  A shorter length (one byte past a chunk
boundary at a large sc) is the share of a short last stripe -- Slicer.encode pads the stripe's
data with zeros to k * cs and the decoder takes cs from the slice length -- and is built the same
way here: the data zero-padded to k * cs, the metadata's blob_len the length."""
import random

N = 20
Q = 10            # the table kernel's profiles: q = 10, t = 2, alpha = 100
ALPHA = 100
STRIPES = (100_000, 1_000_000, 10_000_000)
SMALL_STRIPES = 64  # dec_plan.hpp kDecSmallStripes: a call of at most this many stripes runs G = 1
MAXG = 2            # decode_stage.hip TEC_DEC_MAXG


def chunk_size_for(k, alpha, length):
    unit = 2 * alpha * k
    return max(1, -(-length // unit)) * unit // k


def words(sc):
    return (sc + 3) // 4


def stage_g(wps, gmax):
    groups = (wps + 63) // 64
    cap = gmax if gmax and gmax < MAXG else MAXG
    return min(groups, cap)


def stage_wgs(wps, gmax):
    groups = (wps + 63) // 64
    return -(-groups // stage_g(wps, gmax))


def meta_stripe(length):
    """The smallest stripe size that holds the object in one stripe."""
    return next(s for s in STRIPES if length <= s)


# ---- the table-driven kernel (dec_stage_kernel<NK, G>) ------------------------------------------
TABLE_IN_PROCESS = [(20, 8, 17), (20, 9, 18), (20, 10, 19)]
TABLE_CHILD = (20, 7, 16)  # class kernels switched off: one child process
TABLE_PROFILES = TABLE_IN_PROCESS + [TABLE_CHILD]

# sc: (words, G and workgroups per stripe of a small call, of a large call, what it is for).
# Every requested size is even, so the geometry produces each: no substitutions.
TABLE_SC = {
    8: (2, (1, 1), (1, 1), "smallest staged row: one partial wave, 62 lanes alias word 1"),
    10: (3, (1, 1), (1, 1), "tail word (2 bytes, loaded 2 bytes early) in the only wave"),
    254: (64, (1, 1), (1, 1), "exactly one wave, its last word a tail word"),
    256: (64, (1, 1), (1, 1), "exactly one wave, no tail word"),
    258: (65, (1, 2), (2, 1), "second wave / workgroup holds only the tail word"),
    510: (128, (1, 2), (2, 1), "two full waves, tail word"),
    512: (128, (1, 2), (2, 1), "two full waves"),
    514: (129, (1, 3), (2, 2), "G = 2: the second workgroup has lseg = 2, its second wave all aliases"),
    1026: (257, (1, 5), (2, 3), "257 words: the last workgroup holds the tail word alone"),
    1430: (358, (1, 6), (2, 3), "production row of Clay(20,7,16) 1 MB stripes"),
}
LARGE_OBJECTS = 66  # one-stripe objects of a large call


def row_ends(sc):
    """(row from the end, word, bytes into the word) of the four lengths that end inside a data
    row's word: at the row's last word (the tail word when sc = 2 mod 4), at words 63 and 64 (the
    wave edge, where the row has them) and at word 0; 1, 2, 3 and 5 bytes in (5: one byte into the
    next word).  A word index is lowered until the end lies inside the row (before its last byte); in the generic
    kernel's rows of 2, 4 and 6 bytes an end past the row lies in a following row."""
    nw = words(sc)
    out = []
    for back, w, r in ((0, nw - 1, 1), (1, min(63, nw - 1), 2), (4, min(64, nw - 1), 3), (7, 0, 5)):
        while w > 0 and 4 * w + r >= sc:
            w -= 1
        out.append((back, w, r))
    return out


def lengths(k, alpha, sc):
    """[(length, natural?)]: the full k * cs; four lengths ending 1, 2, 3, 5 bytes into a word of one
    of the last chunk's last rows; one byte past the last chunk boundary."""
    cs = sc * alpha
    out = [k * cs]
    out += [(k - 1) * cs + (alpha - 1 - back) * sc + 4 * w + r for back, w, r in row_ends(sc)]
    out.append((k - 1) * cs + 1)
    return [(L, chunk_size_for(k, alpha, L) == cs) for L in out]


def survivor_sets(n, k, extra=0):
    """The first k slices, the last k (parity-heavy), two seeded random sets of exactly k, one of
    k + 2 (padded to n - k erasures by the engine); then `extra` more seeded sets, every third of
    k + 2."""
    rnd = random.Random(1000 * n + k)
    sets = [tuple(range(k)), tuple(range(n - k, n))]
    sets += [tuple(sorted(rnd.sample(range(n), k))) for _ in range(2)]
    sets.append(tuple(sorted(rnd.sample(range(n), k + 2))))
    for i in range(extra):
        sets.append(tuple(sorted(rnd.sample(range(n), k + 2 if i % 3 == 2 else k))))
    return sets


# Survivor sets whose padded erasure pattern has no plane program (ClayHost::dec_prog's steps do
# not pack: more than 16 output rows in a step): the whole call then runs the generic kernel, so
# these run in calls of their own.  Clay(20,10,19): slices 10..19 are one whole column (every data
# node erased); Clay(20,9,18): slices 11..19.  tests/native/dec_stage_sets.cpp restates the rule.
NO_PLANE_PROGRAM = {(20, 9, 18): [tuple(range(11, 20))], (20, 10, 19): [tuple(range(10, 20))]}


def table_sets(params, large):
    """The survivor sets of a table-kernel call: 5 (small call) or 11 (large) less those without a
    plane program."""
    n, k, _ = params
    sets = survivor_sets(n, k, 6 + len(NO_PLANE_PROGRAM.get(params, [])) if large else 0)
    sets = [s for s in sets if s not in NO_PLANE_PROGRAM.get(params, [])]
    return sets[:11] if large else sets


def table_call(params, sc, large):
    """[(length index, survivor set)] of one call: every length under every set."""
    sets = table_sets(params, large)
    nl = len(lengths(params[1], ALPHA, sc))
    return [(i, s) for s in sets for i in range(nl)]


# ---- node recover on the table kernel -----------------------------------------------------------
# recover_batch takes only objects of the slicer's own geometry (slice_len == geometry(blob_len)):
# a stripe is 100,000 B up to 1 MB objects and 1 MB above, so the reachable sub-chunk sizes are the
# even ones up to sc(100,000) and sc(1,000,000).  Requested -> used, per k:
#   10   -> 10: one-stripe objects.
#   258  -> the largest reachable sc = 2 mod 4 below it (one wave with a tail word; 65 words in a
#           second wave are not reachable for recover), one-stripe objects.
#   514  -> sc(100,000), objects of three stripes (rotation: the lost slice is another shard on
#           every stripe); 129 words are not reachable.
#   1430 -> sc(1,000,000), the production row of each profile, objects of two stripes: 1430
#           (358 words), 1250 (313 words, tail word, the last G = 2 workgroup's second wave all
#           aliases), 1112 (278 words), 1000 (250 words).
RECOVER_SC = {
    7: {10: (10, 6_999), 258: (142, 99_399), 514: (144, 250_001), 1430: (1430, 1_000_003)},
    8: {10: (10, 7_999), 258: (126, 99_999), 514: (126, 250_001), 1430: (1250, 1_000_003)},
    9: {10: (10, 8_999), 258: (110, 98_999), 514: (112, 250_001), 1430: (1112, 1_000_003)},
    10: {10: (10, 9_999), 258: (98, 97_999), 514: (100, 250_001), 1430: (1000, 1_000_003)},
}
RECOVER_LARGE_STRIPES = 66


def slicer_geometry(k, length):
    """(stripe size, stripes, sc) of Slicer.geometry for an alpha = 100 profile."""
    stripe = STRIPES[0] if length <= 1_000_000 else STRIPES[1] if length <= 100_000_000 else STRIPES[2]
    ns = -(-length // stripe)
    return stripe, ns, chunk_size_for(k, ALPHA, min(length, stripe)) // ALPHA


def recover_cases(params):
    """[(lost, peers)]: a lost slice in each column, data and parity (data nodes are all in
    column 0; Clay(20,10,19) has no column-0 parity), each under a peer set of exactly k and one
    of k + 3."""
    n, k, _ = params
    rnd = random.Random(77 * k)
    losts = [2, n - 3] + ([Q - 1] if k < Q else []) + [k - 1, Q]
    out = []
    for lost in losts:
        rest = [i for i in range(n) if i != lost]
        for extra in (0, 3):
            out.append((lost, tuple(sorted(rnd.sample(rest, k + extra)))))
    return out


# ---- the generic kernel (gpe_kernel<MAXE>) -------------------------------------------------------
GPE_WORDS = 4  # kernels.hpp kGpeWords: words per block


def clay_layout(n, k, d):
    q = d - k + 1
    nu = (q - n % q) % q
    t = (n + nu) // q
    return q, t, nu, q ** t


def gpe_instance(erased):
    return next(e for e in (4, 8, 13, 20) if erased <= e)


def gpe_lds(maxe, alpha, t):
    return 2 * maxe * alpha * GPE_WORDS * 4 + alpha * t + 16


# params: (MAXE instance, LDS bytes, over the 64 KiB branch?, sub-chunk sizes)
GENERIC_SC = [2, 4, 6, 14, 16, 18, 34, 130]  # 130: 33 words, a ninth block of one live (tail) word
GENERIC = {
    (12, 8, 11): (4, 8_400, False, GENERIC_SC),
    (14, 8, 13): (8, 55_960, False, GENERIC_SC),
    (20, 7, 19): (13, 70_658, True, GENERIC_SC),
    (20, 7, 16): (13, 41_816, False, [2, 4, 6]),  # from sc = 8 on it leaves this kernel
    (20, 5, 14): (20, 64_216, False, GENERIC_SC),
}
# objects of three 100,000 B stripes through the Slicer: the one shape in which the rotated mapping
# differs from the identity (stripe 0 is never rotated), at the sub-chunk size the geometry gives
GENERIC_ROTATED_LEN = 250_001
GENERIC_ROTATED_SC = {(12, 8, 11): 196, (14, 8, 13): 58, (20, 7, 19): 86, (20, 5, 14): 200}


def generic_call(params, sc):
    n, k, _ = params
    alpha = clay_layout(*params)[3]
    nl = len(lengths(k, alpha, sc))
    return [(i, s) for s in survivor_sets(n, k) for i in range(nl)]
