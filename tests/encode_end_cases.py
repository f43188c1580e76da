"""Where a stripe's data can end in the LDS-DMA encode (tape_amd/csrc/encode_dma.hip), and the
objects that put it there: the case table of tests/test_gpu_encode_dma_end.py, checked on the CPU
by tests/test_encode_end_cases.py.

A case is an object of 1,000,000 + r bytes (1 <= r <= 1,000,000: two 1 MB stripes of Clay(20,7,16),
chunk size cs = 143,000, sub-chunk sc = 1,430) whose source address has the low bits src_al, 0 or 2
(an odd address runs the generic kernel).  1,000,000 is a multiple of 4, so both stripes start at
an address with those low bits.  end() restates what the kernel's loader wave computes in fetch()
for the last stripe, of r bytes: the chunk ex, plane ez and row word wi of the last data byte, the
bytes rem of that word that are data, the offset o3 of the word in its aligned dword pair and
whether the launch is the MASKED one.  The compute lane of word wi substitutes the word at plane
ez in own[ex] and in the ring image, and at plane (z0 = ex, s = ez % 10) in the partner row
x = ez // 10."""
from collections import namedtuple

STRIPE, CS, SC = 1_000_000, 143_000, 1430
K, Q = 7, 10
WORDS = (SC + 3) // 4  # 358; the last one holds columns 1428 and 1429 only

End = namedtuple("End", "r src_al ex ez wi rem o3 masked")


def end(r, src_al):
    """fetch() of a stripe of r bytes at a source address = src_al mod 4."""
    assert 1 <= r <= STRIPE and src_al in (0, 2)
    last = r - 1
    ex = last // CS
    ez = last % CS // SC
    wi = last % SC // 4
    rem = r - (ex * CS + ez * SC + wi * 4)
    o3 = (src_al + 2 * (ez & 1)) & 3
    masked = (src_al + r) % 4 != 0
    return End(r, src_al, ex, ez, wi, rem, o3, masked)


def partner_class(e):
    """The partner row x = ez // 10 against the end's chunk ex."""
    x = e.ez // Q
    return f"x={x}" if x >= K else "x<ex" if x < e.ex else "x==ex" if x == e.ex else "ex<x<=6"


# (r, src_al).  The first two lead the batch: in the one-workgroup form a launch's first task has
# no predecessor, so the masked launch starts with the first object's full stripe and the unmasked
# one with the second object's.
CASES = [
    (270_268, 2),    # both stripes masked; ex 1, ez 88: x = 8 = part[K + 1], level 2, wi 356, (2, 4, masked)
    (1_000_000, 0),  # both stripes unmasked; a full stripe as the last one: ex 6, ez 99, wi 107, (2, 2, unmasked)
    (1, 0),          # r = 1: ex 0 = x (red node), ez 0, wi 0, (0, 1, masked)
    (2, 2),          # r = 2: (2, 2, unmasked)
    (2, 0),          # r = 2: (0, 2, masked)
    (3, 0),          # r = 3: (0, 3, masked)
    (4, 0),          # r = 4: (0, 4, unmasked)
    (4, 2),          # r = 4: (2, 4, masked)
    (5, 2),          # r = 5: wi 1, (2, 1, masked)
    (1_430, 0),      # r = sc, a multiple of sc and not of cs: ez 0, wi 357 (the half word), rem 2
    (1_431, 2),      # sc + 1: ez 1 (odd plane, src_al 2), wi 0, rem 1
    (1_437, 0),      # ez 1 (odd plane, src_al 0), wi 1, (2, 3, masked)
    (143_000, 0),    # r = cs, the last byte of chunk 0: ez 99, wi 357, x = 9
    (143_001, 2),    # cs + 1, the first byte of chunk 1: x = 0 < ex
    (143_002, 0),    # cs + 2
    (429_000, 2),    # r = 3 cs, the last byte of chunk 2: ez 99, wi 357, x = 9
    (429_001, 0),    # 3 cs + 1, the first byte of chunk 3
    (429_002, 2),    # 3 cs + 2
    (858_000, 0),    # r = 6 cs, the last byte of chunk 5: ez 99, wi 357, x = 9
    (858_001, 0),    # 6 cs + 1, the first byte of chunk 6
    (858_002, 2),    # 6 cs + 2
    (390_645, 0),    # ex 2, ez 73: x = 7 = part[K + 0], level 2, ez % 10 = 3, wi 63 (the end of wave 0)
    (693_810, 0),    # ex 4, ez 85: x = 8 = part[K + 1], level 2, wi 64 (the start of wave 1), (2, 4, masked)
    (844_721, 2),    # ex 5, ez 90: x = 9 = part[K + 2], level 2, ez % 10 = 0, wi 255 (the end of wave 3)
    (971_996, 0),    # ex 6, ez 79: x = 7, level 2, ez % 10 = 9, wi 256 (the start of wave 4)
    (480_479, 0),    # ex 3, ez 35: x == ex (red node), level-1 row 3, wi 357 with rem 1
    (949_524, 0),    # ex 6, ez 64: x == ex (red node), level-1 row 6, wi 0, (0, 4, unmasked)
    (958_097, 2),    # ex 6, ez 69: x == ex, level-1 row 6, ez % 10 = 9, wi 356, (0, 3, masked)
    (589_414, 2),    # ex 4, ez 12: x = 1 < ex, wi 63
    (866_173, 0),    # ex 6, ez 5: x = 0 < ex, wi 255
    (758_157, 0),    # ex 5, ez 30: x = 3 < ex, level-1 row 3, ez % 10 = 0, wi 64
    (211_238, 0),    # ex 1, ez 47: ex < x = 4 <= 6, wi 256
    (371_807, 2),    # ex 2, ez 60: ex < x = 6, level-1 row 6, ez % 10 = 0, wi 1
    (57_200, 2),     # ex 0, ez 39: ex < x = 3, level-1 row 3, ez % 10 = 9, wi 357 (a multiple of sc)
    (94_640, 2),     # ex 0, ez 66: ex < x = 6, level-1 row 6, wi 64
    (510_510, 2),    # 3 cs + 57 sc, a multiple of sc and not of cs: ex 3, ez 56, wi 357
    (510_511, 0),    # ... and the next byte: ez 57, wi 0, rem 1
    (713_572, 2),    # ex 4, ez 99 away from a chunk end: wi 0, x = 9
    (717_855, 0),    # ex 5, ez 1 (a plane the previous task's loader prefetches), wi 356
    (430_022, 2),    # ex 3, ez 0 (the other prefetched plane), wi 255
]

# The per-call form (Slicer.encode: its device input buffer is dword aligned, src_al = 0) runs
# these r, each in CASES with src_al 0: every ex, every partner class and wi = 357.
PER_CALL_R = [1, 3, 4, 1_430, 143_000, 143_002, 429_001, 858_001, 390_645, 693_810, 971_996, 480_479, 949_524,
              866_173, 758_157, 211_238, 1_000_000]


def ends(cases=None):
    return [end(r, al) for r, al in (CASES if cases is None else cases)]


def per_call_cases():
    return [(r, 0) for r in PER_CALL_R]


def stripes(cases=None):
    """(case index, stripe, src_len, masked) of every stripe, in the order the engine lists them."""
    out = []
    for i, (r, al) in enumerate(CASES if cases is None else cases):
        out.append((i, 0, STRIPE, (al + STRIPE) % 4 != 0))
        out.append((i, 1, r, (al + r) % 4 != 0))
    return out


def xcd_tile(b, nb):
    """enc_xcd_tile (tape_amd/csrc/kernels.hpp): the task at queue position b of nb."""
    full = nb & ~7
    return b if b >= full else (b & 7) * (full >> 3) + (b >> 3)


def one_workgroup_walk(masked, cases=None):
    """The stripes of the masked (or unmasked) launch of one unsplit batch call over the table, in
    the order a single workgroup runs them: queue positions 0, 1, 2, ... of that launch's jobs."""
    jobs = [s for s in stripes(cases) if s[3] == masked]
    return [jobs[xcd_tile(t, len(jobs))] for t in range(len(jobs))]
