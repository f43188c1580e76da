"""The case table of the LDS-DMA encode's data-end tests (tests/encode_end_cases.py) covers every
class of end position that the kernel treats differently.  No GPU: this checks the table against
the model of the loader's fetch(), and the model against a brute-force restatement."""
import numpy as np

import encode_end_cases as E

ENDS = E.ends()


def test_table_is_small_and_distinct():
    assert 36 <= len(E.CASES) <= 44
    assert len(set(E.CASES)) == len(E.CASES)
    assert all(1 <= r <= E.STRIPE and al in (0, 2) for r, al in E.CASES)


def test_model_against_byte_positions():
    """end() places the last byte: stripe byte r - 1 is column 4 wi + rem - 1 of plane ez of chunk ex,
    the word's rem bytes end the data, and the word lies within the sub-chunk's 358 words."""
    for e in ENDS + [E.end(r, al) for r in range(1, 20_000, 7) for al in (0, 2)]:
        assert e.ex * E.CS + e.ez * E.SC + e.wi * 4 + e.rem == e.r
        assert 0 <= e.ex < E.K and 0 <= e.ez < E.Q * E.Q and 0 <= e.wi < E.WORDS and 1 <= e.rem <= 4
        assert e.wi < E.WORDS - 1 or e.rem <= 2
        o = e.src_al + e.r - e.rem  # the word's address, mod 4 (cs is a multiple of 4)
        assert e.o3 == o % 4 and e.masked == ((o + e.rem) % 4 != 0)


def test_every_chunk():
    assert {e.ex for e in ENDS} == set(range(E.K))


def test_partner_row_against_chunk():
    assert {E.partner_class(e) for e in ENDS} == {"x<ex", "x==ex", "ex<x<=6", "x=7", "x=8", "x=9"}
    # a partner row 7..9 is a level-1 substitution only for a chunk that has level-1 planes: all do
    # (ex <= 6), but the end's own plane is then a level-2 one
    assert all(e.ez >= 70 for e in ENDS if E.partner_class(e) in ("x=7", "x=8", "x=9"))


def test_planes():
    digits = {e.ez % E.Q for e in ENDS}
    assert {0, 9} <= digits and digits & set(range(1, 9))
    assert {0, 1, 99} <= {e.ez for e in ENDS}
    assert {(e.ez & 1, e.src_al) for e in ENDS} == {(0, 0), (0, 2), (1, 0), (1, 2)}
    assert sum(e.ez >= 70 for e in ENDS) >= 3
    for row in (0, 3, 6):
        assert sum(e.ez // E.Q == row for e in ENDS) >= 3, row


def test_row_words():
    assert {0, 1, 63, 64, 255, 256, 356, 357} <= {e.wi for e in ENDS}
    assert {e.rem for e in ENDS if e.wi == 357} == {1, 2}


def test_every_reachable_alignment_triple():
    """(o3, rem, masked) over every r and both src_al, by enumeration; the table has exactly these."""
    r = np.arange(1, E.STRIPE + 1, dtype=np.int64)
    last = r - 1
    ez, wi = last % E.CS // E.SC, last % E.SC // 4
    rem = r - (last // E.CS * E.CS + ez * E.SC + wi * 4)
    reach = set()
    for al in (0, 2):
        o3, masked = (al + 2 * (ez & 1)) & 3, (al + r) % 4 != 0
        reach |= {(int(c) >> 4, int(c) >> 1 & 7, bool(c & 1)) for c in np.unique(o3 << 4 | rem << 1 | masked)}
        for i in range(0, E.STRIPE, 9973):  # the vectorised restatement is the model
            e = E.end(int(r[i]), al)
            assert (e.o3, e.rem, e.masked, e.ez, e.wi) == (o3[i], rem[i], masked[i], ez[i], wi[i])
    assert reach == {(0, 4, False), (2, 2, False), (0, 1, True), (0, 2, True), (0, 3, True), (2, 1, True),
                     (2, 3, True), (2, 4, True)}
    assert {(e.o3, e.rem, e.masked) for e in ENDS} == reach


def test_boundaries():
    rs = {r for r, _ in E.CASES}
    for j in (1, 3, 6):
        assert {j * E.CS, j * E.CS + 1, j * E.CS + 2} <= rs, j
        assert (E.end(j * E.CS, 0).ex, E.end(j * E.CS + 1, 0).ex) == (j - 1, j)
    assert any(r % E.SC == 0 and r % E.CS != 0 and r + 1 in rs for r in rs)
    assert {1, 2, 3, 4, 5} <= rs
    assert E.STRIPE in rs  # a full stripe as an object's last one (2,000,000 bytes are two stripes)


def test_per_call_subset():
    """Slicer.encode's device input is dword aligned: the subset is table cases with src_al = 0 and
    keeps every chunk, every partner class and the half word."""
    sub = E.per_call_cases()
    assert len(sub) >= 12 and len(set(sub)) == len(sub) and set(sub) <= set(E.CASES)
    se = E.ends(sub)
    assert {e.ex for e in se} == set(range(E.K))
    assert {E.partner_class(e) for e in se} == {"x<ex", "x==ex", "ex<x<=6", "x=7", "x=8", "x=9"}
    assert 357 in {e.wi for e in se}
    assert {e.masked for e in se} == {False, True}


def test_one_workgroup_order():
    """With one workgroup per launch the tasks run in queue order.  Neither launch starts with a
    short stripe, so every short stripe -- those ending in the prefetched planes 0 and 1 among them
    -- is prefetched by the task before it, and each launch crosses from a full stripe into a short
    one and back."""
    for masked in (False, True):
        walk = E.one_workgroup_walk(masked)
        assert len(walk) >= 8 and sorted(walk) == sorted(s for s in E.stripes() if s[3] == masked)
        assert walk[0][2] == E.STRIPE
        kinds = [s[2] == E.STRIPE for s in walk]
        steps = set(zip(kinds, kinds[1:]))
        assert (True, False) in steps and (False, True) in steps
        short_after = [walk[t] for t in range(1, len(walk)) if walk[t][2] < E.STRIPE]
        assert any(E.end(s[2], E.CASES[s[0]][1]).ez in (0, 1) for s in short_after)
    short01 = [s for s in E.stripes() if s[2] < E.STRIPE and E.end(s[2], E.CASES[s[0]][1]).ez in (0, 1)]
    first = {E.one_workgroup_walk(m)[0] for m in (False, True)}
    assert short01 and not first & set(short01)


def test_xcd_tile_is_a_permutation():
    for nb in (1, 7, 8, 9, 37, 40, 43, 64):
        assert sorted(E.xcd_tile(b, nb) for b in range(nb)) == list(range(nb))
