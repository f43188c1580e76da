"""The case table of the multi-output rebuild kernel's geometry test
(tests/recover_multi_geometry_cases.py), checked on the CPU: which sub-chunk sizes the recover entry
points can give the kernel at all (against Slicer.geometry, over every object length of a stripe
size), the (G, workgroups) of every call against the launch rule, that every
recover_multi_kernel<NK, G> instance is reached at every row it can be reached at, every claim about
a lost set -- it splits, it parks values in scratch, it fills the 16 flush items, its pair is or is
not lost together -- and the passes the GPU test expects, through the report mode of
tests/native/rec_multi_check.cpp, and that put_out's byte-by-byte branch is never taken.  No device."""
import random

import pytest

import decode_geometry_cases as G
import rec_multi_native as native
import recover_multi_geometry_cases as R
import tape_amd as T


def test_reachable_sub_chunk_sizes():
    """The slicer's geometry of every object length up to 1 MB (every 7th, and both sides of every
    multiple of the stripe size) and of lengths above: the sub-chunk sizes are those of
    reachable_sc, so the rows of 64 to 129 words do not occur."""
    for n, k, d in R.PROFILES:
        s = T.Slicer(T.ClayCoder(n, k, d))
        one, top, prod = R.reachable_sc(k)
        assert top == max(one) and prod == {7: 1430, 8: 1250, 9: 1112, 10: 1000}[k] and top == {7: 144, 8: 126, 9: 112, 10: 100}[k]
        lens = (set(range(1, 1_000_001, 7)) | {m * 100_000 + e for m in range(1, 11) for e in (-1, 0, 1)}) - {1_000_001}
        seen = set()
        for L in sorted(lens):
            g = s.geometry(L)
            sc, ns = int(g.sub_chunk_size), int(g.num_stripes)
            assert (int(g.stripe_size), ns, sc) == G.slicer_geometry(k, L)
            assert sc in one if ns == 1 else sc == top, (k, L, sc)
            assert int(g.slice_len) == ns * sc * R.ALPHA + R.META
            seen.add(sc)
        assert seen == set(one)  # every even size up to sc(100,000), nothing else
        for L in (1_000_001, 1_000_003, 2_000_000, 4 << 20, 100_000_000):
            g = s.geometry(L)
            assert int(g.sub_chunk_size) == prod and int(g.num_stripes) >= 2 and int(g.stripe_size) == 1_000_000
        for want in (254, 256, 258, 512, 514):
            assert want not in one and want not in (top, prod) and "not reachable" in R.REQUESTED[want][1]
        assert R.words(top) <= 64 and R.words(prod) > 128  # one partial wave, or the production row


def test_rows_are_the_geometry_of_their_lengths():
    for n, k, d in R.PROFILES:
        s = T.Slicer(T.ClayCoder(n, k, d))
        rows = R.rows(k)
        for name, (sc, L, ns, _) in rows.items():
            g = s.geometry(L)
            assert (int(g.sub_chunk_size), int(g.num_stripes)) == (sc, ns), (k, name)
            assert R.chunk_size_for(k, R.ALPHA, min(L, int(g.stripe_size))) == sc * R.ALPHA  # no substitution within a row
            assert sc >= 8  # staged (dec_geom_staged): the kernel, not the generic path
        assert rows["smallest"][0] == 8 and rows["tail3"][0] == 10 and R.words(8) == 2 and R.words(10) == 3
        assert rows["widest_tail"][0] % 4 == 2 and rows["widest_whole"][0] % 4 == 0
        assert max(rows["widest_tail"][0], rows["widest_whole"][0]) == rows["stripe3"][0] == R.reachable_sc(k)[1]
        assert len({(r[0], r[2]) for r in rows.values()}) == 6  # six (chunk size, slice length) groups
    assert set(R.REQUESTED) == {8, 10, 254, 256, 258, 512, 514, 1430}
    assert all(row in R.rows(7) for row, _ in R.REQUESTED.values())
    # the word-to-lane edges the production rows give in a large call (G = 2: 128 words a workgroup)
    tails = {k: R.words(R.rows(k)["production"][0]) % 128 for k in (7, 8, 9, 10)}
    assert tails == {7: 102, 8: 57, 9: 22, 10: 122}  # k = 8, 9: the last workgroup's second wave is all aliases
    assert [R.rows(k)["production"][0] % 4 for k in (7, 8, 9, 10)] == [2, 2, 0, 0]  # k = 7, 8 end in a tail word


def test_launch_geometry_and_instances():
    seen, reachable = set(), set()
    for n, k, d in R.PROFILES:
        for row, (sc, L, ns, _) in R.rows(k).items():
            for g in (1, 2):  # the instances this row can run at all
                if R.stage_g(R.words(sc), 1 if g == 1 else 0) == g:
                    reachable.add((k, g, sc))
            for large in (False, True):
                call = R.geometry_call(k, row, large)
                assert call[0][1] == "data_and_parity_across"
                for rotated in (False, True):
                    st = R.call_stats(k, call, rotated)
                    assert st["jobs"] == st["stripes"] == len(call) * ns and st["passes"] == 1
                    assert (st["jobs"] > R.SMALL_JOBS) == large and (not large or st["jobs"] == R.LARGE_JOBS)
                    want = R.GEOMETRY[k][row][large]
                    assert R.launch(sc, st["jobs"]) == want, (k, row, large)
                    g, wgs = want
                    nw = R.words(sc)
                    assert g * wgs * 64 >= nw > (wgs - 1) * g * 64  # every word owned, no empty workgroup
                    assert R.call_instances(k, call, rotated) == {(k, g, sc)}
                    seen.add((k, g, sc))
    assert seen == reachable
    assert {(nk, g) for nk, g, _ in seen} == {(nk, g) for nk in (7, 8, 9, 10) for g in (1, 2)}  # all eight instances
    assert {sc for nk, g, sc in seen if g == 2} == {1430, 1250, 1112, 1000}


def test_lost_set_calls():
    for n, k, d in R.PROFILES:
        sets = R.lost_sets(k)
        assert set(sets) == set(R.PASSES[k]) and ("three_passes" in sets) == (k == 7)
        for name, (avail, lost, why) in sets.items():
            assert why and not set(avail) & set(lost) and len(set(lost)) == len(lost) >= 2
            assert k <= len(avail) and len(lost) <= n - k and max(avail + lost) < n
        assert [len(sets[f"{x}_available"][0]) for x in ("k_plus_1", "k_plus_2", "n_minus_2")] == [k + 1, k + 2, n - 2]
        assert len(sets["all_lost"][1]) == n - k and len(sets["all_lost"][0]) == k
        a, l, _ = sets["column0_pair"]
        assert all(x < R.Q for x in l)
        assert all(x >= R.Q for x in sets["column1_pair"][1])
        d_, p_ = sets["data_and_parity_across"][1]
        assert d_ < k <= p_ and d_ < R.Q <= p_
        for rotated in (False, True):
            rows = R.lost_set_call(rotated)
            assert rows[:2] == ["tail3", "widest_tail"] and (len(rows) == 3) == rotated
            for name in sets:
                st = R.call_stats(k, [(r, name) for r in rows], rotated)
                assert st["multi_launches"] == len(rows) >= 2 and st["jobs"] <= R.SMALL_JOBS  # two DecGroupKeys or three
                assert st["stripes"] == (5 if rotated else 2)


def test_output_length_bound():
    """For every job the engine builds (recover_multi_enqueue: out_len = (nlost - 1) * slice_len + cs,
    a row at slot * slice_len + plane * sc), off + sc <= out_len at the last plane of the last slot:
    put_out's byte-by-byte branch is unreachable from this host code."""
    for n, k, d in R.PROFILES:
        one, top, prod = R.reachable_sc(k)
        for sc in one + [prod, 14300]:
            for ns in (1, 2, 3, 7):
                for nlost in range(1, n - k + 1):
                    assert R.out_len_holds(sc, ns * sc * R.ALPHA + R.META, nlost)  # plane 99's row ends at cs exactly


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = native.build(tmp_path_factory)
    return lambda cases: native.report(exe, [(k, R.mask(a), R.mask(lo), rot, st) for k, a, lo, rot, st in cases])


def test_lost_set_claims(report):
    for n, k, d in R.PROFILES:
        sets = R.lost_sets(k)
        names = list(sets)
        # the passes of every stripe of both layouts, as the GPU test will assert them
        cases = [(k, sets[nm][0], sets[nm][1], True, st) for nm in names for st in range(3)]
        got = report(cases)
        for i, nm in enumerate(names):
            per = got[3 * i:3 * i + 3]
            assert tuple(len(p) for p in per) == R.PASSES[k][nm], (k, nm)
            lost = R.mask(sets[nm][1])
            for st, p in enumerate(per):
                subs = [x["sub"] for x in p]
                assert sum(subs) == sum(set(subs)) and bin(sum(subs)).count("1") == len(sets[nm][1])  # a partition
                for x in p:
                    assert x["rows"] == x["nslots"] + 2 <= 64 and x["max_out"] <= 16 and x["nscratch"] <= 255
                    assert x["noslot"] == len(sets[nm][1]) - bin(x["sub"]).count("1")
            assert sum(x["sub"] for x in per[0]) == lost  # stripe 0 is not rotated: node = slice
        ident = report([(k, sets[nm][0], sets[nm][1], False, 2) for nm in names])
        first = {nm: got[3 * i] for i, nm in enumerate(names)}
        for i, nm in enumerate(names):
            assert ident[i] == first[nm]  # an identity layout's stripes are all stripe 0's
        one = lambda nm: first[nm][0]  # noqa: E731
        for nm in R.ONE_PASS_PAIRS:
            assert len(first[nm]) == 1
        assert one("column0_pair")["finish_both"] > 0 and one("column1_pair")["finish_both"] > 0
        assert one("pair_both_lost")["finish_both"] > 0
        for nm in ("pair_one_lost", "data_and_parity_across"):
            assert one(nm)["finish_both"] == 0 and one(nm)["finish_one"] > 0, (k, nm)
        assert len(first["all_lost"]) >= 2 and all(x["noslot"] > 0 for x in first["all_lost"])
        assert len(first["item_limit"]) == 1 and one("item_limit")["max_out"] == 16
        assert one("scratch")["nscratch"] >= 220 and all(x["nscratch"] > 0 for nm in names for x in first[nm])
        assert max(x["rows"] for x in first["lds_rows"]) == 27 == max(x["rows"] for nm in names for x in first[nm])
        if k == 7:
            assert len(first["three_passes"]) == 3
        # the padding: with more than k slices available the erased set is still n - k nodes
        for nm in ("k_plus_1_available", "k_plus_2_available", "n_minus_2_available"):
            assert len(sets[nm][0]) > k and len(first[nm]) == 1


def test_named_extremes_against_a_seeded_sample(report):
    """The search that found the item_limit, scratch and lds_rows sets, kept as a check: over 1,000
    seeded (available, lost) pairs per profile -- k, k + 1, k + 2 or 18 slices available, 2 to n - k
    of the others lost -- no pass needs more LDS rows, flush items or scratch rows than the named
    sets show.  The most a profile can reach is not proven: the figure is the sample's."""
    for n, k, d in R.PROFILES:
        rnd = random.Random(k)
        cases = []
        for _ in range(1000):
            avail = rnd.sample(range(n), rnd.choice([k, k, k, k + 1, k + 2, n - 2]))
            rest = [i for i in range(n) if i not in avail]
            cases.append((k, avail, rnd.sample(rest, rnd.randint(2, min(len(rest), n - k))), False, 0))
        per_case = report(cases)
        sampled = [x for p in per_case for x in p]
        sets = R.lost_sets(k)
        named = [x for p in report([(k, a, lo, False, 0) for a, lo, _ in sets.values()]) for x in p]
        for key in ("rows", "max_out", "nscratch"):
            assert max(x[key] for x in sampled) <= max(x[key] for x in named), (k, key)
        assert max(x["rows"] for x in sampled) == 27 and max(x["max_out"] for x in sampled) == 16
        assert max(len(p) for p in per_case) <= (3 if k == 7 else 2)
