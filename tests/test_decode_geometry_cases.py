"""The case tables of the table-kernel and generic-kernel geometry tests (tests/decode_geometry_cases.py),
checked on the CPU: sub-chunk sizes and word counts of every length, the expected waves per workgroup
and workgroups per stripe against the launch rules, that every (NK, G) instance of dec_stage_kernel
and every MAXE instance of gpe_kernel is covered, the generic kernel's LDS sizes against its 64 KiB
launch branch, and -- through tests/native/dec_stage_sets.cpp, ClayHost's own plane-program compiler --
which survivor sets the table kernel can run at all.  No device."""
import os
import subprocess

import pytest

import decode_geometry_cases as G
import tape_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_sub_chunk_sizes_and_lengths():
    for params in G.TABLE_PROFILES:
        n, k, d = params
        assert G.clay_layout(n, k, d) == (G.Q, 2, 0, G.ALPHA)
        coder = T.ClayCoder(n, k, d)
        for sc, (nw, _, _, _) in G.TABLE_SC.items():
            cs = sc * G.ALPHA
            assert nw == G.words(sc) == -(-sc // 4)
            ls = G.lengths(k, G.ALPHA, sc)
            assert len(ls) == 6 and len({L for L, _ in ls}) == 6
            assert ls[0] == (k * cs, True) and coder.chunk_size_for(k * cs) == cs
            for L, natural in ls:
                assert 0 < L <= k * cs and L <= G.meta_stripe(L)
                assert (coder.chunk_size_for(L) == cs) == natural, (params, sc, L)
            # the four row ends: inside the last chunk, 1, 2, 3 and 5 bytes into a word, all four
            # byte alignments of the end of the output share
            ends = [(L - (k - 1) * cs) % sc for L, _ in ls[1:5]]
            assert [e % 4 if e % 4 else 4 for e in ends][:3] == [1, 2, 3] and ends[3] == 5, (sc, ends)
            assert all((k - 1) * cs < L < k * cs for L, _ in ls[1:5])
            assert {L % 4 for L, _ in ls} == {0, 1, 2, 3}
            assert ls[5][0] == (k - 1) * cs + 1
            if sc >= 2 * k + 2:  # a short last stripe's share, not a length of this chunk size
                assert not ls[5][1]


def test_table_row_end_words():
    assert G.row_ends(8) == [(0, 1, 1), (1, 1, 2), (4, 1, 3), (7, 0, 5)]
    assert G.row_ends(10) == [(0, 2, 1), (1, 1, 2), (4, 1, 3), (7, 0, 5)]     # word 2 is the 2-byte tail word
    assert G.row_ends(258) == [(0, 64, 1), (1, 63, 2), (4, 63, 3), (7, 0, 5)]  # word 64: the tail word alone in wave 1
    assert G.row_ends(514) == [(0, 128, 1), (1, 63, 2), (4, 64, 3), (7, 0, 5)]
    assert G.row_ends(1430) == [(0, 357, 1), (1, 63, 2), (4, 64, 3), (7, 0, 5)]


def test_table_launch_geometry_and_instances():
    seen = set()
    for params in G.TABLE_PROFILES:
        k = params[1]
        for sc, (nw, small, large, _) in G.TABLE_SC.items():
            for is_large, want in ((False, small), (True, large)):
                call = G.table_call(params, sc, is_large)
                stripes = len(call)
                assert (stripes > G.SMALL_STRIPES) == is_large
                assert stripes == G.LARGE_OBJECTS if is_large else stripes <= G.SMALL_STRIPES
                gmax = 0 if stripes > G.SMALL_STRIPES else 1  # decode_enqueue: a.gmax = small_dec ? 1 : 0
                g, wgs = G.stage_g(nw, gmax), G.stage_wgs(nw, gmax)
                assert (g, wgs) == want, (sc, is_large, g, wgs)
                assert g * wgs * 64 >= nw > (wgs - 1) * g * 64  # every word owned, no empty workgroup
                seen.add((k, g))
    assert seen == {(nk, g) for nk in (7, 8, 9, 10) for g in (1, 2)}
    # the edges the table names
    assert G.stage_wgs(G.words(514), 0) == 2 and 514 - 1 * 2 * 256 == 2   # lseg of the second G = 2 workgroup
    assert G.words(258) == 65 and G.words(1026) == 257 and 8 // 4 == 2


def test_survivor_sets():
    for params in G.TABLE_PROFILES + list(G.GENERIC):
        n, k, _ = params
        sets = G.survivor_sets(n, k, 8)
        assert sets[0] == tuple(range(k)) and sets[1] == tuple(range(n - k, n))
        assert [len(s) for s in sets[:5]] == [k, k, k, k, k + 2]
        assert len(set(sets)) == len(sets)
        assert all(len(set(s)) == len(s) and 0 <= min(s) and max(s) < n for s in sets)
    for params in G.TABLE_PROFILES:
        for large in (False, True):
            sets = G.table_sets(params, large)
            assert len(sets) == (11 if large else 5 - len(G.NO_PLANE_PROGRAM.get(params, [])))
            assert any(len(s) == params[1] + 2 for s in sets)


def test_recover_table():
    for params in G.TABLE_PROFILES:
        n, k, d = params
        s = T.Slicer(T.ClayCoder(n, k, d))
        for want, (sc, length) in G.RECOVER_SC[k].items():
            stripe, ns, got = G.slicer_geometry(k, length)
            g = s.geometry(length)
            assert (int(g.stripe_size), int(g.num_stripes), int(g.sub_chunk_size)) == (stripe, ns, got)
            assert got == sc >= 8, (params, want, sc, got)
            assert ns == {10: 1, 258: 1, 514: 3, 1430: 2}[want]
            if want in (10, 258):
                assert sc % 4 == want % 4 == 2  # a tail word
        cases = G.recover_cases(params)
        assert len(cases) == (10 if k < 10 else 8)
        for lost, peers in cases:
            assert lost not in peers and len(peers) in (k, k + 3)
        losts = {lost for lost, _ in cases}
        assert any(x < k for x in losts) and any(x >= G.Q for x in losts)          # data (column 0), column-1 parity
        assert k == G.Q or any(k <= x < G.Q for x in losts)                         # column-0 parity


@pytest.fixture(scope="module")
def stage_sets(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("native") / "dec_stage_sets")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++20", "-I", os.path.join(ROOT, "tape_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "dec_stage_sets.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(params, lines):
        text = "".join(f"{sum(1 << i for i in s):x} {lost} {ns} {rot}\n" for s, lost, ns, rot in lines)
        r = subprocess.run([exe] + [str(x) for x in params], input=text, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [int(x) for x in r.stdout.split()]
        assert len(out) == len(lines)
        return out
    return run


def test_plane_programs_of_the_case_sets(stage_sets):
    """Every survivor set of a table-kernel call has a plane program (else the call would run the
    generic kernel), the sets listed as having none have none, and every node-recover case has one
    on every stripe (else recover_batch would decode and re-encode instead)."""
    for params in G.TABLE_PROFILES:
        k = params[1]
        sets = sorted(set(G.table_sets(params, False) + G.table_sets(params, True)))
        assert stage_sets(params, [(s, -1, 1, 0) for s in sets]) == [1] * len(sets), params
        none = G.NO_PLANE_PROGRAM.get(params, [])
        assert stage_sets(params, [(s, -1, 1, 0) for s in none]) == [0] * len(none), params
        lines = [(peers, lost, 3, 1) for lost, peers in G.recover_cases(params)]
        assert stage_sets(params, lines) == [1] * len(lines), params
    assert G.NO_PLANE_PROGRAM[(20, 10, 19)] == [tuple(range(10, 20))]  # one whole column survives


def test_generic_instances_and_lds():
    seen = set()
    for params, (maxe, lds, over, scs) in G.GENERIC.items():
        n, k, d = params
        q, t, nu, alpha = G.clay_layout(n, k, d)
        coder = T.ClayCoder(n, k, d)
        assert (coder.alpha(), coder.m()) == (alpha, n - k)
        assert G.gpe_instance(n - k) == maxe  # every pattern is padded to n - k erasures
        assert G.gpe_lds(maxe, alpha, t) == lds and (lds > 64 * 1024) == over, (params, G.gpe_lds(maxe, alpha, t))
        seen.add((maxe, over))
        for sc in scs:
            ls = G.lengths(k, alpha, sc)
            assert ls[0] == (k * sc * alpha, True) and coder.chunk_size_for(k * sc * alpha) == sc * alpha
            for L, natural in ls:
                assert (coder.chunk_size_for(L) == sc * alpha) == natural and 0 < L <= G.meta_stripe(L)
            assert len({L for L, _ in ls}) == 6 and len(G.generic_call(params, sc)) == 30
    assert seen == {(4, False), (8, False), (13, True), (13, False), (20, False)}
    assert G.GENERIC[(20, 5, 14)][1] == 64_216 <= 64 * 1024  # just under the branch
    # the 4-word block edge: sc = 14, 16 fill one block, 18 puts one live word into a second
    blocks = {sc: -(-max(1, G.words(sc)) // G.GPE_WORDS) for sc in G.GENERIC_SC}
    assert blocks == {2: 1, 4: 1, 6: 1, 14: 1, 16: 1, 18: 2, 34: 3, 130: 9}
    assert G.words(18) == 5 and G.words(130) == 33 and 130 % 4 == 2
    for params, sc in G.GENERIC_ROTATED_SC.items():
        s = T.Slicer(T.ClayCoder(*params))
        g = s.geometry(G.GENERIC_ROTATED_LEN)
        assert (int(g.num_stripes), int(g.sub_chunk_size)) == (3, sc)
