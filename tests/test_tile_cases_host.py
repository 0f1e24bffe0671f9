"""The scenes of tests/tile_cases.py, checked on the CPU.  From the layout model: every scene is what it claims to be --
family A holds every (residue, r + L, kind) triple, family C its exact totals and k values, family D listed segments in
round 0 and again in round 1 under k = 1, family E crowded tiles on both sides of the role scan's two ranges.  From the
numpy emulation of the gather and the write-out: the emulation as meant reproduces the oracle's hits and bitmaps for
every scene, and every mutant changes them for at least one scene.  tests/test_gpu_tile_pass.py runs the same scenes
through k_bin_partition and k_bin_tiles."""
import numpy as np
import pytest

import height_band_ref as ref
import oracle_lib as ol
import ray_cases as rc
import tile_cases as tc
from tile_cases import GROUND, HIT


def test_constants_mirror_the_kernel_source():
    """the mirrored constants, read back from the sources they mirror"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hpp = open(os.path.join(root, "grid-vision_amd", "csrc", "gv_launch_frame.hpp")).read()
    hip = open(os.path.join(root, "grid-vision_amd", "csrc", "gv_binning.hip")).read()

    def const(txt, name):
        return int(re.search(r"constexpr \w+ " + name + r" = (\d+)", txt).group(1))
    assert const(hpp, "kBinTileLog") == tc.TILE_LOG and const(hpp, "kBinSplitMax") == tc.SPLIT_MAX
    assert const(hpp, "kBinSplitKeys") == tc.SPLIT_KEYS
    assert const(hip, "kTileThreads") == tc.ROUND and const(hip, "kInLaneKeys") == tc.IN_LANE_KEYS
    assert "uint32_t chunk = 2048;" in hip and "> 1536 && chunk < 8192) chunk *= 2;" in hip
    assert "hi > wb + 32u && hi - wb > kInLaneKeys" in hip
    assert [tc.bin_chunk_for(n) for n in (1, 3145728, 3145729, 6291456, 6291457, 10 ** 8)] == [2048, 2048, 4096, 4096, 8192, 8192]


def test_expected_takes_no_liberties_with_compose():
    """expected() hands compose the finite points and each distinct out-of-map point once; on clouds small enough to
    hand over whole -- NaN and infinite points, repeated out-of-map points, ground returns -- the results are equal"""
    geo = rc.Geo(tc.G300, tc.O300)
    s0 = tc.family_b("ground")[0]
    c = tc.Cloud(geo, len(s0.x) + 700)
    c.x[:len(s0.x)], c.y[:len(s0.x)], c.z[:len(s0.x)] = s0.x, s0.y, s0.z
    at = len(s0.x)
    c.put_base(at + np.arange(300), np.full(300, geo.hix + 4.0), np.full(300, 3.0))      # 300 equal out-of-map points
    c.put_cells(at + 300 + np.arange(6), [3, 4, 5, 6, 7, 8], [9, 9, 9, 9, 9, 9], HIT)
    c.x[at + 300], c.y[at + 301], c.z[at + 302] = np.inf, -np.inf, np.nan
    c.x[at + 303] = np.nan
    for scene in (c.scene("whole"), tc.family_b("hit")[1], tc.c_sparse()):
        e = tc.expected(scene)
        og, m = ol.OGrid(*scene.grid), ol.tf_to_matrix4f(scene.tf)
        hits, cell, kind, ex, ey = ref.compose(og, m, scene.x, scene.y, scene.z, tc.BAND)
        assert np.array_equal(e.hits, hits) and np.array_equal(e.cell, cell) and np.array_equal(e.kind, kind)
        live = kind > 0
        assert np.array_equal(e.ex[live], ex[live]) and np.array_equal(e.ey[live], ey[live])
        assert np.array_equal(e.miss, og.march_ends(m, ex, ey, kind).astype(np.int32))
        bad = ~(np.isfinite(scene.x) & np.isfinite(scene.y) & np.isfinite(scene.z))
        assert (cell[bad] == -1).all() and (kind[bad] == 0).all()
        if scene.name == "whole":
            assert bad.sum() >= 4 and (kind == 2).sum() >= 300


# ------------------------------------------------------------------ family A
@pytest.mark.parametrize("sel", tc.A_KINDS)
def test_family_a_holds_every_residue_length_and_kind(sel):
    scene, exp, lay = tc.reference(("A", sel))
    assert lay.chunk == 2048 and lay.T == 9 and lay.T % 8 and lay.n % 2048 and lay.n >= tc.SPLIT_KEYS
    assert lay.n_helpers >= 1 and (lay.k == 1).all()                      # helpers are launched and find no share
    want_kind = {"hit": 1, "clip": 2, "mixed": 3}[sel]
    sk, s = lay.seg_kind(), lay.r + lay.c
    for r, total in tc.a_combos():
        m = (lay.c > 0) & (lay.r == r) & (s == total)
        if sel == "mixed" and total - r < 2:
            assert m.any(), (r, total)
        else:
            assert (m & (sk == want_kind)).any(), (r, total, sel)
    assert {r for r, _ in tc.a_combos()} == set(range(8))
    # the three gather classes at their edges: r + L = 32 | 33 and 128 | 129 at every residue
    for r in range(8):
        for total, listed, in_lane in ((32, False, False), (33, False, True), (128, False, True), (129, True, False)):
            m = (lay.c > 0) & (lay.r == r) & (s == total)
            assert m.any() and (lay.listed[m] == listed).all() and (lay.in_lane[m] == in_lane).all(), (r, total)
    # L = 0 between two non-empty segments; a chunk whose 2048 keys are all in one tile; a ragged last chunk with keys
    nonempty = lay.c > 0
    before, after = np.cumsum(nonempty, axis=1) - nonempty > 0, np.cumsum(nonempty[:, ::-1], axis=1)[:, ::-1] - nonempty > 0
    assert (~nonempty & before & after).any()
    assert (lay.c == 2048).any()
    assert lay.c[-1].sum() > 0 and lay.n - (lay.n_wg - 1) * lay.chunk == 777
    # repeated cells, word-edge cells and the last valid column and row of the partial tiles
    assert exp.hits.max() > 1 or sel == "clip"
    lx, ly = lay.kx & 127, lay.ky & 127
    for e in tc.EDGES:
        assert (lx == e).any() and (ly == e).any(), e
    assert (lay.kx == lay.geo.nx - 1).any() and (lay.ky == lay.geo.ny - 1).any()
    # full windows that hold a clipped-end key exist whenever clipped ends do (the fast path's other condition)
    if sel != "hit":
        assert (exp.kind == 2).sum() > 1000 and exp.clip_bm.sum() > 100
    else:
        assert (exp.kind == 2).sum() == 0


# ------------------------------------------------------------------ family B
@pytest.mark.parametrize("sel", ("hit", "ground"))
def test_family_b_cells_borders_and_corners(sel):
    s1, e1, lay1 = tc.reference(("B", sel, 0))
    s2, e2, lay2 = tc.reference(("B", sel, 1))
    geo = lay1.geo
    bm = e1.hit_bm if sel == "hit" else e1.clip_bm
    for t in range(lay1.T):
        x0, y0, vw, vh = tc.tile_extent(geo, t)
        for a in tc.EDGES:
            for b in tc.EDGES:
                if a < vw and b < vh:
                    assert bm[y0 + b, x0 + a], (t, a, b)
        assert bm[y0, x0] and bm[y0 + vh - 1, x0 + vw - 1] and bm[y0, x0 + vw - 1] and bm[y0 + vh - 1, x0]
        assert bm[y0 + 31, x0 + 30] and not bm[y0 + 32, x0 + 30]          # rows 31 and 32 of a column differ
    if sel == "ground":
        assert e1.hits.sum() == 0
    out = e1.cell < 0
    clip = (e1.kind == 2) & out
    assert clip.sum() >= 60
    ex, ey = e1.ex[clip], e1.ey[clip]
    for m in (ex == 0, ex == geo.nx - 1, ey == 0, ey == geo.ny - 1):
        assert m.sum() >= 10
    assert {(0, 0), (geo.nx - 1, 0), (0, geo.ny - 1), (geo.nx - 1, geo.ny - 1)} <= set(zip(ex.tolist(), ey.tolist()))
    assert not e1.hit_bm[geo.ny:].any() and not e1.hit_bm[:, geo.nx:].any() and not e1.clip_bm[geo.ny:].any()
    # frame 2 is sparse and different: bits of frame 1 that frame 2 must not show, in every quadrant of the bitmaps and
    # in the words that hold the last valid columns and rows
    assert len(s2.x) < 20 and 0 < e2.clip_bm.sum() < 10 and 0 < e2.hit_bm.sum() < 10
    gone_h, gone_c = e1.hit_bm & ~e2.hit_bm, e1.clip_bm & ~e2.clip_bm
    assert gone_c[:, 288:300].any() and gone_c[288:300, :].any() and (gone_h if sel == "hit" else gone_c)[:128, :128].any()
    assert (e2.hit_bm & ~e1.hit_bm).any() or (e2.clip_bm & ~e1.clip_bm).any()


# ------------------------------------------------------------------ family C
@pytest.mark.parametrize("name", list(tc.C_SPECS))
def test_family_c_totals_and_shares_are_exact(name):
    scene, exp, lay = tc.reference(("C", name))
    n, spec = tc.C_SPECS[name]
    assert lay.n == n and lay.chunk == 2048 and lay.n_helpers == n // 32768
    for t in range(lay.T):
        nh, ng, no = spec.get(t, (0, 0, 0))
        assert lay.n_hit[:, t].sum() == nh and lay.n_clip[:, t].sum() == ng + no, t
        assert lay.total[t] == nh + ng + no and lay.k[t] == min(8, max(1, -(-(nh + ng + no) // 32768)))
    extra = int((lay.k - 1).sum())
    k = {t: int(lay.k[t]) for t in spec}
    if name == "t32768_32769":
        assert k == {1: 1, 5: 2}
    elif name == "t65536_65537":
        assert k == {2: 2, 6: 3}
    elif name == "t262144_262145":
        assert k == {0: 8, 8: 8} and lay.k_raw[0] == 8 and lay.k_raw[8] == 9 and lay.n_wg >= 9
    elif name == "two_32769_all_helpers":
        assert k == {3: 2, 7: 2} and lay.n_helpers == extra == 2           # every helper has a share
    elif name == "two_32769_spare_helpers":
        assert k == {3: 2, 7: 2} and lay.n_helpers == 5 and extra == 2     # helpers left over: they return at t < 0
    elif name == "k2_k3_k5":
        assert k == {0: 2, 2: 1, 4: 3, 8: 5} and lay.T - 1 == 8 and tc.tile_extent(lay.geo, 8)[2:] == (44, 44)
    elif name == "border_only":
        assert k == {3: 4, 4: 1} and lay.n_hit[:, 3].sum() == 0
        m = lay.t == 3
        assert lay.clip[m].all() and len(set(zip(lay.kx[m].tolist(), lay.ky[m].tolist()))) == 1
        assert exp.hits.reshape(300, 300)[128:256, :128].sum() == 0        # the shared tile's histogram is empty
        assert (exp.cell[lay.pt[m]] == -1).all()                          # and every one of its keys an out-of-map point
    elif name == "hits40k_clips40k":
        assert k == {1: 1, 4: 3}
    assert lay.n_helpers >= extra
    # every share of a shared tile gets chunks: sp < n_wg
    assert lay.n_wg >= 8


def test_family_c_sequence_ends_sparse():
    assert all(name in tc.C_SPECS for name in tc.C_SEQUENCE) and len(tc.C_SEQUENCE) == 3
    last = tc.reference(("C", tc.C_SEQUENCE[-1]))[1]
    sp_scene, sp, lay = tc.reference(("Csparse",))
    assert (lay.k == 1).all() and lay.n_helpers == 0 and len(lay.pt) == 6
    assert (last.hit_bm & ~sp.hit_bm).sum() > 10000 and (last.clip_bm & ~sp.clip_bm).sum() > 10000


# ------------------------------------------------------------------ family D
@pytest.mark.parametrize("n", tc.D_SIZES)
def test_family_d_rounds_and_chunk_size(n):
    scene, exp, lay = tc.reference(("D", n))
    X, Y, S = tc.D_X, tc.D_Y, tc.D_SHARED
    s = lay.r + lay.c
    assert lay.k[S] == 2 and lay.total[S] == 40000
    # the condition of the second round: every other tile is unshared, so its one share walks every chunk
    for t in range(lay.T):
        if t != S:
            assert lay.total[t] <= tc.SPLIT_KEYS and lay.k[t] == 1, t
    if n == 3145729:
        assert lay.chunk == 4096 and lay.n_wg == 769 and lay.rounds.max() == 1
        # the same blocks, now halves of 4096-point chunks: segments fed by second halves only, and by both halves
        half = (lay.pt % 4096) >= 2048
        for t in (X, Y):
            m = lay.t == t
            lo_half = np.bincount(lay.w[m], weights=~half[m], minlength=lay.n_wg) > 0
            hi_half = np.bincount(lay.w[m], weights=half[m], minlength=lay.n_wg) > 0
            assert (hi_half & ~lo_half).any() and (hi_half & lo_half).any(), t
        assert lay.listed[:, X].sum() >= 20 and lay.c[-1].sum() == 1       # and a last chunk of one point
        return
    assert lay.chunk == 2048 and lay.n_wg == (1075 if n == 2200000 else 1536) and lay.n_wg > tc.ROUND
    assert (lay.rounds[:, [t for t in range(lay.T) if t != S]] == 2).all() and (lay.rounds[:, S] == 1).all()
    w = np.arange(lay.n_wg)
    for rnd, sel in ((0, w < 1024), (1, w >= 1024)):
        m = sel & lay.listed[:, X]
        assert m.sum() == 20 and (lay.round[m, X] == rnd).all() and (abs(s[m, X] - 600) <= 10).all()
        assert len(set(lay.r[m, X].tolist())) == 8 and (lay.seg_kind()[m, X] == 3).all()
    assert lay.listed[1023, X] and lay.listed[1024, X]                   # the last descriptor of round 0, the first of round 1
    assert lay.c[:1024, Y].sum() == 0 and lay.c[1024:, Y].sum() == lay.total[Y] > 0
    wy = lay.c[:, Y] > 0
    assert (wy & (s[:, Y] <= 32)).any() and (wy & lay.in_lane[:, Y]).any() and (wy & lay.listed[:, Y]).any()
    assert (lay.round[wy, Y] == 1).all()
    if n % 2048:
        assert lay.c[-1].sum() > 0


# ------------------------------------------------------------------ family E
def test_family_e_more_than_1024_tiles():
    scene, exp, lay = tc.reference(("E",))
    assert (lay.geo.nx, lay.geo.ny) == (2080, 7712) and (lay.tiles_x, lay.tiles_y, lay.T) == (17, 61, 1037)
    assert not scene.ray and not exp.clip_bm.any() and lay.T % 8
    per = (lay.T + 1023) // 1024
    assert per == 2
    crowded = {int(t): int(lay.k[t]) for t in np.flatnonzero(lay.k > 1)}
    assert crowded == {300: 2, 1030: 3} and lay.total[300] == 40000 and lay.total[1030] == 70000
    assert 1030 // per >= 512 > 300 // per          # owned by lanes of different halves of the scan, tile 1030 past index 1024
    assert lay.n_helpers == 3 == int((lay.k - 1).sum())
    for t in (0, lay.T - 1, lay.T // 2, 1023, 1024):
        assert lay.total[t] == 100, t
    assert 2000 <= len(lay.pt) - 110000 <= 6000 and exp.hits.sum() == len(lay.pt)


# ------------------------------------------------------------------ the emulation and its mutants
@pytest.mark.parametrize("key", tc.ALL_KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_emulation_as_meant_reproduces_the_oracle(key):
    scene, exp, lay = tc.reference(key)
    assert not tc.differs(tc.emulate(lay), exp)
    assert exp.hits.sum() == (lay.n_hit.sum()) and lay.c.sum() == len(lay.pt)


def _detecting(mutant):
    found = []
    for key in tc.ALL_KEYS:
        scene, exp, lay = tc.reference(key)
        prev = None
        if mutant == "stale_padding_clip":
            if key[0] != "B" or key[2] != 1:
                continue
            prev = tc.emulate(tc.reference(("B", key[1], 0))[2])
        if tc.differs(tc.emulate(lay, mutant, prev), exp):
            found.append(key)
    return found


@pytest.mark.parametrize("mutant", tc.MUTANTS)
def test_every_mutant_is_seen_by_a_scene(mutant):
    found = _detecting(mutant)
    assert found, mutant
    fams = {k[0] for k in found}
    want = {"drop_key_at_wb32": "A", "listed_at_128_one_short": "A", "fast_path_on_clip_window": "A", "no_nlong_reset": "D",
            "k8_one_share_fewer": "C", "k_uncapped": "C", "t_rows_31_32_swapped": "B", "stale_padding_clip": "B"}[mutant]
    assert want in fams, (mutant, found)
    if mutant == "no_nlong_reset":
        assert ("D", 2200000) in found and ("D", 3145728) in found and ("D", 3145729) not in found
    if mutant in ("k8_one_share_fewer", "k_uncapped"):
        assert ("C", "t262144_262145") in found
    if mutant == "fast_path_on_clip_window":
        assert ("A", "clip") in found and ("A", "mixed") in found and ("A", "hit") not in found


def test_mutants_hit_what_they_aim_at():
    """each gather mutant changes exactly the segments of its branch: counted on family A"""
    scene, exp, lay = tc.reference(("A", "hit"))
    base = tc.emulate(lay)
    s = lay.r + lay.c
    d1 = int(base.hits.sum() - tc.emulate(lay, "drop_key_at_wb32").hits.sum())
    assert d1 == int((lay.in_lane).sum())                                 # one key per in-lane segment, none of a listed one
    d2 = int(base.hits.sum() - tc.emulate(lay, "listed_at_128_one_short").hits.sum())
    assert d2 == int(((lay.c > 0) & (s == 128)).sum()) == 8
