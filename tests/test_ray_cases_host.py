"""The scenes of tests/ray_cases.py, checked on the CPU: every cloud realises exactly the ends it intends (the oracle's
own ray_ends says so), the oracle's miss grid equals a second literal march written here from traj_ref.line
(grid_map::LineIterator as a Python loop), every gap scene of family C has an unfree shadow, and the families contain
the ends they list.  tests/test_gpu_ray_ends.py runs the same scenes through the sector kernel."""
import numpy as np
import pytest

import oracle_lib as ol
import ray_cases as rc
import traj_ref
from ray_cases import CLIP, HIT

_LINES = {}


def line_cells(geo, ex, ey):
    """cells of LineIterator(origin, end) as iy * nx + ix, both ends included"""
    key = (geo.grid, geo.origin, ex, ey)
    if key not in _LINES:
        _LINES[key] = np.array([cy * geo.nx + cx for cx, cy in traj_ref.line(*geo.origin, ex, ey)], np.int64)
    return _LINES[key]


def literal_counts(geo, ends):
    """how many of the ends' rays traverse each cell: a hit end excludes its own cell, a clipped end includes it;
    equal (cell, kind) ends count once"""
    cnt = np.zeros(geo.nx * geo.ny, np.int32)
    for ix, iy, kind in sorted({tuple(int(v) for v in e) for e in ends}):
        cells = line_cells(geo, ix, iy)
        cnt[cells if kind == CLIP else cells[:-1]] += 1
    return cnt


def check_ends(geo, og, scene):
    """condition 1: every point's end is the intended one, kind included"""
    kind, ex, ey = og.ray_ends(ol.tf_to_matrix4f(scene.tf), scene.x, scene.y, scene.z)
    got = np.stack([ex, ey, kind.astype(np.int32)], axis=1)
    bad = np.flatnonzero((got != scene.ends).any(axis=1))
    assert bad.size == 0, (scene.name, len(bad), [(scene.ends[i].tolist(), got[i].tolist()) for i in bad[:5]])


def check_literal(geo, og, scene):
    """condition 2: the oracle's miss grid equals the second literal march"""
    want = literal_counts(geo, scene.ends) > 0
    got = rc.oracle_miss(og, scene) > 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (scene.name, len(bad), [geo.octant_ab(int(i) % geo.nx, int(i) // geo.nx) for i in bad[:5]])


# ------------------------------------------------------------------ family A
@pytest.mark.parametrize("grid,origin", [(g, o) for g in (rc.G64, rc.G62) for o in ("centre", "corner", "edge", "near_corner")])
def test_family_a(grid, origin):
    geo, scene = rc.family_a(grid, origin)
    og = rc.oracle_grid(geo)
    check_ends(geo, og, scene)
    hit = scene.ends[scene.ends[:, 2] == HIT]
    assert np.array_equal(np.sort(hit[:, 1] * geo.nx + hit[:, 0]), np.arange(geo.nx * geo.ny))   # every cell once
    clip = scene.ends[scene.ends[:, 2] == CLIP]
    on_origin = (clip[:, 0] == geo.origin[0]) & (clip[:, 1] == geo.origin[1])
    assert {(int(a), int(b)) for a, b, _ in clip} == set(geo.perimeter()) | ({geo.origin} if on_origin.any() else set())
    assert on_origin.sum() == (len(geo.faces(*geo.origin)) + 1 if geo.on_border(*geo.origin) else 0)
    m_base = ol.tf_to_matrix4f(scene.tf)
    z = np.zeros(1, np.float32)
    for f in range(len(scene.ends)):   # one frame per end
        ix, iy, kind = (int(v) for v in scene.ends[f])
        cells = line_cells(geo, ix, iy)
        want = np.zeros(geo.nx * geo.ny, np.uint8)
        want[cells if kind == CLIP else cells[:-1]] = 1
        got = og.raymarch(m_base, scene.x[f:f + 1], scene.y[f:f + 1], z)[0]
        assert np.array_equal(got, want), (scene.name, f, ix, iy, kind)


# ------------------------------------------------------------------ family B
B_SETS = rc.SETS


@pytest.mark.parametrize("name", list(B_SETS))
def test_family_b(name):
    geo, scenes, lists = rc.family_b(*B_SETS[name])
    og = rc.oracle_grid(geo)
    seen = set()
    for s in scenes:
        assert len(s.ends) <= 16
        per_octant = {}
        for ix, iy, kind in s.ends:
            per_octant.setdefault(geo.octant_ab(int(ix), int(iy)), set()).add(int(kind))
            seen.add((int(ix), int(iy), int(kind)))
        # at most one end cell per octant (b = 0 and the diagonal are shared by two of the builder's octants)
        assert max(np.bincount([o for o, _, _ in per_octant], minlength=8)) <= 3
        check_ends(geo, og, s)
        check_literal(geo, og, s)
    # every listed (a, b): as a hit, and on the border also clipped
    n_listed = 0
    for o in range(8):
        ln, jmax = geo.wedge(o)
        for a in (rc.b_majors(ln) if ln >= 1 else []):
            for b in rc.b_minors(a, jmax):
                c = geo.cell(o, a, b)
                assert geo.inside(*c) and (*c, HIT) in seen, (o, a, b)
                assert not geo.on_border(*c) or (*c, CLIP) in seen, (o, a, b)
                n_listed += 1
    assert n_listed == sum(len({(a, b) for a, b, _ in l}) for l in lists)
    longest = max(geo.wedge(o)[0] for o in range(8))
    assert {a for l in lists for a, _, _ in l} >= {longest, longest - 1, longest // 2}
    assert len(scenes) == max(len(l) for l in lists) and n_listed > 800


def test_family_b_short():
    geo, scenes, listed = rc.family_b_short()
    og = rc.oracle_grid(geo)
    assert {a for a, _ in listed} == set(range(3, 41)) and len(scenes) == len(listed) == 76
    for s, (a, b) in zip(scenes, listed):
        assert {geo.octant_ab(int(x), int(y))[1:] for x, y, _ in s.ends} == {(a, b)}
        check_ends(geo, og, s)
        check_literal(geo, og, s)


def test_family_b_minor_offsets_sit_on_sector_boundaries():
    """for every power-of-two sector count 2^j (j = 2 .. 5 in full) the first column of each sector boundary,
    ceil(a k / 2^j), and its two neighbours are in the list"""
    for a in (511, 512, 723, 4990):
        bs = set(rc.b_minors(a, a))
        assert {0, 1, a, a - 1, a // 2, a // 2 - 1, a // 2 + 1} <= bs
        for j in range(2, 6):
            for k in range(1, 1 << j, 2):
                assert -(-a * k // (1 << j)) in bs and a * k // (1 << j) in bs, (a, j, k)


# ------------------------------------------------------------------ family C
C_SETS = B_SETS


def _subset_of_base(base, scene):
    """a gap scene's points are points of its base scene, with the same intended ends"""
    key = lambda s: (s.x.view(np.uint32).astype(np.uint64) << np.uint64(32)) | s.y.view(np.uint32).astype(np.uint64)
    kb, ks = key(base), key(scene)
    order = np.argsort(kb)
    pos = np.searchsorted(kb[order], ks)
    pos = np.minimum(pos, len(kb) - 1)
    return np.array_equal(kb[order][pos], ks) and np.array_equal(base.ends[order][pos], scene.ends)


@pytest.mark.parametrize("name", list(C_SETS))
def test_family_c(name):
    geo = rc.Geo(*C_SETS[name])
    og = rc.oracle_grid(geo)
    keys = rc.family_c_keys()
    assert len(keys) == 3 * 3 * 21
    cx, cy = geo.origin
    iy, ix = np.divmod(np.arange(geo.nx * geo.ny), geo.nx)
    dx, dy = ix - cx, iy - cy
    xmaj = np.abs(dx) >= np.abs(dy)
    a_of = np.where(xmaj, np.abs(dx), np.abs(dy))
    len_of = np.where(xmaj, np.where(dx >= 0, geo.nx - 1 - cx, cx), np.where(dy >= 0, geo.ny - 1 - cy, cy))
    far = 2 * a_of > len_of
    for base in rc.C_BASES:
        bscene = rc.family_c_scene(geo, (base, 0, None))
        check_ends(geo, og, bscene)   # the gap scenes' points are a subset of these
        if base == "band":
            assert len(bscene.ends) > (90_000 if geo.grid == rc.G1024 else 200_000)
        bmiss = rc.oracle_miss(og, bscene) > 0
        bkeys = [k for k in keys if k[0] == base]
        scenes = [rc.family_c_scene(geo, k) for k in bkeys]
        for s in scenes:
            assert 0 < len(bscene.ends) - len(s.ends) and _subset_of_base(bscene, s), s.name
        for s, miss in zip(scenes, rc.map_threads(lambda s: rc.oracle_miss(og, s) > 0, scenes)):
            assert not (miss & ~bmiss).any(), s.name
            shadow = bmiss & ~miss
            assert shadow.any(), s.name                # condition 3: an unfree shadow ...
            assert (shadow & far).any(), s.name        # ... that reaches beyond len/2


def test_family_c_second_march_sample():
    """condition 2 for a fixed sample: every ring and clipped-ring scene of G1024 with the centre origin (126 scenes).
    The base scene's rays are counted once per cell with traj_ref.line; a gap scene is the base without a few rays."""
    geo = rc.Geo(rc.G1024, rc.O1024_CENTRE)
    og = rc.oracle_grid(geo)
    n = 0
    for base in ("ring", "clipped_ring"):
        bscene = rc.family_c_scene(geo, (base, 0, None))
        cnt = literal_counts(geo, bscene.ends)
        assert np.array_equal(rc.oracle_miss(og, bscene) > 0, cnt > 0)
        all_ends = {tuple(int(v) for v in e) for e in bscene.ends}
        for k in rc.family_c_keys():
            if k[0] != base:
                continue
            s = rc.family_c_scene(geo, k)
            removed = all_ends - {tuple(int(v) for v in e) for e in s.ends}
            want = (cnt - literal_counts(geo, list(removed))) > 0
            assert np.array_equal(rc.oracle_miss(og, s) > 0, want), s.name
            n += 1
    assert n >= 20


def test_family_c_threshold_column():
    """the wall cells are hit ends nothing else crosses: free in the gap-less band, unfree in the scene, and the cell
    before each of them (column lf - 1) is free"""
    geo, scenes, walls = rc.family_t()
    og = rc.oracle_grid(geo)
    bmiss = rc.oracle_miss(og, rc.family_c_scene(geo, ("band", 0, None)))
    assert len(scenes) == len(rc.T_COLUMNS)
    for s, w in zip(scenes, walls):
        check_ends(geo, og, s)
        miss = rc.oracle_miss(og, s)
        assert len(w) == 8 * len(rc.T_SECTORS)
        for o, lf, j in w:
            ix, iy = geo.cell(o, lf, j)
            assert geo.octant_ab(ix, iy) == (o, lf, j)
            assert bmiss[iy * geo.nx + ix] == 1 and miss[iy * geo.nx + ix] == 0, (s.name, o, lf, j)
            px, py = traj_ref.line(*geo.origin, ix, iy)[-2]
            assert miss[py * geo.nx + px] == 1, (s.name, o, lf, j)
    check_literal(geo, og, rc.Scene(*scenes[0][:4], *(v[-len(walls[0]):] for v in scenes[0][4:])))   # the wall rays alone


# ------------------------------------------------------------------ family D
def test_family_d():
    geo, scenes, lines = rc.family_d()
    og = rc.oracle_grid(geo)
    assert len(scenes) == len(rc.D_SLOPES) * len(rc.D_COUNTS) * 2 and len(lines) == 8 * len(scenes)
    for s in scenes:
        check_ends(geo, og, s)
        check_literal(geo, og, s)
    assert {n for _, _, _, n, _, _, _ in lines} == {8, 9, 23, 24, 25, 64}
    for o, p, q, n, variant, pts, strangers in lines:
        ln, jmax = geo.wedge(o)
        assert len(set(pts)) == n and all(b * q == a * p and 1 <= a <= ln and b <= jmax for a, b in pts)
        longest = max(pts)
        kmax = min(ln // q, jmax // p if p else ln)
        if variant == "far":
            assert longest == (kmax * q, kmax * p) and pts[-1] == longest
        else:
            assert longest[0] < kmax * q and pts[-1] != longest
        for a, b in strangers:   # beside the line, not on it, and as long as the wedge allows
            assert b * q != a * p and abs(b * q - a * p) <= 2 * q and a >= longest[0] - 3 * q and geo.inside(*geo.cell(o, a, b))


# ------------------------------------------------------------------ family E
def test_family_e():
    geo, scene, long_ab = rc.family_e()
    og = rc.oracle_grid(geo)
    check_ends(geo, og, scene)
    check_literal(geo, og, scene)
    assert len(long_ab) >= 12 and all(a > 4096 and b > 4096 for _, a, b in long_ab)
    assert max(a // 2 + (a - 1) * b for _, a, b in long_ab) > 1 << 24
    assert (scene.ends[:, 2] == CLIP).sum() >= 4 and len(scene.ends) >= 3000 + 12
