"""fp64 linear-algebra references for the Eigen restatements (test infrastructure).

The restated factorisations (lo_math.h jacobi_svd3 / surfel_fit / so3_project_svd, lo_kdtree.hip smallest_eigvec3d,
lo_exact.h ldlt6_solve / so3_exp) are pinned bit for bit to the oracle's copy of the same algorithm.  This module
holds what is independent of them: input generators, numpy fp64 references (eigh, svd, solve, Rodrigues) and
perturbation bounds.  Every constant below is a derivation allowance, none is a measurement of the code under test.
tests/test_linalg_ref.py runs the checks through the host entry points, tests/test_gpu_linalg_*.py through the
device ones.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)
FLT_MIN = np.float32(1.17549435e-38)

# ====================================================================================================
# A. surfel fit
# ====================================================================================================
VOXEL = 0.5
FACTOR = 3
L1 = VOXEL * FACTOR
SURFEL_FAMILIES = ("planes", "planes_far", "isotropic", "rank_deficient", "axis_aligned")
# families whose voxels must be well enough conditioned for the angle check (a condition on the inputs)
ANGLE_FAMILIES = ("planes", "isotropic", "axis_aligned")


class SurfelCase:
    """points: float32 [n, 3] (one per L0 cell); vox: L1 voxel of each point; keys: int [V, 3] L1 keys; small: the
    indices of voxels with fewer than five children (never fitted)."""

    def __init__(self, points, vox, keys):
        self.points = np.ascontiguousarray(points, np.float32)
        self.vox = np.asarray(vox, np.int64)
        self.keys = np.asarray(keys, np.int64)
        self.m = np.bincount(self.vox, minlength=len(self.keys))
        self.small = np.nonzero(self.m < 5)[0]
        self.fitted = np.nonzero(self.m >= 5)[0]

    def shuffled(self, seed):
        p = np.random.default_rng(seed).permutation(len(self.points))
        return self.points[p]

    def moved(self, t):
        """The case translated by t (whole multiples of the L1 size on dyadic coordinates: exact in fp32)."""
        t = np.asarray(t, np.float64)
        k = t / L1
        assert np.array_equal(k, np.round(k))
        p = self.points.astype(np.float64) + t
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p), "translation is not exact in fp32"
        return SurfelCase(p, self.vox, self.keys + k.astype(np.int64))


def _lattice_keys():
    """400 L1 keys, no two adjacent (a voxel's points never meet a neighbour's)."""
    g = np.stack(np.meshgrid(np.arange(-5, 5), np.arange(-5, 5), np.arange(-2, 2), indexing="ij"), -1).reshape(-1, 3)
    return 2 * g


def _cells_ok(local, lo=0.04, hi=0.96):
    f = local / VOXEL
    fr = f - np.floor(f)
    return np.all((fr > lo) & (fr < hi), axis=-1) & np.all((local > 0) & (local < L1), axis=-1)


def _first_per_cell(local):
    cell = np.floor(local / VOXEL).astype(int)
    code = cell[:, 0] * 9 + cell[:, 1] * 3 + cell[:, 2]
    _, first = np.unique(code, return_index=True)
    return np.sort(first)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _squashed_cloud(rng, n, f, m_target):
    """Points uniform in the voxel, squashed by f along n about a centre, one per L0 cell, at most m_target."""
    for _ in range(200):
        ctr = 0.75 + rng.uniform(-0.1, 0.1, 3)
        p = rng.uniform(0.03, 1.47, (160, 3))
        p = p - (1.0 - f) * np.outer((p - ctr) @ n, n)
        p = p[_cells_ok(p)]
        if len(p) == 0:
            continue
        p = p[_first_per_cell(p)]
        if len(p) >= 5:
            return p[:max(5, m_target)]
    raise RuntimeError("no cloud with five cells")


def _ratio(p):
    d = p - p.mean(0)
    s = np.linalg.eigvalsh(d.T @ d / len(p))
    return s[0] / s[2]


def _line_cloud(rng):
    """Dyadic points on one line (rank 1), one per L0 cell."""
    for _ in range(500):
        d = np.array([rng.integers(2, 5), rng.integers(1, 4), rng.integers(1, 3)], float)[rng.permutation(3)] / 32.0
        d *= rng.choice([-1.0, 1.0], 3)
        s = np.where(d > 0, rng.integers(2, 8, 3), 48 - rng.integers(2, 8, 3)) / 32.0
        p = s + np.arange(0, 48)[:, None] * d
        p = p[_cells_ok(p, 0.1, 0.9)]
        if len(p) == 0:
            continue
        p = p[_first_per_cell(p)]
        if len(p) >= 5:
            return p
    raise RuntimeError("no line with five cells")


def _dyadic_plane_cloud(rng):
    """Exactly coplanar dyadic points (s2 = 0): w = w0 + a u + b v with dyadic slopes, one point per (u, v) column."""
    for _ in range(500):
        a, b = rng.choice([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0], 2)
        w0 = rng.integers(16, 33) / 32.0
        cu, cv = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
        u = cu.ravel() * VOXEL + rng.integers(2, 7, 9) / 16.0
        v = cv.ravel() * VOXEL + rng.integers(2, 7, 9) / 16.0
        w = w0 + a * (u - 0.75) + b * (v - 0.75)
        p = np.stack([u, v, w], 1)[:, rng.permutation(3)]
        p = p[_cells_ok(p, 0.05, 0.95)]
        if len(p) >= 5:
            return p[rng.permutation(len(p))][:rng.integers(5, len(p) + 1)]
    raise RuntimeError("no dyadic plane with five cells")


def _tie_cloud(rng, j):
    """Symmetric dyadic layouts about the voxel centre: the covariance is exactly diagonal in fp32 with two equal
    entries (the sums and the division by m are exact), in every order of the three axes."""
    ctr = np.full(3, 0.75)
    a = [0.375, 0.4375, 0.5][j % 3]
    kind = (j // 3) % 4
    w = (j // 12) % 3
    u, v = [x for x in range(3) if x != w]
    e = np.eye(3)
    if kind == 0:      # s0 = s1 > s2 = 0
        pts = [ctr, ctr + a * e[u], ctr - a * e[u], ctr + a * e[v], ctr - a * e[v]]
    elif kind == 1:    # the same on the cells' diagonals
        pts = [ctr] + [ctr + a * (su * e[u] + sv * e[v]) for su in (-1, 1) for sv in (-1, 1)]
    else:              # kind 2: s0 = s1 > s2 > 0; kind 3: s0 > s1 = s2 (the normal is free in a plane)
        b = 0.3125 if kind == 2 else 0.5625
        pts = [ctr, ctr + a * e[u], ctr - a * e[u], ctr + a * e[v], ctr - a * e[v], ctr + b * e[w], ctr - b * e[w]]
    p = np.asarray(pts)
    assert _cells_ok(p, 0.05, 0.95).all() and len(_first_per_cell(p)) == len(p)
    return p[rng.permutation(len(p))]


def _axis_cloud(rng, j):
    """Axis-aligned product grids, symmetric and dyadic: the fp32 covariance is exactly diagonal (zero sweeps), its
    entries in every order."""
    order = list(itertools.permutations(range(3)))[j % 6]
    layers = 1 + (j // 6) % 3
    half = [6, 7, 8, 9]
    hu, hv = rng.choice(half, 2, replace=False) / 16.0
    cu, cv = 0.75 + rng.integers(-1, 2, 2) / 16.0
    if layers == 1:
        ws = [rng.integers(0, 3) * VOXEL + rng.integers(2, 7) / 16.0]
    elif layers == 2:
        b, k = rng.choice([0.5, 1.0]), rng.integers(1, 4) / 16.0
        ws = [b - k, b + k]
    else:
        cw, hw = 0.75, rng.choice([5, 10]) / 16.0
        ws = [cw - hw, cw, cw + hw]
    g = np.asarray([[x, y, z] for x in (cu - hu, cu, cu + hu) for y in (cv - hv, cv, cv + hv) for z in ws])
    p = g[:, list(order)]
    assert _cells_ok(p, 0.05, 0.95).all() and len(_first_per_cell(p)) == len(p), (j, p)
    return p[rng.permutation(len(p))]


@functools.lru_cache(maxsize=None)
def surfel_case(family: str, with_small: bool = False) -> SurfelCase:
    """About 400 L1 voxels at voxel_size 0.5, factor 3: m in [5, 27] points per voxel, exactly one per L0 cell (a
    child's centroid is then that point to the bit).  Coordinates are dyadic (multiples of 2^-16 near the origin,
    2^-10 far out), so that a translation by whole L1 sizes is exact in fp32.  with_small adds voxels with three
    and four children."""
    assert family in SURFEL_FAMILIES
    rng = np.random.default_rng(1000 + SURFEL_FAMILIES.index(family))
    keys = _lattice_keys().astype(np.int64)
    quantum = 2.0 ** -16
    if family == "planes_far":                        # +-1000 m and +-8000 m: fp32 centroid cancellation
        grp = np.arange(len(keys)) % 4
        off = np.array([666, -666, 5300, -5300])[grp]
        sgn = np.stack([np.ones(len(keys)), np.where(grp % 2, 1, -1), np.ones(len(keys))], 1)
        keys = keys + (off[:, None] * sgn).astype(np.int64)
        quantum = 2.0 ** -10
    pts, vox = [], []
    for j, key in enumerate(keys):
        if family in ("planes", "planes_far"):
            p = _squashed_cloud(rng, _unit(rng), 10 ** rng.uniform(-4, np.log10(0.3)), int(rng.integers(5, 28)))
        elif family == "isotropic":
            while True:
                p = _squashed_cloud(rng, _unit(rng), np.sqrt(10 ** rng.uniform(np.log10(0.05), np.log10(0.9))),
                                    int(rng.integers(8, 28)))
                if 0.05 <= _ratio(p) <= 0.9:
                    break
        elif family == "rank_deficient":
            p = (_line_cloud(rng), _dyadic_plane_cloud(rng), _tie_cloud(rng, j // 3))[j % 3]
        else:
            p = _axis_cloud(rng, j)
        pts.append(key * L1 + p)
        vox.append(np.full(len(p), j))
    if with_small:
        base = len(keys)
        extra = [(2 * i - 8, 2 * (i % 3), 6) for i in range(8)]
        for i, key in enumerate(extra):
            p = _dyadic_plane_cloud(rng)[:3 + i % 2]
            pts.append(np.asarray(key) * L1 + p)
            vox.append(np.full(len(p), base + i))
        keys = np.concatenate([keys, np.asarray(extra, np.int64)])
    p = np.round(np.concatenate(pts) / quantum) * quantum
    vox = np.concatenate(vox)
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p), "coordinates are not exact in fp32"
    # one point per L0 cell, clear of the cell faces, each cell's parent the intended L1 voxel
    k0 = np.floor(p / VOXEL).astype(np.int64)
    fr = p / VOXEL - k0
    assert np.all((fr > 0.02) & (fr < 0.98))
    assert len(np.unique(k0, axis=0)) == len(p)
    assert np.array_equal(np.floor_divide(k0, FACTOR), keys[vox])
    return SurfelCase(p32, vox, keys)


class SurfelRef:
    """Per fitted voxel, from the fp32 points in fp64: mean c, covariance C = sum d d^T / m, eigh -> s0 >= s1 >= s2
    and the eigenvector of s2, and the bounds
        delta = (m + 1) eps32 max|coord|                          (fp32 running sum and division of the centroid)
        E     = (4 m + 16) eps32 trace(C) + delta^2               (fp32 covariance rounding + the Jacobi SVD's backward
                                                                   error + the shift of the fp32 centroid)."""

    def __init__(self, case: SurfelCase):
        self.case = case
        idx = case.fitted
        self.idx = idx
        self.keys = case.keys[idx]
        P = case.points.astype(np.float64)
        V = len(idx)
        self.m = case.m[idx].astype(np.float64)
        self.c = np.zeros((V, 3))
        self.C = np.zeros((V, 3, 3))
        self.maxabs = np.zeros(V)
        order = np.argsort(case.vox, kind="stable")
        bounds = np.searchsorted(case.vox[order], np.arange(len(case.keys) + 1))
        for a, v in enumerate(idx):
            p = P[order[bounds[v]:bounds[v + 1]]]
            self.c[a] = p.mean(0)
            d = p - self.c[a]
            self.C[a] = d.T @ d / len(p)
            self.maxabs[a] = np.abs(p).max()
        w, U = np.linalg.eigh(self.C)
        self.s = np.maximum(w[:, ::-1], 0.0)                      # s0 >= s1 >= s2
        self.vmin = U[:, :, 0]
        self.delta = (self.m + 1) * EPS32 * self.maxabs
        self.E = (4 * self.m + 16) * EPS32 * np.trace(self.C, axis1=1, axis2=2) + self.delta ** 2
        self.planarity = self.s[:, 2] / (self.s[:, 0] + 1e-6)
        self.planarity_tol = 2 * self.E / (self.s[:, 0] + 1e-6) + 4 * EPS32
        gap = self.s[:, 1] - self.s[:, 2]
        with np.errstate(divide="ignore"):
            self.angle_bound = np.where(gap > 0, 2 * self.E / np.where(gap > 0, gap, 1.0), np.inf)
        self.angle_regime = self.angle_bound <= 0.05

    def band(self, thr=0.1):
        """Voxels whose fp64 planarity is too close to thr to call."""
        return np.abs(self.planarity - thr) <= self.planarity_tol


@functools.lru_cache(maxsize=None)
def surfel_ref(family: str, with_small: bool = False, shift: tuple | None = None) -> SurfelRef:
    c = surfel_case(family, with_small)
    return SurfelRef(c.moved(shift) if shift is not None else c)


def _rows_of(ref_keys, keys):
    """Index into the reference of each reported key (-1: unknown)."""
    lut = {tuple(k): i for i, k in enumerate(ref_keys.tolist())}
    return np.asarray([lut.get(tuple(k), -1) for k in np.asarray(keys).tolist()], np.int64)


def check_surfels(ref: SurfelRef, got, expect_all=True, label=""):
    """got = (keys, normals, centroids, planarity) of the voxels that have a surfel.  Every bound of the issue, per
    voxel; returns the reference rows of the reported voxels."""
    keys, nrm, cen, pl = (np.asarray(x) for x in got)
    rows = _rows_of(ref.keys, keys)
    assert np.all(rows >= 0), (label, "surfel on a voxel that has none in the reference", keys[rows < 0][:5])
    assert len(np.unique(rows)) == len(rows), (label, "a voxel reported twice")
    if expect_all:
        assert len(rows) == len(ref.keys), (label, "voxels without a surfel", len(rows), len(ref.keys))
    n = nrm.astype(np.float64)
    c, C, s, E, d = ref.c[rows], ref.C[rows], ref.s[rows], ref.E[rows], ref.delta[rows]

    def worst(x, bound):
        r = x / bound
        i = int(np.argmax(r))
        return f"{label}: worst ratio {r[i]:.3g} at voxel {tuple(keys[i])} (value {x[i]:.3g}, bound {bound[i]:.3g}, m {ref.m[rows][i]:.0f})"

    e = np.abs(cen.astype(np.float64) - c).max(1)
    assert np.all(e <= d), "centroid, " + worst(e, d)
    ln = np.linalg.norm(n, axis=1)
    assert np.all(np.abs(ln - 1) <= 8 * EPS32), "normal length, " + worst(np.abs(ln - 1), np.full(len(ln), 8 * EPS32))
    u = n / ln[:, None]
    ray = np.einsum("vi,vij,vj->v", u, C, u)
    assert np.all(ray <= s[:, 2] + 2 * E), "Rayleigh quotient, " + worst(ray - s[:, 2], 2 * E)
    reg = ref.angle_regime[rows]
    sin = np.linalg.norm(np.cross(u, ref.vmin[rows]), axis=1)
    ab = ref.angle_bound[rows]
    if reg.any():
        assert np.all(sin[reg] <= ab[reg]), "angle, " + worst(np.where(reg, sin, 0.0), np.where(reg, ab, 1.0))
    pe = np.abs(pl.astype(np.float64) - ref.planarity[rows])
    assert np.all(pe <= ref.planarity_tol[rows]), "planarity, " + worst(pe, ref.planarity_tol[rows])
    return rows


def check_threshold_side(ref: SurfelRef, rows, pl, thr=0.1, label=""):
    """Outside the band around thr every voxel's planarity falls on the reference's side."""
    clear = ~ref.band(thr)[rows]
    a = np.asarray(pl, np.float64)[clear] > thr
    b = ref.planarity[rows][clear] > thr
    assert np.array_equal(a, b), (label, "planarity on the wrong side of the threshold", int((a != b).sum()))


def check_survivors(ref: SurfelRef, keys, thr=0.1, label=""):
    """A map built with the production threshold keeps exactly the reference's voxels, apart from the band."""
    rows = _rows_of(ref.keys, keys)
    assert np.all(rows >= 0), (label, "unknown voxel")
    have = np.zeros(len(ref.keys), bool)
    have[rows] = True
    want = ref.planarity <= thr
    clear = ~ref.band(thr)
    bad = np.nonzero((have != want) & clear)[0]
    assert len(bad) == 0, (label, "survivor set differs", ref.keys[bad][:5], ref.planarity[bad][:5])
    assert want[clear].any() and (~want[clear]).any(), (label, "the family does not cross the threshold")


def surfel_input_conditions(family: str):
    """The conditions on the inputs that the checks rely on, from the fp64 reference alone."""
    ref = surfel_ref(family)
    m = ref.case.m[ref.case.fitted]
    assert 350 <= len(ref.keys) <= 450 and m.min() >= 5 and m.max() <= 27 and len(ref.case.points) <= 10000
    if family in ANGLE_FAMILIES:
        share = ref.angle_regime.mean()
        assert share >= 0.9, (family, "angle regime share", share)
    if family == "isotropic":
        r = ref.s[:, 2] / ref.s[:, 0]
        assert r.min() >= 0.05 - 1e-9 and r.max() <= 0.9 + 1e-9
        assert (ref.planarity < 0.1).mean() > 0.1 and (ref.planarity > 0.1).mean() > 0.1
        assert ref.band().mean() <= 0.05, ("threshold band", ref.band().mean())
    if family == "rank_deficient":
        j = np.arange(len(ref.keys))
        assert np.all(ref.s[j % 3 == 0, 1] <= 1e-12 * ref.s[j % 3 == 0, 0]), "the lines are not rank 1"
        assert np.all(ref.s[j % 3 == 1, 2] <= 1e-12 * ref.s[j % 3 == 1, 0]), "the dyadic planes are not rank 2"
        t = j % 3 == 2
        tie = np.minimum(ref.s[t, 0] - ref.s[t, 1], ref.s[t, 1] - ref.s[t, 2]) <= 1e-12 * ref.s[t, 0]
        assert tie.all(), "the tie layouts have no two equal singular values"
    if family == "axis_aligned":
        off = np.abs(ref.C - np.einsum("vii->vi", ref.C)[:, :, None] * np.eye(3)).max((1, 2))
        assert np.all(off <= 1e-12), "the covariance is not diagonal"
        order = {tuple(np.argsort(-np.einsum("ii->i", C), kind="stable")) for C in ref.C}
        assert len(order) == 6, ("orders of the diagonal", order)


SHIFT = (3.0, -4.5, 1.5)           # ApplyTransformAndRehash's translation: whole multiples of the 1.5 m L1 size


def shift_pose():
    T = np.eye(3, 4, dtype=np.float32)
    T[:, 3] = SHIFT
    return T


# ====================================================================================================
# B. KDTree plane fit
# ====================================================================================================
OFFSET_BASE = np.array([5000.0, -5000.0, 5000.0])
PLANE_FAMILIES = ("noisy", "coplanar", "slabs", "strips", "offset", "gate")
MAX_CORR = 1.0
GATE = 0.5
KD_VOXEL = 1e-4                     # the oracle map that carries the cloud: one point per cell of this size


class PlaneCase:
    def __init__(self, cloud, queries, family):
        self.cloud = np.ascontiguousarray(cloud, np.float32)
        self.queries = np.ascontiguousarray(queries, np.float32)
        self.family = family


def _patch(rng, family, centre):
    """One patch of map points about centre in a random orientation (u, v in the plane, w off it), and 50 queries
    above it: off the plane by up to 0.3 m, four of them near the 1 m limit."""
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    a = b = 0.0
    if family == "strips":
        # tight triangles (size eps) strung along a line at 0.2 m: a query's first three neighbours are one triangle
        # (they pass the collinearity gate), the five are nearly a line: sigma2 / sigma1 ~ eps / 0.2 down to 1e-3
        eps = 0.2 * 10 ** rng.uniform(-3, -1)
        cu = np.repeat(np.arange(25) * 0.2, 3)
        ang = np.tile(np.array([0.0, 2.1, 4.2]), 25) + rng.uniform(-0.35, 0.35, 75) + np.repeat(rng.uniform(0, 6.3, 25), 3)
        rad = eps * rng.uniform(0.5, 1.0, 75)
        u, v = cu + rad * np.cos(ang), rad * np.sin(ang)
        w = rng.normal(0, 10 ** rng.uniform(-7, -6), 75)
        j = rng.integers(1, 24, 50)
        qu = j * 0.2 + rng.uniform(-0.03, 0.03, 50)
        qv = rng.uniform(-0.05, 0.05, 50)
    else:
        nu, nv, su, sv, sigma = 10, 10, 0.22, 0.22, 0.0
        if family in ("noisy", "offset"):
            sigma = 10 ** rng.uniform(-3, -1.5)
        elif family == "gate":                                    # stretched cells: the first three neighbours' cross
            nu, nv, su, sv = 14, 7, 0.12, 0.3                     # product spreads over both sides of the 0.5 gate
            sigma = 10 ** rng.uniform(-3, -2)
        elif family == "slabs":
            sigma = 0.3 * 10 ** rng.uniform(-6, -2)               # thickness 1e-6 .. 1e-2 of the neighbours' spread
        gu, gv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
        u = (gu.ravel() + rng.uniform(-0.35, 0.35, gu.size)) * su
        v = (gv.ravel() + rng.uniform(-0.35, 0.35, gv.size)) * sv
        if family == "coplanar":                                  # dyadic coordinates on a dyadic plane: sigma3 = 0
            u, v = np.round(u * 256) / 256, np.round(v * 256) / 256
            Q = np.eye(3)[rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)[:, None]
            a, b = rng.choice([-0.5, -0.25, 0.0, 0.25, 0.5], 2)
            centre = np.round(centre * 64) / 64
            w = a * u + b * v
        else:
            w = rng.normal(0, sigma, u.size)
        qu = rng.uniform(np.percentile(u, 15), np.percentile(u, 85), 50)
        qv = rng.uniform(np.percentile(v, 15), np.percentile(v, 85), 50)
    h = rng.uniform(-0.3, 0.3, 50)
    h[:4] = rng.choice([-1.0, 1.0], 4) * rng.uniform(0.9, 1.1, 4)
    pts = centre + np.stack([u, v, w], 1) @ Q
    q = centre + np.stack([qu, qv, a * qu + b * qv + h], 1) @ Q
    return pts, q


@functools.lru_cache(maxsize=None)
def plane_pose(which: str, far: bool = False):
    """identity, or a 0.01 rad / 4 cm perturbation about the cloud's middle (far: the offset family's)."""
    if which == "identity":
        return np.eye(3, 4, dtype=np.float32).reshape(12)
    rng = np.random.default_rng(77)
    w = rng.normal(size=3)
    w *= 0.01 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    base = OFFSET_BASE if far else np.zeros(3)
    t = np.array([0.03, -0.02, 0.01]) + base - R @ base
    T = np.concatenate([R, t[:, None]], 1)
    return T.astype(np.float32).reshape(12)


def transform_f32(T, pts):
    """The kernel's fp32 transform (lo_device.h transform_pt): ((T0 x + T1 y) + T2 z) + T3, every step rounded."""
    T = np.asarray(T, np.float32).reshape(3, 4)
    p = np.asarray(pts, np.float32)
    out = np.empty_like(p)
    for r in range(3):
        a = T[r, 0] * p[:, 0]
        a = T[r, 1] * p[:, 1] + a
        a = T[r, 2] * p[:, 2] + a
        out[:, r] = T[r, 3] * np.float32(1.0) + a
    return out


def _knn6(cloud64, q64, chunk=256):
    """Brute-force six nearest in fp64: indices and squared distances, ascending."""
    idx = np.empty((len(q64), 6), np.int64)
    d2 = np.empty((len(q64), 6))
    for a in range(0, len(q64), chunk):
        D = ((q64[a:a + chunk, None, :] - cloud64[None, :, :]) ** 2).sum(-1)
        part = np.argpartition(D, 6, axis=1)[:, :6]
        dd = np.take_along_axis(D, part, 1)
        o = np.argsort(dd, axis=1, kind="stable")
        idx[a:a + chunk] = np.take_along_axis(part, o, 1)
        d2[a:a + chunk] = np.take_along_axis(dd, o, 1)
    return idx, d2


TIE_MARGIN = 1e-4                   # relative gap between consecutive squared distances of the six nearest


@functools.lru_cache(maxsize=None)
def plane_case(family: str) -> PlaneCase:
    """About 4k map points in 40 patches, about 2k queries.  Queries with two of their six nearest map points
    within a relative TIE_MARGIN of each other (under either test pose) are left out: ties are
    tests/test_gpu_kdtree.py's business."""
    assert family in PLANE_FAMILIES
    rng = np.random.default_rng(2000 + PLANE_FAMILIES.index(family))
    grid = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    base = OFFSET_BASE if family == "offset" else np.zeros(3)
    cl, qs = [], []
    for g in grid:
        centre = base + (g - [2, 1.5, 0.5]) * 8.0 + rng.uniform(-1, 1, 3)
        p, q = _patch(rng, family, centre)
        cl.append(p)
        qs.append(q)
    cloud = np.concatenate(cl).astype(np.float32)
    q = np.concatenate(qs).astype(np.float32)
    # one map point per KD_VOXEL cell (the oracle's map carries the cloud as L0 centroids)
    cell = np.floor(cloud / np.float32(KD_VOXEL)).astype(np.int64)
    _, first = np.unique(cell, axis=0, return_index=True)
    cloud = cloud[np.sort(first)]
    c64 = cloud.astype(np.float64)
    keep = np.ones(len(q), bool)
    for which in ("identity", "perturbed"):
        qt = transform_f32(plane_pose(which, family == "offset"), q).astype(np.float64)
        _, d2 = _knn6(c64, qt)
        keep &= np.all(np.diff(d2, axis=1) > TIE_MARGIN * d2[:, 1:], axis=1)
    return PlaneCase(cloud, q[keep], family)


class PlaneRef:
    """Per query in fp64: brute-force 5-NN of the fp32-transformed query, the collinearity gate, A = neighbours -
    mean, np.linalg.svd(A) -> normal = V[:, 2], dist = |n . (q' - mean)|, and the conditioning
    kappa = sigma1^2 / (sigma2^2 - sigma3^2) of that eigenvector of A^T A."""

    def __init__(self, case: PlaneCase, which: str):
        self.case = case
        c64 = case.cloud.astype(np.float64)
        self.pose = plane_pose(which, case.family == "offset")
        self.q = transform_f32(self.pose, case.queries).astype(np.float64)
        idx, d2 = _knn6(c64, self.q)
        self.tie_gap = np.min(np.diff(d2, axis=1) / d2[:, 1:], axis=1)
        self.idx = idx[:, :5]
        P = c64[self.idx]                                          # [n, 5, 3]
        v1, v2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        v1 /= np.linalg.norm(v1, axis=1)[:, None]
        v2 /= np.linalg.norm(v2, axis=1)[:, None]
        self.cross = np.linalg.norm(np.cross(v1, v2), axis=1)
        self.gate_pass = ~(self.cross < GATE)
        self.gate_band = np.abs(self.cross - GATE) <= 0.01 * GATE
        self.mean = P.mean(1)
        A = P - self.mean[:, None, :]
        _, S, Vt = np.linalg.svd(A)
        self.S = S
        self.normal = Vt[:, 2, :]
        self.rel = self.q - self.mean
        self.dist = np.abs(np.einsum("ni,ni->n", self.normal, self.rel))
        gap = S[:, 1] ** 2 - S[:, 2] ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            self.kappa = np.where(gap > 0, S[:, 0] ** 2 / np.where(gap > 0, gap, 1.0), np.inf)
        self.term1 = 64 * EPS64 * self.kappa * np.linalg.norm(self.rel, axis=1)
        self.bound = self.term1 + 64 * EPS64 * (np.linalg.norm(self.q, axis=1) + np.linalg.norm(self.mean, axis=1))
        self.dist_band = np.abs(self.dist - MAX_CORR) <= 1e-9 * MAX_CORR
        self.valid = self.gate_pass & ~(self.dist > MAX_CORR)
        self.comparable = ~self.gate_band & ~self.dist_band       # where the valid set must agree
        self.bounded = self.valid & self.comparable & (self.term1 < 1e-6)


@functools.lru_cache(maxsize=None)
def plane_ref(family: str, which: str) -> PlaneRef:
    return PlaneRef(plane_case(family), which)


def plane_input_conditions(family: str, which: str):
    ref = plane_ref(family, which)
    n = len(ref.q)
    assert 3000 <= len(ref.case.cloud) <= 4100 and 1200 <= n <= 4000, (len(ref.case.cloud), n)
    assert ref.tie_gap.min() > TIE_MARGIN, ("distance tie among the six nearest", ref.tie_gap.min())
    assert ref.gate_band.mean() <= 0.02, ("queries at the collinearity gate", ref.gate_band.mean())
    nv = int((ref.valid & ref.comparable).sum())
    assert nv >= 0.5 * n, ("valid queries", nv, n)
    assert (~ref.valid).sum() >= 10, "hardly a query is rejected"
    if family != "strips":
        share = ref.bounded.sum() / nv
        assert share >= 0.95, (family, "share of valid queries under the 1e-6 m conditioning limit", share)
    else:
        assert np.min(ref.S[ref.valid, 1] / ref.S[ref.valid, 0]) < 3e-3, "the strips are not anisotropic"
    if family == "coplanar":
        assert np.median(ref.S[:, 2] / ref.S[:, 0]) <= 1e-12, "the patches are not coplanar"


def check_planes(ref: PlaneRef, valid, res, knn_idx=None, label=""):
    """valid / res: the correspondence flags and fp64 plane distances under test; knn_idx: its 5-NN ids of the
    transformed queries.  Returns (worst |dist - ref| over all valid comparable queries, kappa there, worst kappa)."""
    valid = np.asarray(valid, bool)
    res = np.asarray(res, np.float64)
    if knn_idx is not None:
        bad = np.nonzero((np.asarray(knn_idx, np.int64) != ref.idx).any(1))[0]
        assert len(bad) == 0, (label, "5-NN differs from the fp64 brute force", len(bad), bad[:5])
    cmp_ = ref.comparable
    bad = np.nonzero((valid != ref.valid) & cmp_)[0]
    assert len(bad) == 0, (label, "valid set differs", len(bad), bad[:5], ref.dist[bad[:5]], ref.cross[bad[:5]])
    both = valid & ref.valid & cmp_
    err = np.abs(res - ref.dist)
    chk = both & ref.bounded
    ratio = err[chk] / ref.bound[chk]
    k = int(np.argmax(err * both))
    kmax = float(ref.kappa[both].max())
    note = (f"{label}: worst |dist - ref| {err[k]:.3e} m at kappa {ref.kappa[k]:.3e}; worst kappa {kmax:.3e}; "
            f"worst err/bound {ratio.max():.3g} over {int(chk.sum())} of {int(both.sum())} valid queries")
    assert np.all(ratio <= 1.0), note
    return float(err[k]), float(ref.kappa[k]), kmax, note


def kitti_like_kappa(frame: int = 11):
    """The worst kappa among the valid correspondences of tests/_data.py's KITTI-like case (map of keyframes 0-20,
    scan `frame` at its perturbed pose), with the bound's first term there: how ill-conditioned the A^T A route
    gets on the project's own test map."""
    from tests import _data
    m, pts, Ti, _ = _data.kitti_case(frame)
    case = PlaneCase(m.l0_cloud(), pts, "kitti")
    ref = PlaneRef.__new__(PlaneRef)
    c64 = case.cloud.astype(np.float64)
    q = transform_f32(Ti, case.queries).astype(np.float64)
    idx, _ = _knn6(c64, q)
    P = c64[idx[:, :5]]
    mean = P.mean(1)
    _, S, Vt = np.linalg.svd(P - mean[:, None, :])
    v1, v2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    cr = np.linalg.norm(np.cross(v1 / np.linalg.norm(v1, axis=1)[:, None], v2 / np.linalg.norm(v2, axis=1)[:, None]), axis=1)
    dist = np.abs(np.einsum("ni,ni->n", Vt[:, 2, :], q - mean))
    ok = ~(cr < GATE) & ~(dist > MAX_CORR)
    kappa = S[:, 0] ** 2 / (S[:, 1] ** 2 - S[:, 2] ** 2)
    t1 = 64 * EPS64 * kappa * np.linalg.norm(q - mean, axis=1)
    return float(kappa[ok].max()), float(t1[ok].max()), int(ok.sum())


# ====================================================================================================
# C. exact GN step: fp32 pivoted LDLT, SO3::Exp, SVD re-projection
# ====================================================================================================
TOL = 1e-4


def poses(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]                 # proper rotations
    assert np.all(np.linalg.det(q) > 0.99)
    T = np.concatenate([q, rng.uniform(-50, 50, (n, 3, 1))], axis=2)
    return T.astype(np.float32).reshape(n, 12)


def totals(H, g, cost=None):
    n = len(H)
    tot = np.zeros((n, 43), np.float32)
    tot[:, :36] = np.asarray(H, np.float32).reshape(n, 36)
    tot[:, 36:42] = np.asarray(g, np.float32).reshape(n, 6)
    if cost is not None:
        tot[:, 42] = cost
    return tot


def realistic(rng, n):
    """H, g, cost in fp32 from 30-200 random point-to-plane rows (J, w, r) per system."""
    rows = rng.integers(30, 201, n)
    live = (np.arange(200)[None, :] < rows[:, None]).astype(np.float32)
    J = (rng.normal(size=(n, 200, 6)) * np.array([1, 1, 1, 10, 10, 10])).astype(np.float32)
    w = (rng.uniform(0.05, 1.0, (n, 200)).astype(np.float32)) * live
    r = rng.normal(0, 0.05, (n, 200)).astype(np.float32)
    wJ = w[:, :, None] * J
    H = np.einsum("npc,npr->nrc", J, wJ, dtype=np.float32)          # H[row][col] = sum J[col] * (w J[row])
    wr = w * r
    g = np.einsum("np,npj->nj", wr, J, dtype=np.float32)
    cost = np.einsum("np,np->n", wr, r, dtype=np.float32)
    return totals(H, g, cost)


def pivot_replay(H):
    """The LDLT's pivot choices: the first largest |diagonal| of the rows not yet eliminated (the diagonal entries
    ahead of step k are the input's, only permuted).  Returns transp[5], and whether a step saw a tie at its maximum
    or chose a negative pivot."""
    d = np.abs(np.diagonal(H).astype(np.float32)).copy()
    sgn = np.diagonal(H) < 0
    sgn = sgn.copy()
    tr, tie, neg = [], False, False
    for k in range(5):
        big = k + int(np.argmax(d[k:]))                              # argmax: the first of equal maxima
        tie |= int((d[k:] == d[big]).sum()) > 1
        neg |= bool(sgn[big])
        tr.append(big)
        d[[k, big]] = d[[big, k]]
        sgn[[k, big]] = sgn[[big, k]]
    return tr, tie, neg


def pivoting_systems(rng):
    """Diagonal scales in every order (every pivot choice at every step, exact ties), a quarter of the diagonal
    entries negated (indefinite systems).  Returns (H float32 [n, 6, 6], flip bool [n, 6])."""
    Hs = []
    perms = list(itertools.permutations(range(6)))
    for scales in ([3200, 1600, 800, 400, 200, 100], [800, 800, 400, 400, 200, 200], [500, 500, 500, 500, 500, 500]):
        for p in (perms[j] for j in rng.permutation(len(perms))[:400]):
            A = rng.uniform(-0.3, 0.3, (6, 6))
            np.fill_diagonal(A, 0.0)                                 # equal scales stay exact ties
            H = (A + A.T) * 10 + np.diag(np.asarray(scales, np.float64)[list(p)])
            Hs.append(H)
    Hs = np.asarray(Hs, np.float32)
    n = len(Hs)
    flip = rng.random((n, 6)) < 0.25                                 # negative diagonals (indefinite systems)
    idx = np.arange(6)
    Hs[:, idx, idx] = np.where(flip, -Hs[:, idx, idx], Hs[:, idx, idx])
    return Hs, flip


def graded_indefinite_systems(rng, n=1024):
    """Indefinite systems on which the pivot ORDER decides the accuracy: two diagonal entries of order 1, four of
    1e-6 .. 1e-2 with either sign, in random positions, off-diagonal entries of order 0.3.  Taking the largest
    |diagonal| first keeps the factors small; any tiny diagonal entry taken early makes them ~1e3 .. 1e6 times
    larger.  (The scales of pivoting_systems dominate their off-diagonal part, so every order is stable there.)"""
    A = rng.uniform(-0.3, 0.3, (n, 6, 6))
    H = A + np.transpose(A, (0, 2, 1))
    d = 10 ** rng.uniform(-6, -2, (n, 6)) * rng.choice([-1.0, 1.0], (n, 6))
    for i in range(n):
        big = rng.choice(6, 2, replace=False)
        d[i, big] = rng.uniform(1.0, 4.0, 2) * rng.choice([-1.0, 1.0], 2)
    idx = np.arange(6)
    H[:, idx, idx] = d
    return H.astype(np.float32)


def edge_cases(rng):
    eye = np.eye(6, dtype=np.float32)
    cases = []

    def add(name, H, g):
        cases.append((name, np.asarray(H, np.float32), np.asarray(g, np.float32)))

    g0 = [0.01, -0.02, 0.03, 0.001, 0.002, -0.001]
    add("H = 0", np.zeros((6, 6)), g0)
    add("zero pivot at k = 1", np.diag([1, 0, 0, 0, 0, 0]), g0)
    add("zero pivot at k = 3", np.diag([4, 2, 1, 0, 0, 0]), g0)
    H = 100 * eye + 1.0
    H[2] = H[1]; H[:, 2] = H[:, 1]                                   # rows 1 and 2 equal: a pivot cancels to zero
    add("cancelled pivot", H, g0)
    add("subnormal diagonal", np.diag([1, 1, 1, 1, 1, 1e-39]), g0)
    add("diagonal = FLT_MIN", np.diag([1, 1, 1, 1, float(FLT_MIN), 1]), g0)
    add("diagonal just above FLT_MIN", np.diag([1, 1, 1, 1, 1, 1.2e-38]), g0)
    for th in (0.0, 3e-11, 9.9e-11, 1.01e-10, 3e-8, 9.9e-7, 1.001e-6, 1.5e-6, 1e-4, 2.4e-4, 0.01, 0.3, 0.78, 0.8,
               0.79, 1.2, 2.0, 3.1):
        for axis in ([1, 0, 0], [0.6, -0.64, 0.48]):
            w = th * np.asarray(axis)
            add(f"theta {th}", eye, [-0.01, 0.02, 0.005, -w[0], -w[1], -w[2]])
    for _ in range(40):                                              # angles log-uniform over every Exp branch
        w = rng.normal(size=3)
        w *= 10 ** rng.uniform(-11, 0.5) / np.linalg.norm(w)
        add("theta random", eye, np.concatenate([rng.normal(0, 0.01, 3), -w]))
    # step norms on both sides of tol_t and tol_r (H = I: delta = -g)
    for nt, nr in ((5e-5, 5e-5), (2e-4, 5e-5), (5e-5, 2e-4), (2e-4, 2e-4), (0.99e-4, 0.99e-4), (1.01e-4, 0.99e-4),
                   (0.99e-4, 1.01e-4)):
        add(f"conv {nt} {nr}", eye, [nt, 0, 0, 0, nr, 0])
    for k, v in ((0, np.nan), (7, np.inf), (35, -np.inf), (14, np.nan), (36, np.nan), (38, np.inf), (41, -np.inf)):
        Hn = (50 * eye + 0.5).reshape(36).copy()
        gn = np.asarray(g0, np.float32).copy()
        if k < 36:
            Hn[k] = v
        else:
            gn[k - 36] = v
        add(f"non-finite total {k}", Hn.reshape(6, 6), gn)
    return cases


def oracle_step(tot, pose):
    """The oracle's own GN step from one system's 43 totals: (new pose 12, delta 6), fp32."""
    import oracle
    H, g = tot[:36], tot[36:42]
    delta = oracle.ldlt6_solve(H, -g)
    dw = delta[3:]
    with np.errstate(over="ignore"):                                 # a huge step's norm is inf, as in fp32
        nw = np.sqrt(np.float32(dw[0] * dw[0]) + (np.float32(dw[1] * dw[1]) + np.float32(dw[2] * dw[2])))
    Rd = oracle.so3_normalize(np.eye(3, dtype=np.float32)) if nw < np.float32(1e-10) else oracle.so3_exp(dw)
    B = np.concatenate([Rd, delta[:3].reshape(3, 1)], axis=1).astype(np.float32).reshape(12)
    return oracle.se3_compose(pose, B), delta


def oracle_steps(tot, pose, tol_t=TOL, tol_r=TOL):
    """oracle_step for every system, in lo_exact_solve_both's record layout: uint32 [n, 19] (pose, delta, converged as
    the fp32 norms decide it)."""
    out = np.zeros((len(tot), 19), np.uint32)
    for i in range(len(tot)):
        pn, d = oracle_step(tot[i], pose[i])
        out[i, :12] = np.asarray(pn, np.float32).view(np.uint32)
        out[i, 12:18] = np.asarray(d, np.float32).view(np.uint32)
        out[i, 18] = int(np.linalg.norm(d[:3].astype(np.float64)) < tol_t and np.linalg.norm(d[3:].astype(np.float64)) < tol_r)
    return out


def lower_sym(H):
    """The matrix the LDLT factors: it reads the lower triangle only (the 36 totals are not symmetrised)."""
    H = np.asarray(H, np.float64).reshape(-1, 6, 6)
    L = np.tril(H)
    return L + np.transpose(np.tril(H, -1), (0, 2, 1))


def ldlt_growth(H):
    """fp64 replay of the same pivot order (pivot_replay: the first largest |input diagonal| at each step):
    growth = || |L| |D| |L^T| ||_2 / ||H||_2 and min |D| / max |D| per system."""
    H = lower_sym(H)
    n = len(H)
    growth = np.zeros(n)
    drange = np.zeros(n)
    for s in range(n):
        tr, _, _ = pivot_replay(H[s].astype(np.float32))
        perm = np.arange(6)
        for k, b in enumerate(tr):
            perm[[k, b]] = perm[[b, k]]
        A = H[s][np.ix_(perm, perm)].copy()
        Lm, D = np.eye(6), np.zeros(6)
        for k in range(6):
            D[k] = A[k, k] - (Lm[k, :k] ** 2 * D[:k]).sum()
            if D[k] == 0.0:
                break
            for i in range(k + 1, 6):
                Lm[i, k] = (A[i, k] - (Lm[i, :k] * Lm[k, :k] * D[:k]).sum()) / D[k]
        aD = np.abs(D)
        drange[s] = aD.min() / aD.max() if aD.max() > 0 else 0.0
        nH = np.linalg.norm(H[s], 2)
        growth[s] = np.linalg.norm(np.abs(Lm) @ np.diag(aD) @ np.abs(Lm).T, 2) / nH if nH > 0 else np.inf
    return growth, drange


def rodrigues64(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=1)
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    small = th < 1e-8
    t = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th ** 2 / 6, np.sin(t) / t)
    b = np.where(small, 0.5 - th ** 2 / 24, (1 - np.cos(t)) / t ** 2)
    return np.eye(3) + a[:, None, None] * K + b[:, None, None] * (K @ K)


class SolveSelection:
    """Which systems each check covers, from fp64 alone: finite inputs, non-degenerate pivots (fp64 replay:
    min |D| > 1e-6 max |D|), growth of the replayed factorisation."""

    def __init__(self, tot, pose):
        tot = np.asarray(tot, np.float32)
        self.finite = np.isfinite(tot).all(1) & np.isfinite(np.asarray(pose)).all(1)
        H = np.where(self.finite[:, None, None], lower_sym(tot[:, :36]), np.eye(6))
        self.H = H
        self.growth, self.drange = ldlt_growth(H)
        self.nondegenerate = self.finite & (self.drange > 1e-6)
        self.spd = self.nondegenerate & (np.linalg.eigvalsh(H)[:, 0] > 0)
        self.low_growth = self.growth <= 1e3


def check_solve(tot, pose, out, tol_t=TOL, tol_r=TOL, label="", max_skipped=0.0, expect_all=False):
    """out: uint32 [n, 19] records (new pose 12, delta 6, converged) of the step under test.  Every system that is
    finite and non-degenerate is checked; returns the SolveSelection."""
    tot = np.asarray(tot, np.float32)
    pose = np.asarray(pose, np.float32)
    out = np.asarray(out, np.uint32)
    n = len(tot)
    sel = SolveSelection(tot, pose)
    if expect_all:
        assert sel.nondegenerate.all(), (label, "degenerate systems in a family that should have none")
    pn = out[:, :12].view(np.float32).astype(np.float64).reshape(n, 3, 4)
    d = out[:, 12:18].view(np.float32).astype(np.float64)
    conv = out[:, 18].astype(bool)
    g = tot[:, 36:42].astype(np.float64)
    ok = sel.nondegenerate
    assert np.isfinite(d[ok]).all() and np.isfinite(pn[ok]).all(), (label, "non-finite step")

    def worst(x, bound, mask):
        r = np.where(mask, x / np.where(bound > 0, bound, 1.0), 0.0)
        i = int(np.argmax(r))
        return f"{label}: worst ratio {r[i]:.3g} at system {i} (value {x[i]:.3g}, bound {bound[i]:.3g}, growth {sel.growth[i]:.3g})"

    # residual: backward stability of the 6x6 pivoted LDLT, with the factor growth folded in for indefinite systems
    res = np.linalg.norm(np.einsum("nij,nj->ni", sel.H, d) + g, axis=1)
    nH = np.linalg.norm(sel.H, 2, axis=(1, 2))
    rho = np.where(sel.spd, 1.0, np.maximum(sel.growth, 1.0))
    with np.errstate(invalid="ignore"):                              # degenerate systems (not checked): inf * 0
        bound = 64 * EPS32 * (rho * nH * np.linalg.norm(d, axis=1) + np.linalg.norm(g, axis=1))
    chk = ok & (sel.spd | sel.low_growth)
    skipped = ok & ~chk
    assert skipped.sum() <= max_skipped * n, (label, "systems skipped for growth", int(skipped.sum()), n)
    assert np.all(res[chk] <= bound[chk]), "residual, " + worst(res, bound, chk)
    # the new rotation: orthonormal, proper, and polar(R_old) Exp(delta_w)
    R = pn[:, :, :3]
    Ro = pose.reshape(n, 3, 4)[:, :, :3].astype(np.float64)
    to = pose.reshape(n, 3, 4)[:, :, 3].astype(np.float64)
    Ro = np.where(ok[:, None, None], Ro, np.eye(3))
    R = np.where(ok[:, None, None], R, np.eye(3))
    orth = np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).max((1, 2))
    assert np.all(orth[ok] <= 8 * EPS32), "orthonormality, " + worst(orth, np.full(n, 8 * EPS32), ok)
    assert np.all(np.linalg.det(R)[ok] > 0), (label, "improper rotation")
    U, _, Vt = np.linalg.svd(Ro)
    dw = np.where(ok[:, None], d[:, 3:], 0.0)
    dt = np.where(ok[:, None], d[:, :3], 0.0)
    nw32 = np.linalg.norm(dw, axis=1)
    Rd = np.where((nw32 < 1e-10)[:, None, None], np.eye(3), rodrigues64(dw))     # :427-431: identity below 1e-10
    want = (U @ Vt) @ Rd
    re = np.abs(R - want).max((1, 2))
    assert np.all(re[ok] <= 16 * EPS32), "rotation, " + worst(re, np.full(n, 16 * EPS32), ok)
    # the new translation
    tw = to + np.einsum("nij,nj->ni", Ro, dt)
    te = np.abs(np.where(ok[:, None], pn[:, :, 3], 0.0) - np.where(ok[:, None], tw, 0.0)).max(1)
    tb = 4 * EPS32 * (np.abs(np.where(ok[:, None], to, 0.0)).max(1) + np.abs(dt).max(1))
    assert np.all(te[ok] <= tb[ok]), "translation, " + worst(te, tb, ok)
    # the convergence flag, except within a relative 1e-5 of a tolerance
    nt, nr = np.linalg.norm(dt, axis=1), np.linalg.norm(dw, axis=1)
    near = (np.abs(nt - tol_t) <= 1e-5 * tol_t) | (np.abs(nr - tol_r) <= 1e-5 * tol_r)
    cw = (nt < tol_t) & (nr < tol_r)
    c = ok & ~near
    assert np.array_equal(conv[c], cw[c]), (label, "convergence flag", np.nonzero(c & (conv != cw))[0][:8])
    return sel


def solve_families():
    """name -> (totals [n, 43], poses [n, 12], expect_all, max_skipped): the realistic, pivoting, graded indefinite
    and edge families of the exact step."""
    out = {}
    rng = np.random.default_rng(11)
    out["realistic"] = (realistic(rng, 4096), poses(rng, 4096), True, 0.0)
    rng = np.random.default_rng(12)
    Hs, _ = pivoting_systems(rng)
    out["pivoting"] = (totals(Hs, rng.normal(0, 1.0, (len(Hs), 6)), rng.uniform(0, 1, len(Hs))), poses(rng, len(Hs)),
                       True, 0.1)
    rng = np.random.default_rng(14)
    Hg = graded_indefinite_systems(rng)
    x = rng.normal(0, 0.01, (len(Hg), 6))                            # g = -H x: steps of the realistic families' size
    gg = -np.einsum("nij,nj->ni", lower_sym(Hg), x)
    out["graded"] = (totals(Hg, gg, rng.uniform(0, 1, len(Hg))), poses(rng, len(Hg)), False, 0.1)
    rng = np.random.default_rng(13)
    cases = edge_cases(rng)
    tot = totals([c[1] for c in cases], [c[2] for c in cases], rng.uniform(0, 1, len(cases)))
    out["edge"] = (tot, poses(rng, len(cases)), False, 0.0)
    return out
