"""The wave-cooperative reference-exact GN solve (lo_exact.h exact_solve_step_wave, run by wave 0 of every exact PKO
candidate workgroup) against the one-lane exact_solve_step, bit for bit: the new pose, delta and the convergence flag
of lo_exact_solve_both's two forms on the same 43 totals and pose.  The one-lane form is pinned to the oracle by
tests/test_gpu_exact.py; a subset here is also compared with the oracle's own LDLT / SO3::Exp / SE3 product."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

FLT_MIN = np.float32(1.17549435e-38)
TOL = 1e-4


@pytest.fixture(scope="module")
def ctx():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 12)
    yield o
    o.close()


def _solve_both(o, tot, pose, tol_t=TOL, tol_r=TOL):
    from lidar_odometry_amd import lib
    tot = np.ascontiguousarray(tot, np.float32).reshape(-1, 43)
    pose = np.ascontiguousarray(pose, np.float32).reshape(-1, 12)
    n = len(tot)
    assert len(pose) == n
    a = np.full((n, 19), 0xdeadbeef, np.uint32)
    b = np.full((n, 19), 0xfeedf00d, np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = lib().lo_exact_solve_both(o.ctx, tot.ctypes.data_as(fp), pose.ctypes.data_as(fp), n, tol_t, tol_r,
                                   a.ctypes.data_as(up), b.ctypes.data_as(up))
    assert rc == 0, rc
    return a, b


def _assert_same(a, b):
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:8], a[bad[:2]], b[bad[:2]])


def _poses(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.einsum("nii->ni", r))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]                 # proper rotations
    assert np.all(np.linalg.det(q) > 0.99)
    T = np.concatenate([q, rng.uniform(-50, 50, (n, 3, 1))], axis=2)
    return T.astype(np.float32).reshape(n, 12)


def _totals(H, g, cost=None):
    n = len(H)
    tot = np.zeros((n, 43), np.float32)
    tot[:, :36] = np.asarray(H, np.float32).reshape(n, 36)
    tot[:, 36:42] = np.asarray(g, np.float32).reshape(n, 6)
    if cost is not None:
        tot[:, 42] = cost
    return tot


def _realistic(rng, n):
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
    return _totals(H, g, cost)


def _oracle_step(tot, pose):
    H, g = tot[:36], tot[36:42]
    delta = oracle.ldlt6_solve(H, -g)
    dw = delta[3:]
    nw = np.sqrt(np.float32(dw[0] * dw[0]) + (np.float32(dw[1] * dw[1]) + np.float32(dw[2] * dw[2])))
    Rd = oracle.so3_normalize(np.eye(3, dtype=np.float32)) if nw < np.float32(1e-10) else oracle.so3_exp(dw)
    B = np.concatenate([Rd, delta[:3].reshape(3, 1)], axis=1).astype(np.float32).reshape(12)
    return oracle.se3_compose(pose, B), delta


def test_realistic_systems_bitwise(ctx):
    rng = np.random.default_rng(11)
    n = 4096
    tot, pose = _realistic(rng, n), _poses(rng, n)
    a, b = _solve_both(ctx, tot, pose)
    _assert_same(a, b)
    # the hook ran: delta solves H x = -g
    d = a[:, 12:18].view(np.float32).astype(np.float64)
    H = tot[:, :36].reshape(n, 6, 6).astype(np.float64)
    x = np.linalg.solve(H, -tot[:, 36:42].astype(np.float64)[:, :, None])[:, :, 0]
    err = np.linalg.norm(d - x, axis=1) / np.linalg.norm(x, axis=1)
    assert np.median(err) < 1e-4, np.median(err)
    for i in range(0, n, 32):                                        # ... and both equal the oracle's own step
        pn_o, d_o = _oracle_step(tot[i], pose[i])
        np.testing.assert_array_equal(b[i, :12], pn_o.view(np.uint32), err_msg=f"system {i} pose")
        np.testing.assert_array_equal(b[i, 12:18], d_o.view(np.uint32), err_msg=f"system {i} delta")


def _pivot_replay(H):
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


def test_pivoting_bitwise(ctx):
    rng = np.random.default_rng(12)
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
    count = np.zeros((5, 6), int)
    ties = negs = 0
    for H in Hs:
        tr, tie, neg = _pivot_replay(H)
        for k, q in enumerate(tr):
            count[k, q] += 1
        ties += tie
        negs += neg
    for k in range(5):
        for q in range(k, 6):
            assert count[k, q] > 0, ("pivot choice never taken", k, q)
    assert ties > 0 and negs > 0, (ties, negs)
    g = rng.normal(0, 1.0, (n, 6))
    tot = _totals(Hs, g, rng.uniform(0, 1, n))
    pose = _poses(rng, n)
    a, b = _solve_both(ctx, tot, pose)
    _assert_same(a, b)
    for i in range(0, n, 16):
        d_o = oracle.ldlt6_solve(tot[i, :36], -tot[i, 36:42])
        np.testing.assert_array_equal(b[i, 12:18], d_o.view(np.uint32), err_msg=f"system {i} delta")


def _edge_cases(rng):
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


def test_edge_paths_bitwise(ctx):
    rng = np.random.default_rng(13)
    cases = _edge_cases(rng)
    n = len(cases)
    tot = _totals([c[1] for c in cases], [c[2] for c in cases], rng.uniform(0, 1, n))
    tot[-1, 42] = np.nan
    pose = _poses(rng, n)
    a, b = _solve_both(ctx, tot, pose)
    bad = [cases[i][0] for i in np.nonzero((a != b).any(axis=1))[0]]
    assert not bad, bad
    names = [c[0] for c in cases]
    d = a[:, 12:18].view(np.float32)
    assert not d[names.index("H = 0")].any()                         # the zero_all return
    assert d[names.index("subnormal diagonal"), 5] == 0 and d[names.index("diagonal = FLT_MIN"), 4] == 0
    assert d[names.index("diagonal just above FLT_MIN"), 5] != 0
    conv = {nm: int(a[i, 18]) for i, nm in enumerate(names) if nm.startswith("conv")}
    assert conv["conv 5e-05 5e-05"] == 1 and conv["conv 0.0002 5e-05"] == 0 and conv["conv 5e-05 0.0002"] == 0
    assert conv["conv 9.9e-05 9.9e-05"] == 1 and conv["conv 0.000101 9.9e-05"] == 0 and conv["conv 9.9e-05 0.000101"] == 0
    # a non-finite pose as well: the SVD's non-finite return
    pose2 = pose[:8].copy()
    pose2[0, 0] = np.nan; pose2[1, 5] = np.inf; pose2[2, 3] = np.nan; pose2[3, 10] = -np.inf
    a2, b2 = _solve_both(ctx, tot[7:15], pose2)
    _assert_same(a2, b2)


def test_small_scan_end_to_end_bitwise():
    """A 500-point synthetic scan through optimize in exact mode (its PKO launches solve the candidates across wave 0):
    every iteration's log equals the oracle's."""
    from lidar_odometry_amd import IterativeClosestPointOptimizer, synth
    sc = synth.patch_scene(n_patches=60, seed=3, extent=15.0)
    vm = oracle.VoxelMap(0.5, 3, 0.1, True)
    vm.update(synth.sample_patches(sc, 60000, 4, outlier_frac=0.0), np.zeros(3), 1e3, True)
    T = synth.se3(synth.rot_z(0.1), [0.4, -0.2, 0.1])
    pts = synth.transform(np.linalg.inv(T), synth.sample_patches(sc, 500, 5))
    Ti = synth.perturb(T, np.random.default_rng(0))[:3].astype(np.float32).reshape(12)
    ok_o, To_o, it_o, logs_o = oracle.icp_optimize(vm, pts, Ti)
    o = IterativeClosestPointOptimizer(device=0, max_points=1024)
    try:
        o.set_exact(True)
        k, n, c, _ = vm.surfels()
        o.set_surfels(k, n, c)
        ok_g, To_g = o.optimize(None, pts, Ti)
        st = o.get_last_stats()
        # the scan took the fused candidate path: only its PKO launches write candidate records, and the last
        # launch's chosen candidate is the last iteration's GN step
        from lidar_odometry_amd import lib
        rec = np.zeros((256, 48), np.float32)
        ncand = lib().lo_debug_cand_records(o.ctx, rec.ctypes.data_as(C.POINTER(C.c_float)), rec.size)
        assert ncand > 1, ncand
        rec = rec[:ncand].view(np.uint32)
    finally:
        o.close()
    steps = [np.asarray(lg["delta"], np.float32).view(np.uint32) for lg in st.iterations[:st.num_iterations]]
    hit = [(rec[c, 40:46] == d).all() and d.any() for c in range(ncand) for d in steps]
    assert any(hit), "no candidate record holds a logged GN step: the candidates did not solve it"
    assert ok_g == ok_o and st.num_iterations == it_o and it_o >= 2
    for k, (lo, lg) in enumerate(zip(logs_o, st.iterations)):
        for key in ("pose", "H", "g", "delta"):
            np.testing.assert_array_equal(np.asarray(lg[key], np.float32).view(np.uint32),
                                          np.asarray(lo[key], np.float32).view(np.uint32), err_msg=f"iter {k} {key}")
        assert lg["n_corr"] == lo["n_corr"] and lg["scale"] == lo["scale"] and lg["alpha"] == lo["alpha"], k
        assert np.float32(lg["cost"]) == np.float32(lo["cost"]), k
    np.testing.assert_array_equal(np.asarray(To_g, np.float32).reshape(12).view(np.uint32),
                                  np.asarray(To_o, np.float32).reshape(12).view(np.uint32))
