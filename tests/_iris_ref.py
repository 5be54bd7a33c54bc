"""Numpy restatement of the LiDAR-Iris definitions the GPU detector is pinned to (test infrastructure).

The pin is the MATHEMATICAL definition in fp64 (np.fft), not OpenCV's fp32 results: the image (GetIris), the
log-Gabor encode, the masked Hamming distance at a column shift, its minimum over all 360 shifts, and the
detector's candidate selection rule.  Written from the definitions in include/lo_iris.h; shares no code with the
library.
"""
from __future__ import annotations

import numpy as np

ROWS, COLS, SCALES = 80, 360, 4
BITS = 2 * SCALES * ROWS * COLS


# ------------------------------------------------------------------------------------------------ image
def bins_f64(pts):
    """The three binned quantities in fp64: (range, yaw + 0.5, z + 5) -- for edge-margin checks."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    rng = np.hypot(p[:, 0], p[:, 1])
    yaw = np.degrees(np.arctan2(p[:, 1], p[:, 0])) + 180.0 + 0.5
    return rng, yaw, p[:, 2] + 5.0


def edge_margin(pts) -> float:
    """Smallest fp64 distance of any binned quantity from an integer (a bin edge of floor / ceil).  A range of
    exactly 0 (the point (0, 0, z)) is exempt: sqrt(0) = 0 in every precision, so its bin is not in doubt."""
    rng, yaw, arc = bins_f64(pts)
    rng = rng[rng != 0.0]
    return min(float(np.min(np.abs(q - np.round(q)))) for q in (rng, yaw, arc) if len(q))


def image(pts) -> np.ndarray:
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    dis = np.sqrt(x * x + y * y)                                                      # fp32
    yaw = ((np.arctan2(y, x) * np.float32(180.0)).astype(np.float64) / np.pi + 180.0).astype(np.float32)
    q_dis = np.clip(np.floor(dis.astype(np.float64)), 0, ROWS - 1).astype(np.int64)
    q_arc = np.clip(np.ceil((z + np.float32(5.0)).astype(np.float64)), 0, 7).astype(np.int64)
    q_yaw = np.clip(np.floor(yaw.astype(np.float64) + 0.5), 0, COLS - 1).astype(np.int64)
    img = np.zeros((ROWS, COLS), np.uint8)
    np.bitwise_or.at(img, (q_dis, q_yaw), (1 << q_arc).astype(np.uint8))
    return img


# ------------------------------------------------------------------------------------------------ encode
def log_gabor_filters() -> np.ndarray:
    """(4, 360) one-sided filters: nscale 4, minWaveLength 18, mult (double)2.1f, sigmaOnf 0.75."""
    radius = np.arange(COLS // 2 + 1, dtype=np.float64) / COLS
    radius[0] = 1.0
    F = np.zeros((SCALES, COLS))
    wavelength, mult, sigma = 18.0, float(np.float32(2.1)), 0.75
    for s in range(SCALES):
        fo = 1.0 / wavelength
        F[s, :COLS // 2 + 1] = np.exp(-np.log(radius / fo) ** 2 / (2.0 * np.log(sigma) ** 2))
        F[s, 0] = 0.0
        wavelength *= mult
    return F


def responses(img) -> np.ndarray:
    """(4, 80, 360) complex: unscaled inverse DFT of (row DFT x filter)."""
    X = np.fft.fft(np.asarray(img, np.float64), axis=1)
    return np.stack([np.fft.ifft(X * f[None, :], axis=1) * COLS for f in log_gabor_filters()])


def encode(img):
    """-> (T, M) 640 x 360 uint8 (0 / 255), and the responses they were cut from."""
    V = responses(img)
    T = np.concatenate([V.real[s] > 0 for s in range(SCALES)] + [V.imag[s] > 0 for s in range(SCALES)])
    m = [np.abs(V[s]) < 1e-4 for s in range(SCALES)]
    M = np.concatenate(m + m)
    return T.astype(np.uint8) * 255, M.astype(np.uint8) * 255, V


# ------------------------------------------------------------------------------------------------ distance
def hamming_at_shift(T1, M1, T2, M2, s: int):
    """(diff, total) with the QUERY (T1, M1) rolled right by s columns -- the definition, unoptimised."""
    T1s, M1s = np.roll(T1 > 0, s, axis=1), np.roll(M1 > 0, s, axis=1)
    mask = M1s | (M2 > 0)
    total = T1s.size - int(mask.sum())
    diff = int(((T1s ^ (T2 > 0)) & ~mask).sum())
    return diff, total


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_all_shifts(T1, M1, T2, M2):
    """(diff[360], total[360]) int64: hamming_at_shift for every s, on bytes packed along the row axis."""
    t1, m1, t2, m2 = (np.packbits(a > 0, axis=0) for a in (T1, M1, T2, M2))
    diff = np.zeros(COLS, np.int64)
    total = np.zeros(COLS, np.int64)
    for s in range(COLS):
        mask = np.roll(m1, s, axis=1) | m2
        total[s] = T1.size - _POP8[mask].sum()
        diff[s] = _POP8[(np.roll(t1, s, axis=1) ^ t2) & ~mask].sum()
    return diff, total


def best_shift(diff, total):
    """-> (distance float32, bias, diff, total): the minimum fp32 quotient over s, ties to the smallest s; NaN
    shifts (total = 0) lose to any number; all NaN -> (NaN, -1, 0, 0)."""
    diff, total = np.asarray(diff, np.int64), np.asarray(total, np.int64)
    ok = total > 0
    if not ok.any():
        return np.float32(np.nan), -1, 0, 0
    d = np.full(len(diff), np.inf, np.float32)
    d[ok] = diff[ok].astype(np.float32) / total[ok].astype(np.float32)
    s = int(np.argmin(d))                                   # first minimum
    return d[s], s, int(diff[s]), int(total[s])


# ------------------------------------------------------------------------------------------------ selection
def select(threshold, min_gap, max_dist, current_id, current_pos, ids, positions, dist) -> int:
    """detect_loop_closures' choice: database index or -1."""
    cur = np.asarray(current_pos, np.float32)
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    best = -1
    for i in range(len(ids)):
        if int(np.int64(current_id).astype(np.int32)) - int(np.int64(ids[i]).astype(np.int32)) < int(min_gap):
            continue
        d = cur - pos[i]
        norm = np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if norm > np.float32(max_dist):
            continue
        if np.isnan(dist[i]):
            continue
        if best < 0 or np.float32(dist[i]) < np.float32(dist[best]):
            best = i
    if best >= 0 and np.float32(dist[best]) > np.float32(threshold):
        return -1
    return best


# ------------------------------------------------------------------------------------------------ scenes
def scene(seed: int, n_ground: int = 2500, n_walls: int = 12, per_wall: int = 220) -> np.ndarray:
    """A ground disc plus vertical wall segments around the sensor, (N, 3) float32, sensor frame."""
    rng = np.random.default_rng(seed)
    r = 60.0 * np.sqrt(rng.random(n_ground))
    a = rng.uniform(-np.pi, np.pi, n_ground)
    parts = [np.stack([r * np.cos(a), r * np.sin(a), -1.7 + 0.02 * rng.standard_normal(n_ground)], 1)]
    for _ in range(n_walls):
        c = rng.uniform(-45.0, 45.0, 2)
        if np.hypot(*c) < 4.0:
            c += 8.0
        th = rng.uniform(0, np.pi)
        length, height = rng.uniform(4.0, 20.0), rng.uniform(1.5, 4.5)
        u = rng.uniform(-0.5, 0.5, per_wall) * length
        parts.append(np.stack([c[0] + u * np.cos(th), c[1] + u * np.sin(th),
                               -1.7 + height * rng.random(per_wall)], 1))
    return np.concatenate(parts).astype(np.float32)


def yawed(pts, degrees: float, translation=(0.0, 0.0, 0.0), sigma: float = 0.0, seed: int = 0) -> np.ndarray:
    """R_z(degrees) * pts + translation + noise: the scene as a sensor turned by -degrees sees it."""
    a = np.radians(degrees)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    out = np.asarray(pts, np.float64) @ R.T + np.asarray(translation, np.float64)
    if sigma > 0:
        out = out + sigma * np.random.default_rng(seed).standard_normal(out.shape)
    return out.astype(np.float32)
