"""CPU: the conservative record test of the frustum packet kernel (csrc/trace_frustum.h), restated in numpy float32, against the per-ray arithmetic of
box_pair_hit_m (csrc/trace_w4.h).  For a sign group with the interval hull o_lo / o_hi, inv_lo / inv_hi and tmax_bound = max t_max:
    i > 0: xn = b.min - o_hi, xf = b.max - o_lo;   i < 0: xn = b.max - o_lo, xf = b.min - o_hi
    L_axis = min(xn * inv_lo, xn * inv_hi), U_axis = max(xf * inv_lo, xf * inv_hi), L = max3(L_axis), U = min3(U_axis) * widen
    taken iff L <= U && L < tmax_bound && U > 0
Rounding is monotone, so L <= every lane's m and U >= every lane's M with no epsilon: the assertions are inequalities, there is no tolerance.
The kernel evaluates L_axis / U_axis as the min / max of all four products (b.min - o_hi, b.max - o_lo) x (inv_lo, inv_hi), which needs no select by
sign; the test holds that form to the sign-selected one bit for bit."""
import itertools

import numpy as np
import pytest

F = np.float32
WIDEN = F(1.0) + F(2.0) * (F(3.0) * F(2.0 ** -24) / (F(1.0) - F(3.0) * F(2.0 ** -24)))   # 1 + 2 gamma(3)
CONES = (1e-4, 1e-3, 3e-3, 1e-2, 3e-2)
N_BOXES = 2000


def per_ray(bmin, bmax, o, inv, t_max):
    """box_pair_hit_m for one slot: (m, M, hit) per lane; bmin / bmax [B, 1, 3], o / inv [1, 64, 3], t_max [1, 64]"""
    lo, hi = (bmin - o) * inv, (bmax - o) * inv
    near, far = np.fmin(lo, hi), np.fmax(lo, hi)
    m = np.fmax(np.fmax(near[..., 0], near[..., 1]), near[..., 2])
    M = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2]) * WIDEN
    with np.errstate(invalid="ignore"):
        return m, M, (m <= M) & (m < t_max) & (M > 0)


def frustum(bmin, bmax, o, inv, t_max, neg):
    """the group's test of the same slots: (L, U, taken, L4, U4) per box — L4 / U4 the kernel's four-product form; bmin / bmax [B, 3]"""
    o_lo, o_hi, inv_lo, inv_hi = o.min(axis=0), o.max(axis=0), inv.min(axis=0), inv.max(axis=0)
    tmax_bound = t_max.max()
    a, b = bmin - o_hi, bmax - o_lo
    xn, xf = np.where(neg, b, a), np.where(neg, a, b)
    L_axis, U_axis = np.fmin(xn * inv_lo, xn * inv_hi), np.fmax(xf * inv_lo, xf * inv_hi)
    L = np.fmax(np.fmax(L_axis[:, 0], L_axis[:, 1]), L_axis[:, 2])
    U = np.fmin(np.fmin(U_axis[:, 0], U_axis[:, 1]), U_axis[:, 2]) * WIDEN
    p = [a * inv_lo, a * inv_hi, b * inv_lo, b * inv_hi]
    L4a, U4a = np.fmin(np.fmin(np.fmin(p[0], p[1]), p[2]), p[3]), np.fmax(np.fmax(np.fmax(p[0], p[1]), p[2]), p[3])
    L4 = np.fmax(np.fmax(L4a[:, 0], L4a[:, 1]), L4a[:, 2])
    U4 = np.fmin(np.fmin(U4a[:, 0], U4a[:, 1]), U4a[:, 2]) * WIDEN
    with np.errstate(invalid="ignore"):
        return L, U, (L <= U) & (L < tmax_bound) & (U > 0), L4, U4


def packet(rng, signs, cone, jitter, finite_t):
    """64 rays of one sign group: a cone of half-angle ~cone around a direction with the given signs, a shared or lens-jittered origin"""
    c = rng.uniform(0.15, 1.0, 3) * signs
    d = c + rng.uniform(-cone, cone, (64, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = rng.uniform(-2, 2, 3) + (rng.uniform(-0.05, 0.05, (64, 3)) if jitter else 0.0) * np.ones((64, 3))
    d = d.astype(F)
    inv = F(1.0) / d
    assert ((inv < 0) == (signs < 0)).all()
    t_max = rng.uniform(0.5, 9.0, 64).astype(F) if finite_t else np.full(64, np.inf, F)
    return o.astype(F), d, inv, t_max


def boxes(rng, o, d):
    """boxes around the packet's axis (so that lanes hit, graze and miss them), from point-sized to scene-sized, some degenerate on an axis, the
    last ones the NaN box of an empty slot"""
    t = rng.uniform(-1.0, 8.0, (N_BOXES, 1))
    size = 10.0 ** rng.uniform(-5, 0.6, (N_BOXES, 1)) * rng.uniform(0.2, 1.0, (N_BOXES, 3))
    centre = o.mean(axis=0) + t * d.mean(axis=0) + rng.normal(size=(N_BOXES, 3)) * size * rng.choice([0.0, 0.5, 1.5], (N_BOXES, 1))
    flat = rng.integers(0, 4, N_BOXES)
    for axis in range(3):
        size[flat == axis, axis] = 0.0
    bmin, bmax = (centre - size).astype(F), (centre + size).astype(F)
    bmin[-8:] = np.nan
    bmax[-8:] = np.nan
    return bmin, bmax


def test_widen_is_the_kernels_constant():
    assert WIDEN.view(np.uint32) == 0x3F800003


@pytest.mark.parametrize("jitter", [False, True], ids=["shared_origin", "jittered_origin"])
@pytest.mark.parametrize("finite_t", [False, True], ids=["t_inf", "t_finite"])
def test_frustum_interval_bounds_every_lane(jitter, finite_t):
    rng = np.random.default_rng(41 + 2 * jitter + finite_t)
    n_boxes = n_hit = n_taken = 0
    for signs, cone in itertools.product(itertools.product((1.0, -1.0), repeat=3), CONES):   # all eight sign groups
        signs = np.array(signs)
        o, d, inv, t_max = packet(rng, signs, cone, jitter, finite_t)
        bmin, bmax = boxes(rng, o.astype(np.float64), d.astype(np.float64))
        m, M, hit = per_ray(bmin[:, None, :], bmax[:, None, :], o[None], inv[None], t_max[None])
        L, U, taken, L4, U4 = frustum(bmin, bmax, o, inv, t_max, signs < 0)
        real = ~np.isnan(bmin[:, 0])
        assert (L[real, None] <= m[real]).all()
        assert (U[real, None] >= M[real]).all()
        assert (taken | ~hit.any(axis=1)).all()          # any lane hits -> the slot is taken
        assert not taken[~real].any() and not hit[~real].any()   # the NaN box of an empty slot is never taken
        assert L4.tobytes() == L.tobytes() and U4.tobytes() == U.tobytes()   # the kernel's four-product form is the sign-selected one
        n_boxes += int(real.sum()); n_hit += int(hit.any(axis=1).sum()); n_taken += int(taken.sum())
    # the inputs exercise the test: boxes that some lane hits, boxes taken without any lane hitting, boxes not taken
    assert n_hit > n_boxes // 20 and n_taken > n_hit and n_taken < n_boxes
