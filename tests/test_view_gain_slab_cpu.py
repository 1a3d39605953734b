"""CPU: the ray record and the slab cut of gnbv_view_gain_slab (gennbv_amd/csrc/viewgain.hip: k_vg_fate, k_vg_slab; the walk
is gennbv_amd/csrc/ray_walk.h: walk_axes, minor_range, walk_at, make_walk / run_walk, make_slab_cut / walk_steps) as a Python
model, against the oracle's sequential Bresenham.  tests/test_ray_walk_host_cpu.py runs the C++ itself on the same rays; this
model stays for what the C++ cannot show: that every 32-bit intermediate fits.

k_vg_fate walks a ray once against the whole grid (make_walk's closed-form entry, then the reference's decision variables)
and records the first in-grid step, the number of steps up to the voxel in front of the first occupied one, and the x-extent
of those steps.  k_vg_slab rejects a ray on that extent, cuts the recorded steps to its x-planes [X0, X1) (make_slab_cut)
-- exactly if x is the dominant axis, by the closed form of the minors (one step wide on both sides, guarded by a test of the
slab-local index) if not -- and walks them.  Here the same arithmetic, line by line, with Python integers (the header's
floor_div is exact, so `//` stands for it): every in-grid voxel before the stop must be visited exactly once, by the slab that
owns its x, in order.  The slab set-up of a ray of fewer than 2^14 steps runs in 32-bit integers (walk_at<int>): the model
asserts that every intermediate of such a ray fits.
"""
import numpy as np
import pytest

from oracle import oracle as orc


def _axes(src, tgt, g):
    """make_walk's axis order: (pa, pb, pc), (da, db, dc), (sa, sb, sc), linear strides (sta, stb, stc), x_dominant."""
    x0, y0, z0 = src
    x1, y1, z1 = tgt
    dx, dy, dz = abs(x1 - x0), abs(y1 - y0), abs(z1 - z0)
    sx, sy, sz = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1), (1 if z0 < z1 else -1)
    dm, gg = max(dx, dy, dz), g * g
    if dm == dx:
        return (x0, y0, z0), (dx, dy, dz), (sx, sy, sz), (gg, g, 1), True
    if dm == dy:
        return (y0, x0, z0), (dy, dx, dz), (sy, sx, sz), (g, gg, 1), False
    return (z0, x0, y0), (dz, dx, dy), (sz, sx, sy), (1, gg, g), False


def _fits(small, *values):
    """On the kernel's 32-bit path every intermediate must fit an int."""
    assert not small or all(abs(v) < 2 ** 31 for v in values), values


def _minor_range(p0, s, d, da, b0, b1, lo, hi, small=False):
    mlo = (b0 - p0) if s > 0 else (p0 - b1)
    mhi = (b1 - p0) if s > 0 else (p0 - b0)
    _fits(small, mlo, mhi)
    if mhi < 0 or (mlo > 0 and d == 0):
        return lo, -1
    if d == 0:
        return lo, hi
    if mlo > 0:
        _fits(small, 2 * da * mlo, 2 * da * mlo - da + 2 * d - 1)
        lo = max(lo, (2 * da * mlo - da + 2 * d - 1) // (2 * d) - 1)
    _fits(small, 2 * da * (mhi + 1), 2 * da * (mhi + 1) - da + 2 * d - 1)
    hi = min(hi, (2 * da * (mhi + 1) - da + 2 * d - 1) // (2 * d))
    return lo, hi


def _state_at(p, d, s, st, lo, small=False):
    """Coordinates, decision variables and linear index in front of step lo -> lo + 1."""
    (pa, pb, pc), (da, db, dc), (sa, sb, sc) = p, d, s
    nb = nc = 0
    if da > 0 and lo > 0:
        _fits(small, 2 * db * lo + da, 2 * dc * lo + da)
        nb, nc = (2 * db * lo + da) // (2 * da), (2 * dc * lo + da) // (2 * da)
    pa, pb, pc = pa + sa * lo, pb + sb * nb, pc + sc * nc
    _fits(small, 2 * db * (lo + 1) - da, 2 * da * nb, 2 * dc * (lo + 1) - da, 2 * da * nc)
    p1, p2 = 2 * db * (lo + 1) - da - 2 * da * nb, 2 * dc * (lo + 1) - da - 2 * da * nc
    return pa, pb, pc, p1, p2, pa * st[0] + pb * st[1] + pc * st[2]


def _fate(src, tgt, g, occupied):
    """k_vg_fate: (first step, count, blocked, xa, xb); `occupied` is a set of linear indices."""
    p, d, s, st, _ = _axes(src, tgt, g)
    (pa, pb, pc), (da, db, dc), (sa, sb, sc) = p, d, s
    lo = max(-pa if sa > 0 else pa - (g - 1), 0)
    hi = min((g - 1) - pa if sa > 0 else pa, da)
    if da > 0:
        lo, hi = _minor_range(pb, sb, db, da, 0, g - 1, lo, hi)
        if hi >= lo:
            lo, hi = _minor_range(pc, sc, dc, da, 0, g - 1, lo, hi)
    if hi < lo:
        return 0, 0, False, 0, 0
    assert hi - lo + 1 <= g + 2
    _, pb, pc, p1, p2, lin = _state_at(p, d, s, st, lo)
    first, last, lin_first, lin_last, blocked = 0, -1, 0, 0, False
    for i in range(hi - lo + 1):
        if 0 <= pb < g and 0 <= pc < g:
            if lin in occupied:
                blocked = True
                break
            if last < 0:
                first, lin_first = i, lin
            last, lin_last = i, lin
        if p1 >= 0:
            pb, lin, p1 = pb + sb, lin + sb * st[1], p1 - 2 * da
        if p2 >= 0:
            pc, lin, p2 = pc + sc, lin + sc * st[2], p2 - 2 * da
        lin += sa * st[0]
        p1 += 2 * db
        p2 += 2 * dc
    count = 0 if last < 0 else last - first + 1
    xf, xl = lin_first // (g * g), lin_last // (g * g)
    return (lo + first if count else 0), count, blocked, min(xf, xl), max(xf, xl)


def _slab_voxels(src, tgt, g, first, count, xa, xb, X0, X1):
    """k_vg_slab for one ray: the voxels (x, y, z) it marks in slab [X0, X1), in order."""
    out = []
    if count == 0 or xb < X0 or xa >= X1:
        return out
    p, d, s, st, xdom = _axes(src, tgt, g)
    (pa, pb, pc), (da, db, dc), (sa, sb, sc) = p, d, s
    small = da < (1 << 14)  # the kernel's 32-bit set-up
    lo, hi = first, first + count - 1
    if xdom:
        lo = max(lo, (X0 - pa) if sa > 0 else (pa - (X1 - 1)))
        hi = min(hi, ((X1 - 1) - pa) if sa > 0 else (pa - X0))
    else:
        lo, hi = _minor_range(pb, sb, db, da, X0, X1 - 1, lo, hi, small)
    if hi < lo:
        return out
    gg = g * g
    _, _, _, p1, p2, lin = _state_at(p, d, s, st, lo, small)
    lin -= X0 * gg
    svox = (X1 - X0) * gg
    for _ in range(hi - lo + 1):
        if 0 <= lin < svox:
            glin = lin + X0 * gg
            out.append((glin // gg, (glin // g) % g, glin % g))
        if p1 >= 0:
            lin, p1 = lin + sb * st[1], p1 - 2 * da
        if p2 >= 0:
            lin, p2 = lin + sc * st[2], p2 - 2 * da
        lin += sa * st[0]
        p1 += 2 * db
        p2 += 2 * dc
    return out


@pytest.mark.parametrize("g,heights,sources,targets", [(20, (1, 3, 7, 20), 70, 100), (65, (5, 24, 33), 70, 100),
                                                       (128, (5, 16, 19), 70, 100)])
def test_record_and_slab_cut_equal_the_oracle_trajectory(g, heights, sources, targets):
    rs = np.random.RandomState(g)
    nonempty = stopped = 0
    for si in range(sources):
        kind = si % 4  # inside, near, 3 000 voxels outside, on a face
        if kind == 0:
            src = rs.randint(0, g, 3)
        elif kind == 1:
            src = rs.randint(-g, 2 * g, 3)
        elif kind == 2:
            src = rs.randint(0, g, 3)
            ax = rs.randint(0, 3)
            src[ax] = 3000 * (1 if rs.rand() < 0.5 else -1) + rs.randint(-50, 50)
            if rs.rand() < 0.3:
                src[(ax + 1) % 3] += rs.randint(-3000, 3000)
        else:
            src = rs.randint(0, g, 3)
            src[rs.randint(0, 3)] = (0, g - 1, -1, g)[rs.randint(0, 4)]
        # targets: through a point of the grid and beyond it, so that far sources meet the grid; some degenerate
        q = rs.randint(0, g, (targets, 3))
        f = rs.uniform(1.0, 3.0, (targets, 1))
        tgt = np.where(rs.rand(targets, 1) < 0.5, q, np.rint(src + (q - src) * f)).astype(np.int64)
        for ax in range(3):
            rows = slice(10 * ax, 10 * ax + 10)
            tgt[rows, ax] = src[ax]                       # one axis constant
        tgt[30:35, 1:] = src[1:]                          # two axes constant
        tgt[35] = src                                     # a single point
        traj, lens = orc.bresenham3d(src.astype(np.int32), tgt.astype(np.int32), g)
        s = [int(v) for v in src]
        height = heights[si % len(heights)]
        for ti in range(targets):
            ref = [tuple(int(v) for v in p) for p in traj[ti, :lens[ti]]]
            # a random stop: the k-th in-grid voxel is occupied (none for a third of the rays)
            k = len(ref)
            occupied = set()
            if ref and rs.rand() < 0.67:
                k = int(rs.randint(0, len(ref)))
                x, y, z = ref[k]
                occupied.add((x * g + y) * g + z)
            t = [int(v) for v in tgt[ti]]
            first, count, blocked, xa, xb = _fate(s, t, g, occupied)
            assert blocked == bool(occupied) and count == k, (s, t)
            nonempty += k > 0
            stopped += blocked
            got = []
            for X0 in range(0, g, height):
                X1 = min(g, X0 + height)
                part = _slab_voxels(s, t, g, first, count, xa, xb, X0, X1)
                assert part == [v for v in ref[:k] if X0 <= v[0] < X1], (s, t, X0, X1)
                got += part
            assert len(got) == k and len(set(got)) == k, (s, t)
    assert nonempty > sources * targets // 3 and stopped > sources * targets // 4
