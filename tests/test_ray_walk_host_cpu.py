"""CPU: the C++ walk itself (gennbv_amd/csrc/ray_walk.h compiled for the host), against the oracle's sequential Bresenham.

tests/ray_walk_host.hip is a stand-alone program around the header's make_walk / run_walk (the ray record of k_vg_fate) and
make_slab_cut / walk_steps (the slab cut of k_vg_slab); it is compiled here and run as a child process on the rays of
tests/test_view_gain_slab_cpu.py: sources inside the grid, within one grid of it, 3 000 voxels out and on a face; targets with one
axis constant, two axes constant and a single point.  Every in-grid voxel before the stop must be visited exactly once, by the
slab that owns its x, in order.  (The Python model of the same arithmetic stays in test_view_gain_slab_cpu.py; it owns the
"every 32-bit intermediate fits" assertion.)
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
CASES = [(20, (1, 3, 7, 20)), (65, (5, 24, 33)), (128, (5, 16, 19))]
SOURCES, TARGETS = 70, 100


def _rays(g, heights):
    """(src, tgt, height, ref voxels, index of the occupied one or None) per ray; test_view_gain_slab_cpu's sources and targets"""
    rs = np.random.RandomState(g)
    for si in range(SOURCES):
        kind = si % 4  # inside, near, 3 000 voxels outside, on a face
        src = rs.randint(0, g, 3)
        if kind == 1:
            src = rs.randint(-g, 2 * g, 3)
        elif kind == 2:
            ax = rs.randint(0, 3)
            src[ax] = 3000 * (1 if rs.rand() < 0.5 else -1) + rs.randint(-50, 50)
            if rs.rand() < 0.3:
                src[(ax + 1) % 3] += rs.randint(-3000, 3000)
        elif kind == 3:
            src[rs.randint(0, 3)] = (0, g - 1, -1, g)[rs.randint(0, 4)]
        # targets: through a point of the grid and beyond it, so that far sources meet the grid; some degenerate
        q = rs.randint(0, g, (TARGETS, 3))
        f = rs.uniform(1.0, 3.0, (TARGETS, 1))
        tgt = np.where(rs.rand(TARGETS, 1) < 0.5, q, np.rint(src + (q - src) * f)).astype(np.int64)
        for ax in range(3):
            tgt[10 * ax:10 * ax + 10, ax] = src[ax]   # one axis constant
        tgt[30:35, 1:] = src[1:]                      # two axes constant
        tgt[35] = src                                 # a single point
        traj, lens = orc.bresenham3d(src.astype(np.int32), tgt.astype(np.int32), g)
        for ti in range(TARGETS):
            ref = [tuple(int(v) for v in p) for p in traj[ti, :lens[ti]]]
            stop = int(rs.randint(0, len(ref))) if ref and rs.rand() < 0.67 else None  # a third of the rays are never stopped
            yield [int(v) for v in src], [int(v) for v in tgt[ti]], heights[si % len(heights)], ref, stop


@pytest.fixture(scope="module")
def walk_program(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc needed to compile ray_walk.h for the host")
    exe = str(tmp_path_factory.mktemp("ray_walk") / "ray_walk_host")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "gennbv_amd", "csrc"),
           os.path.join(ROOT, "tests", "ray_walk_host.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("g,heights", CASES)
def test_host_compiled_walk_and_slab_cut_equal_the_oracle_trajectory(walk_program, g, heights):
    rays = list(_rays(g, heights))
    lin = lambda v: (v[0] * g + v[1]) * g + v[2]
    text = "".join("%d %d %d %d %d %d %d %d %d\n" % (g, h, *s, *t, lin(ref[stop]) if stop is not None else -1) for s, t, h, ref, stop in rays)
    r = subprocess.run([walk_program], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    records = []  # per ray: [record, {X0: [lin, ...]}]
    for line in r.stdout.split("\n"):
        w = line.split()
        if w and w[0] == "R":
            records.append(([int(v) for v in w[1:]], {}))
        elif w:
            assert w[0] == "S" and int(w[1]) not in records[-1][1], line
            records[-1][1][int(w[1])] = [int(v) for v in w[2:]]
    assert len(records) == len(rays)
    nonempty = stopped = 0
    for (s, t, h, ref, stop), ((first, count, blocked, xa, xb), slabs) in zip(rays, records):
        k = len(ref) if stop is None else stop
        assert blocked == (stop is not None) and count == k, (s, t)
        if k:
            xs = [v[0] for v in ref[:k]]
            assert (xa, xb) == (min(xs), max(xs)), (s, t)
        assert all(X0 % h == 0 for X0 in slabs), (s, t)
        got = []
        for X0 in range(0, g, h):  # every slab: exactly its voxels, in the oracle's order
            part = slabs.get(X0, [])
            assert part == [lin(v) for v in ref[:k] if X0 <= v[0] < X0 + h], (s, t, X0)
            got += part
        assert len(got) == k and len(set(got)) == k, (s, t)
        nonempty += k > 0
        stopped += blocked
    assert nonempty > len(rays) // 3 and stopped > len(rays) // 4
