"""Shared by tests/test_scan_abi_gpu.py and tests/test_scan_abi_regimes_cpu.py: the scan set, key sort and accuracy scorer of
csrc/scan.hip (and gnbv_chamfer_distance of csrc/chamfer.hip) at the C ABI.

  * frames whose keys are known without the Morton layout: keys enter a set only through gnbv_scan_add_frame;
  * the numpy oracle of the set (oracle.post_process_depth + oracle.back_projection, the bit-exact fp32 chain, then rint(100 p));
  * a GT packer that builds GnbvScanGt exactly as include/gennbv_hip.h words it, in the GIVEN order of the points, and a checker
    of the header's invariants for any packed GT (ScanAccumulator._gt_tree's included);
  * the sort / tree geometry of csrc/scan.hip restated from its constants, and check_regime(): from the oracle alone, a case
    reaches what its id names;
  * device buffers the test places itself, every one between sentinel bytes that must come back unchanged.

Nothing here touches the GPU at import; only `Buf`, `GtDev`, `ScanCall` and `device_chamfer` do.

The tolerance against the fp64 brute force is derived, not measured (u = 2^-24):
  dx = fl(qx - yx) carries (1 + u); dx * dx (1 + u)^3; each of the two fmas adds one rounding to a sum of non-negative terms, so the
  pair value fmaf(dz, dz, fmaf(dy, dy, dx * dx)) is within (1 + u)^5 of the true squared distance of the two fp32 points; a minimum
  and a sum of non-negative terms keep a relative bound; the fp64 sums and means add nothing visible at this scale; the cast to
  fp32 and the fp32 product with 100 add one u each: (1 + u)^7 - 1 < 8 u.  gnbv_chamfer_distance has no x 100: 6 u, checked at 8 u.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import oracle as orc

DEV = "cuda:0"
f32 = np.float32
SENSE = -50.0
FILL = 0x5B  # sentinel byte around (and in the unwritten parts of) every buffer: 0x5B5B5B5B is 6.2e16 as fp32
TOL_REL, TOL_ABS = 8 * 2.0 ** -24, 1e-30

# ---------------------------------------------------------------------------
# csrc/scan.hip: constants and launch geometry
# ---------------------------------------------------------------------------
K_SORT_TILE = 2048     # kSortTile: keys per radix tile
K_LEAF = 32            # kLeaf: points per tree leaf
K_SCAN_CHUNK = 256     # k_radix_scan: [digit][tile] entries per trip of its outer loop
K_CLEAR_THREADS = 256  # k_scan_clear: threads per block, one uint4 (two slots) each per trip
KEY_LIMIT = 1 << 20    # |k| < 2^20
FLAG_OVERFLOW, FLAG_RANGE = 1, 2


def blocks_per_env(n):
    return max(4, min(256, -(-4096 // n)))


def tiles_of(count):
    return -(-count // K_SORT_TILE)


def scan_chunks(count):
    """Trips of k_radix_scan's outer loop."""
    return -(-16 * tiles_of(count) // K_SCAN_CHUNK)


def tree_pow2(count):
    leaves, p = -(-count // K_LEAF), 1
    while p < leaves:
        p <<= 1
    return p


def clear_trips(n, cap):
    """Trips of k_scan_clear's grid-stride loop."""
    per = -(-(cap // 2) // K_CLEAR_THREADS)
    blocks = min(per, blocks_per_env(n))
    return -(-(cap // 2) // (blocks * K_CLEAR_THREADS))


# ---------------------------------------------------------------------------
# frames: identity rotation in c2w
# ---------------------------------------------------------------------------
def _c2w(t):
    t = np.asarray(t, f32).reshape(-1, 3)
    m = np.zeros((t.shape[0], 4, 4), f32)
    m[:, np.arange(4), np.arange(4)] = 1.0
    m[:, :3, 3] = t
    return m


def lattice_frame(t, h, w, s=0.01, fg=None, depth=None):
    """Raw depth -1 (d = 1) and inv_intri = diag(s, s, 1): pixel (v, u) of env e is the world point (s u + tx, s v + ty, 1 + tz).
    fg: [n, h*w] bool, the foreground pixels (default all); depth: another raw depth image."""
    t = np.asarray(t, f32).reshape(-1, 3)
    n = t.shape[0]
    d = np.full((n, h, w), -1.0, f32) if depth is None else np.ascontiguousarray(depth, f32).reshape(n, h, w)
    fg = np.ones((n, h * w), bool) if fg is None else np.asarray(fg, bool).reshape(n, h * w)
    seg = np.where(fg, f32(255.0), f32(0.0)).astype(f32).reshape(n, h, w)
    return SimpleNamespace(n=n, h=h, w=w, depth=d, seg=seg, c2w=_c2w(t), kinv=np.diag([s, s, 1.0]).astype(f32))


def point_frame(t, fg=None, h=1, w=1):
    """Raw depth 0: every foreground pixel is the translation column exactly (1 x 1: one chosen point per env)."""
    t = np.asarray(t, f32).reshape(-1, 3)
    fr = lattice_frame(t, h, w, fg=None if fg is None else np.repeat(np.asarray(fg, bool).reshape(-1, 1), h * w, 1),
                       depth=np.zeros((t.shape[0], h, w), f32))
    return fr


def first_pixels(counts, hw):
    """fg[e, p] = p < counts[e]."""
    return np.arange(hw)[None, :] < np.asarray(counts).reshape(-1, 1)


def layered_frames(counts, t0, h=32, w=64, s=0.01):
    """Lattice frames that give env e exactly counts[e] distinct keys: layer f (tz + 0.01 f) holds pixels f h w .. of each env."""
    counts, t0 = np.asarray(counts, np.int64), np.asarray(t0, np.float64).reshape(-1, 3)
    hw, out = h * w, []
    for f in range(max(1, -(-int(counts.max()) // hw))):
        t = np.round(t0 + np.asarray([0.0, 0.0, 0.01 * f]), 2)
        out.append(lattice_frame(t, h, w, s, fg=first_pixels(np.clip(counts - f * hw, 0, hw), hw)))
    return out


def base_translations(n):
    """A translation of its own for every env, multiples of 1 cm, both signs."""
    e = np.arange(n)
    return np.round(np.stack([(e % 17) * 0.37 - 3.0, 1.0 - (e % 13) * 0.23, (e % 7) * 0.11 - 0.3], -1), 2)


# ---------------------------------------------------------------------------
# the oracle of the set
# ---------------------------------------------------------------------------
class SetOracle:
    """Per env the integer keys [m, 3] in lexicographic order and the flags, as include/gennbv_hip.h words them."""

    def __init__(self, n, cap):
        self.n, self.cap = n, cap
        self.keys = [np.zeros((0, 3), np.int64) for _ in range(n)]
        self.flags = np.zeros(n, np.int32)

    def add(self, fr):
        dp, sp = orc.post_process_depth(fr.depth, fr.seg, SENSE)
        world, fg = orc.back_projection(dp, sp, fr.c2w, fr.kinv)
        for e in np.nonzero(fg.any(1))[0]:
            with np.errstate(invalid="ignore", over="ignore"):
                k = np.rint(world[e][fg[e]].astype(f32) * f32(100))
                bad = ~np.isfinite(k).all(1) | (np.abs(k) >= KEY_LIMIT).any(1)
            if bad.any():
                self.flags[e] |= FLAG_RANGE
            union = np.unique(np.concatenate([self.keys[e], k[~bad].astype(np.int64)]), axis=0)
            if union.shape[0] > self.cap:  # (which keys of an overflowing frame get in is not defined: only a full set may overflow)
                assert self.keys[e].shape[0] == self.cap, "an overflow case must start from a full set"
                self.flags[e] |= FLAG_OVERFLOW
            else:
                self.keys[e] = union
        return self

    def clear(self, mask):
        for e in np.nonzero(np.asarray(mask))[0]:
            self.keys[e] = np.zeros((0, 3), np.int64)
        return self

    @property
    def counts(self):
        return np.asarray([k.shape[0] for k in self.keys], np.int32)

    def points(self, e):
        return (self.keys[e].astype(f32) * f32(0.01)).astype(f32)


# ---------------------------------------------------------------------------
# the GT side
# ---------------------------------------------------------------------------
def pack_gt(clouds, perms=None, extra_levels=0):
    """GnbvScanGt of the clouds in the order given (perms[e]: the order env e's points are stored in; orig maps back), built from
    the header's words alone: leaf j = the box of points 32 j .. 32 j + 31, a parent = the union of its children, a node without
    points = (+inf, -inf).  extra_levels: P is that many doublings above the least power of two (the header allows any)."""
    pts, orig, pow2, nodes, starts, node_starts = [], [], [], [], [0], []
    for e, y in enumerate(clouds):
        y = np.ascontiguousarray(y, f32).reshape(-1, 3)
        order = np.arange(y.shape[0]) if perms is None or perms[e] is None else np.asarray(perms[e])
        ys, m = y[order], y.shape[0]
        leaves = -(-m // K_LEAF)
        p = tree_pow2(m) << extra_levels
        lo, hi = np.full((2 * p, 3), np.inf, f32), np.full((2 * p, 3), -np.inf, f32)
        for j in range(leaves):
            lo[p + j], hi[p + j] = ys[K_LEAF * j:K_LEAF * (j + 1)].min(0), ys[K_LEAF * j:K_LEAF * (j + 1)].max(0)
        for i in range(p - 1, 0, -1):
            lo[i], hi[i] = np.minimum(lo[2 * i], lo[2 * i + 1]), np.maximum(hi[2 * i], hi[2 * i + 1])
        nd = np.zeros((2 * p, 2, 4), f32)
        nd[:, 0, :3], nd[:, 1, :3] = lo, hi
        pts.append(np.concatenate([ys, np.zeros((m, 1), f32)], 1))
        orig.append(order.astype(np.int32))
        pow2.append(p)
        node_starts.append(sum(x.shape[0] for x in nodes))
        nodes.append(nd)
        starts.append(starts[-1] + m)
    return SimpleNamespace(n=len(clouds), num_points=starts[-1], pt_start=np.asarray(starts, np.int64), pts=np.concatenate(pts),
                           orig=np.concatenate(orig), node_start=np.asarray(node_starts, np.int64), pow2=np.asarray(pow2, np.int32),
                           nodes=np.concatenate(nodes))


def pack_from_gt_tree(clouds, device="cpu"):
    """The same structure from ScanAccumulator._gt_tree's output (Morton order)."""
    from gennbv_amd.eval.scan_accumulator import _gt_tree
    pts, orig, pow2, nodes, starts, node_starts = [], [], [], [], [0], []
    for y in clouds:
        p4, perm, p, nd = _gt_tree(torch.from_numpy(np.ascontiguousarray(y, f32).reshape(-1, 3)).to(device))
        pts.append(p4.cpu().numpy())
        orig.append(perm.cpu().numpy().astype(np.int32))
        pow2.append(int(p))
        node_starts.append(sum(x.shape[0] for x in nodes))
        nodes.append(nd.cpu().numpy())
        starts.append(starts[-1] + p4.shape[0])
    return SimpleNamespace(n=len(clouds), num_points=starts[-1], pt_start=np.asarray(starts, np.int64), pts=np.concatenate(pts),
                           orig=np.concatenate(orig), node_start=np.asarray(node_starts, np.int64), pow2=np.asarray(pow2, np.int32),
                           nodes=np.concatenate(nodes))


def check_gt_invariants(g, clouds):
    """The header's statements about GnbvScanGt, for any packer."""
    assert g.n == len(clouds) and g.pt_start[0] == 0 and g.num_points == g.pt_start[-1]
    assert g.pts.dtype == f32 and g.pts.shape == (g.num_points, 4) and g.nodes.dtype == f32 and g.nodes.shape[1:] == (2, 4)
    for e, y in enumerate(clouds):
        y = np.ascontiguousarray(y, f32).reshape(-1, 3)
        a, b = int(g.pt_start[e]), int(g.pt_start[e + 1])
        m, p = b - a, int(g.pow2[e])
        assert m == y.shape[0] > 0 and p >= -(-m // K_LEAF) and p & (p - 1) == 0, (e, m, p)
        o = g.orig[a:b]
        assert np.array_equal(np.sort(o), np.arange(m)), f"env {e}: orig is no permutation"
        assert g.pts[a:b, :3].tobytes() == y[o].tobytes(), f"env {e}: pts[i] is not point orig[i] of the given cloud"
        nd = g.nodes[int(g.node_start[e]):int(g.node_start[e]) + 2 * p]
        assert nd.shape[0] == 2 * p
        lo, hi = nd[:, 0, :3], nd[:, 1, :3]
        ys = g.pts[a:b, :3]
        for j in range(p):
            leaf = ys[K_LEAF * j:K_LEAF * (j + 1)]
            if leaf.shape[0]:
                assert lo[p + j].tobytes() == leaf.min(0).tobytes() and hi[p + j].tobytes() == leaf.max(0).tobytes(), (e, "leaf", j)
            else:
                assert np.all(lo[p + j] == np.inf) and np.all(hi[p + j] == -np.inf), (e, "empty leaf", j)
        for i in range(1, p):
            assert np.array_equal(lo[i], np.minimum(lo[2 * i], lo[2 * i + 1])) and np.array_equal(hi[i], np.maximum(hi[2 * i], hi[2 * i + 1])), \
                (e, "node", i)


# ---------------------------------------------------------------------------
# references of a score
# ---------------------------------------------------------------------------
_REF = {}


def ref_chamfer(x, y):
    """oracle.chamfer_distance_ref (fp64 brute force) of two fp32 clouds, chunked to about 48 MB, computed once per pair of clouds."""
    x, y = np.ascontiguousarray(x, f32).reshape(-1, 3), np.ascontiguousarray(y, f32).reshape(-1, 3)
    key = (x.shape[0], y.shape[0], hash(x.tobytes()), hash(y.tobytes()))
    if key not in _REF:
        _REF[key] = float(orc.chamfer_distance_ref(x, y, chunk=max(16, 2_000_000 // max(x.shape[0], y.shape[0]))))
    return _REF[key]


def ref_chamfer_many(pairs):
    """ref_chamfer of several (x, y) at once, one thread per pair (numpy releases the GIL): a case's envs side by side."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda xy: ref_chamfer(*xy), pairs))


def ulps(a, b):
    ia, ib = (int(np.asarray([v], f32).view(np.int32)[0]) for v in (a, b))
    return abs(ia - ib)


def assert_close_to_ref(got, want, where):
    """|got - want| <= 8 * 2^-24 |want| + 1e-30 (the module docstring derives it); prints the figure first."""
    got, want = float(got), float(want)
    err = abs(got - want)
    print(f"{where}: got {got!r} fp64 reference {want!r} error {err / max(abs(want), 1e-300) / 2.0 ** -24:.3f} u")
    assert np.isfinite(got) and err <= TOL_REL * abs(want) + TOL_ABS, (where, got, want, err)


# ---------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------
def libs():
    from gennbv_amd import _lib as L
    return L, L.load()


class Buf:
    """`nbytes` bytes at a 256-byte aligned device address (+ `offset`), sentinel bytes in front of and behind them."""
    GUARD = 512

    def __init__(self, nbytes, fill=FILL, offset=0):
        self.nbytes = int(nbytes)
        self.arena = torch.full((self.GUARD + 256 + offset + self.nbytes + self.GUARD,), FILL, dtype=torch.uint8, device=DEV)
        self.lo = self.GUARD + (-(self.arena.data_ptr() + self.GUARD)) % 256 + offset
        self.ptr = self.arena.data_ptr() + self.lo
        self.data = self.arena[self.lo:self.lo + self.nbytes]
        if fill != FILL:
            self.data.fill_(fill)

    @classmethod
    def of(cls, a, dtype):
        a = np.ascontiguousarray(a, dtype)
        b = cls(a.nbytes)
        b.write(a)
        return b

    def write(self, a):
        a = np.array(a, copy=True, order="C")
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        self.data.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))

    def read(self, dtype, shape=-1):
        return self.data.cpu().numpy().view(dtype).reshape(shape)

    def row(self, r, row_bytes, dtype):
        return self.data[r * row_bytes:(r + 1) * row_bytes].cpu().numpy().view(dtype)

    def intact(self):
        a = self.arena
        return bool((a[:self.lo] == FILL).all()) and bool((a[self.lo + self.nbytes:] == FILL).all())

    def snapshot(self):
        return self.arena.cpu().numpy().tobytes()


class GtDev:
    """A packed GT on the device and its GnbvScanGt."""

    def __init__(self, g):
        L, _ = libs()
        self.g = g
        self.pt_start, self.pts, self.orig = Buf.of(g.pt_start, np.int64), Buf.of(g.pts, f32), Buf.of(g.orig, np.int32)
        self.node_start, self.pow2, self.nodes = Buf.of(g.node_start, np.int64), Buf.of(g.pow2, np.int32), Buf.of(g.nodes, f32)
        self.bufs = [self.pt_start, self.pts, self.orig, self.node_start, self.pow2, self.nodes]
        self.struct = L.GnbvScanGt(g.n, g.num_points, self.pt_start.ptr, self.pts.ptr, self.orig.ptr, self.node_start.ptr, self.pow2.ptr,
                                   self.nodes.ptr)


class ScanCall:
    """The scan entry points on buffers the test owns: table (0xFF bytes), keys, counts, flags, accuracy (sentinel bits), scored,
    and workspaces exactly gnbv_scan_workspace_bytes long."""

    def __init__(self, n, cap, gt=None):
        self.L, self.lib = libs()
        self.n, self.cap = n, cap
        assert int(self.lib.gnbv_scan_set_bytes(n, cap)) == n * cap * 16 + n * 8
        self.table, self.keys = Buf(n * cap * 8, fill=0xFF), Buf(n * cap * 8)
        self.counts, self.flags, self.scored = Buf(n * 4, fill=0), Buf(n * 4, fill=0), Buf(n * 4, fill=0)
        self.accuracy = Buf(n * 4)
        self.set = self.L.GnbvScanSet(n, cap, self.table.ptr, self.keys.ptr, self.counts.ptr, self.flags.ptr)
        self.xws_bytes = int(self.lib.gnbv_scan_workspace_bytes(1, cap, 0))
        self.xws = Buf(self.xws_bytes)
        self.mask = Buf(n)
        self.gt = self.ws = None
        self.ws_bytes = 0
        self.frame_bufs = []
        if gt is not None:
            self.use_gt(gt)

    def use_gt(self, g):
        self.gt = GtDev(g)
        self.ws_bytes = int(self.lib.gnbv_scan_workspace_bytes(self.n, self.cap, g.num_points))
        assert self.ws_bytes > 0 and self.ws_bytes % 256 == 0
        self.ws = Buf(self.ws_bytes)

    # ---- the entry points; each returns the error code ----
    def add(self, fr, set_=None):
        assert fr.n == self.n
        d, s, m = Buf.of(fr.depth, f32), Buf.of(fr.seg, f32), Buf.of(fr.c2w, f32)
        kinv = (C.c_float * 9)(*fr.kinv.reshape(-1).tolist())
        err = self.lib.gnbv_scan_add_frame(C.byref(set_ or self.set), d.ptr, s.ptr, m.ptr, kinv, fr.h, fr.w, SENSE, None)
        torch.cuda.synchronize()
        self.frame_bufs = [d, s, m]
        return err

    def clear(self, mask, set_=None, null_mask=False):
        self.mask.write(np.asarray(mask, np.uint8))
        err = self.lib.gnbv_scan_clear(C.byref(set_ or self.set), None if null_mask else self.mask.ptr, None)
        torch.cuda.synchronize()
        return err

    def score(self, mask, set_=None, gt=None, null_mask=False, ws_ptr=None, ws_bytes=None):
        self.mask.write(np.asarray(mask, np.uint8))
        err = self.lib.gnbv_scan_score(C.byref(set_ or self.set), C.byref(gt or self.gt.struct), None if null_mask else self.mask.ptr,
                                       self.accuracy.ptr, self.scored.ptr, self.ws.ptr if ws_ptr is None else ws_ptr,
                                       self.ws_bytes if ws_bytes is None else ws_bytes, None)
        torch.cuda.synchronize()
        return err

    def export_raw(self, env, out, set_=None, ws_ptr=None, ws_bytes=None):
        err = self.lib.gnbv_scan_export(C.byref(set_ or self.set), env, out.ptr, self.xws.ptr if ws_ptr is None else ws_ptr,
                                        self.xws_bytes if ws_bytes is None else ws_bytes, None)
        torch.cuda.synchronize()
        return err

    def export(self, env):
        """Env's rows [counts[env], 3]; the output buffer is exactly that long, between sentinels."""
        count = int(self.read_counts()[env])
        assert 0 < count <= self.cap
        out = Buf(count * 12)
        assert self.export_raw(env, out) == 0
        assert out.intact() and self.xws.intact(), f"export of env {env} wrote outside its buffers"
        return out.read(f32, (count, 3))

    # ---- state ----
    def read_counts(self):
        return self.counts.read(np.int32)

    def read_flags(self):
        return self.flags.read(np.int32)

    def read_accuracy(self):
        return self.accuracy.read(f32)

    def read_scored(self):
        return self.scored.read(np.int32)

    def keys_row(self, e):
        return self.keys.row(e, self.cap * 8, np.uint64)

    def table_row(self, e):
        return self.table.row(e, self.cap * 8, np.uint64)

    def buffers(self):
        b = [self.table, self.keys, self.counts, self.flags, self.accuracy, self.scored, self.xws, self.mask] + self.frame_bufs
        if self.gt is not None:
            b += [self.ws] + self.gt.bufs
        return b

    def intact(self):
        return all(b.intact() for b in self.buffers())

    def snapshot(self, ws=False):
        """The set, `accuracy` and `scored` (ws: and the workspaces), sentinels included, as bytes."""
        b = [self.table, self.keys, self.counts, self.flags, self.accuracy, self.scored]
        if ws:
            b += [self.xws] + ([self.ws] if self.ws is not None else [])
        return [x.snapshot() for x in b]

    # ---- against the oracle ----
    def check_set(self, oracle, envs, where):
        """counts and flags of every env, and the export of `envs` (those with keys), against the oracle, bit for bit."""
        counts, flags = self.read_counts(), self.read_flags()
        assert np.array_equal(counts, oracle.counts), (where, "counts", counts[:16], oracle.counts[:16])
        assert np.array_equal(flags, oracle.flags), (where, "flags", flags[:16], oracle.flags[:16])
        for e in envs:
            if oracle.counts[e]:
                got, want = self.export(e), oracle.points(e)
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), \
                    (where, "export of env", e, np.nonzero((got.view(np.int32) != want.view(np.int32)).any(1))[0][:8])
        assert self.intact(), f"{where}: bytes outside a buffer were written"

    def check_scores(self, oracle, clouds, envs, where):
        """accuracy[e] of `envs` against 100 x the fp64 brute force (8 u relative) and against gnbv_chamfer_distance x 100.0f over
        the exported points (2 ulps); returns the accuracies."""
        acc = self.read_accuracy()
        ref_chamfer_many([(oracle.points(e), clouds[e]) for e in envs])
        for e in envs:
            x, y = oracle.points(e), np.ascontiguousarray(clouds[e], f32)
            assert_close_to_ref(acc[e], 100.0 * ref_chamfer(x, y), f"{where} env {e} ({x.shape[0]} keys, {y.shape[0]} GT)")
            dev = f32(device_chamfer(x, y)) * f32(100.0)
            assert ulps(acc[e], dev) <= 2, (where, e, float(acc[e]), float(dev))
        return acc


def device_chamfer(x, y, ws_short=0, ws_offset=0):
    """gnbv_chamfer_distance of two clouds: its fp32 result, or the error code when the workspace is made wrong on purpose."""
    _, lib = libs()
    x, y = np.ascontiguousarray(x, f32).reshape(-1, 3), np.ascontiguousarray(y, f32).reshape(-1, 3)
    n, m = x.shape[0], y.shape[0]
    need = int(lib.gnbv_chamfer_workspace_bytes(n, m))
    bx, by, out, ws = Buf.of(x, f32), Buf.of(y, f32), Buf(4), Buf(need, offset=ws_offset)
    before = [b.snapshot() for b in (out, ws)]
    err = lib.gnbv_chamfer_distance(bx.ptr, n, by.ptr, m, out.ptr, ws.ptr, need - ws_short, None)
    torch.cuda.synchronize()
    assert all(b.intact() for b in (bx, by, out, ws)), "gnbv_chamfer_distance wrote outside its buffers"
    if ws_short or ws_offset:
        assert [b.snapshot() for b in (out, ws)] == before, "a refused call wrote"
        return err
    assert err == 0
    return out.read(f32)[0]


# ---------------------------------------------------------------------------
# the cases: id -> inputs (built once, numpy only)
# ---------------------------------------------------------------------------
cached = functools.lru_cache(maxsize=None)


def final_oracle(n, cap, frames):
    o = SetOracle(n, cap)
    for fr in frames:
        o.add(fr)
    return o


def gt_near(points, m, seed, margin=0.05):
    """m uniform points in the (slightly grown) bounding box of `points`."""
    rs = np.random.RandomState(seed)
    lo, hi = points.min(0).astype(np.float64) - margin, points.max(0).astype(np.float64) + margin
    return (lo + (hi - lo) * rs.rand(m, 3)).astype(f32)


def _counted_case(counts, cap, gt_sizes, seed, t0=None):
    """Lattice sets of the given sizes and, per env, a random GT cloud of gt_sizes[e] points around its keys."""
    n = len(counts)
    frames = layered_frames(counts, base_translations(n) if t0 is None else t0)
    o = final_oracle(n, cap, frames)
    anchor = [o.points(e) if o.counts[e] else np.zeros((1, 3), f32) for e in range(n)]
    clouds = [gt_near(anchor[e], gt_sizes[e], seed + e) for e in range(n)]
    return SimpleNamespace(n=n, cap=cap, frames=frames, final=o, clouds=clouds, counts=list(counts))


def _case_cap64():
    t0 = np.asarray([[0.03, 0.03, 0.03], [-0.37, -0.33, 0.03]])  # env 1: negative keys, still = 3 mod 4
    dz = np.asarray([0.0, 0.0, 0.04])
    frames = [lattice_frame(np.round(t0 + f * dz, 2), 4, 8, s=0.04) for f in range(2)]
    frames[1].seg[1] = 0.0  # env 1 stops at 32 keys
    extra = lattice_frame(np.round(t0 + 2 * dz, 2), 1, 1, s=0.04)
    o = final_oracle(2, 64, frames)
    clouds = [gt_near(o.points(e), 33, 640 + e) for e in range(2)]
    return SimpleNamespace(n=2, cap=64, frames=frames, extra=extra, final=o, clouds=clouds)


def _case_load_factor_one():
    t0 = np.asarray([[0.5, -0.25, 0.0], [-7.13, -2.4, -1.5]])
    frames = layered_frames([4096, 4096], t0)
    half = lattice_frame(np.round(t0, 2), 32, 64)  # the first layer again: half of the keys
    return SimpleNamespace(n=2, cap=4096, frames=frames + [half], final=final_oracle(2, 4096, frames + [half]))


def _two_key_frame(t, h, w, every=True):
    """inv_intri = diag(0, 0, 1): a pixel of raw depth 0 is t, one of raw depth -1 is t + (0, 0, 1); they alternate lane by lane."""
    n = len(t)
    depth = np.where(np.arange(h * w) % 2 == 0, 0.0, -1.0 if every else 0.0).astype(f32)
    return lattice_frame(t, h, w, s=0.0, depth=np.tile(depth, (n, 1)))


def _case_duplicates():
    t = np.asarray([[1.0, 2.0, 3.0], [-0.07, 0.0, 10.24], [-5.11, 7.77, -0.01]])
    subs = {"16x16-one-key": [_two_key_frame(t, 16, 16, every=False)], "16x16-two-keys": [_two_key_frame(t, 16, 16)],
            "5x13-two-keys": [_two_key_frame(t, 5, 13)], "1x1": [point_frame(t)]}
    return SimpleNamespace(n=3, cap=64, subs=subs, finals={k: final_oracle(3, 64, v) for k, v in subs.items()})


EDGE = 10485.75  # fp32 exactly; 100 x = 2^20 - 1 exactly
OVER = 10485.76  # fp32 10485.759765625; fl(100 x) = 2^20


def _case_key_range():
    sign = np.asarray([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)
    t = np.zeros((16, 3))
    t[:8] = sign * EDGE
    t[8], t[9], t[10], t[11] = (OVER, 1.0, 2.0), (1.0, -OVER, 2.0), (1.0, 2.0, OVER), (-OVER, -1.0, -2.0)
    t[12], t[13], t[14] = (1.0, np.nan, 2.0), (1.0, 2.0, np.inf), (-np.inf, 1.0, 2.0)
    t[15] = (EDGE, 0.5, -0.25)
    # 1 x 2 frames, inv_intri = diag(0.01, 0.01, 1): pixel 0 has raw depth 0 (the translation itself); pixel 1 is background except
    # in env 15, where raw depth -1 makes it (0.01 + EDGE, 0.5, 0.75): x is out of range
    depth = np.zeros((16, 1, 2), f32)
    depth[15, 0, 1] = -1.0
    fg = np.zeros((16, 2), bool)
    fg[:, 0] = True
    fg[15, 1] = True
    with np.errstate(invalid="ignore"):
        fr = lattice_frame(t, 1, 2, fg=fg, depth=depth)
    want = np.zeros((16, 3), np.int64)
    want[:8] = (sign * (KEY_LIMIT - 1)).astype(np.int64)
    want[15] = (KEY_LIMIT - 1, 50, -25)
    return SimpleNamespace(n=16, cap=64, frames=[fr], final=final_oracle(16, 64, [fr]), want=want, accepted=list(range(8)) + [15],
                           refused=list(range(8, 15)))


def _case_masked_clear():
    n, t0 = 5, base_translations(5)
    a = lattice_frame(t0, 8, 8)
    bad = np.zeros((n, 3))
    bad[0, 0] = bad[1, 2] = np.inf
    b = point_frame(bad, fg=[1, 1, 0, 0, 0])  # flag bit 1 on env 0 (cleared below) and env 1 (kept)
    c = lattice_frame(np.round(t0 + 0.5, 2), 8, 8, fg=first_pixels([40, 41, 42, 43, 44], 64))
    return SimpleNamespace(n=n, cap=128, before=[a, b], mask=np.asarray([1, 0, 1, 0, 0], np.uint8), after=[c],
                           final=final_oracle(n, 128, [a, b]))


def _case_insertion_order():
    rs = np.random.RandomState(11)
    n, h, w = 2, 24, 40
    t0 = base_translations(n)
    frames = []
    for f in range(4):  # depths 1.00 .. 1.07 m per pixel: overlapping, irregular key sets
        depth = -(1.0 + 0.01 * rs.randint(0, 8, (n, h, w))).astype(f32)
        frames.append(lattice_frame(np.round(t0 + 0.02 * f, 2), h, w, fg=rs.rand(n, h * w) < 0.8, depth=depth))
    cap = 4096
    o3, o4 = final_oracle(n, cap, frames[:3]), final_oracle(n, cap, frames)
    clouds = [gt_near(o4.points(e), 700 + 37 * e, 110 + e) for e in range(n)]
    return SimpleNamespace(n=n, cap=cap, frames=frames, orders=[(0, 1, 2), (2, 0, 1)], final=o3, final4=o4, clouds=clouds)


TREE_COUNTS = [1, 32, 33, 64, 65, 1024, 1025]
TREE_GT = [1, 32, 33, 1025, 1, 32, 33]  # the four GT sizes run along the diagonal of the seven counts


def _case_degenerate():
    counts = [300, 300, 300, 2049, 300]
    c = _counted_case(counts, 2112, [1] * 5, 0)
    o = c.final
    p2 = o.points(2)
    row = p2[(p2[:, 1] == p2[0, 1]) & (p2[:, 2] == p2[0, 2])]  # the lattice points that share the first key's y and z
    line = np.concatenate([row, row + np.asarray([0.64, 0.0, 0.0], f32), row - np.asarray([0.3, 0.0, 0.0], f32)]).astype(f32)
    p3 = o.points(3)
    ties = np.concatenate([p3 + s * np.eye(3, dtype=f32)[a] * f32(0.005) for a in range(3) for s in (f32(1), f32(-1))]).astype(f32)
    c.clouds = [o.points(0).copy(), np.tile(np.asarray([[0.31, -0.2, 1.0]], f32), (100, 1)), line, ties,
                (np.random.RandomState(5).rand(200, 3) + np.asarray([40.0, 0.0, 0.0])).astype(f32)]
    c.row = row
    return c


def _case_gt_order():
    c = _counted_case([500, 1025, 2049], 2112, [1000, 33, 2500], 300)
    rs = np.random.RandomState(9)
    c.perms = [rs.permutation(y.shape[0]) for y in c.clouds]
    return c


def _case_mask_semantics():
    n, t0 = 6, base_translations(6)
    a = lattice_frame(t0, 8, 8, fg=first_pixels([64, 50, 40, 0, 30, 33], 64))
    bad = np.zeros((n, 3))
    bad[4, 1] = np.nan
    b = point_frame(bad, fg=[0, 0, 0, 0, 1, 0])
    o = final_oracle(n, 128, [a, b])
    anchor = [o.points(e) if o.counts[e] else np.zeros((1, 3), f32) for e in range(n)]
    clouds = [gt_near(anchor[e], 40 + e, 500 + e) for e in range(n)]
    return SimpleNamespace(n=n, cap=128, frames=[a, b], final=o, clouds=clouds, mask=np.asarray([1, 0, 1, 1, 1, 1], np.uint8),
                           prescored=2, active=[0, 5], inactive=[1, 2, 3, 4])


def _case_tiles_over_blocks():
    n, cap = 1024, 10240
    counts = np.zeros(n, np.int64)
    counts[0], counts[511], counts[1023] = 10240, 8193, 2049
    frames = layered_frames(counts, base_translations(n))
    o = final_oracle(n, cap, frames)
    clouds = [np.asarray([[0.1 * (e % 5), 0.2, 0.3]], f32) for e in range(n)]
    for e in (0, 511, 1023):
        clouds[e] = gt_near(o.points(e), 2048, 700 + e)
    return SimpleNamespace(n=n, cap=cap, frames=frames, final=o, clouds=clouds, loaded=[0, 511, 1023], counts=counts.tolist())


def _case_clear_grid_stride():
    return SimpleNamespace(n=1024, cap=4096)


CASES = {
    "cap64-fill-wrap": _case_cap64,
    "load-factor-one": _case_load_factor_one,
    "duplicates-in-a-wave": _case_duplicates,
    "key-range-edges": _case_key_range,
    "masked-clear": _case_masked_clear,
    "clear-grid-stride": _case_clear_grid_stride,
    "tile-edges": lambda: _counted_case([1, 8, 2047, 2048, 2049, 0], 4096, [40, 41, 42, 43, 44, 45], 100),
    "scan-carry": lambda: _counted_case([32768, 34817], 36864, [2048, 2048], 200, t0=[[0.5, -0.25, 0.0], [-7.13, -2.4, -1.5]]),
    "tiles-over-blocks": _case_tiles_over_blocks,
    "insertion-order": _case_insertion_order,
    "tree-sizes": lambda: _counted_case(TREE_COUNTS, 1088, TREE_GT, 400),
    "degenerate-gt": _case_degenerate,
    "gt-order": _case_gt_order,
    "mask-semantics": _case_mask_semantics,
}
CHAMFER_SHAPES = [(1024, 1024), (1025, 1023), (4, 1), (5, 2049), (4096, 3)]
K_NN_TILE, K_NN_PER_WG = 1024, 256 * 4  # csrc/chamfer.hip: kTile; kNNThreads * kPtsPerThread queries per workgroup


@cached
def case(cid):
    return CASES[cid]()


@cached
def chamfer_clouds(n, m):
    rs = np.random.RandomState(n * 7 + m)
    return ((rs.rand(n, 3) - 0.5) * 4.0).astype(f32), ((rs.rand(m, 3) - 0.5) * 4.0 + 0.25).astype(f32)


def _sort_info(n, counts):
    b, counts = blocks_per_env(n), [int(c) for c in counts]
    return dict(blocks=b, counts=counts, tiles=[tiles_of(c) for c in counts],
                tile_trips=[-(-tiles_of(c) // b) for c in counts], scan_chunks=[scan_chunks(c) for c in counts],
                P=[tree_pow2(c) for c in counts])


def _mod4(o, e):
    return np.unique(o.keys[e] % 4).tolist()


def check_regime(cid):
    """The case reaches what its id names -- from n, the shapes and the ORACLE's sets alone; returns the figures it used."""
    c = case(cid)
    if cid == "clear-grid-stride":
        info = dict(uint4_per_env=c.cap // 2, threads_per_env=blocks_per_env(c.n) * K_CLEAR_THREADS, trips=clear_trips(c.n, c.cap))
        assert blocks_per_env(c.n) == 4 and c.cap // 2 > 4 * K_CLEAR_THREADS and info["trips"] == 2
        assert clear_trips(5, 128) == 1  # (masked-clear: one trip)
        return info
    if cid == "duplicates-in-a-wave":
        info = {k: o.counts.tolist() for k, o in c.finals.items()}
        assert info == {"16x16-one-key": [1] * 3, "16x16-two-keys": [2] * 3, "5x13-two-keys": [2] * 3, "1x1": [1] * 3}
        fr = c.subs["5x13-two-keys"][0]
        assert fr.h * fr.w == 65 and 65 % 64 == 1  # the second wave has one pixel: lanes >= hw take part in the ballots
        assert all(not o.flags.any() for o in c.finals.values())
        return info
    o = c.final
    counts = o.counts
    info = _sort_info(c.n, counts[counts > 0][:8]) if c.n > 16 else _sort_info(c.n, counts)
    info["flags"] = o.flags[:16].tolist()
    if cid == "cap64-fill-wrap":
        info["mod4"] = [_mod4(o, e) for e in range(2)]
        # cap >> 6 == 1: the first slot of a key is its low six code bits = the low two bits of its three fields (2^20 = 0 mod 4)
        assert c.cap >> 6 == 1 and counts.tolist() == [64, 32] and info["mod4"] == [[3], [3]] and not o.flags.any()
        assert all(fr.h * fr.w == 32 for fr in c.frames) and (o.keys[1] < 0).any()
        full = final_oracle(2, 64, c.frames + [c.extra])
        assert full.counts.tolist() == [64, 33] and full.flags.tolist() == [FLAG_OVERFLOW, 0]
        assert _mod4(full, 1) == [3]
    elif cid == "load-factor-one":
        two = final_oracle(2, c.cap, c.frames[:2])
        assert two.counts.tolist() == [4096, 4096] == counts.tolist() and c.cap == 4096 and not o.flags.any()
        half = final_oracle(2, c.cap, c.frames[2:])
        assert half.counts.tolist() == [2048, 2048] and all(np.array_equal(o.keys[e], two.keys[e]) for e in range(2))
    elif cid == "key-range-edges":
        assert f32(EDGE) * f32(100) == f32(KEY_LIMIT - 1) and f32(OVER) * f32(100) == f32(KEY_LIMIT)  # the fp32 products land on them
        for e in c.accepted:
            assert o.keys[e].tolist() == [c.want[e].tolist()], (e, o.keys[e])
        assert sorted({tuple(np.sign(o.keys[e][0])) for e in range(8)}) == sorted({(a, b, d) for a in (1, -1) for b in (1, -1) for d in (1, -1)})
        assert all(np.abs(o.keys[e]).max() == KEY_LIMIT - 1 for e in c.accepted)
        assert all(o.counts[e] == 0 and o.flags[e] == FLAG_RANGE for e in c.refused)
        assert o.flags[:8].tolist() == [0] * 8 and o.counts[15] == 1 and o.flags[15] == FLAG_RANGE
        assert np.array_equal(o.points(0), (f32(KEY_LIMIT - 1) * f32(0.01)) * np.ones((1, 3), f32))
    elif cid == "masked-clear":
        assert c.n == 5 and c.cap == 128 and counts.tolist() == [64] * 5 and o.flags.tolist() == [2, 2, 0, 0, 0]
        after = final_oracle(c.n, c.cap, c.after)
        assert after.counts.tolist() == [40, 41, 42, 43, 44]
        assert not (set(map(tuple, after.keys[0])) & set(map(tuple, o.keys[0])))  # the re-added keys are new ones
    elif cid == "tile-edges":
        assert counts.tolist() == [1, 8, 2047, 2048, 2049, 0] and info["tiles"] == [1, 1, 1, 1, 2, 0] and c.cap == 4096
    elif cid == "scan-carry":
        assert counts.tolist() == [32768, 34817] and info["tiles"] == [16, 18] and info["scan_chunks"] == [1, 2]
        assert 16 * 16 == K_SCAN_CHUNK and info["blocks"] == 256 and all(y.shape[0] == 2048 for y in c.clouds)
    elif cid == "tiles-over-blocks":
        assert info["blocks"] == 4 and [int(counts[e]) for e in c.loaded] == [10240, 8193, 2049] and int(counts.sum()) == 20482
        assert info["tiles"] == [5, 5, 2] and info["tile_trips"] == [2, 2, 1] and c.cap == 10240
        assert all(c.clouds[e].shape[0] == 1 for e in range(c.n) if e not in c.loaded)
    elif cid == "insertion-order":
        assert sorted(c.orders[0]) == sorted(c.orders[1]) and c.orders[0] != c.orders[1]
        singles = [final_oracle(c.n, c.cap, [fr]) for fr in c.frames]
        for e in range(c.n):  # the frames overlap without repeating each other, and the fourth adds keys
            assert max(s.counts[e] for s in singles[:3]) < counts[e] < sum(s.counts[e] for s in singles[:3])
            assert c.final4.counts[e] > counts[e]
        info["counts_after_4"] = c.final4.counts.tolist()
    elif cid == "tree-sizes":
        assert counts.tolist() == TREE_COUNTS and info["P"] == [1, 1, 2, 2, 4, 32, 64]
        g = pack_gt(c.clouds)
        assert [y.shape[0] for y in c.clouds] == TREE_GT and g.pow2.tolist() == [1, 1, 2, 64, 1, 1, 2]
        info["gt_P"] = g.pow2.tolist()
    elif cid == "degenerate-gt":
        g = pack_gt(c.clouds)
        lo, hi = g.nodes[:, 0, :3], g.nodes[:, 1, :3]
        nodes_of = lambda e: slice(int(g.node_start[e]) + 1, int(g.node_start[e]) + 2 * int(g.pow2[e]))  # noqa: E731
        assert counts.tolist() == [300, 300, 300, 2049, 300] and c.clouds[0].tobytes() == o.points(0).tobytes()
        assert np.unique(c.clouds[1], axis=0).shape[0] == 1 and c.clouds[1].shape[0] == 100 and np.array_equal(lo[nodes_of(1)][-4:], hi[nodes_of(1)][-4:])
        s = nodes_of(2)  # every box of the line has zero extent in y and z, there are several leaves, and lattice points lie in them
        full = np.isfinite(lo[s]).all(1)
        assert c.row.shape[0] == 64 and g.pow2[2] >= 4 and np.array_equal(lo[s][full][:, 1:], hi[s][full][:, 1:])
        assert (o.points(2)[:, None, :] == c.clouds[2][None, :, :]).all(-1).any(1).sum() == 64  # lb == 0 for these queries
        assert c.clouds[3].shape[0] == 6 * 2049 and np.unique(c.clouds[3], axis=0).shape[0] > 3 * 2049
        assert np.abs(c.clouds[4] - o.points(4).mean(0)).max() > 35.0
        info["gt_P"] = g.pow2.tolist()
    elif cid == "gt-order":
        assert counts.tolist() == [500, 1025, 2049] and all(not np.array_equal(p, np.arange(p.size)) for p in c.perms)
        for g in (pack_gt(c.clouds), pack_gt(c.clouds, c.perms, extra_levels=1), pack_from_gt_tree(c.clouds)):
            check_gt_invariants(g, c.clouds)
        info["gt_P"] = [pack_gt(c.clouds).pow2.tolist(), pack_gt(c.clouds, c.perms, extra_levels=1).pow2.tolist(), pack_from_gt_tree(c.clouds).pow2.tolist()]
    elif cid == "mask-semantics":
        assert counts.tolist() == [64, 50, 40, 0, 30, 33] and o.flags.tolist() == [0, 0, 0, 0, FLAG_RANGE, 0]
        assert c.mask.tolist() == [1, 0, 1, 1, 1, 1] and c.prescored == 2 and c.active == [0, 5]
    else:
        raise KeyError(cid)
    return info
