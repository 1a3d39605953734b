"""CPU: the numpy references of tests/voxel_ops_ref.py against the CPU oracle, bit for bit, on the exact inputs of
tests/test_voxel_ops_abi_gpu.py, the back-projection bound for the oracle, and the conditions that keep every GPU case from being vacuous
(each planted class present and classified as the case intends, the shares of kept and dropped points, counts beyond one pass of the
grid-stride loops).  A case that stops exercising an edge fails here first.  The measured shares are printed (pytest -s)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import voxel_abi_util as U
from tests import voxel_ops_ref as R
from tests.voxel_ops_ref import f32

FILL32 = np.frombuffer(bytes([U.FILL]) * 4, np.int32)[0]


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("sense", R.DEPTH_SENSE)
@pytest.mark.parametrize("count", R.DEPTH_COUNTS)
def test_post_process_depth_ref_vs_oracle(count, sense):
    c = R.depth_case(count, sense)
    d, s = R.post_process_depth(c.depth, c.seg, sense)
    do, so = orc.post_process_depth(c.depth, c.seg, sense)
    _same(d, do)
    _same(s, so)
    if count == 1:
        assert R.bits_of(d)[0] == 0 and R.bits_of(s)[0] == 0x80000000  # -0.0: the depth loses its sign, the seg keeps it
    if count > 1:
        assert count > U.GRID_STRIDE_THREADS
        for a in (c.depth, c.seg):
            for ends in (a[:16], a[-16:], a[16:-16]):
                assert R.bitset(c.specials) <= R.bitset(ends)
        assert not np.isnan(d).any() and (d >= 0).all() and not np.signbit(d).any() and d.max() == R.FLT_MAX
        assert (d == f32(-sense)).sum() > 1000 and (d < f32(-sense)).sum() > 1000 and (d[d < f32(-sense)] > 0).any()
        keep = np.isfinite(c.seg)
        _same(s[keep], c.seg[keep])
        assert (R.bits_of(s) == 0x80000000).any() and not np.isnan(s).any() and np.isfinite(s).all()


@pytest.mark.parametrize("pinhole", [True, False], ids=["pinhole", "generic"])
@pytest.mark.parametrize("n,h,w", R.BACKPROJ_SHAPES)
def test_back_projection_oracle_within_bound(n, h, w, pinhole):
    """The oracle's worst err/bound on these inputs: 1x1x1 0.08 / 0.00, 3x7x9 0.16 / 0.14, 2x48x64 0.20 / 0.19, 7x240x320 0.26 / 0.29
    (pinhole / generic)."""
    c = R.backproj_case(n, h, w, pinhole)
    assert (c.kinv != 0).sum() == (5 if pinhole else 9) and np.isnan(c.c2w[:, 3]).all()
    world, fg = orc.back_projection(c.depth, c.seg, c.c2w, c.kinv)
    want, bound, fg64 = R.back_projection_f64(c.depth, c.seg, c.c2w, c.kinv)
    assert np.array_equal(fg, c.is_fg) and np.array_equal(fg64, c.is_fg)
    assert np.isfinite(world).all() and np.isfinite(want).all()
    worst = R.err_over_bound(world, want, bound)
    shares = c.is_fg.mean(1)
    print(f"back_projection {n}x{h}x{w} {'pinhole' if pinhole else 'generic'}: oracle err/bound {worst:.3f}, fg share per env {np.round(shares, 3).tolist()}")
    assert worst <= 1.0
    t = np.broadcast_to(c.c2w[:, None, :3, 3], world.shape)
    _same(world[~c.is_fg], np.ascontiguousarray(t[~c.is_fg]))   # a background pixel lands on the translation column, whatever its depth
    assert not np.isfinite(c.depth.reshape(n, -1)[~c.is_fg]).any()
    if h * w > 1:
        assert (shares >= 0.1).all() and (shares <= 0.9).all()
        seg_bits = R.bitset(c.seg)
        assert R.bitset(np.concatenate([R.SEG_BG, R.SEG_FG])) <= seg_bits
    if (n, h, w) == R.BACKPROJ_SHAPES[-1]:
        assert n * h * w > U.GRID_STRIDE_THREADS


@pytest.mark.parametrize("n,hw,g", R.POINTS_CASES)
def test_points_to_idx_ref_vs_oracle(n, hw, g):
    c = R.points_case(n, hw, g)
    idx = R.points_to_idx(c.world, c.fg, c.range_gt, c.voxel_size, g)
    _same(idx, orc.points_to_idx(c.world, c.fg, c.range_gt, c.voxel_size, g))
    kept = idx[..., 0] >= 0
    assert ((idx >= 0).all(-1) == kept).all() and (idx[kept] < g).all() and (idx[~kept] == -1).all()
    for name, where in c.classes.items():
        for e, p, a in where:
            if name in R.POINT_CLASSES_DROPPED:
                assert not kept[e, p], (name, e, p)
            else:
                assert kept[e, p], (name, e, p)
            if name == "ulp_inside_vmin":
                assert idx[e, p, a] == 0
            if name == "ulp_inside_vmax":
                assert idx[e, p, a] == g - 1
    assert set(np.unique(c.fg).tolist()) <= {0, 1, 2, 255}
    if hw == 1:
        assert kept.reshape(-1).tolist() == [True, False, True] and c.fg[2, 0] == 255
        return
    assert all(len(w) >= n for w in c.classes.values()), "a planted class is missing"
    assert set(np.unique(c.fg).tolist()) == {0, 1, 2, 255}
    for b in (2, 255):  # any non-zero byte is foreground
        assert kept[c.fg == b].any()
    shares = kept.mean(1)
    print(f"points_to_idx n={n} hw={hw} g={g}: kept share per env {np.round(shares, 3).tolist()}")
    assert (shares >= 0.25).all() and (1 - shares >= 0.1).all()
    if hw > 37:
        assert n * hw > U.GRID_STRIDE_THREADS


@pytest.mark.parametrize("n", R.POSE_NS)
def test_pose_to_idx_ref_vs_oracle(n):
    c = R.pose_case(n)
    idx = R.pose_to_idx(c.poses, c.range_gt, c.voxel_size)
    _same(idx, orc.pose_to_idx(c.poses, c.range_gt, c.voxel_size))
    q = R.pose_quotient(c.poses, c.range_gt, c.voxel_size)
    assert (idx < 0).any() and ((q > -1) & (q < 0)).any() and (idx[(q > -1) & (q < 0)] == -1).all()
    assert (np.abs(q) < 2.0 ** 31).all()
    if n >= 3:
        assert (idx > 15).any() and ((idx >= 0) & (idx < 16)).any() and (q == np.floor(q)).any()
    if n == 300:
        assert 3 * n > 256 and np.abs(idx).max() > 1e5


def test_bresenham_sources_cover_every_class():
    for g in (2, 7, 33, 128):
        s = np.stack(R.bresenham_sources(g))
        inside = ((s >= 0) & (s < g)).all(1)
        assert inside.any() and (s[inside] == 0).all(1).any() and (s < 0).any() and (s >= g).any() and np.abs(s).max() == 10 * g


@pytest.mark.parametrize("rays,g", R.BRESENHAM_CASES)
def test_bresenham_ref_vs_oracle(rays, g):
    c = R.bresenham_case(rays, g)
    assert len(c.runs) >= (1 if g == 1 else 5)
    for src, tgt in c.runs:
        assert tgt.shape == (rays, 3)
        traj, lens = orc.bresenham3d(src, tgt, g)
        if rays == 0:
            continue
        k = min(rays, R.BRESENHAM_PY_RAYS)
        t_py, l_py = R.bresenham3d(src, tgt[:k], g, 0)
        _same(l_py, lens[:k])
        _same(t_py, traj[:k])
        filled = np.where(np.arange(3 * g)[None, :, None] < lens[:, None, None], traj, FILL32)
        R.check_ray_properties(src, tgt, filled, lens, g, FILL32)
        cls = R.ray_classes(src, tgt)
        if rays >= 255 and g > 2:
            assert all(v > 0 for v in cls.values()), cls
            inb = ((tgt >= 0) & (tgt < g)).all(1)
            assert inb.any() and (~inb).any()
    if rays == 1:
        assert R.ray_classes(*c.runs[0])["tie_xy"] == 1  # the one ray of the case ties its two largest deltas


@pytest.mark.parametrize("n", R.PACK_NS)
@pytest.mark.parametrize("g", R.PACK_GS)
def test_bit_pack_refs_agree(n, g):
    c = R.pack_case(n, g)
    words = U.mask_words(g)
    assert words % 64 == 0 and words * 32 >= g ** 3
    for grid in (c.binary, c.mixed):
        bits = R.pack_bits(grid, g)
        _same(bits, U.pack_bits(grid, g))
        with np.errstate(invalid="ignore"):
            _same(R.unpack_bits(bits, g), (grid != 0).astype(f32))
        assert not bits[:, (g ** 3 + 31) // 32:].any()
    assert R.not_binary(c.binary) == 0 and R.not_binary(c.mixed) == 1
    assert (R.bits_of(c.binary) == 0x80000000).any() or g == 1
    for v in R.OTHER_VALUES:
        x = c.binary.copy()
        x[-1, -1] = v
        assert R.not_binary(x) == 1
    if g ** 3 >= 16:
        assert R.bitset(np.concatenate([R.BINARY_VALUES, R.OTHER_VALUES])) <= R.bitset(c.mixed)
        assert R.pack_bits(c.mixed, g)[0, 0] & 0xFF == 0b11111010  # 0, 1, -0.0, 0.5, -1, NaN, inf, a denormal
    pad = R.unpack_bits(c.words, g)
    _same(R.pack_bits(pad, g)[:, :g ** 3 // 32], c.words[:, :g ** 3 // 32])
    assert c.words[:, -1].any()
    assert (g == 65) == (g ** 3 > 1024 * 256) or g < 65


def test_code_tables_and_decode_cases():
    prob, tri = R.prob_code_tables()
    assert prob[0] == 0 and prob[128] == 1 and prob[129] == f32(f32(1) - f32(0.05)) and (np.diff(prob[:128]) < 0).all()
    assert set(tri.tolist()) == {-1.0, 0.0, 1.0} and tri[0] == 0 and tri[1] == -1 and tri[128] == 1
    for count in R.DECODE_COUNTS:
        c = R.decode_case(count)
        if count > 1:
            assert count > U.GRID_STRIDE_THREADS and len(np.unique(c.code)) == 256
        assert np.isnan(c.odd_lut).any() and (R.bits_of(c.odd_lut) == 0x80000000).any()


def test_unpack_masks_cases():
    big = [n * g ** 3 > U.GRID_STRIDE_THREADS for n, g in R.UNPACK_MASK_CASES]
    assert big == [False, False, True]
    for n, g in R.UNPACK_MASK_CASES:
        c = R.unpack_masks_case(n, g)
        assert c.mask.shape == (2, n, U.mask_words(g)) and not np.array_equal(c.mask[0], c.mask[1])


@pytest.mark.parametrize("cid", sorted(R.FUSED_CASES))
def test_fused_update_equals_operator_chain_on_the_oracle(cid):
    """The oracle's update against the chain of its own operators and against the numpy references with the plain-Python line walk."""
    case = R.fused_case(cid)
    n, g, sc, f = case.n, case.g, case.scene, case.frames[0]
    ref = U.run_oracle(case)[0]
    dp, sp = orc.post_process_depth(f.depth, f.seg)
    world, fg = orc.back_projection(dp, sp, f.c2w, case.kinv)
    idx = orc.points_to_idx(world, fg, sc.range_gt, sc.voxel_size, g)
    src = orc.pose_to_idx(f.poses, sc.range_gt, sc.voxel_size)
    hit, path, targets = R.chain_masks(idx, src, g, orc.bresenham3d)
    _same(hit, ref.hit)
    _same(path, ref.path)
    d2, s2 = R.post_process_depth(f.depth, f.seg, -50.0)
    _same(d2, dp)
    idx2 = R.points_to_idx(world, fg, sc.range_gt, sc.voxel_size, g)
    src2 = R.pose_to_idx(f.poses, sc.range_gt, sc.voxel_size)
    hit2, path2, _ = R.chain_masks(idx2, src2, g, lambda s, t, gg: R.bresenham3d(s, t, gg, 0))
    _same(hit2, ref.hit)
    _same(path2, ref.path)
    nh, npth = ref.hit.sum(1), ref.path.sum(1)
    outside = ((src < 0) | (src >= g)).any(1)
    dropped = fg.sum(1) - (idx[..., 0] >= 0).sum(1)
    print(f"fused {cid}: hit {nh.tolist()} path {npth.tolist()} camera outside {outside.tolist()} foreground points dropped {dropped.tolist()}")
    assert nh.sum() > 0 and (npth > nh).any() and (npth[nh == 0] == 0).all()
    assert outside.any() and not outside.all() and (nh[outside] > 0).any() and (dropped > 0).any()
    if n == 3:
        assert nh[0] == 0 and not fg[0].any()
