"""GPU: the function-granular voxel operators and bit packers of csrc/voxel.hip at their C ABI -- gnbv_post_process_depth,
gnbv_back_projection, gnbv_points_to_idx, gnbv_pose_to_idx, gnbv_bresenham3d, gnbv_grid_bit_words, gnbv_pack_grid_bits,
gnbv_unpack_grid_bits, gnbv_prob_code_tables, gnbv_decode_prob_grid and gnbv_unpack_masks -- through ctypes, outputs in sentinel-filled
arenas, byte for byte against the numpy references of tests/voxel_ops_ref.py AND the CPU oracle; gnbv_back_projection (an fmaf chain)
against the oracle's bits and an fp64 evaluation within 8 roundings.  Then the fused update against the chain of these operators, the
refusals of every entry point, and the drop-in wrappers of gennbv_amd/utils.py.

The inputs, and the conditions that keep a case from being vacuous, are those of tests/test_voxel_ops_cpu.py (same builders)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import voxel_abi_util as U
from tests import voxel_ops_ref as R
from tests.voxel_abi_util import DEV, INVALID, f32

pytestmark = pytest.mark.gpu


def sentinel(dtype):
    return np.frombuffer(bytes([U.FILL]) * np.dtype(dtype).itemsize, dtype)[0]


FILL32 = sentinel(np.int32)


def out_rows(rows, cols, dtype):
    """An output buffer whose elements hold the sentinel too: whatever a kernel does not write stays recognisable."""
    return U.Rows(rows, cols, dtype, init=np.full((rows, cols), sentinel(dtype), dtype))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(name, got, want):
    U._same(name, got, want, name)


def unchanged(t, a):
    assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "the call wrote to an input"


def ok(err, what):
    torch.cuda.synchronize()
    assert err == 0, (what, err)


# ---------------------------------------------------------------------------
# 1. gnbv_post_process_depth
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sense", R.DEPTH_SENSE)
@pytest.mark.parametrize("count", R.DEPTH_COUNTS)
def test_post_process_depth_bit_exact(count, sense):
    """depth = |max(nan_to_num(x), sense)| and seg = nan_to_num(x) with every other bit pattern kept: NaN, +-inf, +-0, the clamp value
    and its two neighbours, +-FLT_MAX, denormals, at both ends and at random places; no element, one (-0.0), and more than 2048 * 256."""
    _, lib = U.libs()
    c = R.depth_case(count, sense)
    m = max(count, 1)
    d, s = dev(c.depth), dev(c.seg)
    dout, sout = out_rows(1, m, f32), out_rows(1, m, f32)
    ok(lib.gnbv_post_process_depth(d.data_ptr(), s.data_ptr(), count, C.c_float(sense), dout.ptr, sout.ptr, None), "post_process_depth")
    want_d, want_s = np.full(m, sentinel(f32), f32), np.full(m, sentinel(f32), f32)
    want_d[:count], want_s[:count] = (a[:count] for a in R.post_process_depth(c.depth, c.seg, sense))
    same("depth", dout.read().reshape(-1), want_d)
    same("seg", sout.read().reshape(-1), want_s)
    od, os_ = orc.post_process_depth(c.depth, c.seg, sense)
    same("depth vs oracle", dout.read().reshape(-1)[:count], od[:count])
    same("seg vs oracle", sout.read().reshape(-1)[:count], os_[:count])
    assert dout.padding_intact() and sout.padding_intact()
    unchanged(d, c.depth)
    unchanged(s, c.seg)


# ---------------------------------------------------------------------------
# 2. gnbv_back_projection
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pinhole", [True, False], ids=["pinhole", "generic"])
@pytest.mark.parametrize("n,h,w", R.BACKPROJ_SHAPES)
def test_back_projection_vs_oracle_bits_and_fp64(n, h, w, pinhole):
    """World points: the oracle's bits, and within 8 * 2^-24 * (|M| |Kinv| |p| + |t|) of the fp64 product (at most 8 roundings per
    result: d*u, three in the Kinv row, four in the c2w row).  fg bytes are 0 / 1 with the threshold strict at 50; a background pixel
    (seg 0, exactly 50 or NaN; its depth NaN or inf) lands on the translation column exactly; the fourth row of c2w is NaN and
    unread.  7x240x320 has more than 2048 * 256 pixels.
    Worst err/bound of the kernel, printed per case; measured (pinhole / generic): 1x1x1 0.08 / 0.00, 3x7x9 0.16 / 0.14,
    2x48x64 0.20 / 0.19, 7x240x320 0.26 / 0.29 -- the oracle's figures, as the bits are the oracle's."""
    _, lib = U.libs()
    c = R.backproj_case(n, h, w, pinhole)
    hw = h * w
    d, s, m = dev(c.depth), dev(c.seg), dev(c.c2w)
    kinv = (C.c_float * 9)(*c.kinv.reshape(-1).tolist())
    world, fg = out_rows(n, hw * 3, f32), out_rows(n, hw, np.uint8)
    ok(lib.gnbv_back_projection(d.data_ptr(), s.data_ptr(), m.data_ptr(), kinv, n, h, w, world.ptr, fg.ptr, None), "back_projection")
    got, got_fg = world.read().reshape(n, hw, 3), fg.read()
    o_world, o_fg = orc.back_projection(c.depth, c.seg, c.c2w, c.kinv)
    same("fg", got_fg, c.is_fg.astype(np.uint8))
    same("fg vs oracle", got_fg, o_fg.astype(np.uint8))
    same("world vs oracle", got, o_world)
    want, bound, _ = R.back_projection_f64(c.depth, c.seg, c.c2w, c.kinv)
    assert np.isfinite(got).all()
    worst = R.err_over_bound(got, want, bound)
    print(f"back_projection {n}x{h}x{w} {'pinhole' if pinhole else 'generic'}: kernel worst err/bound {worst:.3f}")
    assert worst <= 1.0
    t = np.broadcast_to(c.c2w[:, None, :3, 3], got.shape)
    same("background points", got[~c.is_fg], np.ascontiguousarray(t[~c.is_fg]))
    assert world.padding_intact() and fg.padding_intact()
    unchanged(d, c.depth)
    unchanged(s, c.seg)
    unchanged(m, c.c2w)


# ---------------------------------------------------------------------------
# 3. gnbv_points_to_idx
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,g", R.POINTS_CASES)
def test_points_to_idx_bit_exact(n, hw, g):
    """floor((p - vmin) / v) clamped, under strict bounds: points on vmin and vmax dropped, one ulp inside kept at 0 / g - 1, points on
    interior faces, NaN / +-inf / +-1e30 dropped, fg bytes 0 / 1 / 2 / 255, anisotropic frames off the origin; dropped points are -1."""
    _, lib = U.libs()
    c = R.points_case(n, hw, g)
    wd, fg, rg, vs = dev(c.world), dev(c.fg), dev(c.range_gt), dev(c.voxel_size)
    idx = out_rows(n, hw * 3, np.int32)
    ok(lib.gnbv_points_to_idx(wd.data_ptr(), fg.data_ptr(), rg.data_ptr(), vs.data_ptr(), n, hw, g, idx.ptr, None), "points_to_idx")
    got = idx.read().reshape(n, hw, 3)
    same("idx", got, R.points_to_idx(c.world, c.fg, c.range_gt, c.voxel_size, g))
    same("idx vs oracle", got, orc.points_to_idx(c.world, c.fg, c.range_gt, c.voxel_size, g))
    assert idx.padding_intact()
    for t, a in ((wd, c.world), (fg, c.fg), (rg, c.range_gt), (vs, c.voxel_size)):
        unchanged(t, a)


# ---------------------------------------------------------------------------
# 4. gnbv_pose_to_idx
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.POSE_NS)
def test_pose_to_idx_floors_and_does_not_clamp(n):
    """int64 floor((p - vmin) / v): poses inside, on faces, outside on both sides up to 1e6 voxels, and 0.3 voxels below vmin (-1, where
    truncation gives 0); 300 envs are more than one block."""
    _, lib = U.libs()
    c = R.pose_case(n)
    p, rg, vs = dev(c.poses), dev(c.range_gt), dev(c.voxel_size)
    out = out_rows(n, 3, np.int64)
    ok(lib.gnbv_pose_to_idx(p.data_ptr(), rg.data_ptr(), vs.data_ptr(), n, out.ptr, None), "pose_to_idx")
    same("pose idx", out.read(), R.pose_to_idx(c.poses, c.range_gt, c.voxel_size))
    same("pose idx vs oracle", out.read(), orc.pose_to_idx(c.poses, c.range_gt, c.voxel_size))
    assert out.padding_intact()
    for t, a in ((p, c.poses), (rg, c.range_gt), (vs, c.voxel_size)):
        unchanged(t, a)


# ---------------------------------------------------------------------------
# 5. gnbv_bresenham3d
# ---------------------------------------------------------------------------
def _bresenham(lib, src, tgt, g, traj, lens):
    s, t = dev(np.asarray(src, np.int32)), dev(np.asarray(tgt, np.int32).reshape(-1, 3))
    err = lib.gnbv_bresenham3d(s.data_ptr(), t.data_ptr(), t.shape[0], g, traj, lens, None)
    torch.cuda.synchronize()
    unchanged(s, np.asarray(src, np.int32))
    unchanged(t, np.asarray(tgt, np.int32))
    return err


@pytest.mark.parametrize("rays,g", R.BRESENHAM_CASES)
def test_bresenham3d_exact_lengths_points_and_fill(rays, g):
    """Per source (inside, two corners, outside on either side, 10 g away): lens exact, the first lens[r] points exact, the sentinel
    behind them -- against the oracle on every ray and the plain-Python walk on the first 300 (targets equal to the source, outside,
    axis-aligned, full and two-way ties come first).  Ray counts around one block of 256, grids of one voxel to 128."""
    _, lib = U.libs()
    c = R.bresenham_case(rays, g)
    if rays == 0:
        assert lib.gnbv_bresenham3d(None, None, 0, g, None, None, None) == 0
    for src, tgt in c.runs:
        traj, lens = out_rows(max(rays, 1), 9 * g, np.int32), out_rows(1, max(rays, 1), np.int32)
        before = (traj.snapshot(), lens.snapshot())
        assert _bresenham(lib, src, tgt, g, traj.ptr, lens.ptr) == 0
        if rays == 0:
            assert (traj.snapshot(), lens.snapshot()) == before
            continue
        got_t, got_l = traj.read().reshape(rays, 3 * g, 3), lens.read().reshape(-1)
        o_t, o_l = orc.bresenham3d(src, tgt, g)
        valid = np.arange(3 * g)[None, :, None] < o_l[:, None, None]
        same("lens vs oracle", got_l, o_l)
        same("points vs oracle", got_t, np.where(valid, o_t, FILL32))
        k = min(rays, R.BRESENHAM_PY_RAYS)
        p_t, p_l = R.bresenham3d(src, tgt[:k], g, FILL32)
        same("lens", got_l[:k], p_l)
        same("points", got_t[:k], p_t)
        R.check_ray_properties(src, tgt, got_t, got_l, g, FILL32)
        assert traj.padding_intact() and lens.padding_intact()


# ---------------------------------------------------------------------------
# 6. gnbv_grid_bit_words, gnbv_pack_grid_bits, gnbv_unpack_grid_bits
# ---------------------------------------------------------------------------
def test_grid_bit_words():
    _, lib = U.libs()
    for g in range(1, 131):
        assert lib.gnbv_grid_bit_words(g) == U.mask_words(g), g
    assert [lib.gnbv_grid_bit_words(g) for g in (0, -1, -65)] == [0, 0, 0]


def _pack(lib, grid, n, g, flag=True):
    """(bits [n, words], *not_binary or None) of one call on a bits buffer prefilled with 0xFF; the row padding must stay."""
    src = dev(grid)
    bits = U.Rows(n, U.mask_words(g), np.uint32, init=np.full((n, U.mask_words(g)), 0xFFFFFFFF, np.uint32))
    nb = U.Rows(1, 1, np.int32, init=np.full((1, 1), 7, np.int32)) if flag else None
    ok(lib.gnbv_pack_grid_bits(src.data_ptr(), n, g, bits.ptr, nb.ptr if flag else None, None), "pack_grid_bits")
    assert bits.padding_intact() and (nb is None or nb.padding_intact())
    unchanged(src, grid)
    return bits.read(), (int(nb.read()[0, 0]) if flag else None)


@pytest.mark.parametrize("n", R.PACK_NS)
@pytest.mark.parametrize("g", R.PACK_GS)
def test_pack_grid_bits(n, g):
    """bit = (x != 0): a denormal, NaN, inf, 0.5 and -1 set it, -0.0 does not.  Every word of a row is written: the bits past g^3 of
    the last data word and the pad words are zero.  *not_binary is 0 for {0, 1, -0.0} and 1 for one other value at the very last voxel
    of the last env; it may be NULL.  g = 65 is the first grid past 1024 blocks of 256 lanes per env."""
    _, lib = U.libs()
    c = R.pack_case(n, g)
    for grid in (c.binary, c.mixed):
        bits, nb = _pack(lib, grid, n, g)
        same("bits", bits, R.pack_bits(grid, g))
        same("bits vs pack_bits", bits, U.pack_bits(grid, g))
        assert nb == R.not_binary(grid) == (grid is c.mixed)
    bits, _ = _pack(lib, c.mixed, n, g, flag=False)
    same("bits, not_binary NULL", bits, R.pack_bits(c.mixed, g))
    for v in R.OTHER_VALUES:
        x = c.binary.copy()
        x[-1, -1] = v
        bits, nb = _pack(lib, x, n, g)
        same("bits", bits, R.pack_bits(x, g))
        assert nb == 1, float(v)


@pytest.mark.parametrize("n", R.PACK_NS)
@pytest.mark.parametrize("g", R.PACK_GS)
def test_unpack_grid_bits_and_round_trip(n, g):
    """Random words with garbage in the pad bits and pad words: exactly n g^3 floats, each 0.0 or 1.0; unpack(pack(x)) == (x != 0)."""
    _, lib = U.libs()
    c = R.pack_case(n, g)
    g3 = g ** 3
    packed, _ = _pack(lib, c.mixed, n, g)
    with np.errstate(invalid="ignore"):
        cases = ((c.words, R.unpack_bits(c.words, g)), (packed, (c.mixed != 0).astype(f32)))
    for words, want in cases:
        src = dev(words.view(np.int32))
        out = out_rows(n, g3, f32)
        ok(lib.gnbv_unpack_grid_bits(src.data_ptr(), n, g, out.ptr, None), "unpack_grid_bits")
        same("grid", out.read(), want)
        assert out.padding_intact()
        unchanged(src, words)


# ---------------------------------------------------------------------------
# 7. gnbv_prob_code_tables, gnbv_decode_prob_grid
# ---------------------------------------------------------------------------
def test_prob_code_tables_vs_numpy_iteration():
    _, lib = U.libs()
    prob, tri = R.prob_code_tables()
    pl, tl = (C.c_float * 256)(), (C.c_float * 256)()
    lib.gnbv_prob_code_tables(pl, tl)
    same("prob_lut", np.asarray(pl[:], f32), prob)
    same("tri_lut", np.asarray(tl[:], f32), tri)
    p2, t2 = (C.c_float * 256)(), (C.c_float * 256)()
    lib.gnbv_prob_code_tables(p2, None)
    lib.gnbv_prob_code_tables(None, t2)
    lib.gnbv_prob_code_tables(None, None)
    same("prob_lut alone", np.asarray(p2[:], f32), prob)
    same("tri_lut alone", np.asarray(t2[:], f32), tri)


@pytest.mark.parametrize("count", R.DECODE_COUNTS)
def test_decode_prob_grid(count):
    """out = lut[code] as bytes, for the real table and for a table of arbitrary bit patterns (NaN payloads, -0.0, -inf)."""
    _, lib = U.libs()
    c = R.decode_case(count)
    m = max(count, 1)
    code = dev(c.code)
    for lut in (R.prob_code_tables()[0], c.odd_lut):
        table = dev(lut)
        out = out_rows(1, m, f32)
        ok(lib.gnbv_decode_prob_grid(code.data_ptr(), count, table.data_ptr(), out.ptr, None), "decode_prob_grid")
        want = np.full(m, sentinel(f32), f32)
        want[:count] = lut[c.code[:count]]
        same("decoded", out.read().reshape(-1).view(np.uint32), want.view(np.uint32))
        assert out.padding_intact()
        unchanged(table, lut)
    unchanged(code, c.code)


# ---------------------------------------------------------------------------
# 8. gnbv_unpack_masks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,g", R.UNPACK_MASK_CASES)
def test_unpack_masks(n, g):
    """A workspace of gnbv_voxel_workspace_bytes(n, g) random bytes: the hit rows first, the path rows from word n * words; with one
    output NULL the other is still right and nothing else is written.  2 * 65^3 > 2048 * 256."""
    _, lib = U.libs()
    c = R.unpack_masks_case(n, g)
    ws_bytes = int(lib.gnbv_voxel_workspace_bytes(n, g))
    assert ws_bytes == c.mask.nbytes
    ws = U.Rows(1, ws_bytes, np.uint8, init=c.mask.view(np.uint8).reshape(1, -1))
    want = [R.unpack_bits(c.mask[k], g, np.uint8) for k in (0, 1)]
    for use_hit, use_path in ((True, True), (True, False), (False, True)):
        hit, path = out_rows(n, g ** 3, np.uint8), out_rows(n, g ** 3, np.uint8)
        before = (hit.snapshot(), path.snapshot(), ws.snapshot())
        ok(lib.gnbv_unpack_masks(ws.ptr, n, g, hit.ptr if use_hit else None, path.ptr if use_path else None, None), "unpack_masks")
        if use_hit:
            same("hit", hit.read(), want[0])
        else:
            assert hit.snapshot() == before[0]
        if use_path:
            same("path", path.read(), want[1])
        else:
            assert path.snapshot() == before[1]
        assert ws.snapshot() == before[2] and hit.padding_intact() and path.padding_intact()


# ---------------------------------------------------------------------------
# 9. the fused update equals the operator chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(R.FUSED_CASES))
def test_fused_update_equals_operator_chain(cid):
    """gnbv_update_occ_grid's hit and path masks against post_process_depth -> back_projection -> points_to_idx (the kept voxels are
    the hit set) and pose_to_idx -> one gnbv_bresenham3d per env from that source to the hit voxels (the union of the lines is the path
    set), all on the GPU.  An env without foreground, cameras inside and outside the grid, points that leave it."""
    L, lib = U.libs()
    case = R.fused_case(cid)
    n, g, h, w, sc, f = case.n, case.g, case.h, case.w, case.scene, case.frames[0]
    ref = U.run_oracle(case)
    U.assert_masks_not_vacuous(ref)
    call = U.VoxelCall("f32", case)
    assert call.step(0) == 0
    fused = call.outputs()
    U.compare(call, fused, ref[0], cid)

    hw = h * w
    d, s, m, p, rg, vs = (dev(a) for a in (f.depth, f.seg, f.c2w, f.poses, sc.range_gt, sc.voxel_size))
    dp, sp = torch.empty_like(d), torch.empty_like(s)
    world = torch.empty((n, hw, 3), dtype=torch.float32, device=DEV)
    fg = torch.empty((n, hw), dtype=torch.uint8, device=DEV)
    idx = torch.empty((n, hw, 3), dtype=torch.int32, device=DEV)
    src = torch.empty((n, 3), dtype=torch.int64, device=DEV)
    kinv = (C.c_float * 9)(*case.kinv.reshape(-1).tolist())
    ok(lib.gnbv_post_process_depth(d.data_ptr(), s.data_ptr(), n * hw, C.c_float(-50.0), dp.data_ptr(), sp.data_ptr(), None), "depth")
    ok(lib.gnbv_back_projection(dp.data_ptr(), sp.data_ptr(), m.data_ptr(), kinv, n, h, w, world.data_ptr(), fg.data_ptr(), None), "world")
    ok(lib.gnbv_points_to_idx(world.data_ptr(), fg.data_ptr(), rg.data_ptr(), vs.data_ptr(), n, hw, g, idx.data_ptr(), None), "idx")
    ok(lib.gnbv_pose_to_idx(p.data_ptr(), rg.data_ptr(), vs.data_ptr(), n, src.data_ptr(), None), "pose")

    def walk(source, targets, gg):
        traj = torch.zeros((targets.shape[0], 3 * gg, 3), dtype=torch.int32, device=DEV)
        lens = torch.zeros(targets.shape[0], dtype=torch.int32, device=DEV)
        assert _bresenham(lib, source, targets, gg, traj.data_ptr(), lens.data_ptr()) == 0
        return traj.cpu().numpy(), lens.cpu().numpy()

    hit, path, targets = R.chain_masks(idx.cpu().numpy(), src.cpu().numpy(), g, walk)
    same("hit: fused vs chain", fused.hit, hit)
    same("path: fused vs chain", fused.path, path)
    nh, npth = hit.sum(1), path.sum(1)
    assert (npth > nh).any() and (npth[nh == 0] == 0).all() and [len(t) for t in targets] == nh.tolist()


# ---------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------
def _refusal_specs(lib, zeros, outs):
    """name -> (function, a valid argument list over zero inputs, positions of the required pointers, (position, bad value) pairs)."""
    z, sense = zeros.data_ptr(), C.c_float(-50.0)
    kinv = (C.c_float * 9)(*([1.0] * 9))
    o = {k: r.ptr for k, r in outs.items()}
    return {
        "post_process_depth": (lib.gnbv_post_process_depth, [z, z, 8, sense, o["a"], o["b"], None], (0, 1, 4, 5), ((2, -1),)),
        "back_projection": (lib.gnbv_back_projection, [z, z, z, kinv, 2, 2, 2, o["a"], o["b"], None], (0, 1, 2, 3, 7, 8),
                            ((4, 0), (4, -1), (5, 0), (5, -2), (6, 0), (6, -2))),
        "points_to_idx": (lib.gnbv_points_to_idx, [z, z, z, z, 2, 4, 4, o["a"], None], (0, 1, 2, 3, 7),
                          ((4, 0), (4, -1), (5, 0), (5, -4), (6, 0), (6, -4))),
        "pose_to_idx": (lib.gnbv_pose_to_idx, [z, z, z, 2, o["a"], None], (0, 1, 2, 4), ((3, 0), (3, -2))),
        "bresenham3d": (lib.gnbv_bresenham3d, [z, z, 4, 4, o["a"], o["b"], None], (0, 1, 4, 5), ((2, -1), (3, 0), (3, -4))),
        "pack_grid_bits": (lib.gnbv_pack_grid_bits, [z, 2, 4, o["a"], o["b"], None], (0, 3), ((1, 0), (1, -2), (2, 0), (2, -4))),
        "unpack_grid_bits": (lib.gnbv_unpack_grid_bits, [z, 2, 4, o["a"], None], (0, 3), ((1, 0), (1, -2), (2, 0), (2, -4))),
        "decode_prob_grid": (lib.gnbv_decode_prob_grid, [z, 8, z, o["a"], None], (0, 2, 3), ((1, -1),)),
        "unpack_masks": (lib.gnbv_unpack_masks, [z, 2, 4, o["a"], o["b"], None], (0,), ((1, 0), (1, -2), (2, 0), (2, -4))),
    }


REFUSING = ("post_process_depth", "back_projection", "points_to_idx", "pose_to_idx", "bresenham3d", "pack_grid_bits", "unpack_grid_bits",
            "decode_prob_grid", "unpack_masks")


@pytest.mark.parametrize("name", REFUSING)
def test_refusals(name):
    """Every required pointer NULL, n <= 0, g <= 0, map_size <= 0, h / w / hw <= 0, count < 0, num_rays < 0: the invalid-argument code,
    and no byte of the outputs written.  The unmodified arguments are then accepted."""
    _, lib = U.libs()
    zeros = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)          # every input of every valid call fits
    outs = {k: out_rows(1, 4096, np.uint8) for k in ("a", "b")}          # and every output
    fn, args, pointers, bad = _refusal_specs(lib, zeros, outs)[name]
    before = [r.snapshot() for r in outs.values()]
    for pos in pointers:
        a = list(args)
        a[pos] = None
        assert fn(*a) == INVALID, (name, "NULL at", pos)
    for pos, value in bad:
        a = list(args)
        a[pos] = value
        assert fn(*a) == INVALID, (name, pos, value)
    torch.cuda.synchronize()
    assert [r.snapshot() for r in outs.values()] == before, "a refused call wrote to its outputs"
    assert not zeros.any()
    ok(fn(*args), name)
    assert all(r.padding_intact() for r in outs.values())


# ---------------------------------------------------------------------------
# 11. the wrappers of gennbv_amd/utils.py
# ---------------------------------------------------------------------------
def strided64(a):
    """The values of `a` as a float64 device tensor that is not contiguous (every other element of the last axis)."""
    a = np.asarray(a)
    t = torch.from_numpy(np.repeat(a.astype(np.float64), 2, axis=-1)).to(DEV)[..., ::2]
    assert not t.is_contiguous() or t.numel() <= 1
    return t


def test_wrapper_points_to_idx_and_scanned_pts():
    """float64, non-contiguous world / range / voxel tensors and a bool fg; scanned_pts_to_idx_3D: unique rows in lexicographic order,
    [] for an env without points and for one whose points are all dropped."""
    from gennbv_amd import utils as G
    n, hw, g = 3, 37, 16
    c = R.points_case(n, hw, g)
    rg, vs = strided64(c.range_gt), strided64(c.voxel_size)
    want = R.points_to_idx(c.world, c.fg, c.range_gt, c.voxel_size, g)
    got = G.points_to_idx(strided64(c.world), dev(c.fg != 0), rg, vs, g)
    assert got.dtype == torch.int32
    same("points_to_idx", got.cpu().numpy(), want)
    away = (c.world[2] + f32(1e6)).astype(f32)
    pts = [strided64(c.world[0]), torch.empty((0, 3), dtype=torch.float32, device=DEV), strided64(away)]
    out = G.scanned_pts_to_idx_3D(pts, rg, vs, g)
    ones = np.ones((1, hw), np.uint8)
    rows = R.points_to_idx(c.world[:1], ones, c.range_gt[:1], c.voxel_size[:1], g)[0]
    rows = np.unique(rows[rows[:, 0] >= 0].astype(np.int64), axis=0)
    assert len(rows) > 5 and isinstance(out, list) and len(out) == 3
    assert out[0].dtype == torch.int64
    same("scanned_pts_to_idx_3D", out[0].cpu().numpy(), rows)
    assert not (R.points_to_idx(away[None], ones, c.range_gt[2:], c.voxel_size[2:], g) >= 0).any()
    assert out[1] == [] and out[2] == []


def test_wrapper_pose_coord_to_idx():
    from gennbv_amd import utils as G
    c = R.pose_case(300)
    want = R.pose_to_idx(c.poses, c.range_gt, c.voxel_size)
    args = (strided64(c.poses), strided64(c.range_gt), strided64(c.voxel_size))
    got = G.pose_coord_to_idx_3D(*args, map_size=16)
    assert got.dtype == torch.int64
    same("pose idx", got.cpu().numpy(), want)
    below, above = (want < 0).any(1), (want > 15).any(1)
    assert (below & ~above).any() and (above & ~below).any() and (~below & ~above).any()
    col = want.copy()
    col[below | above] = -1
    same("pose idx, if_col", G.pose_coord_to_idx_3D(*args, map_size=16, if_col=True).cpu().numpy(), col)


def test_wrapper_bresenham3d():
    """A float source truncates like .int() (-0.7 -> 0, 3.9 -> 3), int64 targets, map_size as a list; the result is the concatenation
    of every ray's in-grid voxels in ray order, int64."""
    from gennbv_amd import utils as G
    g = 7
    tgt = R.bresenham_targets((0, 3, 2), 60, g, 5)
    source = torch.tensor([[-0.7, 3.9, 2.0]], dtype=torch.float32, device=DEV)
    want = np.asarray([p for t in tgt for p in R.bresenham_ray((0, 3, 2), t, g)], np.int64)
    for map_size in ([g, g, g], g):
        got = G.bresenham3D_hip(source, dev(tgt.astype(np.int64)), map_size)
        assert got.dtype == torch.int64
        same("bresenham3D_hip", got.cpu().numpy(), want)
    assert G.bresenham3D_pycuda is G.bresenham3D_hip
    traj, lens = G.bresenham3D_raw(source, dev(tgt.astype(np.int64)), g)
    o_t, o_l = orc.bresenham3d(np.asarray([0, 3, 2], np.int32), tgt, g)
    same("raw lens", lens.cpu().numpy(), o_l)
    same("raw points", traj.cpu().numpy(), o_t)


def test_wrapper_back_projection_fg_and_tri_cls():
    from gennbv_amd import utils as G
    n, h, w = 3, 7, 9
    c = R.backproj_case(n, h, w, False)
    o_world, o_fg = orc.back_projection(c.depth, c.seg, c.c2w, c.kinv)
    pts, world, fg = G.back_projection_fg(strided64(c.depth), strided64(c.seg), strided64(c.c2w), torch.from_numpy(c.kinv).double(),
                                          return_all=True)
    same("world", world.cpu().numpy(), o_world)
    assert fg.dtype == torch.bool
    same("fg", fg.cpu().numpy(), c.is_fg)
    only = G.back_projection_fg(dev(c.depth), dev(c.seg), dev(c.c2w), torch.from_numpy(c.kinv))
    for e in range(n):
        assert len(pts[e]) == len(only[e]) == int(c.is_fg[e].sum())
        same("foreground points", pts[e].cpu().numpy(), o_world[e][c.is_fg[e]])
        same("foreground points", only[e].cpu().numpy(), o_world[e][c.is_fg[e]])
    prob = R.prob_code_tables()[0].reshape(4, 64)
    occ, tri = G.grid_occupancy_tri_cls(strided64(prob), 0.5, 0.0)
    tri_only = G.grid_occupancy_tri_cls(dev(prob), 0.5, 0.0, return_tri_cls_only=True)
    want = (prob > f32(0.5)).astype(f32) - (prob < f32(0.0)).astype(f32)
    assert set(np.unique(want).tolist()) == {-1.0, 0.0, 1.0}
    same("occupancy", occ.cpu().numpy(), (prob > f32(0.5)).astype(f32))
    same("tri", tri.cpu().numpy(), want)
    same("tri only", tri_only.cpu().numpy(), want)
