"""GPU: gnbv_depth_sensor against the numpy oracle, bit for bit, on every case of tests/depth_sensor_cases.py in two buffer
layouts; the identity sensor against the renderer and the env; the NO_RETURN encoding against the voxel update, CarvedMap and
the scan set as they stand; the closed loop with noise on; and the stream-order case of the new entry point.

The stream-order table lives in tests/test_stream_order_gpu.py (`G`), whose parametrisation is fixed when G is imported: this
module registers its case through G's own decorator -- so the census of tests/test_stream_order_cpu.py sees it whenever pytest
collects this file -- and runs the two protocol checks for it itself.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_sensor_cases as DC
from tests import depth_sensor_oracle as DO
from tests import stream_order_util as U
from tests import test_stream_order_gpu as G

pytestmark = pytest.mark.gpu
DEV = U.DEV
FILL = 0xA5
oracle, cpu_base_args = DC.oracle, DC.base_args


# ------------------------------------------------------------------------------------------------------------------- harness
def _lut():
    from gennbv_amd.ops.depth_sensor import gauss_table
    if "lut" not in _CACHE:
        _CACHE["lut"] = gauss_table().to(DEV)
    return _CACHE["lut"]


_CACHE = {}


def _struct(n, h, w, P, frame, lut, d_in, s_in, si, d_out, s_out, so):
    from gennbv_amd import _lib
    a = _lib.GnbvDepthSensor()
    a.n, a.h, a.w = n, h, w
    a.depth_in, a.seg_in, a.in_env_stride = d_in, s_in, si
    a.depth_out, a.seg_out, a.out_env_stride = d_out, s_out, so
    a.frame, a.seed = frame.data_ptr(), P["seed"]
    a.min_range, a.max_range = P["min_range"], P["max_range"]
    a.edge_radius, a.edge_abs, a.edge_rel, a.edge_drop, a.drop = P["edge_radius"], P["edge_abs"], P["edge_rel"], P["edge_drop"], P["drop"]
    a.sigma0, a.sigma1, a.sigma2, a.quant = P["sigma0"], P["sigma1"], P["sigma2"], P["quant"]
    a.gauss_lut = None if lut is None else lut.data_ptr()
    return a


class Buffers:
    """The four frames of a call inside sentinel-filled buffers: env e's block at off + e stride, FILL bytes everywhere else."""

    def __init__(self, shape, kind, depth, seg):
        n, h, w = shape
        self.shape, self.hw = shape, h * w
        self.si, self.so, self.off = DC.layout(shape, kind)
        size_i, size_o = self.off + (n - 1) * self.si + self.hw + 16, self.off + (n - 1) * self.so + self.hw + 16
        mk = lambda size: torch.full((size * 4,), FILL, dtype=torch.uint8, device=DEV).view(torch.float32)
        self.d_in, self.s_in, self.d_out, self.s_out = mk(size_i), mk(size_i), mk(size_o), mk(size_o)
        self.blocks(self.d_in, self.si).copy_(torch.from_numpy(depth).view(n, self.hw))
        self.blocks(self.s_in, self.si).copy_(torch.from_numpy(seg).view(n, self.hw))
        self.in_before = (self.d_in.clone(), self.s_in.clone())

    def blocks(self, buf, stride):
        n = self.shape[0]
        return torch.as_strided(buf, (n, self.hw), (stride, 1), self.off)

    def ptr(self, buf):
        return buf.data_ptr() + 4 * self.off

    def run(self, P, frame, lut, n=None):
        from gennbv_amd import _lib
        _, h, w = self.shape
        a = _struct(self.shape[0] if n is None else n, h, w, P, frame, lut, self.ptr(self.d_in), self.ptr(self.s_in), self.si,
                    self.ptr(self.d_out), self.ptr(self.s_out), self.so)
        _lib.check(_lib.load().gnbv_depth_sensor(C.byref(a), _lib.stream_ptr(DEV)), "gnbv_depth_sensor")
        torch.cuda.synchronize()

    def outputs(self):
        n, h, w = self.shape
        return tuple(self.blocks(b, self.so).cpu().numpy().reshape(n, h, w) for b in (self.d_out, self.s_out))

    def sentinels_intact(self, n=None):
        n = self.shape[0] if n is None else n
        for buf in (self.d_out, self.s_out):
            keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
            torch.as_strided(keep, (n, self.hw), (self.so, 1), self.off).fill_(False)
            if not bool((buf.view(torch.uint8).view(-1, 4)[keep] == FILL).all()):
                return False
        return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((self.d_in, self.s_in), self.in_before))


def same_bits(got, want):
    """bit for bit, NaN payloads excepted"""
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn])


def _run_case(case, kind):
    shape, name = case
    f = DC.frame_of(shape)
    b = Buffers(shape, kind, f["depth"], f["seg"])
    frame = torch.from_numpy(DC.frames_of(case)).to(DEV)
    b.run(DC.PARAMS[name], frame, _lut() if DC.uses_lut(name) else None)
    assert torch.equal(frame.cpu(), torch.from_numpy(DC.frames_of(case)))  # read, never written
    return b


# --------------------------------------------------------------------------------------------------------- kernel against oracle
@pytest.mark.parametrize("kind", DC.LAYOUTS)
@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_kernel_equals_oracle_bit_for_bit(case, kind):
    want_d, want_s, _ = oracle(case)
    b = _run_case(case, kind)
    got_d, got_s = b.outputs()
    bad = np.argwhere(got_d.view(np.uint32) != want_d.view(np.uint32))
    assert same_bits(got_d, want_d), (len(bad), bad[:5].tolist(), [(float(got_d[tuple(p)]), float(want_d[tuple(p)])) for p in bad[:5]])
    assert same_bits(got_s, want_s)
    assert b.sentinels_intact()


def test_the_lut_may_be_given_with_all_sigmas_zero():
    case = ((3, 30, 40), "edge_r2_half")
    shape, name = case
    f = DC.frame_of(shape)
    b = Buffers(shape, "wide", f["depth"], f["seg"])
    b.run(DC.PARAMS[name], torch.from_numpy(DC.frames_of(case)).to(DEV), _lut())
    got_d, got_s = b.outputs()
    assert same_bits(got_d, oracle(case)[0]) and same_bits(got_s, oracle(case)[1])


@pytest.mark.parametrize("shape", [(3, 30, 40), (1025, 2, 4), (2, 7, 37)])
def test_an_env_does_not_depend_on_the_batch(shape):
    """Env e of the batch against the same env in a batch that ends with it, where every other env holds another frame (the env
    number is part of the counter, so it keeps its place); env 0 also truly alone (n = 1)."""
    case = (shape, "all")
    want_d, want_s, _ = oracle(case)
    f = DC.frame_of(shape)
    n = shape[0]
    fr = DC.frames_of(case)
    for e in (0, n - 1):
        depth, seg = np.full_like(f["depth"], -4.0), np.full_like(f["seg"], 9.0)
        depth[e], seg[e] = f["depth"][e], f["seg"][e]
        frame = np.full(n, 12345, np.int32)
        frame[e] = fr[e]
        b = Buffers(shape, "wide", depth, seg)
        b.run(DC.PARAMS["all"], torch.from_numpy(frame).to(DEV), _lut(), n=e + 1)
        got_d, got_s = b.outputs()
        assert same_bits(got_d[e], want_d[e]) and same_bits(got_s[e], want_s[e]), e
        assert b.sentinels_intact(n=e + 1)  # the blocks of the envs past n are not touched either


def test_two_calls_are_identical_and_the_frame_counter_changes_the_noise():
    case = ((3, 30, 40), "all")
    a, b = _run_case(case, "wide"), _run_case(case, "wide")
    assert torch.equal(a.d_out.view(torch.int32), b.d_out.view(torch.int32)) and torch.equal(a.s_out.view(torch.int32), b.s_out.view(torch.int32))
    shape, name = case
    f = DC.frame_of(shape)
    c = Buffers(shape, "wide", f["depth"], f["seg"])
    c.run(DC.PARAMS[name], torch.from_numpy(DC.frames_of(case) + 1).to(DEV), _lut())
    want = DO.sensor(f["depth"], f["seg"], DC.frames_of(case) + 1, DC.PARAMS[name], lut=DO.gauss_table().astype(np.float32))
    assert same_bits(c.outputs()[0], want[0])
    for e in range(shape[0]):
        assert not np.array_equal(c.outputs()[0][e], a.outputs()[0][e])


def test_the_refusal_tests_base_arguments_are_accepted():
    """tests/test_depth_sensor_cpu.py refuses variations of one struct on made-up pointers; the same values on real buffers run."""
    from gennbv_amd import _lib
    base = cpu_base_args()
    n, h, w = base.n, base.h, base.w
    bufs = [torch.zeros(n * base.in_env_stride, device=DEV) for _ in range(4)]
    frame = torch.zeros(n, dtype=torch.int32, device=DEV)
    a = cpu_base_args(depth_in=bufs[0].data_ptr(), seg_in=bufs[1].data_ptr(), depth_out=bufs[2].data_ptr(), seg_out=bufs[3].data_ptr(),
                      frame=frame.data_ptr(), gauss_lut=_lut().data_ptr())
    assert _lib.load().gnbv_depth_sensor(C.byref(a), _lib.stream_ptr(DEV)) == 0
    torch.cuda.synchronize()
    # inputs that alias each other are no overlap of an output with anything
    a.seg_in = a.depth_in
    assert _lib.load().gnbv_depth_sensor(C.byref(a), _lib.stream_ptr(DEV)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ identity and parity
FLT_MAX = float(np.finfo(np.float32).max)


def _identity(n, h, w):
    from gennbv_amd.ops.depth_sensor import DepthSensor
    s = DepthSensor(n, h, w, min_range_m=2.0 ** -90, max_range_m=FLT_MAX, device=DEV)
    assert s.is_identity
    return s


def _noisy(n, h, w):
    from gennbv_amd.ops.depth_sensor import DepthSensor
    s = DepthSensor(n, h, w, seed=3, min_range_m=0.3, max_range_m=30.0, edge_radius=1, edge_abs_m=0.05, edge_rel=0.02, edge_drop=0.7,
                    drop=0.02, sigma=(0.002, 0.0, 0.003), quant=600.0, device=DEV)
    assert not s.is_identity
    return s


def _rendered(n, g, h, w, sensor=None):
    from gennbv_amd.env.render_feed import RenderFeed
    cfg = G._cfg(h, w, g)
    scene, mesh = G._mesh(n, g)
    feed = RenderFeed(mesh, cfg, with_rgba=False, sensor=sensor)
    poses = G._look_poses(1, n, 1, cfg)[:, 0].contiguous()
    feed.render(poses)
    torch.cuda.synchronize()
    return cfg, scene, feed, poses


def test_identity_sensor_reproduces_a_rendered_frame():
    n, g, h, w = 3, 16, 30, 40
    _, _, plain, _ = _rendered(n, g, h, w)
    sensor = _identity(n, h, w)
    _, _, feed, _ = _rendered(n, g, h, w, sensor)
    d = plain.depth_raw
    assert bool(torch.isneginf(d).any()) and bool(torch.isfinite(d).any()) and bool((plain.seg_raw != 0).any())
    assert torch.equal(feed.ideal_depth_raw.view(torch.int32), d.view(torch.int32))
    assert torch.equal(feed.depth_raw.view(torch.int32), d.view(torch.int32))
    assert torch.equal(feed.seg_raw.view(torch.int32), plain.seg_raw.view(torch.int32))
    assert feed.last[0] is feed.depth_raw and feed.last[1] is feed.seg_raw and plain.ideal_depth_raw is None
    assert sensor.frame.tolist() == [1] * n and sensor.frame.dtype == torch.int32
    own_d, own_s = sensor(d, plain.seg_raw)  # buffers of the operator's own
    assert own_d.dtype == torch.float32 and torch.equal(own_d.view(torch.int32), d.view(torch.int32)) and torch.equal(own_s, plain.seg_raw)
    assert sensor.frame.tolist() == [2] * n


def test_render_feed_refuses_a_sensor_of_another_shape():
    from gennbv_amd import _lib
    from gennbv_amd.env.render_feed import RenderFeed
    cfg = G._cfg(30, 40, 16)
    _, mesh = G._mesh(3, 16)
    for shape in ((2, 30, 40), (3, 30, 37), (3, 31, 40)):
        with pytest.raises(_lib.GennbvHipError, match="sensor"):
            RenderFeed(mesh, cfg, sensor=_identity(*shape))


def _env(n, g, h, w, sensor, max_len=4, seed=3):
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    cfg = G._cfg(h, w, g)
    scene = S.make_scenes(n, g, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg, sensor=sensor), DEV, max_episode_length=max_len), cfg


def _fly(envs, cfg, n, steps=5):
    """the same random actions to every env of `envs`; yields the per-env (obs, rew, done) of each step, reset first"""
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    pol = RandomLatticePolicy(cfg, n, seed=11)
    obs = [e.reset() for e in envs]
    yield [(o, None, None) for o in obs]
    for _ in range(steps):
        act = pol(obs[0])[0]
        out = [e.step(act) for e in envs]
        obs = [o[0] for o in out]
        yield [(o[0], o[1], o[2]) for o in out]


def test_env_over_the_identity_sensor_is_byte_identical():
    n, g, h, w = 4, 16, 30, 40
    env, cfg = _env(n, g, h, w, _identity(n, h, w))
    ref, _ = _env(n, g, h, w, None)
    resets = 0
    for step, ((o, r, d), (o0, r0, d0)) in enumerate(_fly([env, ref], cfg, n)):
        assert torch.equal(o.view(torch.int32), o0.view(torch.int32)), step
        if r is not None:
            assert torch.equal(r.view(torch.int32), r0.view(torch.int32)) and torch.equal(d, d0), step
            resets += int(d.sum())
    assert resets > 0  # (max_episode_length 4: the five steps cross an episode's end)
    frames = env.feed.sensor.frame.tolist()
    assert len(set(frames)) == 1 and frames[0] >= 6  # one per rendered frame: the reset's and the five steps'


def test_closed_loop_with_noise_on():
    n, g, h, w = 4, 16, 30, 40
    env, cfg = _env(n, g, h, w, _noisy(n, h, w))
    ref, _ = _env(n, g, h, w, None)
    differs = 0
    for step, ((o, r, d), (o0, r0, d0)) in enumerate(_fly([env, ref], cfg, n)):
        assert bool(torch.isfinite(o).all())
        differs += int(not torch.equal(o, o0))
        # the same actions give the same poses: the feed's ideal frame is the frame of the env without a sensor
        assert torch.equal(env.feed.ideal_depth_raw.view(torch.int32), ref.feed.depth_raw.view(torch.int32)), step
        assert torch.equal(env.feed.ideal_seg_raw, ref.feed.seg_raw)
        assert not torch.equal(env.feed.depth_raw, ref.feed.depth_raw)
        assert not bool(torch.isnan(env.feed.depth_raw).any())
    assert differs > 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- NO_RETURN against the kernels as they stand
def _no_return_frames(n, h, w):
    from gennbv_amd.ops.depth_sensor import NO_RETURN
    nr = torch.full((n, h, w), NO_RETURN, device=DEV)
    assert float(nr[0, 0, 0]) == -2.0 ** -100
    return nr, torch.full((n, h, w), float("-inf"), device=DEV), torch.zeros(n, h, w, device=DEV)


def test_no_return_frame_updates_the_grid_like_an_all_miss_frame():
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.state_encoding import OccupancyGridUpdater
    n, g, h, w = 2, 16, 30, 40
    cfg, scene, feed, poses = _rendered(n, g, h, w)
    nr, miss, seg0 = _no_return_frames(n, h, w)
    out = []
    for depth in (nr, miss):
        up = OccupancyGridUpdater(n, g, h, w, S.inverse_intrinsics(h, w), scene.range_gt, scene.voxel_size, scene.grid_gt, DEV)
        tri = torch.empty(n, g ** 3, device=DEV)
        up.update(feed.depth_raw, feed.seg_raw, feed.c2w, poses, tri_out=tri, tri_row_stride=g ** 3)  # a real frame first: a map to keep
        assert bool((tri != 0).any()) and int(up.coverage_count.sum()) > 0
        up.update(depth, seg0, feed.c2w, poses, tri_out=tri, tri_row_stride=g ** 3)
        torch.cuda.synchronize()
        out.append((tri.clone(), up.prob_grid.clone(), up.scanned_bits.clone(), up.coverage_count.clone()))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_no_return_frame_carves_nothing_and_a_half_dropped_frame_carves_a_subset():
    from gennbv_amd.ops.carve import CarvedMap
    from gennbv_amd.ops.depth_sensor import NO_RETURN
    n, g, h, w = 2, 16, 30, 40
    cfg, scene, feed, poses = _rendered(n, g, h, w)
    nr, _, _ = _no_return_frames(n, h, w)
    tri = G._tri(4, n, g)
    cm = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, stride=1, device=DEV)
    cm.update(tri, nr, poses)
    assert cm.last_gain[:, 0, 0].tolist() == [0] * n
    assert torch.equal(cm.map_i8, tri)
    # on an empty map: the ideal frame, and the frame with every other pixel dropped
    empty = torch.zeros(n, g ** 3, dtype=torch.int8, device=DEV)
    ideal = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, stride=1, device=DEV)
    ideal.update(empty, feed.depth_raw, poses)
    half = feed.depth_raw.clone()
    half.view(n, -1)[:, ::2] = NO_RETURN
    part = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, stride=1, device=DEV)
    part.update(empty, half, poses)
    a, b = ideal.map_i8 < 0, part.map_i8 < 0
    assert bool(b.any()) and not bool((b & ~a).any())
    assert bool((part.last_gain[:, 0, 0] > 0).all()) and bool((part.last_gain[:, 0, 0] <= ideal.last_gain[:, 0, 0]).all())


def test_no_return_frame_adds_no_scan_key():
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.eval.scan_accumulator import ScanAccumulator
    n, g, h, w = 2, 16, 30, 40
    cfg, scene, feed, poses = _rendered(n, g, h, w)
    nr, _, seg0 = _no_return_frames(n, h, w)
    acc = ScanAccumulator(n, [G._rand(7 + e, 300, 3, lo=-4.0, hi=6.0) for e in range(n)], h, w, S.inverse_intrinsics(h, w), cfg.depth_sense_dist,
                          capacity_per_env=4096, device=DEV)
    acc.add_frame(nr, seg0, feed.c2w)
    assert acc.counts.tolist() == [0] * n and bool((acc.table == -1).all()) and acc.flags.tolist() == [0] * n
    acc.add_frame(feed.depth_raw, feed.seg_raw, feed.c2w)
    before = acc.counts.clone()
    assert bool((before > 0).all())
    acc.add_frame(nr, seg0, feed.c2w)
    # what the sensor writes for a dropped foreground pixel: NO_RETURN with seg 0, the other pixels as rendered
    half_d, half_s = feed.depth_raw.clone(), feed.seg_raw.clone()
    half_d.view(n, -1)[:, ::2] = float(nr[0, 0, 0])
    half_s.view(n, -1)[:, ::2] = 0.0
    acc.add_frame(half_d, half_s, feed.c2w)
    assert torch.equal(acc.counts, before) and acc.flags.tolist() == [0] * n


# ---------------------------------------------------------------------------------------------------------------- stream order
@G.case("depth_sensor", "gnbv_depth_sensor")
def _c_depth_sensor():
    n, h, w = 2, 30, 37  # w % 4 != 0: the dword path; 1 110 pixels of an env: two tile rows
    sensor = _noisy(n, h, w)
    _, _, fr = G._frames(n, 16, h, w)
    A, D = ({"depth": f["depth"], "seg": f["seg"]} for f in fr)
    A["frame"], D["frame"] = torch.tensor([0, 7], dtype=torch.int32, device=DEV), torch.tensor([40, 41], dtype=torch.int32, device=DEV)
    I = G._bufs({k: A[k] for k in ("depth", "seg")})
    I["frame"] = sensor.frame  # in/out state: reloaded before every call, one higher after it
    O = {"depth_out": torch.empty(n, h, w, device=DEV), "seg_out": torch.empty(n, h, w, device=DEV)}
    return U.Live(I, A, D, O, G._on(lambda: sensor(I["depth"], I["seg"], out=(O["depth_out"], O["seg_out"]))), ["depth_out", "seg_out", "frame"])


@pytest.fixture(scope="module")
def stream_built():
    from gennbv_amd import _lib
    mp = pytest.MonkeyPatch()
    proxy = U.RecordingProxy(_lib.load())
    mp.setattr(_lib, "_lib", proxy)
    U.side_stream()
    live = G.CASES["depth_sensor"][1]()
    torch.cuda.synchronize()
    proxy.clear()
    vacuous = U.reference_runs(live)
    default_calls = proxy.streams()
    cal = U.delay_for([live.host_ms])
    yield live, vacuous, default_calls, cal, proxy
    mp.undo()


def test_the_case_is_in_the_table():
    assert G.CASES["depth_sensor"][0] == ("gnbv_depth_sensor",) and "gnbv_depth_sensor" in G.covered_entry_points()
    assert "gnbv_depth_sensor" in U.stream_entry_points()


def test_c_layer_keeps_to_the_stream(stream_built):
    live, vacuous, _, cal, proxy = stream_built
    assert vacuous == [], vacuous
    proxy.clear()
    problems = U.run_protocol(live, U.side_stream(), cal["cycles"])
    live.side_calls = proxy.streams()
    assert problems == [], problems
    assert live.R_A["frame"].tolist() == [1, 8]


def test_python_layer_passes_the_callers_stream(stream_built):
    live, _, default_calls, _, proxy = stream_built
    side = U.side_stream()
    if not hasattr(live, "side_calls"):  # run alone: no delay needed for the handles
        proxy.clear()
        U.run_protocol(live, side, 1000)
        live.side_calls = proxy.streams()
    want, null = side.cuda_stream, torch.cuda.default_stream().cuda_stream
    assert want != null
    assert {n for n, _ in live.side_calls} == {"gnbv_depth_sensor"}
    assert all(s == want for _, s in live.side_calls), (hex(want), live.side_calls)
    assert default_calls and all(s == null for _, s in default_calls), default_calls
    # a second call under the default stream AFTER the side-stream one: the default stream's handle again, the same result
    proxy.clear()
    got = U._enqueue(live, live.A, torch.cuda.default_stream())
    torch.cuda.synchronize()
    again = proxy.streams()
    assert again and all(s == null for _, s in again), again
    for k in live.compare:
        assert U._same(live, got[k], live.R_A[k]), k
