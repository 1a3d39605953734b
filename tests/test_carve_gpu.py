"""GPU: the view gain of a measured frame (GnbvViewGain depth_raw / carve_i8; csrc/viewgain.hip k_view_carve, k_vg_fate_depth,
k_vg_carve_slab) against the CPU oracle (tests/carve_oracle.py) over the case table of tests/carve_cases.py, exactly; CarvedMap
(ops/carve.py) over a closed-loop episode against the oracle's replay; the env with `carve`; the stream order of both.
All comparisons are ==: integers and bytes with one right answer."""
import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from tests import carve_cases as CC
from tests import carve_oracle as CO
from tests import gain_masks_oracle as MO
from tests import stream_order_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, RANGE = CC.H, CC.W, CC.RANGE


# ------------------------------------------------------------------------------------------------------------ the built cases
def _render(scene, poses):
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    cfg = CC.cfg_of(scene.grid_gt.shape[1])
    depth, seg, _, _ = RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg, with_rgba=False).render(poses.to(DEV))
    return depth.clone(), seg.clone()


def _update(scene, cfg, depth, seg, poses):
    """The updater's own output of the frame."""
    from gennbv_amd.env.state_encoding import OccupancyGridUpdater
    n, g = depth.shape[0], cfg.grid_size
    upd = OccupancyGridUpdater(n, g, H, W, S.inverse_intrinsics(H, W, cfg.horizontal_fov), scene.range_gt, scene.voxel_size, scene.grid_gt,
                               DEV, cfg.depth_sense_dist)
    c2w = S.camera_to_world(poses).float()
    return upd.update(depth.to(DEV), seg.to(DEV), c2w.to(DEV), poses.to(DEV).contiguous()).reshape(n, -1).cpu()


_BUILT = {}


def built(case, n=CC.N):
    """The case on the device, with the kernel's own camera matrices and the oracle's answer over them: computed once."""
    from gennbv_amd.ops.view_gain import make_view_gain
    key = (case, n)
    if key not in _BUILT:
        b = CC.build(case, _render, _update, n=n)
        g, stride, k = case
        b["words"] = MO.min_words(g) + 4  # pad words past ceil(g^3 / 32)
        b["dev"] = {x: b[x].to(DEV) for x in ("tri", "poses", "depth")}
        cam = make_view_gain(n, k, b["cfg"], b["scene"].range_gt, b["scene"].voxel_size, stride=stride, range_m=RANGE, device=DEV,
                             with_c2w=True)
        cam(b["dev"]["tri"], b["dev"]["poses"])
        b["c2w"] = cam.c2w.cpu().numpy()
        b["want"] = CO.measured(b["tri"].numpy(), b["c2w"], b["depth"].numpy(), b["scene"].range_gt.numpy(), b["scene"].voxel_size.numpy(),
                                b["kinv"], H, W, stride, RANGE, b["sense"], words=b["words"])
        _BUILT[key] = b
    return _BUILT[key]


def _pattern(n, g3):
    """int8 [n, g3] bytes none of which is -1"""
    return ((torch.arange(n * g3, dtype=torch.int64) * 7 + 3) % 100).to(torch.int8).view(n, g3).to(DEV)


def _masks_op(b, chunk=0, slab=None, n=None):
    from gennbv_amd.ops.gain_masks import ViewGainMasks, ViewGainMasksSlab
    kw = dict(stride=b["stride"], range_m=RANGE, device=DEV, words=b["words"], with_c2w=True, chunk=chunk)
    args = (b["n"], b["k"], b["cfg"], b["scene"].range_gt, b["scene"].voxel_size)
    return ViewGainMasks(*args, **kw) if slab is None else ViewGainMasksSlab(*args, slab=slab, **kw)


def _plain_op(b, chunk=0, slab=None):
    from gennbv_amd.ops.view_gain import ViewGain, ViewGainSlab
    kw = dict(stride=b["stride"], range_m=RANGE, device=DEV, with_c2w=True, chunk=chunk)
    args = (b["n"], b["k"], b["cfg"], b["scene"].range_gt, b["scene"].voxel_size)
    return ViewGain(*args, **kw) if slab is None else ViewGainSlab(*args, slab=slab, **kw)


def _check(b, op, masks, alias_ok):
    """One operator against the oracle: gain, camera, the mask rows with their pad words, the carve bytes over a pattern, and the
    aliased call (or its refusal)."""
    from gennbv_amd import _lib
    d = b["dev"]
    want_gain, want_ub, want_hb, want_carve = b["want"]
    n, g3 = b["n"], b["g"] ** 3
    pattern = _pattern(n, g3)
    carve = pattern.clone()
    op.gain.fill_(-77)
    if masks:
        op.unknown_bits.fill_(-1)
        op.hit_bits.fill_(-1)
    gain = op(d["tri"], d["poses"], depth=d["depth"], carve_out=carve).cpu().numpy()
    assert np.array_equal(op.c2w.cpu().numpy().view(np.uint32), b["c2w"].view(np.uint32))
    print("gain sum", gain.sum(axis=(0, 1)), "oracle", want_gain.sum(axis=(0, 1)), "carved", int(want_carve.sum()))
    assert np.array_equal(gain, want_gain)
    if masks:
        assert np.array_equal(op.unknown_bits.cpu().numpy().view(np.uint32), want_ub)
        assert np.array_equal(op.hit_bits.cpu().numpy().view(np.uint32), want_hb)
    want_bytes = np.where(want_carve, np.int8(-1), pattern.cpu().numpy())
    assert np.array_equal(carve.cpu().numpy(), want_bytes)  # every byte outside the carve set is unchanged
    # without carve_out: the same integers, and nothing else is written
    assert np.array_equal(op(d["tri"], d["poses"], depth=d["depth"]).cpu().numpy(), want_gain)
    tri = d["tri"].clone()
    if alias_ok:
        assert np.array_equal(op(tri, d["poses"], depth=d["depth"], carve_out=tri).cpu().numpy(), want_gain)
        assert np.array_equal(tri.cpu().numpy(), np.where(want_carve, np.int8(-1), b["tri"].numpy()))
    else:
        with pytest.raises(_lib.GennbvHipError):
            op(tri, d["poses"], depth=d["depth"], carve_out=tri)
        assert torch.equal(tri, d["tri"])
    return gain


# --------------------------------------------------------------------------------------------------------- C ABI, the LDS kernel
@pytest.mark.parametrize("case", CC.CASES)
def test_lds_kernel_equals_oracle(case):
    b = built(case)
    classes = CC.ray_classes(b, b["c2w"])  # the case is not degenerate with the mesh renderer's depth either
    print(case, classes)
    assert all(classes[c] > 0 for c in CC.CLASSES), classes
    assert b["want"][3].any()
    for chunk in CC.CHUNKS:
        _check(b, _masks_op(b, chunk), True, alias_ok=b["k"] == 1)
        _check(b, _plain_op(b, chunk), False, alias_ok=b["k"] == 1)


# ----------------------------------------------------------------------------------------------------------------- slab kernels
@pytest.mark.parametrize("case,slab", [((33, 1, 3), 5), ((33, 3, 1), 5), ((33, 1, 3), 33), ((33, 3, 1), 33)])
def test_slab_kernels_equal_oracle_and_lds_kernel(case, slab):
    b = built(case)
    for chunk in (0, 2):
        gain = _check(b, _masks_op(b, chunk, slab=slab), True, alias_ok=True)
        _check(b, _plain_op(b, chunk, slab=slab), False, alias_ok=True)
    # the LDS kernel, directly: integers, both mask rows and the carve bytes
    lds, sl = _masks_op(b), _masks_op(b, slab=slab)
    carve_l, carve_s = _pattern(b["n"], b["g"] ** 3), _pattern(b["n"], b["g"] ** 3)
    d = b["dev"]
    got_l = lds(d["tri"], d["poses"], depth=d["depth"], carve_out=carve_l)
    got_s = sl(d["tri"], d["poses"], depth=d["depth"], carve_out=carve_s)
    assert np.array_equal(got_l.cpu().numpy(), gain) and torch.equal(got_l, got_s)
    assert torch.equal(lds.unknown_bits, sl.unknown_bits) and torch.equal(lds.hit_bits, sl.hit_bits) and torch.equal(carve_l, carve_s)


@pytest.mark.parametrize("case,n", [((65, 1, 2), 2), ((128, 3, 2), 1)])
def test_slab_kernels_above_the_lds_limit(case, n):
    b = built(case, n=n)
    assert b["want"][3].any() and (b["want"][0][..., 2] > 0).any()
    _check(b, _masks_op(b, slab=0), True, alias_ok=True)
    if case[0] == 65:
        _check(b, _plain_op(b, slab=7), False, alias_ok=True)


def test_the_refusal_tests_base_arguments_are_accepted():
    """tests/test_carve_cpu.py refuses variations of one base struct on made-up pointers.  The same values on real buffers are
    accepted by all four entry points, so each refusal there is the varied field's."""
    import ctypes as C
    from gennbv_amd import _lib
    from tests import test_carve_cpu as TC
    lib = _lib.load()
    scene = S.make_scenes(2, 20, seed=1)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    kinv = S.inverse_intrinsics(60, 80).contiguous()
    poses = torch.tensor([4.0, 3.0, 6.0, 0.0, 0.5, 3.6], device=DEV).repeat(2, 3, 1).contiguous()
    bufs = dict(tri_i8=z(2, 8000, dt=torch.int8), poses=poses, range_gt=scene.range_gt.to(DEV).contiguous(),
                voxel_size=scene.voxel_size.to(DEV).contiguous(), gain=z(2, 3, 3, dt=torch.int32),
                depth_raw=torch.full((2, 3, 60, 80), -4.0, device=DEV), carve_i8=z(2, 8000, dt=torch.int8))
    a = TC._args(inv_intri=kinv.data_ptr(), **{k: v.data_ptr() for k, v in bufs.items()})
    ub, hb = z(2, 3, 252, dt=torch.int32), z(2, 3, 252, dt=torch.int32)
    ws_bytes = int(lib.gnbv_view_gain_slab_workspace_bytes(2, 3, 20, 60, 80, 4))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(torch.device(DEV))
    assert lib.gnbv_view_gain(C.byref(a), st) == 0
    first = bufs["gain"].clone()
    assert lib.gnbv_view_gain_masks(C.byref(a), 252, ub.data_ptr(), hb.data_ptr(), st) == 0
    assert lib.gnbv_view_gain_slab(C.byref(a), 0, ws.data_ptr(), ws_bytes, st) == 0
    assert lib.gnbv_view_gain_slab_masks(C.byref(a), 0, ws.data_ptr(), ws_bytes, 252, ub.data_ptr(), hb.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs["gain"], first) and int(first[..., 0].sum()) > 0 and bool((bufs["carve_i8"] == -1).any())


# -------------------------------------------------------------------------------------------------------------- all-miss depth
@pytest.mark.parametrize("case,slab", [((16, 1, 3), None), ((33, 3, 1), None), ((33, 1, 3), 5)])
def test_all_miss_depth_gives_the_outputs_without_depth(case, slab):
    b = built(case)
    d = b["dev"]
    op = _masks_op(b, slab=slab)
    base = {k: v.clone() for k, v in (("gain", op(d["tri"], d["poses"])), ("ub", op.unknown_bits), ("hb", op.hit_bits), ("c2w", op.c2w))}
    assert int(base["gain"][..., 0].sum()) > 0 and int(base["gain"][..., 2].sum()) > 0
    for t in (op.gain, op.unknown_bits, op.hit_bits):
        t.fill_(-5)
    op.c2w.fill_(float("nan"))
    miss = torch.full_like(d["depth"], float("-inf"))
    got = op(d["tri"], d["poses"], depth=miss)
    for k, v in (("gain", got), ("ub", op.unknown_bits), ("hb", op.hit_bits), ("c2w", op.c2w)):
        assert torch.equal(v.view(torch.int32), base[k].view(torch.int32)), k


# ------------------------------------------------------------------------------------- CarvedMap over a closed-loop episode; the env
def _env(n, g, h, w, carve, max_len=4, flight=None, seed=3):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.config import TaskConfig
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.carve import CarvedMap
    cfg = TaskConfig(camera_width=w, camera_height=h, grid_size=g)
    scene = S.make_scenes(n, g, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    cm = CarvedMap(n, cfg, scene.range_gt, scene.voxel_size, device=DEV) if carve else None
    kw = {}
    if flight is not None:
        kw = dict(collision=CollisionBody(sweep=True), flight=flight(cfg, scene))
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=max_len, carve=cm, **kw), cfg, scene


def _grid(cfg, obs):
    return obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]


def test_carved_map_follows_the_oracle_replay_and_the_env_is_unchanged():
    """6 steps, 4 envs, 16^3, 30 x 40; env 1 runs out of time two steps before the others, so it restarts mid-episode."""
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    n, g, h, w = 4, 16, 30, 40
    env, cfg, scene = _env(n, g, h, w, True)
    ref, _, _ = _env(n, g, h, w, False)
    assert ref.map_tri is None and env.map_tri is env.carve.map_i8 and env.carve.stride == 2 and env.carve.range_m == 50.0
    pol = RandomLatticePolicy(cfg, n, seed=11)
    kinv = S.inverse_intrinsics(h, w, cfg.horizontal_fov).numpy()
    rng, vox = scene.range_gt.numpy(), scene.voxel_size.numpy()
    model = np.zeros((n, g ** 3), np.int8)
    partial_reset = False

    def replay(obs, reset):
        nonlocal model
        model, newly = CO.carved_update(model, _grid(cfg, obs).cpu().numpy(), env.feed.depth_raw.cpu().numpy(), env.feed.c2w.cpu().numpy(),
                                        rng, vox, kinv, h, w, 2, 50.0, cfg.depth_sense_dist, reset)
        got = env.map_tri.cpu().numpy()
        assert np.array_equal(got, model)
        assert np.array_equal(env.carve.last_gain[:, 0, 0].cpu().numpy(), newly) and newly.sum() > 0
        tri = np.sign(_grid(cfg, obs).cpu().numpy()).astype(np.int8)
        assert ((got < 0) | ~(tri < 0)).all()          # the free set is a superset of the observation's
        assert np.array_equal(got > 0, tri > 0)        # occupied voxels are the observation's
        assert ((got < 0) & (tri == 0)).any()          # and something was carved that the observation does not know

    obs, obs_ref = env.reset(), ref.reset()
    assert torch.equal(obs, obs_ref)
    replay(obs, np.ones(n, np.uint8))
    for step in range(6):
        if step == 0:
            env.episode_length_buf[1] = 2
            ref.episode_length_buf[1] = 2
        reset = env.reset_mask.cpu().numpy().copy()
        partial_reset |= bool(0 < reset.sum() < n)
        act = pol(obs)[0]
        obs, rew, done, _ = env.step(act)
        obs_ref, rew_ref, done_ref, _ = ref.step(act)
        assert torch.equal(obs.view(torch.int32), obs_ref.view(torch.int32)), step  # observation bytes
        assert torch.equal(rew.view(torch.int32), rew_ref.view(torch.int32)) and torch.equal(done, done_ref), step
        assert torch.equal(env.updater.coverage_count, ref.updater.coverage_count)
        replay(obs, reset)
    assert partial_reset


def test_belief_field_blocks_less_on_the_carved_map():
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.flight import FlightLattice
    from gennbv_amd.eval.baselines import RandomLatticePolicy
    from gennbv_amd.ops.flight_field import BeliefFlightField
    n, g, h, w = 4, 16, 30, 40

    def flight(cfg, scene):
        return BeliefFlightField(n, FlightLattice(cfg, stride=2), CollisionBody(sweep=True), scene.range_gt, scene.voxel_size, g,
                                 unknown="blocked", device=DEV)
    env, cfg, scene = _env(n, g, h, w, True, max_len=10, flight=flight)
    raw = flight(cfg, scene)
    pol = RandomLatticePolicy(cfg, n, seed=5)
    obs = env.reset()
    fewer = 0
    for step in range(4):
        obs = env.step(pol(obs)[0])[0]
        mine = env.flight.blocked_map.clone()
        assert torch.equal(raw.refresh(env.map_tri).blocked_map, mine)       # the env refreshed from env.map_tri
        theirs = raw.refresh(_grid(cfg, obs)).blocked_map
        assert not bool((mine & ~theirs).any())                              # bitwise a subset of the raw grid's
        fewer += int((mine != theirs).sum())
    assert fewer > 0


def test_env_refuses_an_open_loop_feed():
    from gennbv_amd import _lib
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    from gennbv_amd.ops.carve import CarvedMap
    cfg = CC.cfg_of(16)
    scene = S.make_scenes(2, 16, seed=1)
    cm = CarvedMap(2, cfg, scene.range_gt, scene.voxel_size, device=DEV)
    feed = ReplayFeed.synthetic(scene, cfg, 2, with_rgba=False)
    with pytest.raises(_lib.GennbvHipError, match="closed-loop"):
        ReplayFeedEnv(cfg, scene, feed, DEV, carve=cm)


def test_planners_read_the_carved_map():
    from gennbv_amd.eval.baselines import GreedyGainPolicy, planning_grid
    n, g, h, w = 4, 16, 30, 40
    env, cfg, _ = _env(n, g, h, w, True)
    ref, _, _ = _env(n, g, h, w, False)
    seen = []
    pol = GreedyGainPolicy(env, k=4, seed=2, gain_backend=lambda tri, poses: (seen.append(tri), torch.zeros(n, 4, 3, dtype=torch.int32, device=DEV))[1])
    obs = env.reset()
    pol(obs)
    assert seen[0] is env.map_tri and planning_grid(env, obs) is env.map_tri
    obs_ref = ref.reset()
    assert torch.equal(planning_grid(ref, obs_ref), _grid(cfg, obs_ref))


# ---------------------------------------------------------------------------------------------------------------- stream order
def _stream_cases():
    """Live objects in the way tests/test_stream_order_gpu.py writes its cases: the depth mode of each kernel family, and
    CarvedMap.update."""
    from gennbv_amd.ops.carve import CarvedMap
    out = {}
    a = built((16, 1, 3))
    # the decoy: the frames of the envs in reverse order (every env has the same voxel frame) over another random grid
    d = {"dev": {"tri": MO.random_tri(a["n"], 16, 0.05, seed=99).to(DEV), "poses": a["dev"]["poses"].flip(0).contiguous(),
                 "depth": a["dev"]["depth"].flip(0).contiguous()}}
    for name, slab in (("depth_lds", None), ("depth_slab", 5)):
        op = _masks_op(a, chunk=2, slab=slab)
        A = {k: a["dev"][k].clone() for k in ("tri", "poses", "depth")}
        D = {k: d["dev"][k].clone() for k in ("tri", "poses", "depth")}
        I = {k: torch.empty_like(v) for k, v in A.items()}
        O = {"gain": op.gain, "c2w": op.c2w, "ub": op.unknown_bits, "hb": op.hit_bits, "carve": torch.empty(a["n"], 16 ** 3, dtype=torch.int8, device=DEV)}
        if slab:
            O["workspace"] = op.workspace

        def call(stream, op=op, I=I, O=O):
            with torch.cuda.stream(stream):
                op(I["tri"], I["poses"], depth=I["depth"], carve_out=O["carve"])
        out[name] = U.Live(I, A, D, O, call, ["gain", "c2w", "ub", "hb", "carve"])
    cm = CarvedMap(a["n"], a["cfg"], a["scene"].range_gt, a["scene"].voxel_size, stride=1, range_m=RANGE, device=DEV)
    A = {"tri": a["dev"]["tri"].clone(), "poses": a["dev"]["poses"][:, 0].contiguous(), "depth": a["dev"]["depth"][:, 0].contiguous(),
         "map": MO.random_tri(a["n"], 16, 0.0, seed=1).to(DEV)}
    D = {"tri": d["dev"]["tri"].clone(), "poses": d["dev"]["poses"][:, 1].contiguous(), "depth": d["dev"]["depth"][:, 1].contiguous(),
         "map": MO.random_tri(a["n"], 16, 0.0, seed=2).to(DEV)}
    I = {"tri": torch.empty_like(A["tri"]), "poses": torch.empty_like(A["poses"]), "depth": torch.empty_like(A["depth"]), "map": cm.map_i8}

    def update(stream):
        with torch.cuda.stream(stream):
            cm.update(I["tri"], I["depth"], I["poses"])
    out["carved_map_update"] = U.Live(I, A, D, {"gain": cm.last_gain}, update, ["map", "gain"])
    return out


@pytest.fixture(scope="module")
def stream_built(request):
    from gennbv_amd import _lib
    mp = pytest.MonkeyPatch()
    proxy = U.RecordingProxy(_lib.load())
    mp.setattr(_lib, "_lib", proxy)
    U.side_stream()
    lives = _stream_cases()
    vacuous, default_calls = {}, {}
    for name, live in lives.items():
        torch.cuda.synchronize()
        proxy.clear()
        vacuous[name] = U.reference_runs(live)
        default_calls[name] = proxy.streams()
    cal = U.delay_for([l.host_ms for l in lives.values()])
    yield lives, vacuous, default_calls, cal, proxy
    mp.undo()


@pytest.mark.parametrize("name,entry", [("depth_lds", "gnbv_view_gain_masks"), ("depth_slab", "gnbv_view_gain_slab_masks"),
                                        ("carved_map_update", "gnbv_view_gain")])
def test_depth_mode_keeps_to_the_callers_stream(stream_built, name, entry):
    lives, vacuous, default_calls, cal, proxy = stream_built
    live = lives[name]
    assert vacuous[name] == [], vacuous[name]
    proxy.clear()
    side = U.side_stream()
    problems = U.run_protocol(live, side, cal["cycles"])
    calls = proxy.streams()
    assert problems == [], problems
    want, null = side.cuda_stream, torch.cuda.default_stream().cuda_stream
    assert want != null and entry in {n for n, _ in calls}
    assert all(s == want for _, s in calls), (hex(want), calls)
    assert all(s == null for _, s in default_calls[name]), default_calls[name]
