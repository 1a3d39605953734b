"""GPU: the frontier viewpoints -- gnbv_frontier_viewpoints (csrc/frontview.hip) against the CPU oracle (tests/frontview_oracle.py,
over ALL nodes: no window) with == on every element of the three outputs, pre-filled with a pattern: grid sizes with and without
the LDS planes, lattices that stick out of the grid (one with a single-node axis), both grid forms with junk of the occupied class
round every row, both modes, every chunking; then the op and FrontierViewPolicy on a real closed-loop env.  The mechanism is
asserted, not planning quality.  tests/test_frontview_cpu.py checks, with the oracle alone, that the cases are not trivial."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import PI, TaskConfig
from tests import frontview_cases as FC
from tests import frontview_oracle as VO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def _forms(g):
    """The two grid forms on the device, with junk of the OCCUPIED class round every row: int8 rows with a padded row stride (127),
    fp32 rows inside an observation-shaped buffer (5.0) -- a read past a row shows up as a false wall."""
    tri = FC.grid_case(g)[0]
    n, g3 = tri.shape[0], g ** 3
    rows = torch.tensor(tri.reshape(n, g3)).to(DEV)  # (a copy: the cached case is read-only)
    i8 = torch.full((n, 7 + g3 + 5), 127, dtype=torch.int8, device=DEV)
    i8[:, 7:7 + g3] = rows
    obs = torch.full((n, 7 + g3 + 3), 5.0, dtype=torch.float32, device=DEV)  # [state | grid | rgb]
    obs[:, 7:7 + g3] = rows.float()
    return {"i8": i8[:, 7:7 + g3], "f32": obs[:, 7:7 + g3]}


def _launch(tri_t, g, c, mode, chunk):
    """gnbv_frontier_viewpoints at the C ABI into buffers pre-filled with 0x5A5A5A5A -> (return code, node, cost, count)."""
    from gennbv_amd import _lib
    lib = _lib.load()
    n, t = c["targets"].shape[:2]
    frame = [torch.tensor(np.array(c[k])).to(DEV) for k in ("range_gt", "voxel_size")]
    field = torch.tensor(c["field"].view(np.int32).copy()).to(DEV)
    targets = torch.tensor(c["targets"].copy()).to(DEV)
    node = torch.full((n, t), FILL, dtype=torch.int32, device=DEV)
    cost = torch.full((n, t), FILL, dtype=torch.int32, device=DEV)
    count = torch.full((n, t, 2), FILL, dtype=torch.int32, device=DEV)
    i8 = tri_t.dtype == torch.int8
    row = int(tri_t.stride(0))
    a = _lib.GnbvFrontView(n=n, t=t, g=g, tri_i8=tri_t.data_ptr() if i8 else None, tri_i8_row_stride=row if i8 else 0,
                           tri_f32=None if i8 else tri_t.data_ptr(), tri_f32_row_stride=0 if i8 else row, range_gt=frame[0].data_ptr(),
                           voxel_size=frame[1].data_ptr(), nx=c["dims"][0], ny=c["dims"][1], nz=c["dims"][2],
                           lo=(C.c_double * 3)(*c["lo"]), h=(C.c_double * 3)(*c["h"]), field=field.data_ptr(), targets=targets.data_ptr(),
                           r_min=c["r_min"], r_max=c["r_max"], max_unknown=c["max_unknown"], node_out=node.data_ptr(),
                           cost_out=cost.data_ptr(), count_out=count.data_ptr(), chunk=chunk, mode=mode)
    err = lib.gnbv_frontier_viewpoints(C.byref(a), None)
    torch.cuda.synchronize()
    return err, node.cpu().numpy(), cost.cpu().numpy().view(np.uint32), count.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(FC.CONFIGS)))
@pytest.mark.parametrize("g", FC.GRIDS)
def test_viewpoints_equal_the_oracle_on_every_element(g, ci):
    from gennbv_amd import _lib
    c, w = FC.case(g, ci), FC.want(g, ci)
    t = c["targets"].shape[1]
    fits = g <= int(_lib.load().gnbv_frontview_lds_max_grid())
    ran = 0
    for name, tri_t in _forms(g).items():
        for mode in (0, 1, 2):
            if mode == 1 and not fits:
                assert _launch(tri_t, g, c, 1, 0)[0] == 1  # hipErrorInvalidValue: the planes do not fit
                continue
            for chunk in sorted({0, 1, 2, t, t + 5}) if mode else (0,):
                err, node, cost, count = _launch(tri_t, g, c, mode, chunk)
                what = (name, mode, chunk)
                assert err == 0, what
                assert np.array_equal(node, w["node"]), (what, np.argwhere(node != w["node"])[:5].tolist())
                assert np.array_equal(cost, w["cost"]), (what, np.argwhere(cost != w["cost"])[:5].tolist())
                assert np.array_equal(count, w["count"]), (what, np.argwhere(count != w["count"])[:5].tolist())
                ran += 1
    assert ran >= 2 * (1 + 3)


# ---------------------------------------------------------------------------
# 2. the op and the policy on a real closed-loop env
# ---------------------------------------------------------------------------
ENV_N, ENV_G, BLOCK, TOP = 4, 20, 4, 6


def _env_cfg():
    """The default task's volume on a coarser pose lattice (0.5 m), as the belief-flight tests have it."""
    return TaskConfig(camera_width=80, camera_height=60, grid_size=ENV_G, clip_pose_idx_up=[32, 32, 20, 0, 12, 12],
                      action_unit=[0.5, 0.5, 0.5, 0.0, PI / 12.0, PI / 6.0], init_action=[16, 16, 20, 0, 12, 0])


def _env(max_len=12, seed=2):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.env.flight import FlightLattice
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    from gennbv_amd.ops.flight_field import BeliefFlightField
    cfg = _env_cfg()
    scene = S.make_scenes(ENV_N, ENV_G, seed=seed)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    body = CollisionBody(sweep=True)
    flight = BeliefFlightField(ENV_N, FlightLattice(cfg, stride=2), body, scene.range_gt, scene.voxel_size, ENV_G, unknown="free", device=DEV)
    return ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=max_len, collision=body, flight=flight), cfg, scene


def _tri(obs, cfg):
    return obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]


def test_op_and_policy_on_a_closed_loop_env():
    from gennbv_amd import _lib
    from gennbv_amd.eval.baselines import FrontierViewPolicy, MapGreedyPolicy, RandomLatticePolicy
    from gennbv_amd.ops.flight_field import field_u32
    from gennbv_amd.ops.frontier import Frontier
    from gennbv_amd.ops.frontier_view import FrontierViewpoints, block_target_voxels
    env, cfg, scene = _env()
    lat = env.flight.lattice
    rnd = RandomLatticePolicy(cfg, ENV_N, seed=3)
    obs = env.reset()
    for _ in range(4):
        obs = env.step(rnd(obs)[0])[0]
    # ---- the op against the oracle on the env's own map and field
    tri = _tri(obs, cfg)
    fr = Frontier(ENV_N, ENV_G, block=BLOCK, device=DEV)
    blocks = fr(tri)
    idx, cnt = fr.top(TOP)
    vox = block_target_voxels(blocks, idx)
    assert bool((cnt[:, 0] > 0).all())
    host = tri.reshape(ENV_N, ENV_G, ENV_G, ENV_G).cpu().numpy()
    r_min, r_max, mu = 1.0, 4.0, BLOCK
    want = VO.viewpoints(host, scene.range_gt.numpy(), scene.voxel_size.numpy(), lat.dims, lat.lo, lat.h, field_u32(env.flight.field),
                         vox.cpu().numpy(), r_min, r_max, mu)
    assert (want["node"] >= 0).any() and (want["count"][..., 0] > 0).any()
    snapshot = torch.sign(tri).to(torch.int8).contiguous()
    for mode in (0, 1, 2):
        fv = FrontierViewpoints(ENV_N, ENV_G, lat, scene.range_gt, scene.voxel_size, TOP, r_min, r_max, max_unknown=mu, mode=mode, device=DEV)
        for t, field in ((tri, env.flight), (snapshot, env.flight.field)):
            for buf in (fv.node, fv.cost_mm, fv.count):
                buf.fill_(FILL)
            node, cost, count = fv(t, field, vox)
            assert node is fv.node and cost is fv.cost_mm and count is fv.count
            assert np.array_equal(node.cpu().numpy(), want["node"]) and np.array_equal(field_u32(cost), want["cost"])
            assert np.array_equal(count.cpu().numpy(), want["count"])
        assert fv.launches == 2
    for bad in (dict(tri=tri.cpu()), dict(tri=tri[:2]), dict(vox=vox.long()), dict(vox=vox[:, :2]), dict(field=env.flight.field[:, :-1]),
                dict(field=env.flight.field.float())):
        kw = dict(tri=tri, field=env.flight.field, vox=vox)
        kw.update(bad)
        with pytest.raises(_lib.GennbvHipError):
            fv(kw["tri"], kw["field"], kw["vox"])

    # ---- the policy for an episode, host synchronisation made an error inside every decision
    # (the fallback's own decision is the fallback's business: MapGreedyPolicy builds small host tensors per decision, which the
    # sync debug mode reports, so the episode under that mode falls back to a random lattice pose, whose draw is asynchronous;
    # MapGreedyPolicy as the fallback runs a few decisions at the end, without the mode)
    fallback = RandomLatticePolicy(cfg, ENV_N, seed=5)
    pol = FrontierViewPolicy(env, fallback, top=TOP, block=BLOCK, r_min_m=r_min, r_max_m=r_max)
    assert pol.max_unknown == BLOCK and pol.policy is pol
    low, up = torch.tensor(cfg.clip_pose_idx_low, device=DEV), torch.tensor(cfg.clip_pose_idx_up, device=DEV)
    obs = env.reset()
    # (warm-up on a policy of its own, so that `pol` starts without memory: the first use of a torch op may synchronise)
    FrontierViewPolicy(env, fallback, top=TOP, block=BLOCK, r_min_m=r_min, r_max_m=r_max)(obs)
    node_pos = torch.as_tensor(lat.node_positions(), device=DEV)

    def decide(o):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            return pol(o)[0]
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # an empty map has no frontier: every env falls back.  (reset() already scans from the init pose, so the env's own first
    # observation is not empty; the empty map is shown to the policy directly.)
    empty = obs.clone()
    _tri(empty, cfg).zero_()
    act = decide(empty)
    assert bool(pol.fell_back.all()) and bool((pol.last_node == -1).all()) and bool((pol.tried_count == -1).all())
    assert bool((act >= low).all()) and bool((act <= up).all())
    own = 0
    for step in range(10):
        act = decide(obs)
        assert act.dtype == torch.int64 and act.shape == (ENV_N, 6) and bool((act >= low).all()) and bool((act <= up).all())
        took = ~pol.fell_back
        own += int(took.sum())
        if bool(took.any()):
            # every action of the policy's own stands on its node, which the field reaches
            pose = S.poses_from_actions(act, cfg).float()
            assert bool(env.flight.reachable(pose[:, None])[:, 0][took].all())
            at = node_pos[pol.last_node.clamp(min=0)]
            assert torch.allclose(pose[took, :3].double(), at[took], rtol=0, atol=1e-5)
            assert bool((pol.last_cost_mm[took] < 0xFFFFFFFF).all()) and bool((pol.last_count[took] > 0).all())
        assert bool((pol.last_node[pol.fell_back] == -1).all())
        obs = env.step(act)[0]
    assert own > 0  # the planner planned: not every decision fell back
    both = FrontierViewPolicy(env, MapGreedyPolicy(env, k=8, seed=5), top=TOP, block=BLOCK, r_min_m=r_min, r_max_m=r_max, voxel_value_mm=50)
    obs = env.reset()
    for _ in range(3):
        act = both(obs)[0]
        assert act.dtype == torch.int64 and bool((act >= low).all()) and bool((act <= up).all())
        obs = env.step(act)[0]
