"""Baseline view planners to compare a learned policy against: a uniformly random lattice pose, the greedy
next-best-view planner over the view gain (ops/view_gain.py, csrc/viewgain.hip; grids up to 128^3), the one-step
oracle over the view coverage (ops/view_cover.py, csrc/viewcover.hip): the candidate that really adds the most
ground-truth voxels, and the greedy set-cover planner over a fixed pool of views whose visible ground truth is cached
as bit masks (ops/view_pool.py, csrc/covergreedy.hip) -- online, or as the plan-then-fly baseline: the set-cover plan ordered
into a short flight tour (ops/tour.py, csrc/tour.hip) and flown by TourPolicy.  FrontierViewPolicy is the nearest-frontier
baseline of the pilot that knows only its own map (ops/frontier_view.py, csrc/frontview.hip); MapCoverPolicy plans several
views ahead on that map: greedy set cover over the view gain's voxel masks (ops/gain_masks.py), optionally routed into a tour.

All speak the protocol `evaluate_policy_grid_obs` uses: `.policy(obs, deterministic=True) -> (actions, None, None)`,
and `predict(obs)`; actions are int64 [N,6] on the lattice of the task (inside clip_pose_idx_low / clip_pose_idx_up).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import torch

from ..env import synthetic as S
from ..env.config import TaskConfig


class LatticeCandidates:
    """[N,K,6] int64 lattice actions from a seeded CPU generator (the same numbers whatever device they are used on),
    uniform inside clip_pose_idx_low / clip_pose_idx_up; `look_at_scene` aims them like synthetic.sample_actions."""

    def __init__(self, cfg: TaskConfig, k: int, seed: int, look_at_scene: bool = False):
        self.cfg, self.k, self.look_at_scene = cfg, int(k), bool(look_at_scene)
        self.gen = torch.Generator(device="cpu").manual_seed(int(seed))
        self.low = torch.tensor(cfg.clip_pose_idx_low, dtype=torch.int64)
        self.up = torch.tensor(cfg.clip_pose_idx_up, dtype=torch.int64)

    def sample(self, num_envs: int, device="cpu") -> torch.Tensor:
        m = int(num_envs) * self.k
        if self.look_at_scene:
            a = S.sample_actions(m, self.cfg, self.gen, look_at_scene=True)
            a = torch.minimum(torch.maximum(a, self.low), self.up)
        else:
            a = torch.stack([torch.randint(int(lo), int(u) + 1, (m,), generator=self.gen) for lo, u in zip(self.low, self.up)], -1)
        a = a.view(int(num_envs), self.k, 6)
        dev = torch.device(device)
        if dev.type == "cuda":  # pinned staging + asynchronous copy: no host synchronisation
            a = a.pin_memory().to(dev, non_blocking=True)
        return a

    def poses(self, actions: torch.Tensor) -> torch.Tensor:
        """poses_from_actions' arithmetic: action * action_unit + clip_pose_low, fp32."""
        return S.poses_from_actions(actions, self.cfg).float()


class FrontierCandidates:
    """LatticeCandidates aimed at the frontier of the scanned map (ops/frontier.py, csrc/frontier.hip): the same `sample` / `poses`
    protocol plus `observe(tri)`, which the greedy planners call with the step's tri slice before `sample`.

    `sample` first makes exactly the draw LatticeCandidates(cfg, k, seed) makes (the same generator calls: with equal seeds the base
    actions are equal).  Then, per env, with M' the number of non-empty blocks among the `top` blocks holding the most frontier
    voxels (Frontier.top: ties to the lowest block index): M' = 0 -- nothing scanned yet, or nothing left -- returns the base
    candidates unchanged; otherwise candidate j looks at the frontier centroid c of the block of rank j mod M'.  Yaw is the lattice
    index in [low, up] whose angle is circularly nearest to atan2(c_y - p_y, c_x - p_x), pitch the index nearest to
    atan2(p_z - c_z, hypot(c_x - p_x, c_y - p_y)) (camera_to_world's sign: forward = (cos p cos y, cos p sin y, -sin p)); both are an
    argmin over the lattice angles in fp64, lowest index on ties; where the horizontal offset is zero the base yaw stays.  With
    `radius_m` the position is replaced too: per axis the lattice index nearest to c_a plus base_a mod (2 r_a + 1) - r_a,
    r_a = floor(radius_m / unit_a) (0 where the unit is 0), clamped to clip_pose_idx_low / up; with None the base position stays, so
    the two sources differ in aim only.  `set_blocks` injects a block summary [N, nb^3, 4] in place of a launch (tests).  All torch
    on the device, no host synchronisation; the pinned asynchronous copy of the base draw is LatticeCandidates' own."""

    def __init__(self, cfg: TaskConfig, k: int, seed: int, frontier, range_gt: torch.Tensor, voxel_size: torch.Tensor, top: int = 8,
                 radius_m: Optional[float] = None):
        if int(top) < 1:
            raise ValueError(f"FrontierCandidates: top must be >= 1, got {top}")
        if radius_m is not None and not float(radius_m) >= 0.0:  # (a NaN fails too)
            raise ValueError(f"FrontierCandidates: radius_m must be >= 0 or None, got {radius_m}")
        self.cfg, self.k, self.top = cfg, int(k), int(top)
        self.base = LatticeCandidates(cfg, k, seed)
        self.frontier, self.range_gt, self.voxel_size = frontier, range_gt, voxel_size
        self.radius_m = None if radius_m is None else float(radius_m)
        self.blocks = None
        self._consts = {}

    def observe(self, tri: torch.Tensor) -> None:
        self.blocks = self.frontier(tri)

    def set_blocks(self, blocks: torch.Tensor) -> None:
        self.blocks = blocks

    def _lattice(self, device):
        """The lattice as fp64 / int64 tensors on `device`, built once per device."""
        c = self._consts.get(device)
        if c is None:
            cfg = self.cfg
            f = lambda v: torch.tensor(v, dtype=torch.float64, device=device)  # noqa: E731
            low_i, up_i = self.base.low.to(device), self.base.up.to(device)
            unit, low = f(cfg.action_unit), f(cfg.clip_pose_low)
            r = torch.zeros(3, dtype=torch.int64, device=device)
            if self.radius_m is not None:
                r = torch.tensor([int(self.radius_m // u) if u > 0 else 0 for u in cfg.action_unit[:3]], dtype=torch.int64, device=device)
            angles = {ax: torch.arange(int(cfg.clip_pose_idx_low[ax]), int(cfg.clip_pose_idx_up[ax]) + 1, device=device).double() * unit[ax]
                      + low[ax] for ax in (4, 5)}
            c = self._consts[device] = (low_i, up_i, unit, low, r, angles, self.range_gt.to(device), self.voxel_size.to(device))
        return c

    def sample(self, num_envs: int, device="cpu") -> torch.Tensor:
        from ..ops.frontier import block_centroids, top_blocks
        from ..ops.frontier_view import aim_indices
        a = self.base.sample(num_envs, device)
        if self.blocks is None:
            return a
        device = a.device
        low_i, up_i, unit, low, r, angles, range_gt, voxel_size = self._lattice(device)
        blocks = self.blocks.to(device)
        idx, cnt = top_blocks(blocks, min(self.top, blocks.shape[1]))
        live = (cnt > 0).sum(dim=1)  # M' [N]: topk sorts by count, so the non-empty blocks come first
        aimed = (live > 0)[:, None]
        rank = torch.arange(self.k, device=device)[None] % live.clamp(min=1)[:, None]
        cent = block_centroids(blocks, idx, range_gt, voxel_size)
        c = cent.gather(1, rank[..., None].expand(-1, -1, 3))
        c = torch.where(aimed[..., None], c, torch.zeros_like(c))  # (an empty block's centroid is NaN: never used, never converted)
        pos_i = a[..., :3]
        if self.radius_m is not None:
            safe = torch.where(unit[:3] > 0, unit[:3], torch.ones_like(unit[:3]))
            near = torch.where(unit[:3] > 0, torch.round((c - low[:3]) / safe), torch.zeros_like(c)).long()
            near = torch.minimum(torch.maximum(near, low_i[:3]), up_i[:3])
            pos_i = torch.minimum(torch.maximum(near + a[..., :3] % (2 * r + 1) - r, low_i[:3]), up_i[:3])
        p = pos_i.double() * unit[:3] + low[:3]
        pitch, yaw = aim_indices(p, c, angles[4], angles[5], low_i[4], low_i[5], a[..., 5])
        out = torch.cat([pos_i, a[..., 3:4], pitch[..., None], yaw[..., None]], dim=-1)
        return torch.where(aimed[..., None], out, a)

    def poses(self, actions: torch.Tensor) -> torch.Tensor:
        return self.base.poses(actions)


def planning_grid(env, obs: torch.Tensor) -> torch.Tensor:
    """The tri-class grid the planners score and route on (GreedyGainPolicy, MapGreedyPolicy, MapCoverPolicy, FrontierViewPolicy
    and, through them, FrontierCandidates.observe): `env.map_tri`, int8 [N, G^3], where the env keeps a CarvedMap (ops/carve.py:
    the observation's grid plus the free space along every camera ray), otherwise the observation's grid slice, as ever."""
    carved = getattr(env, "map_tri", None)
    if carved is not None:
        return carved
    cfg = env.cfg
    return obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]


def _candidates(cfg: TaskConfig, k: int, seed: int, look_at_scene: bool, candidates):
    """The planners' candidate source: LatticeCandidates unless one is given, whose k must be the planner's."""
    if candidates is None:
        return LatticeCandidates(cfg, k, seed, look_at_scene)
    if int(getattr(candidates, "k", -1)) != int(k):
        raise ValueError(f"candidates.k = {getattr(candidates, 'k', None)} must equal the policy's k = {k}")
    return candidates


class RandomLatticePolicy:
    """A uniformly random lattice pose per env and step."""

    def __init__(self, cfg: TaskConfig, num_envs: int, seed: int):
        self.num_envs = int(num_envs)
        self.cands = LatticeCandidates(cfg, 1, seed)

    def __call__(self, obs, deterministic: bool = True):
        return self.cands.sample(self.num_envs, obs.device)[:, 0], None, None

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


def _sweeps(env) -> bool:
    """The env's CollisionBody also tests the flight between poses (CollisionBody.sweep)."""
    return bool(getattr(getattr(env, "collision", None), "sweep", False))


def candidate_contact(env, poses: torch.Tensor, out: torch.Tensor, sweep: bool, static: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The planners' "contact | sweep" block: out [N,K] u8 = the body at poses [N,K,6] (collide_candidates; or a copy of
    `static`, a contact computed before) and, with `sweep`, | the path code of the straight flight from env.poses to each pose.
    Where the env flies detours (`env.flight`, ops/flight_field.py) a candidate is refused for its path only if its straight
    flight is blocked AND no route over the flight lattice reaches it: the path bits of a candidate with a finite detour cost
    are dropped.  Without `env.flight` the launches are the ones the planners always made."""
    mesh, body = env.collision_mesh, env.collision
    contact = mesh.collide_candidates(poses, body, out=out) if static is None else out.copy_(static)
    if sweep:
        flight = getattr(env, "flight", None)
        if flight is None:
            mesh.sweep_candidates(env.poses, poses, body, out=contact, accumulate=True)
        else:
            path = mesh.sweep_candidates(env.poses, poses, body)
            contact |= torch.where(flight.reachable(poses), torch.zeros_like(path), path)
    return contact


def choose(gain: torch.Tensor, weights: Sequence[int], contact: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gain [N,K,3] int -> index [N] of the candidate with the largest w0 * unknown + w1 * unknown_hit (int64); candidates
    with contact[N,K] != 0 score -1; ties go to the lowest candidate index."""
    return choose_scored(gain, weights, contact)[0]


def candidate_score(gain: torch.Tensor, weights: Sequence[int], contact: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The score `choose` ranks, int64 [N,K]: w0 * unknown + w1 * unknown_hit, -1 where contact[N,K] != 0 (refused)."""
    score = int(weights[0]) * gain[..., 0].to(torch.int64) + int(weights[1]) * gain[..., 1].to(torch.int64)
    if contact is not None:
        score = torch.where(contact != 0, torch.full_like(score, -1), score)
    return score


def choose_scored(gain: torch.Tensor, weights: Sequence[int], contact: Optional[torch.Tensor] = None):
    """(`choose`'s index [N], the score [N,K] it ranked): what a teacher exposes to imitation (sb3/imitation.py)."""
    k = gain.shape[1]
    score = candidate_score(gain, weights, contact)
    # one key per candidate, strictly larger for the lower index at equal score: argmax has a single answer
    key = score * k + (k - 1 - torch.arange(k, device=score.device))
    return key.argmax(dim=1), score


def soft_targets(score: torch.Tensor, temperature: float) -> torch.Tensor:
    """Candidate weights fp32 [N,K] from a planner's scores int [N,K] (`last_score`; -1 = refused): over the candidates with
    score >= 0, q_j = exp((s_j - s_max) / (temperature * max(1, s_max))), normalised over them; refused candidates get 0; a row whose
    candidates are all refused is all zero (a dead sample of the imitation loss).  Computed in fp64 and rounded once."""
    if not float(temperature) > 0.0:  # (a NaN fails too)
        raise ValueError(f"soft_targets: temperature must be > 0, got {temperature}")
    s = score.to(torch.float64)
    ok = score >= 0
    s_max = torch.where(ok, s, torch.full_like(s, -1.0)).amax(dim=1, keepdim=True)
    z = (s - s_max) / (float(temperature) * s_max.clamp(min=1.0))
    e = torch.where(ok, torch.exp(z), torch.zeros_like(s))
    tot = e.sum(dim=1, keepdim=True)
    return torch.where(tot > 0, e / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(e)).to(torch.float32)


class GreedyGainPolicy:
    """Greedy next-best view: K random lattice candidates per env and step, the one with the largest
    w0 * unknown + w1 * unknown_hit of the view gain against the observation's grid wins; with a CollisionBody on the
    env (and `avoid_collisions`) candidates whose pose collides are never chosen unless all do; where that body has `sweep`,
    a candidate whose straight flight from `env.poses` is blocked (MeshScene.sweep_candidates, accumulated into the same
    contact buffer) counts exactly like one in contact -- that needs a collision mesh with `sweep_candidates`; where the env also
    flies detours (`env.flight`) only a candidate that no route reaches is refused for its path (`candidate_contact`).  No host
    synchronisation inside a decision.  `gain_backend(tri [N,G^3], poses [N,K,6]) -> gain [N,K,3]` replaces the kernel in
    tests only: the product path has no CPU fallback.  `candidates` (None: LatticeCandidates(cfg, k, seed, look_at_scene)) is
    another source with the same `k`, e.g. FrontierCandidates; if it has `observe`, it is shown the step's tri slice before
    `sample`.  Gain, contact rule and `choose` do not depend on the source."""

    def __init__(self, env, k: int = 32, weights=(1, 4), seed: int = 0, stride: int = 4, avoid_collisions: bool = True,
                 look_at_scene: bool = False, gain_backend: Optional[Callable] = None, candidates=None):
        cfg = env.cfg
        self.env, self.cfg, self.k, self.weights = env, cfg, int(k), (int(weights[0]), int(weights[1]))
        self.num_envs = int(env.num_envs)
        self.cands = _candidates(cfg, k, seed, look_at_scene, candidates)
        self.avoid_collisions = bool(avoid_collisions) and getattr(env, "collision", None) is not None
        self.sweep = self.avoid_collisions and _sweeps(env)
        if self.sweep and not (hasattr(env.collision_mesh, "sweep_candidates") and hasattr(env.collision_mesh, "collide_candidates")):
            from .. import _lib
            raise _lib.GennbvHipError("GreedyGainPolicy: CollisionBody.sweep needs a collision mesh with sweep_candidates")
        if gain_backend is None:
            from ..ops.view_gain import make_view_gain
            u = env.updater
            gain_backend = make_view_gain(self.num_envs, self.k, cfg, u.range_gt, u.voxel_size_gt, inv_intrinsics=u.inv_intri_host,
                                          stride=stride, device=env.device)
        self.gain_backend = gain_backend
        self._contact = None
        self.last_gain = None
        self.last_candidates = self.last_score = None  # the last decision's candidates int64 [N,K,6] and the score `choose` ranked [N,K]

    def __call__(self, obs, deterministic: bool = True):
        cfg, n, k = self.cfg, self.num_envs, self.k
        tri = planning_grid(self.env, obs)
        cand = self._sample(tri)
        poses = self.cands.poses(cand)
        gain = self.gain_backend(tri, poses)
        self.last_gain = gain
        contact = None
        if self.avoid_collisions:
            mesh = self.env.collision_mesh
            if hasattr(mesh, "collide_candidates"):  # all N x K poses in one launch
                if self._contact is None:
                    self._contact = torch.zeros(n, k, dtype=torch.uint8, device=obs.device)
                contact = self.contact(poses)  # | the flight from the current pose
            else:
                if self._contact is None:
                    self._contact = torch.zeros(k, n, dtype=torch.uint8, device=obs.device)
                for j in range(k):  # one call per candidate column ([N,6] rows, stride K * 6)
                    mesh.collide(poses[:, j], self.env.collision, out=self._contact[j])
                contact = self._contact.t()
        best, self.last_score = choose_scored(gain, self.weights, contact)
        self.last_candidates = cand
        return cand[torch.arange(n, device=cand.device), best], None, None

    def _sample(self, tri: torch.Tensor) -> torch.Tensor:
        """The step's candidates [N,K,6]; a source with `observe` (FrontierCandidates) is shown the step's tri slice first."""
        observe = getattr(self.cands, "observe", None)
        if observe is not None:
            observe(tri)
        return self.cands.sample(self.num_envs, tri.device)

    def contact(self, poses: torch.Tensor) -> torch.Tensor:
        """u8 [N,K] into `self._contact`: non-zero where candidate poses [N,K,6] is refused (the hook MapGreedyPolicy replaces)."""
        return candidate_contact(self.env, poses, self._contact, self.sweep)

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


class MapGreedyPolicy(GreedyGainPolicy):
    """GreedyGainPolicy for a pilot that knows only its own map: a candidate is refused iff the env's BeliefFlightField
    (ops/flight_field.py) holds no route to it -- contact = ~env.flight.reachable(poses) and nothing else.  The collision mesh is
    never consulted: not for the candidate's pose, not for the flight to it.  What the drone then really meets is the env's
    business (ReplayFeedEnv flies the field's route and lets the true mesh judge it).
    `shortcut` (None: as env.flight.shortcut) also asks the map about the straight leg from env.poses to the candidate
    (BeliefFlightField.sweep, the body's own radius instead of a node's inflated one): a candidate is then refused iff no route
    reaches it AND its straight leg is blocked on the map -- contact = ~reachable & (sweep != 0).  Still no mesh predicate.
    `max_cost_m` (None: the contact rule above alone) is a risk budget for a field with a price on unknown space
    (BeliefFlightField(unknown="costly")): a candidate with a route is also refused when env.flight.cost to it -- metres plus the
    penalties of the costly nodes entered -- exceeds max_cost_m.  One more query of the field, no mesh predicate."""

    def __init__(self, env, k: int = 32, weights=(1, 4), seed: int = 0, stride: int = 4, look_at_scene: bool = False,
                 gain_backend: Optional[Callable] = None, shortcut: Optional[bool] = None, max_cost_m: Optional[float] = None,
                 candidates=None):
        if max_cost_m is not None and not float(max_cost_m) > 0.0:  # (a NaN fails too)
            raise ValueError(f"MapGreedyPolicy: max_cost_m must be > 0 or None, got {max_cost_m}")
        self.max_cost_m = None if max_cost_m is None else float(max_cost_m)
        if not getattr(getattr(env, "flight", None), "belief", False):
            from .. import _lib
            raise _lib.GennbvHipError("MapGreedyPolicy needs an env whose flight is a BeliefFlightField")
        self.shortcut = bool(getattr(env.flight, "shortcut", False)) if shortcut is None else bool(shortcut)
        if self.shortcut and not getattr(env.flight, "shortcut", False):
            from .. import _lib
            raise _lib.GennbvHipError("MapGreedyPolicy(shortcut=True) needs BeliefFlightField(shortcut=True): the map snapshot")
        super().__init__(env, k=k, weights=weights, seed=seed, stride=stride, avoid_collisions=False, look_at_scene=look_at_scene,
                         gain_backend=gain_backend, candidates=candidates)
        self.avoid_collisions = True  # by the map: `contact` below; `sweep` stays off, no mesh predicate is launched

    def __call__(self, obs, deterministic: bool = True):
        cfg, n = self.cfg, self.num_envs
        tri = planning_grid(self.env, obs)
        cand = self._sample(tri)
        poses = self.cands.poses(cand)
        gain = self.gain_backend(tri, poses)
        self.last_gain = gain
        if self._contact is None:
            self._contact = torch.zeros(n, self.k, dtype=torch.uint8, device=obs.device)
        best, self.last_score = choose_scored(gain, self.weights, self.contact(poses))
        self.last_candidates = cand
        return cand[torch.arange(n, device=cand.device), best], None, None

    def contact(self, poses: torch.Tensor) -> torch.Tensor:
        fl = self.env.flight
        refused = ~fl.reachable(poses)
        if self.shortcut:
            refused &= fl.sweep(self.env.poses, poses) != 0
        if self.max_cost_m is not None:
            cost = fl.cost(poses)
            refused |= torch.isfinite(cost) & (cost > self.max_cost_m)
        return self._contact.copy_(refused)


class MapCoverPolicy(MapGreedyPolicy):
    """Planning ahead on the map: `horizon` views per plan that add DIFFERENT unknown voxels, for the pilot that knows only its own
    map -- the map-only counterpart of PoolCoverPolicy.plan_route / TourPolicy.  MapGreedyPolicy's constructor checks, candidate
    source (with the `observe` hook) and `contact(poses)` are reused as they are: a candidate is refused iff the belief field holds
    no route to it, tightened by `shortcut` / `max_cost_m` as documented there.  No mesh predicate is launched anywhere.

    A decision:
      1. plan: K candidates, their poses, ViewGainMasks(tri, poses) (ops/gain_masks.py: the view gain and its two voxel sets as bit
         masks; make_view_gain_masks picks ViewGainMasksSlab for grids above 64^3, up to 128^3) and
         `plan(horizon, which=mask, contact=self.contact(poses))`, greedy set cover from an empty covered set -- the masks hold only voxels that are unknown NOW;
      2. keep the rounds with gain > 0 whose choice is not refused, in plan order (a repeat has gain 0: the kept views are
         distinct); `views` [N] is their number; an env with none takes round 0's choice -- candidate 0 when all are refused
         (gnbv_cover_greedy's rule), exactly MapGreedyPolicy's fallback;
      3. order (`route`, horizon > 1): the points env.poses[:, :3] and the kept views' positions, legs from
         env.flight.pairwise_mm, order from route_tour, as PoolCoverPolicy.plan_route; a kept view no route reaches from the start
         is left out.  Without `route` the order is the plan's gain order;
      4. adopt: the new plan replaces env e's stored plan (`plan_actions` [N,horizon,6], `plan_views` [N], `cursor` [N]) where
         env.episode_length_buf[e] <= 1, where its cursor has reached min(commit, plan_views[e]), or where its stored plan is
         empty; elsewhere the stored plan continues;
      5. act: plan_actions[e, cursor[e]], and the cursor advances.
    The plan is computed for ALL envs at EVERY decision and selected with torch.where: an env that restarts mid-plan must not fly
    a tour planned on the previous episode's map, and finding out on the host which envs need a plan would synchronise.  The
    policy's own part of a decision reads no per-env state on the host (`contact` is MapGreedyPolicy's).
    commit = 1 is receding-horizon control: fly the first view of a plan whose views do not overlap, then plan again.
    commit = horizon with `route` is plan-then-fly on the map.  horizon = 1 chooses what MapGreedyPolicy chooses with weights
    (1, 0) for mask "unknown" and (0, 1) for mask "hit".
    mask = "mixed" with `weights` = (w_unknown, w_hit) (None: (1, 4); integers >= 0; refused with the other masks) plans under
    MapGreedyPolicy's own score: both masks are kept and step 1 is `plan_weighted(horizon, weights=weights, contact=...)`,
    gnbv_cover_greedy_w's weighted set cover against two covered sets that grow together; `last_gain` is then the weighted score
    and `last_plane_gain` int32 [N,horizon,2] the winners' (unknown, hit) gains (None with the other masks).  Steps 2 to 5 do not
    change.  horizon = 1 with "mixed" and weights w chooses what MapGreedyPolicy(weights=w) chooses.
    The last decision's plan, for every env whether adopted or not: `last_choice`, `last_gain` int32 [N,horizon] (the plan's
    integers, gain order), `last_views` int64 [N], `last_actions` int64 [N,horizon,6] (the views in flight order; the tail repeats
    the last), `last_length_mm` int64 [N] (the tour from env.poses; -1 without route), `last_gain3` [N,K,3] (the view gain),
    `adopted` bool [N].  `masks_backend` (an object with ViewGainMasks' `__call__` and `plan`; `plan_weighted` and `plane_gain` for "mixed") and `tour_backend`
    (`route_tour`'s signature) replace the kernels in tests only: the product path has no CPU fallback."""

    def __init__(self, env, k: int = 32, horizon: int = 3, commit: int = 1, mask: str = "hit", route: bool = False, seed: int = 0,
                 stride: int = 4, look_at_scene: bool = False, shortcut: Optional[bool] = None, max_cost_m: Optional[float] = None,
                 candidates=None, masks_backend=None, tour_backend: Optional[Callable] = None, weights=None):
        horizon, commit = int(horizon), int(commit)
        if not 1 <= horizon <= 16:
            raise ValueError(f"MapCoverPolicy: horizon must be in 1..16, got {horizon}")
        if not 1 <= commit <= horizon:
            raise ValueError(f"MapCoverPolicy: commit must be in 1..horizon = {horizon}, got {commit}")
        if mask not in ("hit", "unknown", "mixed"):
            raise ValueError(f"MapCoverPolicy: mask must be 'hit', 'unknown' or 'mixed', got {mask!r}")
        mixed = mask == "mixed"
        if weights is not None and not mixed:
            raise ValueError(f"MapCoverPolicy: weights belong to mask='mixed'; mask={mask!r} is the plan of one mask")
        if mixed:
            weights = (1, 4) if weights is None else tuple(weights)
            if len(weights) != 2 or any(int(w) != w or int(w) < 0 for w in weights):
                raise ValueError(f"MapCoverPolicy: weights must be two integers >= 0 (w_unknown, w_hit), got {weights!r}")
        else:
            weights = (1, 0) if mask == "unknown" else (0, 1)
        if masks_backend is None:
            from ..ops.gain_masks import make_view_gain_masks  # ViewGainMasks up to 64^3, ViewGainMasksSlab up to 128^3
            u = env.updater
            masks_backend = make_view_gain_masks(int(env.num_envs), int(k), env.cfg, u.range_gt, u.voxel_size_gt, inv_intrinsics=u.inv_intri_host,
                                                 stride=stride, device=env.device, hit=mixed or mask == "hit", unknown=mixed or mask == "unknown")
        super().__init__(env, k=k, weights=weights, seed=seed, stride=stride, look_at_scene=look_at_scene,
                         gain_backend=masks_backend, shortcut=shortcut, max_cost_m=max_cost_m, candidates=candidates)
        self.horizon, self.commit, self.mask, self.route = horizon, commit, mask, bool(route)
        self.tour_backend = tour_backend
        n, dev = self.num_envs, torch.device(env.device)
        self.plan_actions = torch.zeros(n, horizon, 6, dtype=torch.int64, device=dev)
        self.plan_views = torch.zeros(n, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(n, dtype=torch.int64, device=dev)
        self._rows = torch.arange(n, device=dev)
        self._slots = torch.arange(horizon, device=dev)[None]
        self._points = torch.empty(n, horizon + 1, 3, dtype=torch.float32, device=dev)
        self._no_length = torch.full((n,), -1, dtype=torch.int64, device=dev)
        self.last_choice = self.last_gain = self.last_views = self.last_actions = self.last_length_mm = self.last_gain3 = self.adopted = None
        self.last_plane_gain = None

    def __call__(self, obs, deterministic: bool = True):
        cfg, n, t_max = self.cfg, self.num_envs, self.horizon
        env, rows, slots = self.env, self._rows, self._slots
        # ---- 1. plan
        tri = planning_grid(env, obs)
        cand = self._sample(tri)
        poses = self.cands.poses(cand)
        self.last_gain3 = self.gain_backend(tri, poses)
        if self._contact is None:
            self._contact = torch.zeros(n, self.k, dtype=torch.uint8, device=obs.device)
        contact = self.contact(poses)
        if self.mask == "mixed":
            choice, gain, _ = self.gain_backend.plan_weighted(t_max, weights=self.weights, contact=contact)
            self.last_plane_gain = self.gain_backend.plane_gain
        else:
            choice, gain, _ = self.gain_backend.plan(t_max, which=self.mask, contact=contact)
        self.last_choice, self.last_gain = choice, gain
        choice64 = choice.long()
        # ---- 2. keep: the kept rounds to the front, in plan order (a stable sort on a 0 / 1 key)
        keep = (gain > 0) & (contact.gather(1, choice64) == 0)
        front = torch.sort((~keep).to(torch.uint8), dim=1, stable=True)[1]
        kept_views = choice64.gather(1, front)  # [N, T] candidate indices; the first `views` are the kept ones
        views = keep.sum(dim=1)
        length = self._no_length
        # ---- 3. order: slot t of the plan holds position `pick` of kept_views
        if self.route and t_max > 1:
            points = self._points
            points[:, 0] = env.poses[:, :3]
            points[:, 1:] = poses[..., :3].gather(1, kept_views[..., None].expand(-1, -1, 3))
            count = (views + 1).to(torch.int32)
            dist = env.flight.pairwise_mm(points, count)
            if self.tour_backend is None:
                from ..ops.tour import route_tour
                res = route_tour(dist, count)
            else:
                res = self.tour_backend(dist, count)
            routed = res.routed.long()
            views = routed - 1  # a kept view that no route reaches from the start is left out
            point = res.order.long().gather(1, torch.minimum(slots + 1, views[:, None]))  # (0, the start, where nothing is routed)
            pick = (point - 1).clamp(min=0)
            length = res.length_mm.clone()
        else:
            pick = torch.minimum(slots, (views - 1).clamp(min=0)[:, None])
        view = kept_views.gather(1, pick)
        view = torch.where((views > 0)[:, None], view, choice64[:, :1].expand(-1, t_max))  # no view: round 0's choice
        actions = cand.gather(1, view[..., None].expand(-1, -1, 6))
        self.last_views, self.last_actions, self.last_length_mm = views, actions, length
        # ---- 4. adopt
        adopt = (env.episode_length_buf <= 1) | (self.cursor >= torch.clamp(self.plan_views, max=self.commit))
        self.plan_actions = torch.where(adopt[:, None, None], actions, self.plan_actions)
        self.plan_views = torch.where(adopt, views, self.plan_views)
        self.cursor = torch.where(adopt, torch.zeros_like(self.cursor), self.cursor)
        self.adopted = adopt
        # ---- 5. act
        act = self.plan_actions[rows, self.cursor]
        self.cursor = self.cursor + 1
        return act, None, None


class FrontierViewPolicy:
    """The nearest-frontier baseline for the pilot that knows only its own map (Yamauchi's rule on the flight lattice): go to the
    cheapest lattice node that sees a frontier block on the map, and look at the block.  No mesh is consulted.

    Per decision: the tri slice goes to `frontier` (ops/frontier.py Frontier; None builds one with `block`) for the block records.
    A block is ELIGIBLE iff its count is > 0 and differs from `tried_count` [N, nb^3] int32 -- the count it had when this env last
    targeted it, -1 = never: the updater carves only along rays that hit foreground, so a frontier facing the sky never resolves,
    and a nearest-frontier rule without memory returns to it forever.  The `top` fullest eligible blocks (top_blocks' key over the
    masked counts: ties to the lowest block index) give the targets (block_target_voxels: the voxel holding the block's frontier
    centroid); one FrontierViewpoints launch (ops/frontier_view.py, csrc/frontview.hip) against env.flight.field gives each
    target's cheapest node in [r_min_m, r_max_m] with a line of sight that crosses at most `max_unknown` unknown voxels (None:
    `block` -- a block's centroid voxel need not itself border free space; a stated choice, nobody has measured it).  Among the
    targets with a node the winner maximises the int64 score count * voxel_value_mm - cost_mm (voxel_value_mm = 0: the nearest
    frontier), ties to the lowest rank by a distinct key as `choose` builds one.  The action: the node's position (node_actions),
    roll index 0, pitch and yaw aimed at the block's fp64 centroid (aim_indices; where the node is straight above or below it the
    fallback's yaw stays); the winner's count goes to `tried_count`.  Envs without a winner -- nothing scanned yet, the frontier
    exhausted, every frontier tried -- take the action of `fallback` (any policy of this protocol), which is evaluated for all envs
    and selected with torch.where.  `tried_count` rows reset where env.episode_length_buf == 0.  No host synchronisation in the
    policy's own part of a decision (what the fallback does is the fallback's).  `last_node` [N] int64 (-1 on a fallback row), `last_cost_mm` [N] int64, `last_count` [N] int64 and `fell_back`
    [N] bool describe the last decision.  `view_backend(tri, field, target_vox) -> (node, cost_mm, count)` replaces the kernel in
    tests only, as does a callable `frontier(tri) -> blocks`: the product path has no CPU fallback."""

    def __init__(self, env, fallback, top: int = 8, block: int = 4, *, r_min_m: float, r_max_m: float, max_unknown: Optional[int] = None,
                 voxel_value_mm: int = 0, frontier=None, view_backend: Optional[Callable] = None):
        from ..ops.frontier import block_grid
        flight = getattr(env, "flight", None)
        if not getattr(flight, "belief", False):
            from .. import _lib
            raise _lib.GennbvHipError("FrontierViewPolicy needs an env whose flight is a BeliefFlightField")
        cfg = env.cfg
        g, n = int(cfg.grid_size), int(env.num_envs)
        if int(block) < 1 or int(voxel_value_mm) < 0:
            raise ValueError(f"FrontierViewPolicy: block >= 1 and voxel_value_mm >= 0, got {block}, {voxel_value_mm}")
        nblk = block_grid(g, block) ** 3
        if not 1 <= int(top) <= nblk:
            raise ValueError(f"FrontierViewPolicy: top must be in 1..{nblk}, got {top}")
        self.env, self.cfg, self.num_envs, self.fallback = env, cfg, n, fallback
        self.top, self.block, self.voxel_value_mm = int(top), int(block), int(voxel_value_mm)
        self.max_unknown = int(block) if max_unknown is None else int(max_unknown)
        self.r_min_m, self.r_max_m = float(r_min_m), float(r_max_m)
        device = torch.device(env.device)
        if frontier is None:
            from ..ops.frontier import Frontier
            frontier = Frontier(n, g, block=self.block, device=device)
        self.frontier = frontier
        if view_backend is None:
            from ..ops.frontier_view import FrontierViewpoints
            view_backend = FrontierViewpoints(n, g, flight.lattice, flight.range_gt, flight.voxel_size, self.top, self.r_min_m,
                                              self.r_max_m, max_unknown=self.max_unknown, device=device)
        self.view_backend = view_backend
        self.range_gt, self.voxel_size = flight.range_gt, flight.voxel_size
        self.tried_count = torch.full((n, nblk), -1, dtype=torch.int32, device=device)
        f = lambda v: torch.tensor(v, dtype=torch.float64, device=device)  # noqa: E731
        self._unit, self._low = f(cfg.action_unit), f(cfg.clip_pose_low)
        self._low_i = torch.tensor(cfg.clip_pose_idx_low, dtype=torch.int64, device=device)
        self._angles = {ax: torch.arange(int(cfg.clip_pose_idx_low[ax]), int(cfg.clip_pose_idx_up[ax]) + 1, device=device).double()
                        * self._unit[ax] + self._low[ax] for ax in (4, 5)}
        self._roll = min(max(0, int(cfg.clip_pose_idx_low[3])), int(cfg.clip_pose_idx_up[3]))
        self._rank_key = self.top - 1 - torch.arange(self.top, device=device)
        self._rows = torch.arange(n, device=device)
        self.last_node = self.last_cost_mm = self.last_count = self.fell_back = None

    def __call__(self, obs, deterministic: bool = True):
        from ..ops.frontier import block_centroids, top_blocks
        from ..ops.frontier_view import aim_indices, block_target_voxels, node_actions
        cfg, rows = self.cfg, self._rows
        tri = planning_grid(self.env, obs)
        fb = self.fallback(obs, deterministic)[0].to(torch.int64)
        blocks = self.frontier(tri)
        count = blocks[..., 0]
        fresh = (self.env.episode_length_buf == 0)[:, None]
        tried = torch.where(fresh, torch.full_like(self.tried_count, -1), self.tried_count)
        eligible = (count > 0) & (count != tried)
        masked = blocks.clone()
        masked[..., 0] = torch.where(eligible, count, torch.zeros_like(count))
        idx, cnt = top_blocks(masked, self.top)  # cnt: 0 where the rank holds no eligible block
        vox = block_target_voxels(masked, idx)   # (-1 there: no target)
        node, cost, _ = self.view_backend(tri, self.env.flight, vox)
        cost = cost.to(torch.int64) & 0xFFFFFFFF
        valid = (node >= 0) & (cnt > 0)
        # one key per rank, strictly larger for the lower rank at equal score: argmax has a single answer
        score = cnt * self.voxel_value_mm - cost
        key = torch.where(valid, score * self.top + self._rank_key, torch.full_like(score, torch.iinfo(torch.int64).min))
        best = key.argmax(dim=1)
        has = valid.any(dim=1)
        blk, won, n_best = idx[rows, best], cnt[rows, best], node[rows, best].to(torch.int64)
        pos_i = node_actions(self.env.flight.lattice, cfg, n_best)
        cent = block_centroids(blocks, blk[:, None], self.range_gt, self.voxel_size)[:, 0]
        cent = torch.where(has[:, None], cent, torch.zeros_like(cent))  # (an empty block's centroid is NaN: never used)
        p = pos_i.double() * self._unit[:3] + self._low[:3]
        pitch, yaw = aim_indices(p, cent, self._angles[4], self._angles[5], self._low_i[4], self._low_i[5], fb[:, 5])
        act = torch.cat([pos_i, torch.full_like(pitch, self._roll)[:, None], pitch[:, None], yaw[:, None]], dim=-1)
        old = tried[rows, blk]
        self.tried_count.copy_(tried)
        self.tried_count[rows, blk] = torch.where(has, won.to(torch.int32), old)
        self.fell_back = ~has
        self.last_node = torch.where(has, n_best, torch.full_like(n_best, -1))
        self.last_cost_mm = torch.where(has, cost[rows, best], torch.full_like(n_best, 0xFFFFFFFF))
        self.last_count = torch.where(has, won, torch.zeros_like(won))
        return torch.where(has[:, None], act, fb), None, None

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


class OracleGainPolicy:
    """One-step oracle, the upper baseline beside GreedyGainPolicy: K random lattice candidates per env and step, and the
    one whose view really adds the most ground-truth voxels to the scanned set wins -- new_gt of the view coverage
    (ops/view_cover.py) of the env's own scene (`env.feed.mesh`), ground truth and scanned set (`env.updater.gt_bits`,
    `.scanned_bits`), i.e. at stride 1 exactly the coverage_count increment the env pays for the step.  It reads the scene
    geometry and the ground truth, which no deployable planner has.  Ties go to the lowest candidate index; with a
    CollisionBody on the env (and `avoid_collisions`) candidates whose pose collides are never chosen unless all do, and
    where that body has `sweep` neither are candidates whose straight flight from `env.poses` is blocked (with `env.flight`:
    blocked and reached by no route, `candidate_contact`).
    `last_cover` [N,K,3] keeps the last decision's integers.  No host synchronisation inside a decision.  It needs the
    packed updater (a binary ground truth) and a closed-loop feed with a mesh; anything else is refused.
    `cover_backend(poses [N,K,6], gt_bits, scanned_bits) -> cover [N,K,3]` replaces the kernel in tests only: the product
    path has no CPU fallback.

    On a step whose env is done the env resets, and the next step forces the init action whatever is chosen: the choice
    for that env is moot, and its new_gt (computed against the finished episode's scanned set) is not what the step pays."""

    def __init__(self, env, k: int = 32, seed: int = 0, stride: int = 1, avoid_collisions: bool = True,
                 look_at_scene: bool = False, cover_backend: Optional[Callable] = None):
        from .. import _lib
        cfg = env.cfg
        self.env, self.cfg, self.k = env, cfg, int(k)
        self.num_envs = int(env.num_envs)
        self.cands = LatticeCandidates(cfg, k, seed, look_at_scene)
        self.avoid_collisions = bool(avoid_collisions) and getattr(env, "collision", None) is not None
        self.sweep = self.avoid_collisions and _sweeps(env)
        u = env.updater
        if not getattr(u, "packed", False):
            raise _lib.GennbvHipError("OracleGainPolicy needs the packed updater (a binary ground truth: gt_bits / scanned_bits)")
        if cover_backend is None:
            mesh = getattr(env.feed, "mesh", None)
            if mesh is None:
                raise _lib.GennbvHipError("OracleGainPolicy needs the scene's mesh (a closed-loop RenderFeed): env.feed has none")
            from ..ops.view_cover import ViewCover
            cover_backend = ViewCover(mesh, cfg, u.range_gt, u.voxel_size_gt, self.k, stride=stride, inv_intrinsics=u.inv_intri_host,
                                      device=env.device)
        self.cover_backend = cover_backend
        self._contact = None
        self.last_cover = None
        self.last_candidates = self.last_score = None  # as GreedyGainPolicy's

    def __call__(self, obs, deterministic: bool = True):
        n, k = self.num_envs, self.k
        cand = self.cands.sample(n, obs.device)
        poses = self.cands.poses(cand)
        u = self.env.updater
        cover = self.cover_backend(poses, u.gt_bits, u.scanned_bits)
        self.last_cover = cover
        contact = None
        if self.avoid_collisions:
            if self._contact is None:
                self._contact = torch.zeros(n, k, dtype=torch.uint8, device=obs.device)
            contact = candidate_contact(self.env, poses, self._contact, self.sweep)
        best, self.last_score = choose_scored(cover, (1, 0), contact)
        self.last_candidates = cand
        return cand[torch.arange(n, device=cand.device), best], None, None

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


class PoolCoverPolicy:
    """Greedy set cover over a FIXED pool of views, the third upper baseline: `pool_size` lattice candidates per env are drawn
    once (`LatticeCandidates(cfg, pool_size, seed, look_at_scene).sample(n)`), their visible ground truth is traced once into
    bit masks (ops/view_pool.py ViewPool), and every decision is popcount(mask & ~scanned_bits) and an argmax over the pool --
    no ray is traced again.  At stride 1 `last_gain[e]` is exactly the coverage_count increment the env pays for the step
    (for envs that were not reset, as OracleGainPolicy).  Ties go to the lowest pool index; with a CollisionBody on the env (and
    `avoid_collisions`) pool views whose pose collides are never chosen unless all do; where that body has `sweep`, every
    decision also ORs the flight from `env.poses` to each pool pose into a copy of the pool's static contact (one copy, one
    sweep launch; with `env.flight` only for pool views no route reaches, `candidate_contact`) and hands it to the selection --
    the carried bounds stay valid, a bound does not depend on contact.
    `last_choice` [N] is the pool index.
    `persistent_bounds`: every candidate's last gain is kept as an upper bound for the next decision (gains only shrink
    while the scanned set grows), so a decision evaluates only the candidates that can still win; an env whose episode has
    just restarted (episode_length_buf <= 1 at decision time: the post-step kernel zeroes it on the done step, the next step
    forces the init action, clears the scanned set and counts 1) gets its row set back to unknown, on the device.  The
    actions are the same with and without.  `.plan(rounds)` is the offline greedy set-cover plan from the current scanned
    set; it keeps the static contact (an offline plan has no "current pose" per round, so no flight is tested).
    `.plan_route(rounds)` is that plan ordered into a short flight tour (RoutePlan; TourPolicy flies it).  No host
    synchronisation inside a decision.  It needs the packed updater and a closed-loop feed with a mesh, as
    OracleGainPolicy."""

    def __init__(self, env, pool_size: int = 256, seed: int = 0, stride: int = 1, avoid_collisions: bool = True,
                 look_at_scene: bool = True, persistent_bounds: bool = True):
        from .. import _lib
        from ..ops.view_pool import UNKNOWN, ViewPool
        cfg = env.cfg
        self.env, self.cfg, self.pool_size = env, cfg, int(pool_size)
        self.num_envs = n = int(env.num_envs)
        u = env.updater
        if not getattr(u, "packed", False):
            raise _lib.GennbvHipError("PoolCoverPolicy needs the packed updater (a binary ground truth: gt_bits / scanned_bits)")
        mesh = getattr(env.feed, "mesh", None)
        if mesh is None:
            raise _lib.GennbvHipError("PoolCoverPolicy needs the scene's mesh (a closed-loop RenderFeed): env.feed has none")
        self.cands = LatticeCandidates(cfg, pool_size, seed, look_at_scene)
        self.pool_actions = self.cands.sample(n, env.device)
        self.avoid_collisions = bool(avoid_collisions) and getattr(env, "collision", None) is not None
        self.pool = ViewPool(mesh, cfg, u.range_gt, u.voxel_size_gt, u.gt_bits, self.cands.poses(self.pool_actions), stride=stride,
                             inv_intrinsics=u.inv_intri_host, body=env.collision if self.avoid_collisions else None,
                             collision_mesh=env.collision_mesh if self.avoid_collisions else None)
        self.sweep = self.avoid_collisions and _sweeps(env)
        self._contact = torch.empty_like(self.pool.contact) if self.sweep else None
        self.persistent_bounds = bool(persistent_bounds)
        self._unknown = UNKNOWN
        self._ub = torch.full((n, self.pool_size), UNKNOWN, dtype=torch.int32, device=env.device) if self.persistent_bounds else None
        self._rows = torch.arange(n, device=env.device)
        self.last_gain = None
        self.last_choice = None

    def __call__(self, obs, deterministic: bool = True):
        env = self.env
        if self._ub is not None:
            self._ub.masked_fill_((env.episode_length_buf <= 1).unsqueeze(1), self._unknown)
        contact = None
        if self.sweep:  # the static contact | the flight from the current pose to each pool pose
            contact = candidate_contact(env, self.pool.poses, self._contact, True, static=self.pool.contact)
        choice, gain = self.pool.select(env.updater.scanned_bits, self._ub, contact)
        self.last_choice, self.last_gain = choice, gain
        return self.pool_actions[self._rows, choice.long()], None, None

    def plan(self, rounds: int, covered_bits: Optional[torch.Tensor] = None, lazy: bool = True):
        """ViewPool.plan from covered_bits (default: the env's current scanned set) -> (choice [N,T], gain [N,T], covered);
        the planned actions are pool_actions[e, choice[e, t]].  The plan keeps the static contact: no flight is tested."""
        return self.pool.plan(rounds, self.env.updater.scanned_bits if covered_bits is None else covered_bits, lazy)

    def plan_route(self, rounds: int, start: Optional[torch.Tensor] = None, covered_bits: Optional[torch.Tensor] = None) -> "RoutePlan":
        """Plan, then route: `plan(rounds, covered_bits)`, keep the rounds with gain > 0 whose view is not in static contact (a
        repeat has gain 0, so the kept views are distinct), and order them into a short open flight tour from `start` [N, >= 3]
        (default: env.poses).  The legs come from `env.flight.pairwise_mm` (shortest collision-free routes, mm) where the env has
        a flight field, from `euclid_mm` (straight flights) otherwise; the order from `route_tour` (nearest neighbour + 2-opt,
        csrc/tour.hip).  A kept view that no route reaches from the start is left out of the tour.  No host synchronisation."""
        from .. import _lib
        from ..ops.tour import MAX_POINTS, euclid_mm, route_tour
        rounds = int(rounds)
        if not 1 <= rounds <= MAX_POINTS - 1:
            raise _lib.GennbvHipError(f"PoolCoverPolicy.plan_route: rounds in 1..{MAX_POINTS - 1} (the start and the views are {MAX_POINTS} "
                                      f"points at most), got {rounds}")
        env, n, dev = self.env, self.num_envs, self.env.device
        choice, gain, _ = self.plan(rounds, covered_bits)
        choice64 = choice.long()
        keep = gain > 0
        if self.pool.contact is not None:
            keep &= self.pool.contact.gather(1, choice64) == 0
        # the kept rounds to the front, in plan order: a stable sort on a 0 / 1 key
        front = torch.sort((~keep).to(torch.uint8), dim=1, stable=True)[1]
        views = choice64.gather(1, front)  # [N, T] pool indices; the first `kept` are the kept views
        count = (keep.sum(dim=1) + 1).to(torch.int32)
        start = env.poses if start is None else start
        if start.dim() != 2 or start.shape[0] != n or start.shape[1] < 3:
            raise _lib.GennbvHipError(f"PoolCoverPolicy.plan_route: start must be [{n}, >= 3], got {tuple(start.shape)}")
        points = torch.empty(n, rounds + 1, 3, dtype=torch.float32, device=dev)
        points[:, 0] = start[:, :3]
        points[:, 1:] = self.pool.poses[..., :3].gather(1, views[..., None].expand(-1, -1, 3))
        flight = getattr(env, "flight", None)
        dist = flight.pairwise_mm(points, count) if flight is not None else euclid_mm(points, count)
        res = route_tour(dist, count)
        # the routed views in flight order; the tail repeats the last one; the init action where nothing is routed
        routed = res.routed.long()
        slot = torch.minimum(torch.arange(1, rounds + 1, device=dev)[None], (routed - 1)[:, None])
        point = res.order.long().gather(1, slot)
        view = views.gather(1, (point - 1).clamp(min=0))
        actions = self.pool_actions.gather(1, view[..., None].expand(-1, -1, 6))
        init = torch.tensor(self.cfg.init_action, dtype=torch.int64, device=dev)
        actions = torch.where((routed > 1)[:, None, None], actions, init.expand_as(actions))
        # the same views in the plan's own order: the route points in ascending index (the compaction kept the plan order)
        p = rounds + 1
        ranks = torch.arange(p, device=dev)[None]
        member = torch.zeros(n, p, dtype=torch.bool, device=dev).scatter_(1, res.order.long(), ranks < routed[:, None])
        seq = torch.sort((~member).to(torch.uint8), dim=1, stable=True)[1]
        legs = (dist.long() & 0xFFFFFFFF).flatten(1).gather(1, seq[:, :-1] * p + seq[:, 1:])
        flown = ranks[:, :-1] < (routed - 1)[:, None]
        missing = (flown & (legs == 0xFFFFFFFF)).any(dim=1)
        plan_len = torch.where(missing, torch.full_like(routed, -1), torch.where(flown, legs, torch.zeros_like(legs)).sum(dim=1))
        plan_view = views.gather(1, (seq.gather(1, slot) - 1).clamp(min=0))
        plan_actions = self.pool_actions.gather(1, plan_view[..., None].expand(-1, -1, 6))
        plan_actions = torch.where((routed > 1)[:, None, None], plan_actions, init.expand_as(plan_actions))
        return RoutePlan(actions=actions, views=(routed - 1).to(torch.int32), length_mm=res.length_mm.clone(), plan_length_mm=plan_len,
                         status=res.status.clone(), choice=choice.clone(), gain=gain.clone(), plan_actions=plan_actions)

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state


@dataclass
class RoutePlan:
    """PoolCoverPolicy.plan_route's result (tensors on the env's device)."""
    actions: torch.Tensor         # int64 [N, T, 6]: the routed views' pool actions in flight order; the tail repeats the last routed
    #                               view; cfg.init_action where nothing is routed
    views: torch.Tensor           # int32 [N]: routed views (the start not counted)
    length_mm: torch.Tensor       # int64 [N]: the length of the tour, start -> views in flight order
    plan_length_mm: torch.Tensor  # int64 [N]: the same views flown in the plan's gain order, from the same matrix; -1: a missing leg
    status: torch.Tensor          # int32 [N]: gnbv_tour_route's status bits
    choice: torch.Tensor          # int32 [N, T]: the plan's pool indices, in gain order
    gain: torch.Tensor            # int32 [N, T]: the plan's gains
    plan_actions: torch.Tensor    # int64 [N, T, 6]: the routed views in the plan's gain order (what plan_length_mm measures), same tail


class TourPolicy:
    """Plan-then-fly: the greedy set-cover plan of `pool_policy` (a PoolCoverPolicy on `env`) over `rounds` views, ordered into a
    short flight tour and flown view by view -- the classic offline coverage-planning baseline ("how many metres for this
    coverage, for a planner that knows the scene?", against `env.flight_length`).  The plan is computed once, at construction,
    from an empty covered set and the task's init pose (`poses_from_actions(cfg.init_action)`): scene, pool, init pose and empty
    scanned set are the same at every episode start, so one plan serves every episode.  A decision for an env with
    episode_length_buf == t >= 1 is `last_plan.actions[e, min(t, rounds) - 1]`: view t of the tour, the last view once the tour
    is flown; at t == 0 the env has just finished and the next step forces the init action whatever is chosen.  One gather per
    decision, no host synchronisation."""

    def __init__(self, env, pool_policy: PoolCoverPolicy, rounds: int):
        self.env, self.cfg, self.pool_policy, self.rounds = env, env.cfg, pool_policy, int(rounds)
        self.num_envs = n = int(env.num_envs)
        init = torch.tensor(self.cfg.init_action, dtype=torch.int64, device=env.device).repeat(n, 1)
        start = S.poses_from_actions(init, self.cfg).float()
        self.last_plan = pool_policy.plan_route(self.rounds, start=start, covered_bits=torch.zeros_like(env.updater.scanned_bits))
        self._rows = torch.arange(n, device=env.device)

    def __call__(self, obs, deterministic: bool = True):
        slot = (self.env.episode_length_buf.clamp(min=1, max=self.rounds) - 1)
        return self.last_plan.actions[self._rows, slot], None, None

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state
