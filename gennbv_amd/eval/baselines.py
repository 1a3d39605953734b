"""Baseline view planners to compare a learned policy against: a uniformly random lattice pose, the greedy
next-best-view planner over the view gain (ops/view_gain.py, csrc/viewgain.hip; grids up to 128^3), the one-step
oracle over the view coverage (ops/view_cover.py, csrc/viewcover.hip): the candidate that really adds the most
ground-truth voxels, and the greedy set-cover planner over a fixed pool of views whose visible ground truth is cached
as bit masks (ops/view_pool.py, csrc/covergreedy.hip).

All speak the protocol `evaluate_policy_grid_obs` uses: `.policy(obs, deterministic=True) -> (actions, None, None)`,
and `predict(obs)`; actions are int64 [N,6] on the lattice of the task (inside clip_pose_idx_low / clip_pose_idx_up).
"""
from __future__ import annotations

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
    k = gain.shape[1]
    score = int(weights[0]) * gain[..., 0].to(torch.int64) + int(weights[1]) * gain[..., 1].to(torch.int64)
    if contact is not None:
        score = torch.where(contact != 0, torch.full_like(score, -1), score)
    # one key per candidate, strictly larger for the lower index at equal score: argmax has a single answer
    key = score * k + (k - 1 - torch.arange(k, device=score.device))
    return key.argmax(dim=1)


class GreedyGainPolicy:
    """Greedy next-best view: K random lattice candidates per env and step, the one with the largest
    w0 * unknown + w1 * unknown_hit of the view gain against the observation's grid wins; with a CollisionBody on the
    env (and `avoid_collisions`) candidates whose pose collides are never chosen unless all do; where that body has `sweep`,
    a candidate whose straight flight from `env.poses` is blocked (MeshScene.sweep_candidates, accumulated into the same
    contact buffer) counts exactly like one in contact -- that needs a collision mesh with `sweep_candidates`; where the env also
    flies detours (`env.flight`) only a candidate that no route reaches is refused for its path (`candidate_contact`).  No host
    synchronisation inside a decision.  `gain_backend(tri [N,G^3], poses [N,K,6]) -> gain [N,K,3]` replaces the kernel in
    tests only: the product path has no CPU fallback."""

    def __init__(self, env, k: int = 32, weights=(1, 4), seed: int = 0, stride: int = 4, avoid_collisions: bool = True,
                 look_at_scene: bool = False, gain_backend: Optional[Callable] = None):
        cfg = env.cfg
        self.env, self.cfg, self.k, self.weights = env, cfg, int(k), (int(weights[0]), int(weights[1]))
        self.num_envs = int(env.num_envs)
        self.cands = LatticeCandidates(cfg, k, seed, look_at_scene)
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

    def __call__(self, obs, deterministic: bool = True):
        cfg, n, k = self.cfg, self.num_envs, self.k
        cand = self.cands.sample(n, obs.device)
        poses = self.cands.poses(cand)
        tri = obs[:, cfg.state_dim:cfg.state_dim + cfg.grid_dim]
        gain = self.gain_backend(tri, poses)
        self.last_gain = gain
        contact = None
        if self.avoid_collisions:
            mesh = self.env.collision_mesh
            if hasattr(mesh, "collide_candidates"):  # all N x K poses in one launch
                if self._contact is None:
                    self._contact = torch.zeros(n, k, dtype=torch.uint8, device=obs.device)
                contact = candidate_contact(self.env, poses, self._contact, self.sweep)  # | the flight from the current pose
            else:
                if self._contact is None:
                    self._contact = torch.zeros(k, n, dtype=torch.uint8, device=obs.device)
                for j in range(k):  # one call per candidate column ([N,6] rows, stride K * 6)
                    mesh.collide(poses[:, j], self.env.collision, out=self._contact[j])
                contact = self._contact.t()
        best = choose(gain, self.weights, contact)
        return cand[torch.arange(n, device=cand.device), best], None, None

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
        best = choose(cover, (1, 0), contact)
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
    set; it keeps the static contact (an offline plan has no "current pose" per round, so no flight is tested).  No host
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

    @property
    def policy(self):
        return self

    def predict(self, obs, state=None, episode_start=None, deterministic: bool = True):
        return self(obs, deterministic)[0], state
