"""Closed-loop table of DESIGN.md "Imitation from the planners".

    python tools/closed_loop_bc.py [--envs 8] [--grid 20] [--steps 20] [--k 32] [--teacher oracle|greedy] [--collect 40]
                                   [--epochs 4] [--iterations 4] [--temperature 0.05] [--lr 3e-4] [--seed 1] [--out FILE.json]

The set-up of tools/closed_loop_view_cover.py: RenderFeed(MeshScene.from_boxes(make_scenes(envs, grid, seed=1))), 60 x 80 camera,
`steps`-step episodes, K candidates per decision of the teacher.  One policy (PPO_Grid_Obs's, default initialisation) is trained from
the same initial state three ways on a training env -- behaviour cloning on hard labels, on soft targets, and DAgger (beta = 1, 1/2,
1/4, ..; every iteration adds `collect` steps x envs demonstrations) -- and each is flown, deterministic, for one episode per env on a
ReplayFeedEvalEnv beside the random policy, the teacher and the untrained policy.  Per row: final coverage (mean over envs of
coverage_ratio on each env's done step), mean_AUC (evaluate_policy_grid_obs) and agreement with the teacher: the share of
(env, step) decisions, fresh rows aside, at which the flown action equals on every head the action a teacher with the row's seed picks
at the same observation.  The figures are reported, not asserted.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gennbv_amd.env import synthetic as S  # noqa: E402
from gennbv_amd.env.config import TaskConfig  # noqa: E402
from gennbv_amd.env.mesh_scene import MeshScene  # noqa: E402
from gennbv_amd.env.render_feed import RenderFeed  # noqa: E402
from gennbv_amd.env.replay_feed import ReplayFeedEnv  # noqa: E402
from gennbv_amd.env.replay_feed_eval import ReplayFeedEvalEnv  # noqa: E402
from gennbv_amd.eval import evaluate_policy_grid_obs  # noqa: E402
from gennbv_amd.eval.baselines import GreedyGainPolicy, OracleGainPolicy, RandomLatticePolicy  # noqa: E402

DEV = "cuda:0"


def make_teacher(name, env, k, seed):
    return OracleGainPolicy(env, k=k, seed=seed) if name == "oracle" else GreedyGainPolicy(env, k=k, weights=(1, 4), seed=seed)


class Watched:
    """A policy flown beside a teacher that is asked at the same observations: counts the decisions on which both agree."""

    def __init__(self, flown, teacher, env):
        self.flown, self.teacher, self.env, self.same, self.asked = flown, teacher, env, 0, 0

    def __call__(self, obs, deterministic=True):
        a = self.flown(obs, deterministic=deterministic)[0].to(torch.int64)
        if self.teacher is not None:
            t = self.teacher.policy(obs, deterministic=True)[0]
            live = self.env.episode_length_buf != 0
            self.same += int(((a == t).all(1) & live).sum())
            self.asked += int(live.sum())
        return a, None, None

    @property
    def policy(self):
        return self


def fly(flown, teacher, env):
    n = env.num_envs
    final = {}

    def cb(loc, _):
        i = loc["i"]
        if bool(loc["done"]) and i not in final:
            final[i] = float(env.coverage_ratio[i])
    w = Watched(flown, teacher, env)
    _, lens, auc, _ = evaluate_policy_grid_obs(w, env, n_eval_episodes=n, callback=cb)
    return {"episodes": n, "final_coverage": float(np.mean([final[i] for i in range(n)])), "mean_AUC": float(auc.mean()),
            "mean_length": float(np.mean(lens)), "agreement": (w.same / max(1, w.asked)) if teacher is not None else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--teacher", default="oracle", choices=("oracle", "greedy"))
    ap.add_argument("--collect", type=int, default=40, help="env steps per collected block")
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=4, help="DAgger iterations = blocks of the two BC runs")
    ap.add_argument("--temperature", type=float, default=0.05)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_bc needs a GPU")
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    from gennbv_amd.sb3.imitation import BehaviourCloning, collect_demonstrations, dagger
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    n, g = args.envs, args.grid
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(n, g, seed=1)
    mesh = MeshScene.from_boxes(scene, device=DEV)
    train_env = ReplayFeedEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps)
    kw = dict(net_arch=[], features_extractor_class=Hybrid_Encoder, features_extractor_kwargs=dict(
        encoder_param={"hidden_shapes": [256, 256], "visual_dim": 256},
        net_param={"transformer_params": [[1, 256], [1, 256]], "append_hidden_shapes": [256, 256]},
        state_input_shape=(cfg.state_dim,), visual_input_shape=(cfg.stack, cfg.camera_height, cfg.camera_width)))
    model = PPO_Grid_Obs(ActorCriticPolicy_Train_Eval, train_env, learning_rate=1e-4, n_steps=args.collect, batch_size=args.batch, n_epochs=1,
                         seed=args.seed, device=DEV, policy_kwargs=kw)
    init = {k: v.detach().clone() for k, v in model.policy.state_dict().items()}
    trainer_kw = dict(batch_size=args.batch, learning_rate=args.lr, n_epochs=args.epochs, seed=args.seed, max_grad_norm=1.0)
    res = {"envs": n, "grid": g, "steps": args.steps, "k": args.k, "teacher": args.teacher, "collect_steps": args.collect,
           "blocks": args.iterations, "demonstrations": args.iterations * args.collect * n, "epochs": args.epochs, "lr": args.lr,
           "temperature": args.temperature, "rows": []}

    def row(name, flown, extra=None):
        env = ReplayFeedEvalEnv(cfg, scene, RenderFeed(mesh, cfg), DEV, max_episode_length=args.steps)
        if flown == "teacher":
            r = fly(make_teacher(args.teacher, env, args.k, args.seed), None, env)
            r["agreement"] = 1.0
        else:
            if flown is model:
                model.policy.set_training_mode(False)
            r = fly(flown.policy, make_teacher(args.teacher, env, args.k, args.seed), env)
        r = dict({"policy": name}, **r, **(extra or {}))
        print(json.dumps(r), flush=True)
        res["rows"].append(r)

    row("random", RandomLatticePolicy(cfg, n, args.seed))
    row("teacher", "teacher")
    row("untrained", model)
    for name, soft in (("bc_hard", False), ("bc_soft", True)):
        model.policy.load_state_dict(init)
        teacher = make_teacher(args.teacher, train_env, args.k, args.seed + 10)
        demos = None
        for i in range(args.iterations):
            demos = collect_demonstrations(model, train_env, teacher, args.collect, 1.0, args.seed + i, soft=soft,
                                           temperature=args.temperature if soft else None, demos=demos, capacity_blocks=args.iterations)
        stats = BehaviourCloning(model, demos, **trainer_kw).fit()
        row(name, model, {"train_ce": [float(stats[0, 0]), float(stats[-1, 0])], "train_agreement": [float(stats[0, 3]), float(stats[-1, 3])],
                          "fit_steps": int(len(stats))})
    model.policy.load_state_dict(init)
    teacher = make_teacher(args.teacher, train_env, args.k, args.seed + 10)
    betas = [0.5 ** i for i in range(args.iterations)]
    out = dagger(model, train_env, teacher, args.iterations, args.collect, betas, trainer_kw, seed=args.seed, soft=True, temperature=args.temperature)
    row("dagger", model, {"betas": betas, "train_ce": [float(out[0][0, 0]), float(out[-1][-1, 0])],
                          "train_agreement": [float(out[0][0, 3]), float(out[-1][-1, 3])], "fit_steps": int(sum(len(o) for o in out))})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
