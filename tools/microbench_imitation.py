"""Two timings of DESIGN.md "Imitation from the planners" (device events around warmed, repeated work; the two sides of a comparison
alternate inside one process).

    python tools/microbench_imitation.py [--reps 200] [--rounds 5] [--g 64] [--b 128] [--steps 20] [--skip-step]

1. The loss kernel (gnbv_imitation_loss) at B = 128, heads [81, 81, 51, 1, 13, 13], K in {1, 32}, against the torch expression of the
   same loss and its gradient to the logits (per-head log_softmax, scatter_add of the marginal, autograd), each `reps` calls per round.
2. One behaviour-cloning minibatch (BehaviourCloning.fit: gather -> encoder -> head -> loss -> backward -> clip + Adam) at G^3 with
   batch B on synthetic demonstrations, against one eager PPO minibatch of tools/microbench_train.py's step (evaluate_actions + the PPO
   loss in torch + clip_grad_norm_ + torch Adam) on the HIP encoder.
Prints one JSON line per measurement; medians over the rounds, with the spread.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
SIX = [81, 81, 51, 1, 13, 13]


def timed(fn, reps):
    """ms per call: device events around `reps` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(sides, reps, rounds):
    """{name: (median ms, min, max)} of the sides, timed in turn `rounds` times after a warm-up of each."""
    for fn in sides.values():
        timed(fn, max(3, reps // 10))
    got = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            got[k].append(timed(fn, reps))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in got.items()}


def bench_kernel(k, reps, rounds, b=128):
    from gennbv_amd import _lib
    from gennbv_amd.ops.imitation_ops import ImitationLossOp
    from types import SimpleNamespace
    gen = torch.Generator(device=DEV).manual_seed(k)
    n = sum(SIX)
    logits = torch.randn(b, n, generator=gen, device=DEV) * 2
    values, returns = torch.randn(b, generator=gen, device=DEV), torch.randn(b, generator=gen, device=DEV)
    cand = torch.stack([torch.randint(0, d, (b, k), generator=gen, device=DEV) for d in SIX], 2).contiguous()
    cw = (torch.rand(b, k, generator=gen, device=DEV) + 0.05).contiguous()
    sw = (torch.rand(b, generator=gen, device=DEV) + 0.1).contiguous()
    eps, ec, vf = 0.1, 0.01, 0.5
    op = ImitationLossOp(b, SIX, k, DEV, 1, eps, ec, vf)
    op.bind(SimpleNamespace(cand=cand, cand_w=cw, sample_w=sw, returns=returns))
    op.rows.copy_(torch.arange(b, device=DEV))

    def hip():
        op.stats_row.zero_()
        return op(logits, values)

    qn = cw / cw.sum(1, keepdim=True)
    offs = np.cumsum([0] + SIX)

    def eager():
        x = logits.detach().requires_grad_()
        v = values.detach().requires_grad_()
        per = vf * (v - returns) ** 2
        for h, d in enumerate(SIX):
            lp = torch.log_softmax(x[:, offs[h]:offs[h + 1]], 1)
            m = torch.zeros(b, d, device=DEV).scatter_add_(1, cand[:, :, h], qn) * (1 - eps) + eps / d
            per = per - (m * lp).sum(1) + ec * (lp.exp() * lp).sum(1)
        loss = (sw * per).sum() / sw.sum()
        return torch.autograd.grad(loss, (x, v))

    d_hip, d_eager = hip()[0].clone(), eager()[0]
    torch.cuda.synchronize()
    res = alternate({"hip": hip, "torch": eager}, reps, rounds)
    print(json.dumps({"what": "imitation loss + gradient", "B": b, "heads": SIX, "K": k, "reps": reps, "rounds": rounds,
                      "hip_us": [round(1e3 * t, 2) for t in res["hip"]], "torch_us": [round(1e3 * t, 2) for t in res["torch"]],
                      "note": "hip_us includes a 1-element memset of stats_row per call",
                      "max_abs_diff_d_logits": float((d_hip - d_eager).abs().max())}), flush=True)


def bench_step(g, b, steps, rounds):
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.config import TaskConfig
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    from gennbv_amd.sb3.imitation import BehaviourCloning, Demonstrations
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    from tests import policy_util as pu
    cfg = TaskConfig(camera_width=80, camera_height=60, grid_size=g)
    scene = S.make_scenes(4, g, seed=4, device=DEV)
    env = ReplayFeedEnv(cfg, scene, ReplayFeed.synthetic(scene, cfg, 2, seed=4), DEV, max_episode_length=8)
    kw = dict(net_arch=[], features_extractor_class=Hybrid_Encoder, features_extractor_kwargs=dict(
        encoder_param={"hidden_shapes": [256, 256], "visual_dim": 256},
        net_param={"transformer_params": [[1, 256], [1, 256]], "append_hidden_shapes": [256, 256]},
        state_input_shape=(cfg.state_dim,), visual_input_shape=(cfg.stack, cfg.camera_height, cfg.camera_width)))
    model = PPO_Grid_Obs(ActorCriticPolicy_Train_Eval, env, learning_rate=1e-4, n_steps=8, batch_size=b, n_epochs=1, seed=1, device=DEV,
                         policy_kwargs=kw)
    gen = torch.Generator(device=DEV).manual_seed(0)
    m, k = b * steps, 32
    demos = Demonstrations(m, m, cfg.state_dim, cfg.grid_dim, cfg.obs_dim - cfg.state_dim - cfg.grid_dim, k, 6, DEV)
    demos.small.copy_(torch.randn(demos.small.shape, generator=gen, device=DEV) * 0.3)
    demos.grid_i8.copy_(torch.randint(-1, 2, demos.grid_i8.shape, generator=gen, device=DEV))
    demos.cand.copy_(torch.stack([torch.randint(0, d, (m, k), generator=gen, device=DEV) for d in SIX], 2))
    demos.cand_w.copy_(torch.rand(m, k, generator=gen, device=DEV) + 0.05)
    demos.sample_w.fill_(1.0)
    demos.returns.copy_(torch.randn(m, generator=gen, device=DEV))
    demos._finish_block(demos.block_slice())
    bc = BehaviourCloning(model, demos, b, 1e-4, 1, seed=0, label_smoothing=0.1, ent_coef=0.01, vf_coef=0.5, max_grad_norm=1.0)
    compact = bc._compact_input(model.policy.features_extractor)

    # the eager PPO minibatch of tools/microbench_train.py, on a policy of its own
    pol, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=False)
    obs = torch.zeros(b, pu.obs_dim(g), device=DEV)
    obs[:, 600:600 + g ** 3] = torch.randint(-1, 2, (b, g ** 3), device=DEV).float()
    actions = torch.stack([torch.randint(0, n, (b,), device=DEV) for n in pu.NVEC], -1).float()
    adv, ret, oldv = torch.randn(b, device=DEV), torch.randn(b, device=DEV), torch.randn(b, device=DEV)
    oldlp = torch.full((b,), -17.0, device=DEV)

    def ppo_step():
        pol.set_training_mode(True)
        values, log_prob, entropy = pol.evaluate_actions(obs, actions)
        values = values.float().flatten()
        advn = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(log_prob.float() - oldlp)
        pg = -torch.min(advn * ratio, advn * torch.clamp(ratio, 0.8, 1.2)).mean()
        vp = oldv + torch.clamp(values - oldv, -0.2, 0.2)
        loss = 10 * pg + 0.01 * (-entropy.float().mean()) + 0.8 * torch.nn.functional.mse_loss(ret, vp)
        pol.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), 1.0)
        pol.optimizer.step()

    def ppo_steps():
        for _ in range(steps):
            ppo_step()
    bc.fit()
    ppo_steps()
    torch.cuda.synchronize()
    # (a fit() is `steps` minibatches, its permutation and its one read-back: host clock around it, the read-back synchronises)
    import time
    got = {"bc": [], "ppo_eager": []}
    for _ in range(rounds):
        t0 = time.perf_counter()
        bc.fit()
        torch.cuda.synchronize()
        got["bc"].append((time.perf_counter() - t0) / steps * 1e3)
        t0 = time.perf_counter()
        ppo_steps()
        torch.cuda.synchronize()
        got["ppo_eager"].append((time.perf_counter() - t0) / steps * 1e3)
    print(json.dumps({"what": "one minibatch", "G": g, "B": b, "K": k, "steps_per_round": steps, "rounds": rounds, "compact_rows": bool(compact),
                      "bc_ms": [round(float(np.median(got["bc"])), 4), round(min(got["bc"]), 4), round(max(got["bc"]), 4)],
                      "ppo_eager_ms": [round(float(np.median(got["ppo_eager"])), 4), round(min(got["ppo_eager"]), 4), round(max(got["ppo_eager"]), 4)]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--g", type=int, default=64)
    ap.add_argument("--b", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_imitation needs a GPU")
    for k in (1, 32):
        bench_kernel(k, args.reps, args.rounds)
    if not args.skip_step:
        bench_step(args.g, args.b, args.steps, args.rounds)


if __name__ == "__main__":
    main()
