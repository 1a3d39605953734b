"""GPU: the data-parallel FUSED update (`PPO_Grid_Obs._dp_step_body`: phase A -> gradient all-reduce overlapped with the
conv-stack backward -> small all-reduce -> clip + Adam) with the statistics SURVEY 8e requires to be global --
per-minibatch advantage mean / std, BatchNorm-1 and BatchNorm-2 batch statistics IN TRAIN MODE and their backward sums, the
approx-KL of the early stop -- against the single-process update of the global batch.

The ranks (2, 4 and 8: the target world size of BASELINE configs[3]) share cuda:0 on a one-GPU box (world 8 needs a GPU per rank)
and talk over gloo on CUDA tensors; the collectives therefore run eagerly (RCCL refuses two ranks on one device, gloo cannot be captured) -- the same
`_dp_step_body` the bench replays as one hipGraph with RCCL collectives on a multi-GPU node.  With `use_graph=True` the capture of
the gloo collectives is REFUSED, which is exactly the fallback the algorithm must survive: the refused capture is abandoned and the same
step runs as eager launches, sharded update included (the `graph=True` case below)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G, N_LOCAL, T, B_LOCAL, EPOCHS = 16, 8, 4, 8, 2
HW = (48, 64)
# "g64" (round 6): the TIMED kernel set -- G = 64, 64 rows per rank and minibatch (the global minibatch of 128 is the
# bench's), the split-f16 conv kernels, the LDS-DMA weight gradient -- with two ranks
SHAPES = {"g16": (16, 8, 4, 8), "g64": (64, 16, 8, 64)}


def _set_shape(name):
    global G, N_LOCAL, T, B_LOCAL
    G, N_LOCAL, T, B_LOCAL = SHAPES[name]


def _cfg():
    from gennbv_amd.env.config import TaskConfig
    return TaskConfig(camera_width=HW[1], camera_height=HW[0], grid_size=G)


def _kwargs(cfg):
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    return dict(net_arch=[], features_extractor_class=Hybrid_Encoder, features_extractor_kwargs=dict(
        encoder_param={"hidden_shapes": [256, 256], "visual_dim": 256},
        net_param={"transformer_params": [[1, 256], [1, 256]], "append_hidden_shapes": [256, 256]},
        state_input_shape=(cfg.state_dim,), visual_input_shape=(cfg.stack, HW[0], HW[1])))


def _algo(env, batch, target_kl, epochs=EPOCHS):
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    return PPO_Grid_Obs(ActorCriticPolicy_Train_Eval, env, learning_rate=1e-4, n_steps=T, batch_size=batch, n_epochs=epochs, gamma=0.99,
                        gae_lambda=0.95, clip_range=0.2, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.8, max_grad_norm=1.0, target_kl=target_kl,
                        seed=1, device=DEV, compact_obs=True, policy_kwargs=_kwargs(_cfg()))


class _StubEnv:
    """The attributes PPO_Grid_Obs needs to build a policy + compact rollout buffer (no stepping)."""
    supports_grid_i8, device, max_episode_length = True, DEV, 6

    def __init__(self, n):
        from tests import policy_util as pu
        from gennbv_amd.spaces import Box, MultiDiscrete
        cfg = _cfg()
        self.num_envs = n
        self.observation_space = Box(-np.inf, np.inf, (cfg.obs_dim,))
        self.action_space = MultiDiscrete(pu.NVEC)

    def seed(self, s):
        pass


FIELDS = ("observations", "grid_i8", "autocorr", "actions", "values", "log_probs", "advantages", "returns", "rewards")


def _fill(algo, blob, envs):
    buf = algo.rollout_buffer
    for k in FIELDS:
        getattr(buf, k).copy_(blob[k][:, envs].to(DEV))
    buf.step, buf.full = T, True
    algo.policy.load_state_dict({k: v.to(DEV) for k, v in blob["policy"].items()})


def _local_to_global(perm, rank):
    """local flat index i = n*T + t of rank r (n < N_LOCAL) -> the global buffer's flat index (r*N_LOCAL + n)*T + t"""
    return (rank * N_LOCAL + perm // T) * T + perm % T


def _worker(rank, WORLD, path, port, target_kl, out, shard=True, graph=False, epochs=EPOCHS, shape="g16"):  # noqa: N803
    import time
    tm = [time.time()]
    _set_shape(shape)
    if torch.cuda.device_count() >= WORLD > 1:
        # a node with a GPU per rank: every rank on ITS OWN device (what the ranks are in a real run) -- nothing is oversubscribed there,
        # so nothing below may be excused
        global DEV
        DEV = _StubEnv.device = f"cuda:{rank}"
        torch.cuda.set_device(DEV)
    torch.set_num_threads(1)  # WORLD processes on one host: the CPU-side initialisers (orthogonal_ ...) must not each spin up a full thread pool
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    tm.append(time.time())
    from gennbv_amd import parallel
    blob = torch.load(path, weights_only=False)
    tm.append(time.time())
    algo = _algo(_StubEnv(N_LOCAL), B_LOCAL, target_kl, epochs)
    tm.append(time.time())
    _fill(algo, blob, list(range(rank * N_LOCAL, (rank + 1) * N_LOCAL)))
    tm.append(time.time())
    algo.rollout_buffer.indices = blob["perm"].copy()  # the same permutation on every rank, over its own rows
    algo.use_graph = graph
    algo.shard_update = shard
    parallel.attach(algo, WORLD)
    torch.cuda.synchronize()
    tm.append(time.time())
    algo.train()
    torch.cuda.synchronize()
    tm.append(time.time())
    assert algo.policy.features_extractor._dp_sync is not None and algo.policy.features_extractor.training
    opt = algo._hip["opt"]
    if graph:  # gloo collectives cannot be captured: the fallback (eager launches of the same step) must have been taken, on every rank alike
        assert str(getattr(algo, "dp_graph_mode", "")).startswith("eager launches"), getattr(algo, "dp_graph_mode", None)
        assert algo._hip["graph"] is None and algo._hip.get("graph_refused")
    assert (getattr(opt, "shard", None) is not None) == shard
    if shard:
        # fc_grid.weight: reduce-scattered, updated by its owner, all-gathered.  The Adam moments exist on their OWNER during the steps
        # and are gathered into every rank's flat buffers at the end of train() (a point all ranks pass together), so that
        # get_parameters() / save() are NOT collective: rank 0 alone calls it below, which would hang if it were
        sh = opt.shard
        assert sh["hi"] - sh["lo"] == algo.policy.features_extractor.output_layer_grid[0].weight.numel() and sh["sh"] * WORLD == sh["hi"] - sh["lo"]
        assert sh["rank"] == rank and sh["world"] == WORLD
        for r in range(WORLD):  # every rank's shard of the moments is present (non-zero) everywhere after train()
            assert float(opt.exp_avg_sq[sh["lo"] + r * sh["sh"]:sh["lo"] + (r + 1) * sh["sh"]].abs().max()) > 0.0, (rank, r)
        if rank == 0:
            sd = algo.get_parameters()["policy.optimizer"]
            assert len(sd["state"]) > 0
        mom = torch.cat((opt.exp_avg, opt.exp_avg_sq))
        allm = [torch.zeros_like(mom) for _ in range(WORLD)]
        dist.all_gather(allm, mom)
        assert all(torch.equal(allm[0], m) for m in allm[1:]), "Adam moments differ between the ranks after train()"
    vec = torch.cat([p.detach().reshape(-1) for p in algo.policy.parameters()])
    bn = torch.cat([b.detach().reshape(-1).float() for b in algo.policy.buffers()])
    both = [torch.zeros_like(vec) for _ in range(WORLD)]
    dist.all_gather(both, vec)
    if rank == 0:
        out["identical"] = all(bool(torch.equal(both[0], b)) for b in both[1:])
        out["params"], out["bn"] = vec.cpu().numpy(), bn.cpu().numpy()
        out["stats"] = algo.last_train_stats.copy()
        out["steps"] = int(algo._hip["opt"].step_count.item())
        out["phase_s"] = [round(b - a, 2) for a, b in zip(tm, tm[1:] + [time.time()])]  # rendezvous, import + load, build, fill, attach, train(), checks
    dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,target_kl,shard,graph,shape", [(2, None, True, False, "g16"), (2, "auto", True, False, "g16"), (2, None, False, False, "g16"),
                                                               (4, "auto", True, False, "g16"), (8, None, True, False, "g16"),
                                                               (2, "auto", True, True, "g16"), (2, None, True, False, "g64")])
def test_multi_rank_fused_update_equals_the_global_batch_update(tmp_path, world, target_kl, shard, graph, shape):
    """world 4 / 8: the fc_grid.weight shard boundaries (110 592 weights over 4 / 8 owners), gather_shard_state and the stop position at
    the target world size.  graph=True: the capture of the (gloo) collectives is refused -> eager launches of the same step, with 2 ranks."""
    WORLD = world  # noqa: N806
    if WORLD >= 8 and torch.cuda.device_count() < WORLD:
        # eight ranks and this process on ONE device are more processes than a shared GPU may have open: world 8 runs one rank per GPU
        pytest.skip("needs %d GPUs (one per rank), found %d" % (WORLD, torch.cuda.device_count()))
    epochs = EPOCHS
    _set_shape(shape)
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = _cfg()
    n = WORLD * N_LOCAL
    scene = S.make_scenes(n, G, seed=3, device=DEV)
    env = ReplayFeedEnv(cfg, scene, ReplayFeed.synthetic(scene, cfg, 5, seed=3), DEV, max_episode_length=6)
    ref = _algo(env, WORLD * B_LOCAL, None, epochs)
    ref._setup_learn(total_timesteps=10 ** 9)
    ref.collect_rollouts(env, None, ref.rollout_buffer, n_rollout_steps=T)
    buf = ref.rollout_buffer
    assert buf.autocorr is not None and buf.compact_state_dim is not None
    perm = np.random.RandomState(7).permutation(T * N_LOCAL)
    blob = {k: getattr(buf, k).detach().cpu().clone() for k in FIELDS}
    blob["policy"] = {k: v.detach().cpu().clone() for k, v in ref.policy.state_dict().items()}
    blob["perm"] = perm
    path = str(tmp_path / "rollout.pt")
    torch.save(blob, path)
    # the global minibatch k = rank 0's minibatch k ++ rank 1's minibatch k
    glob = np.concatenate([np.concatenate([_local_to_global(perm[k * B_LOCAL:(k + 1) * B_LOCAL], r) for r in range(WORLD)])
                           for k in range(T * N_LOCAL // B_LOCAL)])
    buf.indices = glob

    def run_ref(tkl):
        ref.policy.load_state_dict({k: v.to(DEV) for k, v in blob["policy"].items()})
        ref.target_kl, ref._hip = tkl, None
        ref.policy.optimizer = torch.optim.Adam(ref.policy.parameters(), lr=1e-4, eps=1e-5)
        ref.use_graph = False
        ref.train()
        return ref.last_train_stats.copy()
    stats = run_ref(None)
    if target_kl == "auto":  # a threshold the KL trace crosses in the second epoch: both sides must stop at the same minibatch
        kl = stats[:, 3]
        j = int(np.argmax(kl))
        assert j >= 1
        target_kl = float(0.5 * (kl[j] + np.max(kl[:j])) / 1.5)
        stats = run_ref(target_kl)
        assert len(stats) == j + 1
    want = torch.cat([p.detach().reshape(-1) for p in ref.policy.parameters()]).cpu().numpy()
    want_bn = torch.cat([b.detach().reshape(-1).float() for b in ref.policy.buffers()]).cpu().numpy()
    steps = int(ref._hip["opt"].step_count.item())
    out = mp.get_context("spawn").Manager().dict()  # (a spawned manager never holds the device open; a forked one would)
    import time
    t0 = time.time()
    mp.spawn(_worker, args=(WORLD, path, _free_port(), target_kl, out, shard, graph, epochs, shape), nprocs=WORLD, join=True)
    print("world %d: spawn..join %.1f s; rank 0 phases (rendezvous, import+load, build, fill, attach, train, checks) %s" % (WORLD, time.time() - t0, out.get("phase_s")))
    assert out["identical"], "ranks diverged"
    assert out["steps"] == steps and len(out["stats"]) == len(stats)  # same early-stop position
    # the ranks log the terms of their own rows; the KL (col 3) they act on is the global mean: check it through the stop position,
    # and the local means average to the global ones only for rank-symmetric terms -- compare the outcome instead:
    np.testing.assert_allclose(out["bn"], want_bn, rtol=2e-5, atol=2e-6)  # BatchNorm running statistics = global-batch statistics
    d = np.abs(out["params"] - want)
    assert np.quantile(d, 0.999) <= 2e-6 and d.max() <= 1e-4 * 1.05 * max(steps, 1), (np.quantile(d, 0.999), d.max())
