"""bench.py -- env-steps/sec of the GenNBV state-encoding + PPO hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W      (N > 1 without a launcher environment: starts its N ranks itself, self_launch())
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic input = one PPO
iteration of BASELINE.json configs[1]: 256 envs x 240x320 depth x 64^3 grid,
n_steps=128 env steps (state encoding + policy forward + buffer add per env step),
the GAE scan, and PPO_Grid_Obs.train() (5 epochs x minibatch 128).  The metric is
whole-job env-steps/sec = N_gpus * 256 * 128 * K / time(K iterations); envs shard
across ranks (weak scaling), gradients are all-reduced over RCCL.

Inputs are resident in HBM when the timed region starts (a pool of pre-rendered
synthetic frames).  Rank 0 prints ONE JSON line.

A plain run does what the headline needs: set up, warm up, time the K steps, write
--dump-outputs, print the line (with the figures taken from the timed steps
themselves: per-iteration times, phase breakdown, voxel and minibatch rooflines).
`--full` adds everything that takes work of its own after the timed steps: the
oracle replay of the last timed rollout (timed_state_check), the encoder roofline,
the PPO loss delta vs the reference, the CPU baseline, the flat-row measurement,
the device's rocm-smi clocks and, with N > 1, the exchange probe.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=256, help="envs per GPU")
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--n-epochs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8, help="frames in the synthetic feed pool")
    ap.add_argument("--backend", default="hip", choices=["hip", "torch"])
    ap.add_argument("--obs", default="compact", choices=["flat", "compact"],
                    help="rollout-buffer rows: the reference's flat fp32 rows, or compact rows (grid as int8 only; same values)")
    ap.add_argument("--target-kl", default="off", help="'off' (default): the KL early stop of PPO_Grid_Obs.train (ppo_grid_obs.py:261-268) can never "
                    "trigger, so every timed iteration runs all n_epochs x minibatches (the check itself still runs on the device); "
                    "'ref': the reference's 0.05, under which a random-init policy on the synthetic feed stops some iterations early")
    ap.add_argument("--semantic", action="store_true", help="BASELINE configs[2]: the opt-in semantic branch over the two gray frames "
                    "(Hybrid_Encoder(semantic_branch=True): build-defined, the released reference never reads them)")
    ap.add_argument("--full", action="store_true", help="after the headline, also run the checks and measurements a plain run leaves out "
                    "(state check, encoder roofline, PPO loss delta vs the reference, CPU baseline, flat rows, rocm-smi clocks, exchange probe)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-flat-rows", action="store_true", help="with --full: skip the second, shorter measurement with the reference's flat fp32 rows")
    ap.add_argument("--no-state-check", action="store_true", help="with --full: skip the oracle replay of sampled envs over the last timed rollout")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (rollout buffer, trained policy state, per-minibatch "
                         "training statistics) as DIR/<name>.npy, to compare two builds output for output")
    return ap.parse_args()


def build_algo(args, device, rank, world):
    import torch
    if args.grid % 16 != 0 and args.obs == "compact":
        # (the int8 grid rows / compact observations need G % 16 == 0; the reference's own default grid, 20^3, runs on flat fp32 rows)
        args.obs = "flat"
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.config import TaskConfig, PPOConfig
    from gennbv_amd.env.replay_feed import ReplayFeed, ReplayFeedEnv
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    if args.backend == "torch":  # A/B only: the test suite's plain-torch (MIOpen) reference encoder
        from tests.torch_reference import TorchHybridEncoder as Hybrid_Encoder
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs

    cfg = TaskConfig(camera_width=args.width, camera_height=args.height, grid_size=args.grid)
    pc = PPOConfig()
    scene = S.make_scenes(args.envs, args.grid, seed=1 + rank, device=device)
    feed = ReplayFeed.synthetic(scene, cfg, args.frames, seed=1 + rank, with_rgba=True)
    env = ReplayFeedEnv(cfg, scene, feed, device)
    algo = PPO_Grid_Obs(
        ActorCriticPolicy_Train_Eval, env, learning_rate=pc.learning_rate, n_steps=args.n_steps, batch_size=args.batch_size,
        n_epochs=args.n_epochs, gamma=pc.gamma, gae_lambda=pc.gae_lambda, clip_range=pc.clip_range,
        clip_range_vf=pc.clip_range_vf, ent_coef=pc.ent_coef, vf_coef=pc.vf_coef, max_grad_norm=pc.max_grad_norm,
        target_kl=pc.target_kl if args.target_kl == "ref" else 1e9, seed=1, device=device, compact_obs=args.obs == "compact",
        policy_kwargs=dict(net_arch=[], features_extractor_class=Hybrid_Encoder,
                           features_extractor_kwargs=dict(
                               encoder_param={"hidden_shapes": [256, 256], "visual_dim": 256},
                               net_param={"transformer_params": [[1, 256], [1, 256]], "append_hidden_shapes": [256, 256]},
                               state_input_shape=(cfg.state_dim,),
                               visual_input_shape=(cfg.stack, cfg.camera_height, cfg.camera_width),
                               **({"semantic_branch": True} if args.semantic and args.backend == "hip" else {}))))
    if world > 1 or os.environ.get("GENNBV_FORCE_DP") == "1":
        from gennbv_amd import parallel
        # GENNBV_FORCE_DP=1: run the data-parallel code path with a one-rank communicator (overhead check)
        parallel.attach(algo, world, always_sync=world == 1)
    return algo, cfg, env


class Phase:
    """Accumulates device time of a code region with events on the current stream."""

    def __init__(self):
        self.pairs = []

    def __enter__(self):
        import torch
        if getattr(self, "_pool", None):
            self.e0, self.e1 = self._pool.pop(), self._pool.pop()
        else:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
        self.e0.record()
        return self

    def __exit__(self, *a):
        self.e1.record()
        self.pairs.append((self.e0, self.e1))

    def reserve(self, n_pairs: int):
        """Create the events of `n_pairs` start() / stop() pairs NOW: a torch event gets its HIP event at its first record(), and the
        runtime grows its event / signal pools in steps -- a bench that times every voxel update creates 256 events per iteration, and the
        ~1000th creation inside the timed region cost one iteration ~100 ms (rounds 1-5 carried that in their averages; iteration_ms of
        round 6's first runs: 693 693 694 692 780 and 699 700 701 803 700 ...).  Recording each event once up front moves it out."""
        import torch
        if os.environ.get("GENNBV_BENCH_NO_RESERVE") == "1":  # (A/B of this very effect)
            return
        self._pool = getattr(self, "_pool", None) or []
        for _ in range(2 * n_pairs - len(self._pool)):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._pool.append(e)

    def start(self):
        import torch
        if not getattr(self, "_pool", None):  # (events created ahead of time: nothing but the record between the caller and its launch)
            self._pool = [torch.cuda.Event(enable_timing=True) for _ in range(64)]
        self.e0, self.e1 = self._pool.pop(), self._pool.pop()
        self.e0.record()

    def stop(self):
        self.__exit__()

    def total_ms(self):
        return sum(a.elapsed_time(b) for a, b in self.pairs)

    def count(self):
        return len(self.pairs)


def instrument_voxel(env):
    """HIP events around every gnbv_update_occ_grid call (same stream as the kernels), recorded immediately around the LIBRARY call
    (OccupancyGridUpdater.timing): the three launches, not the Python in front of them.  (Rounds 1-3 bracketed the Python method: on a
    launch-bound rollout the GPU reaches the first event ~12 us before the host has enqueued the first kernel, and that idle time was
    priced as kernel time -- 0.122 against 0.110 ms back to back, VERDICT r3 weak #2.)"""
    ph = Phase()
    upd = env.updater
    if hasattr(upd, "timing") and getattr(upd, "coded", False):
        upd.timing = ph
        return ph
    orig = upd.update

    def timed(*a, **k):
        with ph:
            return orig(*a, **k)
    upd.update = timed
    return ph


DUMP_SAMPLE = 1 << 20  # elements kept of an output larger than this: a fixed, seeded sample (keeps a dump far below 64 MB)


def dump_outputs(algo, out_dir: str) -> dict:
    """What one PPO iteration hands its caller, after the last timed one: the rollout buffer it filled (GAE included), the policy's
    state after train(), and train()'s per-minibatch statistics.  float64 stays float64, everything else is written as float32;
    arrays keep their shapes, except that those above DUMP_SAMPLE elements become a sample at flat indices drawn from RandomState(0),
    the same for every run of a shape."""
    import numpy as np
    import torch
    buf = algo.rollout_buffer
    arrays = {f"rollout_{k}": getattr(buf, k) for k in ("observations", "grid_i8", "actions", "rewards", "episode_starts", "values",
                                                       "log_probs", "advantages", "returns") if getattr(buf, k, None) is not None}
    arrays.update({"policy." + k: v for k, v in algo.policy.state_dict().items()})
    if getattr(algo, "last_train_stats", None) is not None:
        arrays["train_stats"] = torch.from_numpy(np.asarray(algo.last_train_stats))
    os.makedirs(out_dir, exist_ok=True)
    total, files = 0, 0
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.RandomState(0).randint(0, t.numel(), size=DUMP_SAMPLE, dtype=np.int64))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
            name += "_sample"
        a = t.cpu().numpy().astype(np.float64 if t.dtype in (torch.float64, torch.int64) else np.float32)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        total += a.nbytes
        files += 1
    assert total <= 64 << 20, f"--dump-outputs wrote {total} bytes"
    return {"dir": os.path.abspath(out_dir), "files": files, "bytes": total}


def one_iteration(algo, phases):
    import torch
    with phases["rollout"]:
        algo.collect_rollouts(algo.env, None, algo.rollout_buffer, n_rollout_steps=algo.n_steps)
    with phases["train"]:
        algo.train()


def cpu_baseline(args, cfg):
    """The CPU port of the same path on the box's host cores: the oracle's state encoding (oracle/oracle.c, OpenMP, one
    thread per env; proven equal to the reference on the goldens) + torch-CPU fp32 policy forward / GAE / PPO update
    (torch's thread pool at the count that is fastest on the host) on a bounded sample of the workload -- 64 envs x 8 env steps at the full 240x320 / G
    geometry, then one PPO epoch over the 512 samples in minibatches of 128 (the remaining n_epochs - 1 epochs are scaled
    from it).  kind = "port": the reference itself cannot travel to the GPU box (it imports Isaac Gym / pycuda)."""
    import numpy as np
    import torch
    from gennbv_amd.env import synthetic as S
    from oracle.env_oracle import OracleEnv
    from oracle import oracle as orc
    from tests import policy_util as pu

    n, t_steps, mb = 64, 8, 128
    host_cores = os.cpu_count() or 1
    # thread counts that are actually fastest on the box (measured on the 256-core host of the pool: one minibatch
    # forward + backward takes 0.60 / 0.53 / 0.62 / 0.98 s with 16 / 32 / 64 / 128 torch threads; with all 256 the epoch took
    # 74 s instead of ~3): torch 32 threads, the oracle one thread per env
    torch_threads = min(host_cores, 32)
    torch.set_num_threads(torch_threads)
    orc.lib().orc_set_num_threads(min(host_cores, n))
    omp_threads = int(orc.lib().orc_num_threads())
    cores = max(torch_threads, omp_threads)
    scene = S.make_scenes(n, cfg.grid_size, seed=99)
    frames = S.make_frames(scene, cfg, 2, seed=99)  # two frames, alternated
    kinv = S.inverse_intrinsics(cfg.camera_height, cfg.camera_width)
    env = OracleEnv(cfg, kinv.numpy(), scene.range_gt.numpy(), scene.voxel_size.numpy(), scene.grid_gt.numpy(),
                    scene.num_valid_voxel_gt.numpy())
    c2w = [S.c2w_from_view(f.view, scene.env_origins).numpy() for f in frames]
    pol, _, _ = pu.make_policy(g=cfg.grid_size, det_weights=False)
    pol.set_training_mode(False)
    t0 = time.time()
    obs = env.reset(frames[0].depth_raw.numpy(), frames[0].seg_raw.numpy(), frames[0].rgba.numpy(), c2w[0])
    obs_l, val_l, rew_l, act_l, lp_l = [], [], [], [], []
    for t in range(t_steps):
        with torch.no_grad():
            a, v, lp = pol(torch.from_numpy(obs))
        f = frames[(t + 1) % 2]
        nobs, rew, done, info = env.step(a.numpy(), f.depth_raw.numpy(), f.seg_raw.numpy(), f.rgba.numpy(), c2w[(t + 1) % 2])
        obs_l.append(obs); val_l.append(v.numpy().reshape(-1)); rew_l.append(rew); act_l.append(a.numpy()); lp_l.append(lp.numpy())
        obs = nobs
    with torch.no_grad():
        lv = pol.predict_values(torch.from_numpy(obs)).numpy().reshape(-1)
    adv, ret = orc.gae_sb3(np.stack(rew_l), np.stack(val_l), np.zeros((t_steps, n), np.uint8), lv, np.zeros(n, np.uint8))
    t_rollout = time.time() - t0
    # one PPO epoch over the n*t_steps samples in minibatches of `mb` (ppo_grid_obs.py:196-275)
    pol.set_training_mode(True)
    o = torch.from_numpy(np.concatenate(obs_l)); a = torch.from_numpy(np.concatenate(act_l)).float()
    advt = torch.from_numpy(adv.reshape(-1)); rett = torch.from_numpy(ret.reshape(-1))
    oldv = torch.from_numpy(np.concatenate(val_l)); oldlp = torch.from_numpy(np.concatenate(lp_l))
    t_train0 = time.time()
    for k in range(0, n * t_steps, mb):
        sl = slice(k, k + mb)
        values, log_prob, entropy = pol.evaluate_actions(o[sl], a[sl])
        values = values.flatten()
        advn = (advt[sl] - advt[sl].mean()) / (advt[sl].std() + 1e-8)
        ratio = torch.exp(log_prob - oldlp[sl])
        pg = -torch.min(advn * ratio, advn * torch.clamp(ratio, 0.8, 1.2)).mean()
        vp = oldv[sl] + torch.clamp(values - oldv[sl], -0.2, 0.2)
        loss = 10 * pg + 0.01 * (-entropy.mean()) + 0.8 * torch.nn.functional.mse_loss(rett[sl], vp)
        pol.optimizer.zero_grad(); loss.backward()
        torch.nn.utils.clip_grad_norm_(pol.parameters(), 1.0); pol.optimizer.step()
    t_train = time.time() - t_train0
    total = t_rollout + args.n_epochs * t_train
    return {"value": n * t_steps / total, "unit": "env-steps/s", "cores": int(cores), "host_cores": int(host_cores), "kind": "port, extrapolated",
            "sample": f"{n} envs x {t_steps} env steps at {cfg.camera_height}x{cfg.camera_width}, {cfg.grid_size}^3: oracle state "
                      f"encoding (OpenMP, {omp_threads} threads) + torch-CPU fp32 policy / GAE / PPO ({torch.get_num_threads()} threads; "
                      f"1 epoch of {n * t_steps // mb} minibatches of {mb} measured, x{args.n_epochs} epochs)",
            "seconds": {"rollout": t_rollout, "one_epoch": t_train}}


def ppo_loss_delta(args, device):
    """PPO loss delta vs the reference (BASELINE metric, second half), two measurements:

    * `reference_fixture`: train() of the same code path (hipGraph, fused kernels) on the recorded rollout of
      tests/golden/F9_ppo_train.npz against the losses the REFERENCE's own PPO_Grid_Obs.train() logged.  The reference
      hard-codes 20^3 (hybrid_encoder.py:47,90-91), so this runs the G = 20 kernel set, not the timed one;
    * `timed_kernel_set`: train() at the timed configuration's kernel set -- G = 64, minibatch 128, compact int8 rows,
      hipGraph (k_conv1_fwd_lds<int8>, analytic BN1, k_conv2_fwd, k_conv2_wgrad, k_conv2_dgrad_c1w, split-K fc_grid,
      fused head / loss / Adam) -- on a rollout recorded from ReplayFeedEnv, 20 optimizer steps, against the plain-torch
      train() loop of the same class in fp64 on the CPU (the statement proven equal to the reference on F9;
      tests/test_ppo_g64_gpu.py is the same check with assertions)."""
    import numpy as np
    import torch
    from tests import golden_util as gu
    from tests.test_policy_ppo_cpu import _ppo_from_fixture
    out = {"tolerance": 1e-4}
    fx = gu.load("F9_ppo_train")
    ppo = _ppo_from_fixture(fx, device=device, backend=args.backend)
    ppo.train()
    log = ppo.logger.name_to_value
    keys = ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/loss", "train/approx_kl")
    deltas = {k.split("/")[1]: abs(float(log[k]) - float(fx["log/" + k])) for k in keys}
    out["reference_fixture"] = {"fixture": "tests/golden/F9_ppo_train.npz (reference PPO_Grid_Obs.train(), 12 optimizer steps, G=20)",
                                "abs_delta": deltas, "max_abs_delta": max(deltas.values())}
    out["max_abs_delta"] = max(deltas.values())
    if args.backend == "hip" and (args.grid, args.batch_size) == (64, 128) and device.endswith(":0"):
        from tests import test_ppo_g64_gpu as t64
        rec = t64._Recorded()
        ref = rec.oracle(None)
        hip = t64._fresh_hip(rec, None, True)
        hip.train()
        s_h, s_r = hip.last_train_stats, ref.last_train_stats
        names = ("policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss")
        d = np.abs(s_h[:, :6] - s_r[:, :6]) / np.maximum(1.0, np.abs(s_r[:, :6]))
        out["timed_kernel_set"] = {
            "what": "G=64, batch 128, compact int8 rows, hipGraph; 20 optimizer steps on a ReplayFeedEnv rollout vs the fp64 CPU torch loop",
            "optimizer_steps": int(hip._hip["opt"].step_count.item()),
            "max_rel_delta_per_scalar": {n: float(d[:, j].max()) for j, n in enumerate(names)},
            "max_rel_delta": float(d.max()), "oracle_kl_max": float(np.abs(s_r[:, 3]).max())}
        out["max_abs_delta"] = max(out["max_abs_delta"], float(d.max()))
        del rec, ref, hip
        torch.cuda.empty_cache()
    return out


def encoder_roofline(algo, args, device, iters: int = 200, warm_ms: float = 150.0):
    """Second roofline object: the conv stack of the PPO update (conv1/conv2 forward + backward through the C-ABI,
    csrc/encoder.hip) at the minibatch size, timed live with events on the launch stream, priced against BOTH roofs:
    fp32 MFMA (157 TFLOP/s dense) and HBM (8 TB/s).  Algorithmic figures per minibatch of B samples at grid G
    (DESIGN.md section 4): flops = 3 x 2 x B x (27*16*o1^3 + 432*16*o2^3) (forward + two backward contractions);
    bytes = x (R fwd, R bwd) + y1 (W, 3 R; W, 2 R when conv1 + conv2 run as one forward launch) + y2-sized tensors (y2 W + 2 R, dy2 W + 2 R, features W, d_features R)
    [+ dz1 (W, R) on the unfused fallback, which the benchmarked configuration -- int8 rows, G % 16 == 0 -- never takes].
    Since round 2 the conv2 contractions run on the f16 matrix pipe with operands split into two f16 halves (fp32-accurate
    products, fp32 accumulation; csrc/conv_split.h): the stack is HBM-bound, `bound` says so, and the MFMA figure stays the
    ALGORITHMIC fp32 flop rate against the fp32 peak (what an fp32 implementation would need).

    Measurement protocol (round 4; BENCH_r03 carried 4.57 ms here against 0.386 in the builder's own run of the same command): this
    runs right after `timed_state_check`, i.e. after SECONDS of CPU-side oracle replay with the GPU idle, and 3 + 20 iterations of a
    0.4 ms step (9 ms in all) ended before the device had left its idle power state.  Now: >= `warm_ms` of GPU-busy warm-up, `iters`
    iterations timed ONE BY ONE with events, `ms` = the median, the spread reported, and `unstable: true` when max / min of the middle
    80 % exceeds 1.5 (the figure must not be quoted then)."""
    import torch
    from gennbv_amd.ops import encoder_ops
    enc = algo.policy.features_extractor
    if getattr(enc, "backend", "") != "hip":
        return None
    b, g = args.batch_size, args.grid
    o1 = (g - 3) // 2 + 1
    o2 = (o1 - 3) // 2 + 1
    buf = algo.rollout_buffer
    t, n = buf.buffer_size, buf.n_envs
    rows = torch.randint(0, t * n, (b,), device=device, dtype=torch.int64)
    base = buf.observations[:t].view(t * n, -1)
    s_dim = enc.state_input_shape[0]
    was_training = enc.training
    enc.train(True)
    seq = enc.naive_encoder_grid
    stats = [(m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()) for m in (seq[1], seq[4])]
    grads = [p.grad for p in seq.parameters()]
    for p_ in seq.parameters():
        p_.grad = None

    gi8 = None if buf.grid_i8 is None else buf.grid_i8[:t].view(t * n, -1)  # what the update reads when the env provides it
    ac = None if (gi8 is None or buf.autocorr is None) else buf.autocorr[:t].view(t * n, -1)  # (as PPO_Grid_Obs.train() passes it)

    def step():
        f = encoder_ops.grid_encoder(base, rows, s_dim, g, seq, True, grid_i8=gi8, compact=buf.compact_state_dim is not None, autocorr=ac)
        f.backward(torch.ones_like(f))

    ms, spread = _timed_median(step, iters, warm_ms)
    for m, (rm, rv, nb) in zip((seq[1], seq[4]), stats):  # leave the policy exactly as it was
        m.running_mean.copy_(rm); m.running_var.copy_(rv); m.num_batches_tracked.copy_(nb)
    for p_, g_ in zip(seq.parameters(), grads):
        p_.grad = g_
    enc.train(was_training)
    flops = 3 * 2 * b * (27 * 16 * o1 ** 3 + 432 * 16 * o2 ** 3)
    y1 = b * o1 ** 3 * 16 * 4
    x = b * g ** 3 * (4 if gi8 is None else 1)
    y2 = b * o2 ** 3 * 16 * 4
    fused = gi8 is not None and g % 16 == 0
    split = fused and (o1 + 1) // 2 == 16 and os.environ.get("GENNBV_CONV_SPLIT", "1") != "0"
    splitx = fused and 16 < (o1 + 1) // 2 <= 32 and o2 <= 32 and os.environ.get("GENNBV_CONV_SPLIT", "1") != "0"  # (csrc/conv_splitx.h: G = 128 class)
    # conv1 + conv2 forward as ONE launch (BN1 statistics known beforehand from the autocorrelation rows): y1 is written once and
    # read by the two backward kernels only
    one_fwd = split and ac is not None and g == 64 and all(os.environ.get(k, "1") != "0" for k in ("GENNBV_FUSED_TRAIN", "GENNBV_CONV1_SPLIT", "GENNBV_ANALYTIC_BN1"))
    nbytes = 2 * x + (3 if one_fwd else 4) * y1 + (0 if fused else 2 * y1) + 8 * y2
    tf, gbs = flops / (ms * 1e-3) / 1e12, nbytes / (ms * 1e-3) / 1e9
    return {"kernel": "conv stack of one PPO minibatch: gnbv_encoder_grid_forward + _backward (" +
                      ("k_conv12_fwd_split<true>, k_conv2_wgrad_split, k_conv2_dgrad_c1w_split" if one_fwd else
                       "k_conv1_fwd_split, k_conv2_fwd_split, k_conv2_wgrad_split, k_conv2_dgrad_c1w_split" if split else
                       "k_conv1_fwd_lds, k_conv2_fwd_splitx, k_conv2_wgrad_splitx, k_conv2_dgrad_c1w_splitx" if splitx else
                       "k_conv1_fwd_lds, k_conv2_fwd, k_conv2_wgrad, k_conv2_dgrad_c1w" if fused else
                       "k_conv1_fwd_lds, k_conv2_fwd, k_conv2_wgrad, k_conv2_dgrad, k_conv1_wgrad_lds") +
                      " + BN / reduction launches)",
            "bound": "hbm" if (split or splitx) else "mfma",
            "note": ("the split kernels stream at 3-4.5 TB/s each but are NOT byte-bound: letting the two backward kernels share y1 through L2 "
                     "removed 184 MB of HBM reads per minibatch and no time (round-3 experiment, profiles/r03_notes.md); both roofs are context")
                    if (split or splitx) else None,
            "ms": ms, "ms_spread": spread, "unstable": spread["unstable"], "batch": b, "grid_input": "fp32 rows" if gi8 is None else "int8 copy", "algorithmic_flops": flops,
            "algorithmic_bytes": nbytes,
            "mfma": {"achieved": tf, "peak": 157.3, "unit": "TFLOP/s", "frac": tf / 157.3, "dtype": "f32"},
            "hbm": {"achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0}}


def _timed_median(step, iters: int, warm_ms: float):
    """`step()` timed one call at a time with events on the current stream after >= warm_ms of the same work; (median ms, spread)."""
    import torch
    t0 = time.perf_counter()
    n_warm = 0
    while True:
        for _ in range(8):
            step()
        torch.cuda.synchronize()
        n_warm += 8
        if (time.perf_counter() - t0) * 1e3 >= warm_ms and n_warm >= 16:
            break
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    d = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    lo, hi = d[iters // 10], d[iters - 1 - iters // 10]
    med = d[iters // 2]
    return med, {"iters": iters, "warmup_iters": n_warm, "min": d[0], "p10": lo, "median": med, "p90": hi, "max": d[-1], "mean": sum(d) / iters,
                 "unstable": bool(hi > 1.5 * lo)}


def train_roofline(algo, args, train_ms_per_step: float):
    """Third roofline object: ONE WHOLE PPO MINIBATCH (the unit the step is made of: 1280 of them per iteration at configs[1]) priced on
    its compulsory HBM bytes: the conv stack's streams (x R fwd + R bwd, y1 W + 2 R, eight y2-sized tensors),
    fc_grid's weight three times (W read by the forward and by the dx product, dW written), and the optimizer's 28 bytes per parameter
    (p R+W, g R, m R+W, v R+W).  achieved = those bytes / (train phase of a timed iteration / minibatches in it) -- measured on the timed
    region itself, hipGraph replay, both streams, every small kernel included; peak = 8 TB/s."""
    enc = algo.policy.features_extractor
    if getattr(enc, "backend", "") != "hip":
        return None
    b, g = args.batch_size, args.grid
    o1 = (g - 3) // 2 + 1
    o2 = (o1 - 3) // 2 + 1
    n_mb = args.n_epochs * (args.n_steps * args.envs // b)
    if getattr(algo, "last_train_stats", None) is not None:
        n_mb = int(len(algo.last_train_stats))  # (what the last timed iteration ran: all of them unless --target-kl ref stopped it)
    compact = algo.rollout_buffer.grid_i8 is not None
    x = b * g ** 3 * (1 if compact else 4)
    y1, y2 = b * o1 ** 3 * 16 * 4, b * o2 ** 3 * 16 * 4
    conv = 2 * x + 3 * y1 + 8 * y2
    n_par = sum(p.numel() for p in algo.policy.parameters() if p.requires_grad)
    fc = 3 * 4 * enc.output_layer_grid[0].weight.numel()
    adam = 28 * n_par
    total = conv + fc + adam
    ms = train_ms_per_step / max(n_mb, 1)
    gbs = total / (ms * 1e-3) / 1e9
    return {"kernel": "one PPO minibatch of the timed train() phase (captured hipGraph: forward, loss, backward, clip + Adam; both streams)",
            "bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0, "ms_per_minibatch": ms, "minibatches_per_step": n_mb,
            "algorithmic_bytes": total, "bytes": {"conv_stack": conv, "fc_grid_weight_x3": fc, "adam_28B_per_param": adam}, "parameters": n_par,
            "note": "y1 counted W + 2 R (one-launch training forward); bytes are compulsory traffic, not PMC traffic"}


def flat_rows_line(args, device, steps: int = 2):
    """The same iteration with the REFERENCE's rollout-buffer layout -- flat fp32 rows [state | grid | state_rgb]
    (stable_baselines3/common/buffers.py:655-669; `PPO_Grid_Obs(compact_obs=False)`, the API default) -- measured in the same
    process after the headline: 1 warm-up + `steps` timed iterations.  The env still writes the int8 grid rows the conv1
    kernels read as a side copy (`PPO_Grid_Obs.grid_i8_rows`); the fp32 rows are what `get()` / checkpoints / callbacks see."""
    import copy
    import torch
    a2 = copy.copy(args)
    a2.obs = "flat"
    torch.cuda.reset_peak_memory_stats(device)
    algo, cfg, env = build_algo(a2, device, 0, 1)
    algo._setup_learn(total_timesteps=10 ** 12)
    ph = {"rollout": Phase(), "train": Phase()}
    one_iteration(algo, ph)
    ph = {"rollout": Phase(), "train": Phase()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one_iteration(algo, ph)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"value": args.envs * args.n_steps * steps / el, "unit": "env-steps/s", "ms_per_step": 1e3 * el / steps, "steps": steps, "warmup": 1,
            "obs_rows": "flat fp32 rows (the reference's layout, buffers.py:655-669)",
            "breakdown_ms_per_step": {"rollout": ph["rollout"].total_ms() / steps, "train": ph["train"].total_ms() / steps},
            "hbm_peak_allocated_gb": torch.cuda.max_memory_allocated(device) / 1e9}


def _workload_name(args) -> str:
    key = (args.envs, args.height, args.width, args.grid, bool(args.semantic))
    return {(256, 240, 320, 64, False): "BASELINE configs[1]", (256, 240, 320, 64, True): "BASELINE configs[2]",
            (512, 240, 320, 128, False): "BASELINE configs[4]'s per-GPU shard",
            (256, 400, 400, 20, False): "the reference's own default workload (train_gennbv.py:19-93, config_gennbv_train.py:24-25: 400x400 depth, 20^3 grid, pose history 100)",
            }.get(key, "custom workload")


def device_identity(device, smi: bool = True) -> dict:
    """What the timed numbers were taken on: marketing name, architecture, CU count, and -- with `smi`, from rocm-smi, after the timed
    region -- the clocks, power cap and temperature of the device (box-to-box differences of +-1.5 % exceed a round's gains: VERDICT r5 weak #8)."""
    import subprocess
    import torch
    p = torch.cuda.get_device_properties(device)
    out = {"name": p.name, "arch": getattr(p, "gcnArchName", None), "compute_units": p.multi_processor_count,
           "hbm_gb": p.total_memory / 1e9, "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}
    if not smi:
        return out
    try:
        idx = torch.device(device).index or 0
        r = subprocess.run(["rocm-smi", "-d", str(idx), "--showclocks", "--showmaxpower", "--showpower", "--showtemp", "--showperflevel", "--json"],
                           capture_output=True, text=True, timeout=20)
        j = json.loads(r.stdout[r.stdout.index("{"):]) if "{" in r.stdout else {}
        card = next(iter(j.values()), {}) if j else {}
        keep = {}
        for k, v in card.items():
            lk = k.lower()
            if any(t in lk for t in ("sclk", "mclk", "fclk", "socclk", "max graphics package power", "power (w)", "package power", "temperature (sensor junction)",
                                     "temperature (sensor memory)", "performance level")):
                keep[k] = v
        out["rocm_smi"] = keep
    except Exception as ex:  # (never take the bench line down)
        out["rocm_smi"] = {"error": repr(ex)}
    return out


def _flush_c_stdio():
    """RCCL writes a version banner with printf; flush it so that it cannot land after the JSON line."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def self_launch(args) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start the N ranks ourselves -- the command the contract
    names (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`) with a
    free port -- and hand its exit code back.  The ranks' stdout is inherited, so rank 0's JSON line is this process's JSON line."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts (RCCL across processes needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] --gpus {args.gpus} without a launcher environment: starting the ranks with: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def dry_run(args, world: int, rank: int) -> None:
    """GENNBV_BENCH_DRY=1 (tests/test_bench_launch_cpu.py): the launch / rendezvous / max-over-ranks / one-JSON-line skeleton of main() over
    gloo, without a GPU and without the hot path -- what `--gpus N` needs in order to START wherever N devices exist."""
    import torch
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "max_rank_seconds": elapsed}), flush=True)


def main():
    t_start = time.perf_counter()
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if os.environ.get("GENNBV_BENCH_DRY") == "1":
        return dry_run(args, world, int(os.environ.get("RANK", "0")))
    import torch
    import torch.distributed as dist

    if torch.cuda.device_count() < max(1, world):
        raise SystemExit(f"bench.py: {world} rank(s) need {world} GPU(s), this node shows {torch.cuda.device_count()}")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 or os.environ.get("GENNBV_FORCE_DP") == "1":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        torch.cuda.set_device(local_rank)
        from gennbv_amd import parallel as _parallel
        _parallel.capture_safe_env()  # (eager + captured RCCL collectives in one process: see its docstring)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
        dist.barrier()  # creates the communicator now (RCCL prints its banner through C stdio here)
        _flush_c_stdio()
    device = f"cuda:{local_rank}"
    torch.cuda.set_device(device)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    algo, cfg, env = build_algo(args, device, rank, world)
    algo._setup_learn(total_timesteps=10 ** 12)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    dummy = {"rollout": Phase(), "train": Phase()}
    t_warm = time.perf_counter()
    for _ in range(args.warmup):
        one_iteration(algo, dummy)
    phases = {"rollout": Phase(), "train": Phase()}
    vox = instrument_voxel(env)
    iter_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]  # (one record per iteration, no synchronisation inside the timed region)
    # (every event of the timed region exists before it starts: Phase.reserve.  At least 3 072 pairs: the one-off ~100 ms stall of the
    # runtime comes with roughly the 4 096th HIP event a process creates -- with 2 064 events reserved it moved from the fifth timed
    # iteration to the third, profiles/r06_bench_event_reserve_ab.txt -- and belongs in front of the timed region, not inside it)
    vox.reserve(max(args.steps * args.n_steps + 8, 3072))
    for ph_ in phases.values():
        ph_.reserve(args.steps + 1)
    for e in iter_ev:
        e.record()
    barrier()
    t0 = time.perf_counter()
    iter_ev[0].record()
    for i in range(args.steps):
        one_iteration(algo, phases)
        iter_ev[i + 1].record()
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    iter_ms = [iter_ev[i].elapsed_time(iter_ev[i + 1]) for i in range(args.steps)]
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    dumped = dump_outputs(algo, args.dump_outputs) if args.dump_outputs and rank == 0 else None

    env_steps = world * args.envs * args.n_steps * args.steps
    value = env_steps / elapsed
    # roofline of the voxel update.  Two byte counts per launch (= one gnbv_update_occ_grid_coded call over the rank's envs):
    #  * reference layout: depth + seg once, six fp32 passes over G^3 -- what a perfect implementation of the
    #    reference's tensors would move; reported as `vs_reference_layout_floor`;
    #  * this layout: depth + seg once, the 1-byte probability code R + W, the int8 tri-class row W,
    #    seven bitmask passes (hit W + R, path W + R, gt R, scanned R + W) and the ray list W + R -- the bytes `frac` prices.
    # `traffic` = HBM bytes from rocprofv3 --pmc passes of THIS build (profiles/rNN_voxel_traffic.json carries the sha256 of
    # csrc/voxel.hip it was measured on; a different source -> null).
    import hashlib
    g3 = args.grid ** 3
    b_ref = args.height * args.width * 8 + g3 * 4 * 6 + 200
    b_lay = args.height * args.width * 8 + g3 * (3 if args.obs == "compact" else 6) + 7 * (g3 // 8) + 2 * 4 * 1200 + 200  # (rounds 2-5's basis: code R + W)
    vox_ms = vox.total_ms() / max(vox.count(), 1)
    traffic, traffic_src, traffic_json = None, None, None
    src_sha = hashlib.sha256(open(os.path.join(ROOT, "gennbv_amd", "csrc", "voxel.hip"), "rb").read()).hexdigest()
    for name in sorted((f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_voxel_traffic.json")), reverse=True):
        tj = json.load(open(os.path.join(ROOT, "profiles", name)))
        c = tj["config"]
        if tj.get("source_sha256") == src_sha and (c["envs"], c["height"], c["width"], c["grid"], c.get("obs", "flat")) == (
                args.envs, args.height, args.width, args.grid, args.obs):
            traffic, traffic_src, traffic_json = tj["traffic_bytes_per_launch"], "profiles/" + name, tj
            break
    # Since round 5 k_grid_update_coded writes a code word back only where the step touched it (a hit or a walked voxel: ~3 % of the
    # grid per step), so the bytes the launch MOVES are code R + touched-W, not R + W.  `frac` prices those; the
    # touched fraction comes from the PMC write counter of this very build when a matching profiles/*_voxel_traffic.json exists
    # (written bytes of k_grid_update_coded minus the tri-class row it always writes), else the documented 3 %.
    tri_w = g3 * (1 if args.obs == "compact" else 4)
    touched_w, touched_src = 0.03 * g3, "default: a step touches ~3 % of the voxels (profiles/r05_notes.md 1c)"
    b_moved = b_lay - g3 + touched_w
    if traffic_json is not None and "k_grid_update_coded" in traffic_json.get("write_bytes", {}):
        # everything the update kernel writes besides the tri-class row: touched code words, touched scanned words, the clears of the
        # consumed hit / path words -- it replaces the full code W and scanned W passes of the round-2 basis
        touched_w = max(0.0, traffic_json["write_bytes"]["k_grid_update_coded"] / args.envs - tri_w)
        touched_src = "PMC WRITE_SIZE of k_grid_update_coded minus its tri-class row, " + traffic_src
        b_moved = b_lay - g3 - g3 // 8 + touched_w
    achieved = args.envs * b_moved / (vox_ms * 1e-3) / 1e9
    out = {
        "metric": "env-steps/sec at 256 envs x 64^3 grid (state encoding + policy forward + GAE + PPO update)",
        "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        # per-iteration device times (events on the launch stream behind every iteration; nothing synchronises inside the timed region):
        # what a +-1 % difference between two runs has to be read against.  `value` stays total work / total wall time (the contract).
        "iteration_ms": {"min": min(iter_ms), "median": sorted(iter_ms)[len(iter_ms) // 2], "p90": sorted(iter_ms)[min(len(iter_ms) - 1, (9 * len(iter_ms)) // 10)],
                         "max": max(iter_ms), "all": [round(x, 3) for x in iter_ms]},
        "value_at_median_iteration": world * args.envs * args.n_steps / (sorted(iter_ms)[len(iter_ms) // 2] * 1e-3),
        "breakdown_ms_per_step": {"rollout": phases["rollout"].total_ms() / args.steps, "train": phases["train"].total_ms() / args.steps,
                                  "voxel_update_total": vox.total_ms() / args.steps},
        "minibatch_graph_captures_ms": getattr(algo, "graph_capture_ms", None),
        "config": {"workload": f"{_workload_name(args)}: {args.envs} envs/GPU x {args.height}x{args.width} depth x "
                               f"{args.grid}^3 grid, n_steps={args.n_steps}, batch_size={args.batch_size}, "
                               f"n_epochs={args.n_epochs}, one step = one PPO iteration",
                   "global_envs": world * args.envs, "encoder_backend": args.backend, "obs_rows": args.obs,
                   # data-parallel semantics: an optimizer step consumes minibatch k of EVERY rank (statistics and gradient over their
                   # union), so N ranks take the same number of steps per iteration as one rank, each over N x batch_size samples --
                   # not what a single GPU with N x envs would do at the same batch_size (N x the steps)
                   "global_batch": world * args.batch_size,
                   "optimizer_steps_per_iteration": (args.envs * args.n_steps // args.batch_size) * args.n_epochs,
                   "semantic_branch": bool(args.semantic),
                   "kl_early_stop": "reference (0.05)" if args.target_kl == "ref" else "never triggers (full work every iteration)",
                   "minibatches_last_iteration": int(len(algo.last_train_stats)) if getattr(algo, "last_train_stats", None) is not None else None,
                   "hbm_peak_allocated_gb": torch.cuda.max_memory_allocated(device) / 1e9,
                   "parallelism": f"env-sharded dp{world}", "dp_graph_mode": getattr(algo, "dp_graph_mode", None),
                   # ms per masked replay of each captured candidate of the minibatch graph; the fastest is the one train() replays
                   # (PPO_Grid_Obs._best_of_captures: a capture lands in one of several scheduling states for its whole life)
                   "minibatch_graph_captures_ms": getattr(algo, "graph_capture_ms", None),
                   "dp_update": (None if world == 1 else "fc_grid.weight reduce-scattered, updated by its owner rank, all-gathered; the rest all-reduced"
                                 if getattr((algo._hip or {}).get("opt"), "shard", None) is not None else "whole gradient all-reduced, replicated update"),
                   "breakdown_ms_per_step": {"rollout": phases["rollout"].total_ms() / args.steps,
                                             "train": phases["train"].total_ms() / args.steps,
                                             "voxel_update_total": vox.total_ms() / args.steps}},
        "roofline": {"bound": "hbm", "kernel": ("gnbv_update_occ_grid_coded (" + ("k_hit_list + k_ray_list" if args.grid <= 104 else "k_hit_atomic + k_ray_slab") +
                                                " + k_grid_update_coded, which also clears the masks it consumed; 1-byte coded probability grid)"),
                     "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                     "launch_ms": vox_ms, "algorithmic_bytes_per_launch": args.envs * b_moved,
                     "bytes_basis": "the bytes this layout MOVES per launch: depth + seg, 1-byte code R + touched-W (code words are written back "
                                    "only where the step touched them), int8 tri-class W, 7 bitmask passes, ray lists",
                     "touched_write_bytes_per_env": touched_w, "touched_write_source": touched_src,
                     "frac_traffic": None if traffic is None else (traffic / (vox_ms * 1e-3) / 1e9) / 8000.0,
                     "frac_round2_basis": (args.envs * b_lay / (vox_ms * 1e-3) / 1e9) / 8000.0,
                     "frac_round2_basis_note": "rounds 2-5 priced code R + W (untouched words included): kept for continuity only, it overstates "
                                               "what the kernel moves since round 5",
                     "frac_survey_bytes": (args.envs * b_ref / (vox_ms * 1e-3) / 1e9) / 8000.0,
                     "frac_survey_bytes_note": "SURVEY 8(d) bytes (depth + seg + six fp32 passes over G^3) / launch time / 8 TB/s; > 1 reflects the "
                                               "re-layout (1-byte probability code, bit-packed gt / scanned, int8 tri-class rows: 4.2x fewer bytes), "
                                               "not a kernel above the roof -- `frac` prices the bytes moved, `frac_traffic` the PMC-counted bytes",
                     "vs_reference_layout_floor": {"reference_layout_bytes_per_launch": args.envs * b_ref,
                                                   "floor_ms_at_peak": args.envs * b_ref / 8e12 * 1e3,
                                                   "speedup_over_floor": (args.envs * b_ref / 8e12 * 1e3) / vox_ms},
                     "traffic": traffic, "traffic_source": traffic_src},
    }
    if dumped is not None:
        out["dumped_outputs"] = dumped
    if dist.is_initialized():
        if args.full:
            try:  # (every rank: collectives) what the step's exchanges cost by themselves on this node -- ring or direct, answered by the numbers
                from gennbv_amd import parallel as _par
                out["dp_exchange_probe"] = _par.exchange_probe(algo)
            except Exception as ex:
                out["dp_exchange_probe"] = {"error": repr(ex)}
        # Everything timed is done and reduced: the process group goes away NOW, so that ranks > 0 exit instead of sitting in a
        # collective teardown while rank 0 spends seconds in the CPU-side checks below (none of them communicates).
        barrier()
        dist.destroy_process_group()
    if rank == 0 and args.full and args.backend == "hip" and not args.no_state_check:
        # Self-check of the TIMED tensors: sampled envs of the last timed rollout are replayed through the CPU oracle from an
        # episode boundary inside the buffer -- same frames, same actions -- and every stored observation row, reward, done flag and
        # the env's final probability / scanned grids are compared bit for bit (tests/state_check.py; the oracle is the checker only).
        try:
            from tests import state_check
            sel = sorted({0, args.envs // 2 - 27, args.envs - 1} & set(range(args.envs)))
            res = state_check.check_rollout(algo, sel, max_steps=40, across_ends=1)  # + one env replayed ACROSS an episode end
            out["timed_state_check"] = res["status"]
            out["timed_state_check_detail"] = {k: v for k, v in res.items() if k != "status"}
        except Exception as ex:
            out["timed_state_check"] = "error: " + repr(ex)
    if rank == 0:
        out["device"] = device_identity(device, smi=args.full)
        try:
            out["train_roofline"] = train_roofline(algo, args, phases["train"].total_ms() / args.steps)
        except Exception as ex:
            out["train_roofline"] = {"error": repr(ex)}
    if rank == 0 and args.full:
        if world == 1:  # (single-GPU diagnostics: a data-parallel encoder would exchange its BatchNorm sums with ranks that have left)
            try:
                out["encoder_roofline"] = encoder_roofline(algo, args, device)
            except Exception as ex:
                out["encoder_roofline"] = {"error": repr(ex)}
            try:
                out["ppo_loss_delta_vs_ref"] = ppo_loss_delta(args, device)
            except Exception as ex:
                out["ppo_loss_delta_vs_ref"] = {"error": repr(ex)}
        if world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args, cfg)
            except Exception as ex:  # the baseline must never take the bench line down
                out["cpu_baseline"] = {"value": None, "error": repr(ex)}
        flat_bytes = (args.n_steps + 1) * args.envs * cfg.obs_dim * 4
        if world == 1 and args.obs == "compact" and not args.no_flat_rows and flat_bytes < 100e9:
            try:
                del algo, env, vox
                import gc
                gc.collect()
                torch.cuda.empty_cache()
                out["config"]["flat_rows"] = flat_rows_line(args, device)
            except Exception as ex:
                out["config"]["flat_rows"] = {"value": None, "error": repr(ex)}
    _flush_c_stdio()
    if rank == 0:
        # this rank's wall clock around the steps (from the start of main(): interpreter start-up and exit are not in it)
        out["wall_seconds"] = {"setup": t_warm - t_start, "warmup": t0 - t_warm, "timed": t1 - t0, "after_steps": time.perf_counter() - t1}
        sys.stdout.flush()
        print(json.dumps(out), flush=True)  # the ONE JSON line, last thing on stdout


if __name__ == "__main__":
    main()
