"""Imitation from the planners (gennbv_amd/eval/baselines.py): demonstrations, behaviour cloning and DAgger for the policy of
PPO_Grid_Obs, on the soft-target loss kernel (csrc/imitation.hip, ops/imitation_ops.py).

A planner is a privileged teacher -- it reads the mesh, the ground truth or at least its own view-gain kernel --, the policy a
student that sees only its observation.  `collect_demonstrations` flies the env with a beta-mixture of the two and stores the
teacher's label at every visited observation (beta = 1: behaviour cloning data; beta < 1: DAgger, the student visits its own
mistakes); `BehaviourCloning.fit` minimises the cross-entropy between the policy's six heads and the per-head marginal of the
teacher's K weighted candidates (`soft_targets` of its scores; K = 1: a hard label); `dagger` alternates the two.  PPO fine-tuning
afterwards is `model.learn()`: fit() leaves the model as it found it, parameters aside (DESIGN.md "Imitation from the planners").
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..eval.baselines import soft_targets


class Demonstrations:
    """Fixed-capacity store of labelled observations, all on one device; blocks of T * N rows (row = t * N + n inside a block) are
    appended, and once `capacity` rows are filled the oldest block is overwritten.

      small [M, state_dim + rgb_dim] fp32   the observation without its grid slice: [state | state_rgb]
      grid_i8 [M, G^3] int8                 the tri-class grid slice, exactly -1 / 0 / 1: a quarter of the fp32 bytes
      cand [M, K, 6] int64, cand_w [M, K] fp32, sample_w [M] fp32    the teacher's label (GnbvImitationLoss)
      rewards, values, returns [M] fp32, episode_starts [M] uint8    what the value head regresses on (GAE over the block)
      autocorr [M, 768] int32 or None       per-row input autocorrelation of the int8 grid (G % 16 == 0 on the GPU): what the
                                            compact-row conv1 kernels read for BatchNorm-1's analytic statistics
    """

    def __init__(self, capacity: int, block_rows: int, state_dim: int, grid_elems: int, rgb_dim: int, k: int, n_heads: int = 6, device="cpu"):
        capacity, block_rows = int(capacity), int(block_rows)
        if block_rows < 1 or capacity < block_rows or capacity % block_rows:
            raise ValueError(f"Demonstrations: capacity {capacity} must be a positive multiple of the block of {block_rows} rows")
        self.capacity, self.block_rows, self.k = capacity, block_rows, int(k)
        self.state_dim, self.grid_elems, self.rgb_dim = int(state_dim), int(grid_elems), int(rgb_dim)
        self.device = torch.device(device)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=self.device)  # noqa: E731
        m = capacity
        self.small = z(m, self.state_dim + self.rgb_dim)
        self.grid_i8 = z(m, self.grid_elems, dt=torch.int8)
        self.cand = z(m, self.k, int(n_heads), dt=torch.int64)
        self.cand_w, self.sample_w = z(m, self.k), z(m)
        self.rewards, self.values, self.returns = z(m), z(m), z(m)
        self.episode_starts = z(m, dt=torch.uint8)
        self.autocorr = None
        g = round(self.grid_elems ** (1.0 / 3.0))
        self.grid = g if g ** 3 == self.grid_elems else None
        if self.device.type == "cuda" and self.grid is not None:
            from ..ops import encoder_ops
            if encoder_ops.autocorr_supported(self.grid):
                self.autocorr = z(m, 768, dt=torch.int32)
        self.blocks = 0   # blocks appended so far
        self.filled = 0   # rows that hold a demonstration
        self.last = None  # (env, observation, episode_starts) the last collection ended with: the next one goes on from there

    @property
    def n_blocks(self) -> int:
        return self.capacity // self.block_rows

    def block_slice(self, block: Optional[int] = None) -> slice:
        """Rows of the block appended as number `block` (default: the next one to be written)."""
        b = (self.blocks if block is None else int(block)) % self.n_blocks
        return slice(b * self.block_rows, (b + 1) * self.block_rows)

    def append(self, obs, cand, cand_w, sample_w, rewards, values, returns, episode_starts) -> slice:
        """One block: obs [R, D] dense fp32 rows [state | grid | state_rgb], the labels and scalars [R, ...]; returns its rows."""
        r, s, g3 = self.block_rows, self.state_dim, self.grid_elems
        if obs.shape != (r, s + g3 + self.rgb_dim):
            raise ValueError(f"Demonstrations.append: observations must be dense rows [{r}, {s + g3 + self.rgb_dim}], got {tuple(obs.shape)}")
        sl = self.block_slice()
        self.small[sl, :s].copy_(obs[:, :s])
        self.small[sl, s:].copy_(obs[:, s + g3:])
        self.grid_i8[sl].copy_(obs[:, s:s + g3])
        self.cand[sl].copy_(cand.view(r, self.k, -1))
        self.cand_w[sl].copy_(cand_w.view(r, self.k))
        for dst, src in ((self.sample_w, sample_w), (self.rewards, rewards), (self.values, values), (self.returns, returns),
                         (self.episode_starts, episode_starts)):
            dst[sl].copy_(src.reshape(r))
        self._finish_block(sl)
        return sl

    def _finish_block(self, sl: slice) -> None:
        if self.autocorr is not None:
            from ..ops import encoder_ops
            encoder_ops.input_autocorr(self.grid_i8[sl], self.grid, out=self.autocorr[sl])
        self.blocks += 1
        self.filled = min(self.capacity, self.blocks * self.block_rows)

    def dense_rows(self, rows: torch.Tensor) -> torch.Tensor:
        """The reference's flat fp32 observation rows [state | grid | state_rgb] of demonstrations `rows`."""
        from ..ops.encoder_ops import _flat_rows
        return _flat_rows(self.small[rows], self.grid_i8[rows], self.state_dim)


def _teacher_fn(teacher):
    return getattr(teacher, "policy", teacher)


def collect_demonstrations(model, env, teacher, n_steps: int, beta: float, seed: int, soft: bool = False,
                           temperature: Optional[float] = None, demos: Optional[Demonstrations] = None, capacity_blocks: int = 1):
    """Fly `env` for `n_steps` steps and append ONE block of n_steps * N labelled rows to `demos` (None: a new store of
    `capacity_blocks` blocks), which is returned.

    At every step the teacher is asked at the current observation (`teacher.policy(obs, deterministic=True)[0]`, the protocol of
    evaluate_policy_grid_obs) and the student is sampled, without grad and in eval mode, at the same observation.  Env e executes
    the teacher's action where a CPU generator seeded with `seed` draws below `beta`, the student's otherwise (the draw reaches the
    device through pinned memory, no synchronisation).  The teacher's label is stored whichever action is executed: with `soft` its
    K candidates `last_candidates` weighted by soft_targets(`last_score`, temperature), else its action alone (candidate 0, weight
    1).  sample_w is 0 where the env's episode_length_buf is 0 at decision time (the env forces the init action there: the label is
    moot) and where every candidate is refused.  `returns` are GAE(gamma, lambda of the model) over the block with the student's
    values.  The env must hand out dense rows (`env.step(actions)` without obs_out); if `env is model.env`, `model._last_obs` and
    `model._last_episode_starts` are left as collect_rollouts leaves them, so that learn() can go on."""
    from .. import gae as gae_ops
    n = int(env.num_envs)
    n_steps = int(n_steps)
    cfg = env.cfg
    s, g3 = int(cfg.state_dim), int(cfg.grid_dim)
    d_obs = int(env.observation_space.shape[0])
    dev = torch.device(model.device)
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError(f"collect_demonstrations: beta must be in [0, 1], got {beta}")
    if soft and temperature is None:
        raise ValueError("collect_demonstrations(soft=True) needs a temperature (soft_targets has no default)")
    if env is getattr(model, "env", None) and getattr(model.rollout_buffer, "compact_state_dim", None) is not None:
        raise ValueError("collect_demonstrations: the model keeps compact observation rows (compact_obs=True) and its env then writes "
                         "rows without the grid slice the planners read; collect on an env that hands out dense rows")
    fn = _teacher_fn(teacher)
    nh = int(len(model.action_space.nvec))
    k = int(teacher.k) if soft else 1
    if demos is None:
        demos = Demonstrations(int(capacity_blocks) * n_steps * n, n_steps * n, s, g3, d_obs - s - g3, k, nh, dev)
    if demos.block_rows != n_steps * n or demos.k < k or (demos.state_dim, demos.grid_elems, demos.rgb_dim) != (s, g3, d_obs - s - g3):
        raise ValueError(f"collect_demonstrations: demos holds blocks of {demos.block_rows} rows with k = {demos.k}; this call makes "
                         f"{n_steps * n} rows with k = {k}")
    kk = demos.k
    # where the flight goes on from: the previous collection on this env, the model's own rollout state, or a reset
    own = env is getattr(model, "env", None)
    if demos.last is not None and demos.last[0] is env:
        obs, starts = demos.last[1], demos.last[2]
    elif own and model._last_obs is not None:
        obs, starts = model._last_obs, model._last_episode_starts
    else:
        obs = env.reset()
        starts = torch.ones(n, dtype=torch.bool, device=dev)
    if obs.dim() != 2 or obs.shape[1] != d_obs:
        raise ValueError(f"collect_demonstrations: the env must hand out dense observation rows [N, {d_obs}], got {tuple(obs.shape)}")
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    was_training = model.policy.training
    model.policy.set_training_mode(False)
    if hasattr(model, "_check_ranges"):
        model._check_ranges()
    t_, r_ = n_steps, n_steps * n
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)  # noqa: E731
    b_obs = z(t_, n, d_obs)
    b_cand, b_cw, b_sw = z(t_, n, kk, nh, dt=torch.int64), z(t_, n, kk), z(t_, n)
    b_rew, b_val, b_start = z(t_, n), z(t_, n), z(t_, n, dt=torch.uint8)
    executed = z(t_, n, nh, dt=torch.int64)
    took_teacher = z(t_, n, dt=torch.bool)
    dones = None
    try:
        for t in range(t_):
            with torch.no_grad():
                label = fn(obs, deterministic=True)[0].to(torch.int64)
                if soft:
                    cand, score = teacher.last_candidates, teacher.last_score
                    if cand is None or score is None:
                        raise _lib.GennbvHipError("collect_demonstrations(soft=True): the teacher keeps no last_candidates / last_score")
                    b_cand[t, :, :k].copy_(cand)
                    b_cw[t, :, :k].copy_(soft_targets(score, temperature))
                else:
                    b_cand[t, :, 0].copy_(label)
                    b_cw[t, :, 0] = 1.0
                student, values, _ = model.policy(obs)
                draw = torch.rand(n, generator=gen) < float(beta)
                if dev.type == "cuda":
                    draw = draw.pin_memory().to(dev, non_blocking=True)
                actions = torch.where(draw[:, None], label, student.to(torch.int64))
                b_obs[t].copy_(obs)
                b_sw[t].copy_(((env.episode_length_buf != 0) & (b_cw[t].sum(1) > 0)).to(torch.float32))
                b_val[t].copy_(values.reshape(n))
                b_start[t].copy_(starts.reshape(n))
                executed[t].copy_(actions)
                took_teacher[t].copy_(draw)
            obs, rewards, dones, _ = env.step(actions)
            b_rew[t].copy_(rewards.reshape(n))
            starts = dones
        with torch.no_grad():
            last_values = model.policy.predict_values(obs).reshape(n)
        _, returns = gae_ops.compute_returns_and_advantage(b_rew, b_val, b_start, last_values, dones, model.gamma, model.gae_lambda)
    finally:
        model.policy.set_training_mode(was_training)
    if hasattr(model, "_check_ranges"):
        model._check_ranges()
    sl = demos.append(b_obs.view(r_, d_obs), b_cand.view(r_, kk, nh), b_cw.view(r_, kk), b_sw, b_rew, b_val, returns, b_start)
    obs, starts = obs.clone(), dones.clone()  # (the env overwrites both on its next step)
    demos.last = (env, obs, starts)
    demos.last_block = {"rows": sl, "executed": executed.view(r_, nh), "took_teacher": took_teacher.view(r_), "beta": float(beta)}
    if own:
        model._last_obs, model._last_episode_starts, model._pending = obs, starts, None
    return demos


class BehaviourCloning:
    """Supervised training of `model.policy` on `demos` with the soft-target imitation loss.

    fit(): n_epochs passes over a seeded permutation of the filled rows (one permutation per epoch, drawn from one CPU generator
    seeded with `seed`), minibatches of `batch_size` (n_mb = filled // batch_size, the remainder dropped), eager: encoder on its HIP
    kernels in training mode -> logits, values -> gnbv_imitation_loss -> backward -> clip + Adam (FlatAdam.step).  No host
    synchronisation inside fit() but the one read-back of the statistics table and the flags at its end; returns the statistics
    rows [steps, 8] (include/gennbv_hip.h: GnbvImitationLoss).  A minibatch without a live sample takes no optimizer step and no
    BatchNorm update: its flag is computed on the device from the demonstrations' weights before the loop."""

    def __init__(self, model, demos: Demonstrations, batch_size: int, learning_rate: float, n_epochs: int, seed: int,
                 label_smoothing: float = 0.0, ent_coef: float = 0.0, vf_coef: float = 0.0, max_grad_norm: Optional[float] = None):
        self.model, self.demos = model, demos
        self.batch_size, self.learning_rate, self.n_epochs, self.seed = int(batch_size), float(learning_rate), int(n_epochs), int(seed)
        self.label_smoothing, self.ent_coef, self.vf_coef = float(label_smoothing), float(ent_coef), float(vf_coef)
        self.max_grad_norm = max_grad_norm
        if self.batch_size < 1 or self.n_epochs < 1:
            raise ValueError("BehaviourCloning: batch_size and n_epochs must be >= 1")
        self.device = torch.device(model.device)
        self.gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self.op = None
        self.state = None  # BC's own Adam moments and step count (they outlive a fit(): dagger goes on with them)
        self.skip = torch.zeros(1, dtype=torch.int32, device=self.device)  # this minibatch has no live sample: no Adam step, no BatchNorm update
        self.last_stats = None

    # ---- the optimizer: ONE FlatAdam per policy ----
    def _optimizer(self):
        """The flat optimizer whose buffers ARE the policy's parameters: PPO's (`model._hip["opt"]`) when it exists; else one of this
        module's making, kept on the model and rebuilt whenever the parameters no longer live in it.  (FlatAdam re-points every
        p.data / p.grad at its own buffers, so PPO's later _hip_setup -- which builds its own when it finds none -- ends up owning
        live storage, and this one is then never used again.)"""
        from ..ops.ppo_ops import FlatAdam
        model = self.model
        if getattr(model, "_hip", None) and model._hip.get("opt") is not None:
            return model._hip["opt"]
        opt = getattr(model, "_imitation_opt", None)
        alive = opt is not None and all(p.data_ptr() == opt.params.data_ptr() + 4 * off and p.grad is not None
                                        and p.grad.data_ptr() == opt.grads.data_ptr() + 4 * off
                                        for (off, _), p in zip(opt.slices, opt.module_params))
        if not alive:
            old = model.policy.optimizer
            opt = model._imitation_opt = FlatAdam(model.policy, lr=self.learning_rate, eps=old.defaults.get("eps", 1e-5),
                                                  betas=old.defaults.get("betas", (0.9, 0.999)))
        return opt

    def _compact_input(self, enc) -> bool:
        """The encoder's int8 path (the conditions PPO_Grid_Obs._maybe_enable_grid_i8 checks, the env's part being the store's int8
        rows): compact RowGather rows; otherwise dense fp32 rows are materialised per minibatch."""
        g = getattr(enc, "grid_size", 0)
        return (getattr(self.model, "grid_i8_rows", True) and getattr(enc, "backend", "") == "hip" and g % 16 == 0 and g ** 3 == self.demos.grid_elems
                and self.demos.autocorr is not None)

    def fit(self) -> np.ndarray:
        from ..ops import encoder_ops
        from ..ops.encoder_ops import RowGather
        from ..ops.imitation_ops import ImitationLossOp
        from .policies import _IdentityExtractor
        model, demos, dev = self.model, self.demos, self.device
        pol = model.policy
        enc = pol.features_extractor
        if getattr(model, "_sync", None) is not None and model._sync.active:
            raise _lib.GennbvHipError("BehaviourCloning.fit: data-parallel training is not supported (the model has an active GradSync)")
        if getattr(enc, "backend", "") != "hip":
            raise _lib.GennbvHipError("BehaviourCloning.fit needs the encoder on its HIP kernels (backend 'hip'): there is no fallback")
        batch = self.batch_size
        n_mb = demos.filled // batch
        if n_mb < 1:
            raise ValueError(f"BehaviourCloning.fit: {demos.filled} demonstrations do not fill one minibatch of {batch}")
        steps = self.n_epochs * n_mb
        dims = [int(d) for d in model.action_space.nvec]
        if self.op is None or self.op.max_rows < steps or self.op.k != demos.k:
            self.op = ImitationLossOp(batch, dims, demos.k, dev, steps, self.label_smoothing, self.ent_coef, self.vf_coef)
        op = self.op
        op.bind(demos)
        op.stats_row.zero_()
        op.flags.zero_()
        # every epoch's permutation and every minibatch's dead flag, before the loop
        perms = torch.stack([torch.randperm(demos.filled, generator=self.gen)[:n_mb * batch] for _ in range(self.n_epochs)])
        rows_all = perms.to(dev).view(steps, batch)
        live_row = (demos.sample_w[:demos.filled] > 0) & (demos.cand_w[:demos.filled].sum(1) > 0)
        dead_tab = (live_row[rows_all].sum(1) == 0).to(torch.int32).view(steps, 1)
        opt = self._optimizer()
        if self.state is None or self.state[0].numel() != opt.n:
            self.state = (torch.zeros_like(opt.exp_avg), torch.zeros_like(opt.exp_avg_sq), torch.zeros_like(opt.step_count))
        fused_head = (isinstance(pol.mlp_extractor, _IdentityExtractor) and encoder_ops.policy_head_supported(enc, pol.action_net, pol.value_net))
        compact = self._compact_input(enc)
        hip = getattr(model, "_hip", None) or {}
        skip_zero = bool(hip.get("skip_zero")) and hip.get("opt") is opt  # (every slice overwritten: only what PPO's set-up established)
        lin = getattr(enc, "output_layer_grid", [None])[0]
        if hasattr(model, "_check_ranges"):
            model._check_ranges()  # (parameters outside the split-f16 ranges move the encoder to the fp32-MFMA kernels before anything is computed)
        saved = (opt.exp_avg, opt.exp_avg_sq, opt.step_count, opt.lr, getattr(enc, "_bn_skip_flag", None), pol.training)
        opt.exp_avg, opt.exp_avg_sq, opt.step_count = self.state
        opt.lr = self.learning_rate
        enc._bn_skip_flag = self.skip
        pol.set_training_mode(True)
        try:
            for i in range(steps):
                op.rows.copy_(rows_all[i])
                self.skip.copy_(dead_tab[i])
                if compact:
                    obs = RowGather(demos.small, op.rows, demos.grid_i8, demos.state_dim, demos.autocorr)
                else:
                    obs = demos.dense_rows(op.rows)
                enc._defer_pose_backward = True  # (only around this forward: pose_branch_backward below runs what it cut off)
                try:
                    if fused_head:
                        fa, fg = encoder_ops.hybrid_branches(enc, obs)
                        logits, values, _ = encoder_ops.policy_head(enc, pol.action_net, pol.value_net, fa, fg)
                    else:
                        features = pol.extract_features(obs)
                        logits = pol.action_net(features)
                        values = pol.value_net(features).flatten()
                finally:
                    enc._defer_pose_backward = False
                d_logits, d_values = op(logits.contiguous(), values.contiguous())
                if not skip_zero:
                    opt.zero_grad()
                if lin is not None:
                    lin._defer_wgrad = True
                try:
                    torch.autograd.backward([logits, values], [d_logits, d_values])
                finally:
                    if lin is not None:
                        lin._defer_wgrad = False
                encoder_ops.pose_branch_backward(enc, dev)
                encoder_ops.join_async_wgrads(dev)
                opt.step(self.max_grad_norm, self.skip)
        finally:
            opt.exp_avg, opt.exp_avg_sq, opt.step_count, opt.lr = saved[:4]
            enc._bn_skip_flag = saved[4]
            pol.set_training_mode(saved[5])
        # the one read-back
        out = torch.cat([op.stats[:steps].reshape(-1), op.flags.to(torch.float32)]).cpu().numpy()
        stats, flags = out[:-1].reshape(steps, 8).astype(np.float64), int(out[-1])
        self.last_stats = stats
        if flags:
            raise _lib.GennbvHipError(f"BehaviourCloning.fit: the loss kernel flagged the demonstrations (flags {flags}: 1 = a candidate "
                                      "index outside its head, 2 = a negative or non-finite weight); such samples took no part")
        if hasattr(enc, "check_operand_ranges"):
            flag = int(enc.check_operand_ranges(raise_on_flag=False)["flag"])
            if flag:
                raise _lib.GennbvHipError(f"BehaviourCloning.fit: an activation left the split-f16 operand range (flag {flag}); the steps "
                                          "of this call may carry clamped results and are not replayed.  The encoder now runs on the "
                                          "fp32-MFMA kernels (force_fp32): restore the parameters and repeat the call")
        return stats


def dagger(model, env, teacher, iterations: int, n_steps: int, betas: Sequence[float], trainer_kwargs: dict, seed: int = 0,
           soft: bool = False, temperature: Optional[float] = None, demos: Optional[Demonstrations] = None, on_iteration=None):
    """DAgger: iteration i collects one block with betas[i] (generator seed + i) into the same Demonstrations -- `demos`, or a new
    store of `iterations` blocks --, then fits on everything stored with ONE BehaviourCloning trainer, whose Adam moments carry
    over.  `trainer_kwargs` are BehaviourCloning's (batch_size, learning_rate, n_epochs, ...; `seed` defaults to this call's).
    `on_iteration(i, demos, trainer, stats)` is called after every fit (evaluation, logging).  The usual schedule starts at
    beta = 1.  Returns the per-iteration statistics: a list of [steps, 8] arrays."""
    iterations = int(iterations)
    if len(betas) < iterations:
        raise ValueError(f"dagger: {iterations} iterations need as many betas, got {len(betas)}")
    kw = dict(trainer_kwargs)
    kw.setdefault("seed", seed)
    trainer, out = None, []
    for i in range(iterations):
        demos = collect_demonstrations(model, env, teacher, n_steps, betas[i], seed + i, soft=soft, temperature=temperature, demos=demos,
                                       capacity_blocks=iterations)
        if trainer is None:
            trainer = BehaviourCloning(model, demos, **kw)
        out.append(trainer.fit())
        if on_iteration is not None:
            on_iteration(i, demos, trainer, out[-1])
    return out
