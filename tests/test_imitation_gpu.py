"""GPU: imitation from the planners end to end (gennbv_amd/sb3/imitation.py) on the closed-loop env of tests/test_closed_loop_gpu.py:
8 envs, a 48 x 64 camera, G = 20, episodes of 6 steps -- collection with a stub teacher and the beta mixture, what the greedy and
the oracle planner expose, fit() against an fp64 CPU twin (tests/torch_reference.TorchHybridEncoder, torch Adam eps 1e-5,
clip_grad_norm_, the loss written with torch: tests/imitation_oracle.torch_loss) under the rules of tests/test_ppo_g64_gpu.py::_compare,
overfitting, the order of fit() and learn() on one policy, an all-dead minibatch, and two DAgger iterations."""
import numpy as np
import pytest
import torch

from tests import imitation_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, G, MAX_LEN = 8, 20, 6
K = 4
TEMP = 0.5
# fit() against the twin: 64 demonstrations, batch 32, 2 epochs = 4 steps.  lr 1e-3: the twin's ce (about 17.7 = the log of the
# lattice's size at the start) has to move by more than 100 x its tolerance 1e-4 max(1, ce) = 0.18 over those steps; the twin alone
# on random tri-class grids and labels moves it by 0.41 with this lr, by 0.05 with 1e-4.
FIT_LR, FIT_BATCH, FIT_EPOCHS = 1e-3, 32, 2
HYPER = dict(label_smoothing=0.1, ent_coef=0.01, vf_coef=0.5)


def _env(n=N, max_len=MAX_LEN, collision=None, seed=3, g=G):
    from gennbv_amd.env import synthetic as S
    from gennbv_amd.env.config import TaskConfig
    from gennbv_amd.env.mesh_scene import MeshScene
    from gennbv_amd.env.render_feed import RenderFeed
    from gennbv_amd.env.replay_feed import ReplayFeedEnv
    cfg = TaskConfig(camera_width=64, camera_height=48, grid_size=g)
    scene = S.make_scenes(n, g, seed=seed)
    feed = RenderFeed(MeshScene.from_boxes(scene, device=DEV), cfg)
    return ReplayFeedEnv(cfg, scene, feed, DEV, max_episode_length=max_len, collision=collision), cfg


def _kwargs(cfg, cls):
    return dict(net_arch=[], features_extractor_class=cls, features_extractor_kwargs=dict(
        encoder_param={"hidden_shapes": [256, 256], "visual_dim": 256},
        net_param={"transformer_params": [[1, 256], [1, 256]], "append_hidden_shapes": [256, 256]},
        state_input_shape=(cfg.state_dim,), visual_input_shape=(cfg.stack, cfg.camera_height, cfg.camera_width)))


def _model(env, cfg, seed=1):
    from gennbv_amd.network.hybrid_encoder import Hybrid_Encoder
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from gennbv_amd.sb3.ppo_grid_obs import PPO_Grid_Obs
    return PPO_Grid_Obs(ActorCriticPolicy_Train_Eval, env, learning_rate=1e-4, n_steps=8, batch_size=32, n_epochs=1, gamma=0.99,
                        gae_lambda=0.95, clip_range=0.2, clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.8, max_grad_norm=1.0,
                        target_kl=None, seed=seed, device=DEV, policy_kwargs=_kwargs(cfg, Hybrid_Encoder))


class StubTeacher:
    """Fixed candidates [N,K,6] and scores [N,K]: at least two positive scores per row, env 3 all refused.  With `constant` every
    env's best candidate is the same tuple.  Records the env's episode_length_buf at every decision."""

    def __init__(self, env, cfg, constant=False):
        gen = torch.Generator().manual_seed(11)
        self.k = K
        cand = torch.stack([torch.randint(int(lo), int(u) + 1, (N, K), generator=gen) for lo, u in zip(cfg.clip_pose_idx_low, cfg.clip_pose_idx_up)], -1)
        score = torch.randint(1, 60, (N, K), generator=gen)
        score[:, 2] = -1             # a refused candidate in every row
        score[5, 0] = score[5, 1]    # a tie
        score[3] = -1                # every candidate refused
        if constant:
            cand[:, 1] = cand[0, 1]
            score[:, 1] = 100
            score[3] = -1
        self.cand, self.score = cand.to(DEV), score.to(DEV)
        self.env, self.elb = env, []
        self.last_candidates = self.last_score = None

    def __call__(self, obs, deterministic=True):
        from gennbv_amd.eval.baselines import choose_scored
        self.elb.append(self.env.episode_length_buf.clone())
        self.last_candidates, self.last_score = self.cand, self.score
        gain = torch.stack([self.score.clamp(min=0), torch.zeros_like(self.score), torch.zeros_like(self.score)], -1)
        best = choose_scored(gain, (1, 0), (self.score < 0).to(torch.uint8))[0]
        return self.cand[torch.arange(N, device=DEV), best], None, None

    @property
    def policy(self):
        return self


class _Tap:
    """Records what the env hands out and is given, and what the student samples, for the duration of a collection."""

    def __init__(self, env, model):
        self.env, self.model, self.obs, self.actions, self.student = env, model, [], [], []

    def __enter__(self):
        env, pol = self.env, self.model.policy
        step, reset, fwd = env.step, env.reset, pol.forward

        def tap_step(a, *args, **kw):
            self.actions.append(a.clone())
            out = step(a, *args, **kw)
            self.obs.append(out[0].clone())
            return out

        def tap_reset(*args, **kw):
            o = reset(*args, **kw)
            self.obs.append(o.clone())
            return o

        def tap_forward(*args, **kw):
            out = fwd(*args, **kw)
            self.student.append(out[0].clone())
            return out
        env.step, env.reset, pol.forward = tap_step, tap_reset, tap_forward
        return self

    def __exit__(self, *exc):
        for obj, names in ((self.env, ("step", "reset")), (self.model.policy, ("forward",))):
            for nm in names:
                obj.__dict__.pop(nm, None)


@pytest.fixture(scope="module")
def world():
    env, cfg = _env()
    return env, cfg, _model(env, cfg)


@pytest.mark.parametrize("beta", [1.0, 0.0, 0.5])
def test_collection_with_a_stub_teacher(world, beta):
    from gennbv_amd.eval.baselines import soft_targets
    from gennbv_amd.sb3.imitation import collect_demonstrations
    env, cfg, model = world
    teacher = StubTeacher(env, cfg)
    T, seed = 14, 5
    model._last_obs = None  # (a fresh start: the collection resets the env)
    with _Tap(env, model) as tap:
        demos = collect_demonstrations(model, env, teacher, T, beta, seed, soft=True, temperature=TEMP)
    assert demos.blocks == 1 and demos.filled == T * N == demos.capacity and demos.k == K
    rows = torch.arange(T * N, device=DEV)
    # stored observations are bit-equal to what the env handed out: the reset observation, then steps 0 .. T-2
    assert len(tap.obs) == T + 1 and len(tap.actions) == T and len(tap.student) == T
    assert torch.equal(demos.dense_rows(rows).view(T, N, -1), torch.stack(tap.obs[:T]))
    assert set(demos.grid_i8.unique().tolist()) <= {-1, 0, 1}
    # labels and weights are the stub's
    assert torch.equal(demos.cand.view(T, N, K, 6), teacher.cand.expand(T, N, K, 6))
    q = soft_targets(teacher.score, TEMP)
    assert torch.equal(demos.cand_w.view(T, N, K), q.expand(T, N, K)) and bool((q[3] == 0).all()) and bool(((q > 0).sum(1)[[0, 1, 2, 4, 5, 6, 7]] >= 2).all())
    # fresh rows and the all-refused row weigh nothing
    elb = torch.stack(teacher.elb)
    fresh = elb == 0
    assert bool(fresh[1:].any()) and not bool(fresh.all()), "no episode ended inside the block"
    want_w = (~fresh).float()
    want_w[:, 3] = 0.0
    assert torch.equal(demos.sample_w.view(T, N), want_w)
    assert torch.equal(demos.episode_starts.view(T, N)[0], torch.ones(N, dtype=torch.uint8, device=DEV))  # (the reset)
    assert torch.equal(demos.episode_starts.view(T, N)[1:].bool(), fresh[1:]), "an episode starts exactly where the env was reset"
    # which action was executed: the seeded draw
    gen = torch.Generator().manual_seed(seed)
    draw = torch.stack([torch.rand(N, generator=gen) < beta for _ in range(T)]).to(DEV)
    assert bool(draw.all()) if beta == 1.0 else (not bool(draw.any()) if beta == 0.0 else (bool(draw.any()) and not bool(draw.all())))
    label = teacher(None)[0]
    student, given = torch.stack(tap.student), torch.stack(tap.actions)
    assert torch.equal(given, torch.where(draw[..., None], label.expand(T, N, 6), student))
    assert torch.equal(demos.last_block["executed"].view(T, N, 6), given) and torch.equal(demos.last_block["took_teacher"].view(T, N), draw)
    if beta == 0.0:
        assert not torch.equal(given, label.expand(T, N, 6))
    # what the env then really flew: the label on non-fresh rows with beta = 1 (it forces the init action on fresh ones)
    if beta == 1.0:
        assert torch.equal(env.actions[~fresh[T - 1]], label[~fresh[T - 1]])
    # returns: the project's GAE kernel over the block with the student's values
    assert bool(torch.isfinite(demos.returns).all()) and float(demos.returns.abs().max()) > 0
    # the model can go on: its rollout state is where the collection ended
    assert torch.equal(model._last_obs, tap.obs[T]) and model._last_obs.data_ptr() != tap.obs[T].data_ptr() and model._pending is None
    assert model._last_episode_starts.shape == (N,)


def test_collection_refuses_what_it_cannot_label(world):
    from gennbv_amd.sb3.imitation import collect_demonstrations
    env, cfg, model = world
    teacher = StubTeacher(env, cfg)
    with pytest.raises(ValueError, match="temperature"):
        collect_demonstrations(model, env, teacher, 2, 1.0, 0, soft=True)
    with pytest.raises(ValueError, match="beta"):
        collect_demonstrations(model, env, teacher, 2, 1.5, 0)
    model.rollout_buffer.compact_state_dim, keep = cfg.state_dim, model.rollout_buffer.compact_state_dim
    try:
        with pytest.raises(ValueError, match="compact"):
            collect_demonstrations(model, env, teacher, 2, 1.0, 0)
    finally:
        model.rollout_buffer.compact_state_dim = keep


@pytest.mark.parametrize("which", ["greedy", "oracle"])
def test_planners_expose_their_candidates_and_the_score_choose_ranked(which):
    from gennbv_amd.env.collision import CollisionBody
    from gennbv_amd.eval.baselines import GreedyGainPolicy, OracleGainPolicy, candidate_score
    env, cfg = _env(max_len=20, collision=CollisionBody(), seed=1)
    pol = GreedyGainPolicy(env, k=8, weights=(1, 4), seed=2) if which == "greedy" else OracleGainPolicy(env, k=8, seed=2)
    assert pol.last_candidates is None and pol.last_score is None
    obs = env.reset()
    refused = 0
    for _ in range(4):
        a = pol(obs)[0]
        cand, score = pol.last_candidates, pol.last_score
        assert cand.shape == (N, 8, 6) and cand.dtype == torch.int64 and score.shape == (N, 8) and score.dtype == torch.int64
        key = score * 8 + (7 - torch.arange(8, device=DEV))
        assert torch.equal(a, cand[torch.arange(N, device=DEV), key.argmax(1)])
        raw, w = (pol.last_gain, (1, 4)) if which == "greedy" else (pol.last_cover, (1, 0))
        want = w[0] * raw[..., 0].long() + w[1] * raw[..., 1].long()
        want = torch.where(pol._contact != 0, torch.full_like(want, -1), want)
        assert torch.equal(score, want) and torch.equal(score, candidate_score(raw, w, pol._contact))
        refused += int((score < 0).sum())
        obs = env.step(a)[0]
    assert refused > 0, "no candidate was ever refused: the contact buffer's part in the score was not exercised"


# ---------------------------------------------------------------------------------------------------------------------------------
def _cpu_demos(demos):
    rows = torch.arange(demos.filled, device=demos.device)
    return dict(obs=demos.dense_rows(rows).cpu(), cand=demos.cand[:demos.filled].cpu(), cand_w=demos.cand_w[:demos.filled].cpu(),
                sample_w=demos.sample_w[:demos.filled].cpu(), returns=demos.returns[:demos.filled].cpu())


def twin_fit(cfg, spaces, state, d, dims, batch, lr, epochs, seed, hyper, max_grad_norm):
    """BehaviourCloning.fit() restated in fp64 on the CPU: (policy, statistics [steps, 8])."""
    from gennbv_amd.sb3.policies import ActorCriticPolicy_Train_Eval
    from tests.torch_reference import TorchHybridEncoder
    pol = ActorCriticPolicy_Train_Eval(spaces[0], spaces[1], lambda _: lr, **_kwargs(cfg, TorchHybridEncoder))
    pol.load_state_dict(state)
    pol.double()
    opt = torch.optim.Adam(pol.parameters(), lr=lr, eps=1e-5)
    pol.train(True)
    eps, ec, vf = (orc.f32(hyper[k]) for k in ("label_smoothing", "ent_coef", "vf_coef"))
    gen = torch.Generator().manual_seed(seed)
    filled = d["obs"].shape[0]
    n_mb = filled // batch
    stats = []
    for _ in range(epochs):
        perm = torch.randperm(filled, generator=gen)[:n_mb * batch].view(n_mb, batch)
        for rows in perm:
            feats = pol.features_extractor(d["obs"][rows].double())
            logits, values = pol.action_net(feats), pol.value_net(feats).flatten()
            t = orc.torch_loss(dims, logits, values, d["cand"][rows], d["cand_w"][rows], d["sample_w"][rows], d["returns"][rows], eps, ec, vf)
            opt.zero_grad()
            t["loss"].backward()
            if max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(pol.parameters(), max_grad_norm)
            opt.step()
            stats.append(orc.stats_row(t))
    return pol, torch.stack(stats).numpy()


@pytest.fixture(scope="module")
def fixed(world):
    """64 demonstrations of the soft stub teacher (8 steps), the policy's initial state, and a hard-label set of the same size."""
    from gennbv_amd.sb3.imitation import collect_demonstrations
    env, cfg, model = world
    soft = collect_demonstrations(model, env, StubTeacher(env, cfg), 8, 1.0, 3, soft=True, temperature=TEMP)
    hard = collect_demonstrations(model, env, StubTeacher(env, cfg, constant=True), 8, 1.0, 4)
    state = {k: v.detach().cpu().clone() for k, v in model.policy.state_dict().items()}
    return soft, hard, state


def _rearm(model, state):
    model.policy.load_state_dict({k: v.to(DEV) for k, v in state.items()})


def test_fit_matches_the_fp64_twin(world, fixed):
    from gennbv_amd.sb3.imitation import BehaviourCloning
    env, cfg, model = world
    demos, _, state = fixed
    assert demos.filled == 64 and 0 < int((demos.sample_w == 0).sum()) < 40
    _rearm(model, state)
    bc = BehaviourCloning(model, demos, FIT_BATCH, FIT_LR, FIT_EPOCHS, seed=7, max_grad_norm=1.0, **HYPER)
    s_h = bc.fit()
    dims = [int(d) for d in model.action_space.nvec]
    ref, s_r = twin_fit(cfg, (model.observation_space, model.action_space), state, _cpu_demos(demos), dims, FIT_BATCH, FIT_LR, FIT_EPOCHS, 7,
                        HYPER, 1.0)
    steps = FIT_EPOCHS * (64 // FIT_BATCH)
    assert s_h.shape == s_r.shape == (steps, 8) and int(bc.state[2].item()) == steps
    print("ce (twin)", s_r[:, 0].tolist(), "ce (hip)", s_h[:, 0].tolist())
    d = np.abs(s_h - s_r) / np.maximum(1.0, np.abs(s_r))
    assert float(d.max()) <= 1e-4, (d.max(0), s_h, s_r)
    assert float(np.abs(s_r[:, 0] - s_r[0, 0]).max()) > 100 * 1e-4 * max(1.0, abs(s_r[0, 0])), "the twin's ce hardly moves: the comparison shows nothing"
    sd_h, sd_r = model.policy.state_dict(), ref.state_dict()
    for k, v in sd_r.items():
        if "running" in k:
            x = sd_h[k].double().cpu()
            assert float((x - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
        if "num_batches" in k:
            assert int(sd_h[k]) == int(v) , k
    diffs = torch.cat([(p.detach().double().cpu() - q.detach()).abs().reshape(-1)
                       for (_, p), (_, q) in zip(model.policy.named_parameters(), ref.named_parameters())])
    assert float(torch.quantile(diffs[::7].float(), 0.999)) <= 2e-4
    assert float(diffs.max()) <= FIT_LR * steps * 1.05


def test_fit_on_compact_int8_rows_matches_the_fp64_twin():
    """G = 32 (a multiple of 16): the encoder's int8 path applies, fit() feeds compact RowGather rows [state | state_rgb] + int8 grid
    + autocorrelation rows instead of materialised fp32 rows.  Same twin, same rules; 64 demonstrations, 2 steps."""
    from gennbv_amd.sb3.imitation import BehaviourCloning, collect_demonstrations
    env, cfg = _env(g=32)
    model = _model(env, cfg)
    demos = collect_demonstrations(model, env, StubTeacher(env, cfg), 8, 1.0, 3, soft=True, temperature=TEMP)
    assert demos.autocorr is not None and demos.grid == 32
    state = {k: v.detach().cpu().clone() for k, v in model.policy.state_dict().items()}
    bc = BehaviourCloning(model, demos, FIT_BATCH, FIT_LR, 1, seed=7, max_grad_norm=1.0, **HYPER)
    assert bc._compact_input(model.policy.features_extractor)
    s_h = bc.fit()
    dims = [int(d) for d in model.action_space.nvec]
    ref, s_r = twin_fit(cfg, (model.observation_space, model.action_space), state, _cpu_demos(demos), dims, FIT_BATCH, FIT_LR, 1, 7, HYPER, 1.0)
    d = np.abs(s_h - s_r) / np.maximum(1.0, np.abs(s_r))
    assert s_h.shape == (2, 8) and float(d.max()) <= 1e-4, (d.max(0), s_h, s_r)
    sd_h = model.policy.state_dict()
    for k, v in ref.state_dict().items():
        if "running" in k:
            assert float((sd_h[k].double().cpu() - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
    diffs = torch.cat([(p.detach().double().cpu() - q.detach()).abs().reshape(-1)
                       for (_, p), (_, q) in zip(model.policy.named_parameters(), ref.named_parameters())])
    assert float(torch.quantile(diffs[::7].float(), 0.999)) <= 2e-4 and float(diffs.max()) <= FIT_LR * 2 * 1.05


def test_fit_overfits_fixed_demonstrations(world, fixed):
    from gennbv_amd.sb3.imitation import BehaviourCloning
    env, cfg, model = world
    _, demos, state = fixed
    _rearm(model, state)
    s = BehaviourCloning(model, demos, 32, 1e-3, 20, seed=1).fit()
    assert s.shape == (40, 8) and np.isfinite(s).all()
    print("ce", s[0, 0], "->", s[-1, 0], "agreement", s[0, 3], "->", s[-1, 3])
    assert s[-1, 0] < s[0, 0] and s[-1, 3] > s[0, 3]


def _params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.policy.parameters()]).clone()


def _in_storage(model, opt):
    lo = opt.params.data_ptr()
    return all(lo <= p.data_ptr() < lo + 4 * opt.n and p.grad is not None and opt.grads.data_ptr() <= p.grad.data_ptr() < opt.grads.data_ptr() + 4 * opt.n
               for p in model.policy.parameters())


@pytest.mark.parametrize("order", ["learn-fit-learn", "fit-learn"])
def test_fit_and_learn_share_one_policy_in_either_order(fixed, order):
    from gennbv_amd.sb3.imitation import BehaviourCloning
    env, cfg = _env()
    model = _model(env, cfg)
    _, demos, _ = fixed
    bc = BehaviourCloning(model, demos, 32, 1e-4, 1, seed=2, max_grad_norm=1.0, **HYPER)
    before = _params(model)
    for phase in order.split("-"):
        if phase == "learn":
            model.learn(total_timesteps=8 * N)
            assert model._hip is not None and _in_storage(model, model._hip["opt"])
        else:
            ppo_opt = model._hip["opt"] if model._hip else None
            keep = None if ppo_opt is None else [t.clone() for t in (ppo_opt.exp_avg, ppo_opt.exp_avg_sq, ppo_opt.step_count)]
            ptrs = None if ppo_opt is None else [t.data_ptr() for t in (ppo_opt.exp_avg, ppo_opt.exp_avg_sq, ppo_opt.step_count)]
            skip_flag = getattr(model.policy.features_extractor, "_bn_skip_flag", None)
            s = bc.fit()
            assert np.isfinite(s).all() and int(bc.state[2].item()) == 2
            assert getattr(model.policy.features_extractor, "_bn_skip_flag", None) is skip_flag
            if ppo_opt is not None:
                assert model._hip["opt"] is ppo_opt and _in_storage(model, ppo_opt)
                now = (ppo_opt.exp_avg, ppo_opt.exp_avg_sq, ppo_opt.step_count)
                assert [t.data_ptr() for t in now] == ptrs and all(torch.equal(a, b) for a, b in zip(now, keep)), "PPO's Adam state changed"
                assert ppo_opt.lr == model.lr_schedule(model._current_progress_remaining), "PPO's learning rate was not put back"
            else:
                assert _in_storage(model, model._imitation_opt)
        after = _params(model)
        assert bool(torch.isfinite(after).all()) and not torch.equal(after, before), f"{phase}: the parameters did not change"
        before = after


def test_an_all_dead_minibatch_changes_nothing(world, fixed):
    from gennbv_amd.sb3.imitation import BehaviourCloning
    env, cfg, model = world
    demos, _, state = fixed
    _rearm(model, state)
    keep_w = demos.sample_w.clone()
    try:
        demos.sample_w.zero_()
        bc = BehaviourCloning(model, demos, 32, 1e-3, 1, seed=3, **HYPER)
        before = {k: v.clone() for k, v in model.policy.state_dict().items()}
        s = bc.fit()
        assert s.shape == (2, 8) and (s == 0).all()
        assert int(bc.state[2].item()) == 0 and float(bc.state[0].abs().max()) == 0.0
        for k, v in model.policy.state_dict().items():
            assert torch.equal(v, before[k]), k
    finally:
        demos.sample_w.copy_(keep_w)


def test_dagger_two_iterations(world, fixed):
    from gennbv_amd.sb3.imitation import Demonstrations, dagger
    env, cfg, model = world
    _rearm(model, fixed[2])
    T = 8
    d_obs = int(env.observation_space.shape[0])
    demos = Demonstrations(2 * T * N, T * N, cfg.state_dim, cfg.grid_dim, d_obs - cfg.state_dim - cfg.grid_dim, K, 6, DEV)
    seen = []
    out = dagger(model, env, StubTeacher(env, cfg), 2, T, [1.0, 0.5], dict(batch_size=32, learning_rate=1e-4, n_epochs=1, **HYPER), seed=9,
                 soft=True, temperature=TEMP, demos=demos,
                 on_iteration=lambda i, d, tr, s: seen.append((i, d.blocks, d.filled, d.last_block["beta"], int(tr.op.flags.item()),
                                                               float(d.last_block["took_teacher"].float().mean()))))
    assert [s[:5] for s in seen] == [(0, 1, T * N, 1.0, 0), (1, 2, 2 * T * N, 0.5, 0)]
    assert seen[0][5] == 1.0 and 0.0 < seen[1][5] < 1.0
    assert [o.shape for o in out] == [(2, 8), (4, 8)] and all(np.isfinite(o).all() for o in out)
    assert all((o[:, 6] > 0).all() for o in out)
