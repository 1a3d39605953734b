"""GPU: the env-step kernels of csrc/envstep.hip at the C ABI (ctypes, default stream) against tests/envstep_ref.py.

Post-step: every field of the state after every step -- bytes, except episode_info, whose fp64 means have a bound:
  [1..2]  |got - exact mean| <= 2^-52 * sum|x_i|   (a sequential fp64 sum of k terms, (k-1) 2^-53 sum|x| before the division
          by k, plus one rounding of the quotient; the reference is math.fsum / k)
  [3..5]  one fp32 ulp of the reference + count * 2^-53 * sum|s| / (count * max_episode_length_s)   (the order of the fp64
          atomics is free; the second term covers cancelling sums)
Observe: gnbv_env_observe and the three separate entry points on clones of one state, both against the reference, as bytes,
the bytes around the two observation slices included."""
import ctypes as C

import numpy as np
import pytest
import torch

from gennbv_amd.env.config import TaskConfig
from tests import envstep_ref as R
from tests.envstep_util import DEV, PostState

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = 1  # hipErrorInvalidValue
BYTE_FIELDS = ("rewards", "dones", "reset_mask", "step_time_out", "extras_time_outs", "coverage_ratio", "prev_ratio", "episode_length_buf",
               "episode_sums", "cur_reward_sum", "cur_episode_length", "ring_state", "ring_reward", "ring_length")


def _lib():
    from gennbv_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------------------
# post-step
# ---------------------------------------------------------------------------
def _ref_of(st):
    return R.PostRef(st.host(), with_info=st.with_info, **st.scalars())


class _PostRun:
    """A device state and its reference, stepped together and compared after every step."""

    def __init__(self, st):
        self.st, self.ref = st, _ref_of(st)
        self.L, self.lib = _lib()
        self.dict_count, self.dict_sum_abs = 0, [0.0, 0.0, 0.0]  # of the step that created the current extras["episode"] dict
        self.step = 0

    def advance(self, grow):
        """What the env does before the post-step: coverage grows (from 0 after a reset), the step is counted."""
        st, ref = self.st, self.ref
        grow = np.asarray(grow, np.int32)
        ref.coverage_count = np.minimum(np.where(ref.reset_mask != 0, grow, ref.coverage_count + grow), ref.num_valid.astype(np.int32))
        ref.episode_length_buf = ref.episode_length_buf + 1
        gd = torch.from_numpy(grow).to(DEV)
        st.coverage_count.copy_(torch.minimum(torch.where(st.reset_mask.bool(), gd, st.coverage_count + gd), st.num_valid.int()))
        st.episode_length_buf += 1

    def post(self, contact=None):
        st = self.st
        if contact is None:
            self.L.check(self.lib.gnbv_env_post_step(C.byref(st.struct()), None), "gnbv_env_post_step")
        else:
            c_dev = torch.from_numpy(contact).to(DEV)
            self.L.check(self.lib.gnbv_env_post_step_contacts(C.byref(st.struct()), c_dev.data_ptr(), None), "gnbv_env_post_step_contacts")
        info = R.post_step(self.ref, contact)
        self.compare(info)
        self.step += 1
        return info

    def compare(self, info):
        ref, got, where = self.ref, self.st.host(), f"step {self.step}"
        for k in BYTE_FIELDS:
            want = np.ascontiguousarray(getattr(ref, k))
            assert got[k].dtype == want.dtype and got[k].shape == want.shape, (where, k)
            if got[k].tobytes() != want.tobytes():
                bad = np.nonzero(got[k].reshape(-1) != want.reshape(-1))[0]
                raise AssertionError(f"{where}: {k} differs at {bad.size} places, first {bad[:8].tolist()}: "
                                     f"got {got[k].reshape(-1)[bad[:8]].tolist()} want {want.reshape(-1)[bad[:8]].tolist()}")
        if not self.st.with_info:
            assert got["episode_info"].tobytes() == ref.episode_info.tobytes() and got["episode_state"].tobytes() == ref.episode_state.tobytes()
            return
        if info["count"]:
            self.dict_count, self.dict_sum_abs = info["count"], info["sum_abs"]
        ei, want = got["episode_info"], ref.episode_info
        assert ei[0] == want[0], (where, ei[0], want[0])
        for j, s_abs in zip((1, 2), info["mean_abs"]):
            assert abs(ei[j] - want[j]) <= 2.0 ** -52 * s_abs, (where, j, ei[j], want[j], s_abs)
        for j in range(3):
            tol = float(np.spacing(f32(abs(want[3 + j]))))
            if self.dict_count:
                tol += self.dict_count * 2.0 ** -53 * self.dict_sum_abs[j] / (self.dict_count * float(ref.max_episode_length_s))
            assert abs(ei[3 + j] - want[3 + j]) <= tol, (where, j, ei[3 + j], want[3 + j], tol)
            assert got["episode_state"][1 + j] == ei[3 + j]
        assert got["episode_state"][0] == ei[0]


def _preload_env_ids(run):
    """cur_episode_length[e] = e (exact in fp32): every ring entry then names its env."""
    ids = np.arange(run.st.n, dtype=f32)
    run.st.cur_episode_length.copy_(torch.from_numpy(ids).to(DEV))
    run.ref.cur_episode_length = ids.copy()


@pytest.mark.parametrize("n,ring_len", [(101, 100), (257, 100), (1024, 100), (1025, 100), (2500, 100), (2500, 1500), (300, 7)])
def test_mass_reset_keeps_the_highest_env_indices_in_the_ring(n, ring_len):
    """Every env finishes on the same step (twice: the second time on a full ring).  More finished envs than ring slots in one
    1024-env tile: the slot's survivor must be the highest env index, as in deque(maxlen).  (2500, 1500): no tile can hold more
    than ring_len finishes; there the ring wraps across tiles and is summed by the global-memory path (ring_len > 1024)."""
    L = 5
    st = PostState(n, TaskConfig(grid_size=4), L, seed=n + ring_len, ring_len=ring_len)
    st.episode_length_buf.zero_()
    run = _PostRun(st)
    _preload_env_ids(run)
    rs = np.random.RandomState(n)
    crowded = wrapped = 0
    for s in range(2 * L + 1):
        run.advance(rs.randint(0, 8, n))
        info = run.post()
        assert info["count"] in (0, n)
        if info["count"]:
            assert info["time_out"].all()
            crowded += info["max_tile_finished"] > ring_len
            wrapped += info["count"] > ring_len
            _preload_env_ids(run)
    assert wrapped == 2 and crowded == (2 if ring_len < R.TILE else 0)
    # the reference's ring (the device's slots equal it byte for byte) holds the last ring_len envs of the second mass reset, in
    # env order: their preloaded index + the L steps of the episode
    assert int(run.ref.ring_state[0]) == 2 * n
    assert [float(v) for v in run.ref.ring_l.dq] == [float(e + L) for e in range(n - ring_len, n)]


def _staggered_inputs(n, L, seed, steps=40):
    rs = np.random.RandomState(seed)
    init = rs.randint(0, L, n).astype(np.int64)
    grows = [rs.randint(0, 5, n) for _ in range(steps)]
    contacts = [((rs.rand(n) < 0.15) * rs.randint(1, 8, n)).astype(np.uint8) for _ in range(steps)]
    return init, grows, contacts


# (n = 1: a seed whose single env starts late enough, and stays free of contacts long enough, to pass lengths 31 and 32)
STAGGERED_SEED = {1: 9, 63: 0, 300: 0, 1500: 0}


@pytest.mark.parametrize("only_positive", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 300, 1500])
def test_staggered_episodes_with_contacts_and_the_short_path_penalty(n, only_positive):
    L = 34  # lengths 31 .. 34 occur: the short-path term with extra = 1 and extra = 2
    init, grows, contacts = _staggered_inputs(n, L, STAGGERED_SEED[n])
    st = PostState(n, TaskConfig(grid_size=4, only_positive_rewards=bool(only_positive)), L, seed=n)
    st.episode_length_buf.copy_(torch.from_numpy(init).to(DEV))
    run = _PostRun(st)
    extras, resets, by_contact = set(), 0, 0
    for grow, contact in zip(grows, contacts):
        run.advance(grow)
        extra = np.clip(run.ref.episode_length_buf - 30, 0, 2)
        info = run.post(contact)
        extras |= set(extra[info["r_short"] != 0].tolist())
        resets += info["count"]
        by_contact += int((info["reset"] & ~info["time_out"]).sum())
    assert extras == {1, 2}, extras
    assert resets >= 1 and (n < 63 or by_contact > n)


def test_coverage_termination_earns_the_termination_reward():
    n, L = 300, 34
    st = PostState(n, TaskConfig(grid_size=4), L, seed=5)
    run = _PostRun(st)
    rs = np.random.RandomState(6)
    s_term = run.ref.scale_term
    assert s_term > 0
    covered = timed_out = 0
    for s in range(30):
        run.advance(rs.randint(0, 40, n))
        info = run.post()
        cov = info["reset"] & ~info["time_out"]
        assert (run.ref.coverage_ratio[cov] > run.ref.coverage_threshold).all()
        assert (info["r_term"][cov] == s_term).all() and (info["r_term"][~cov] == 0).all()
        # (the device rewards are byte-equal to the reference's, whose last term is r_term)
        assert (run.ref.rewards[cov] >= s_term).all()
        covered += int(cov.sum())
        timed_out += int(info["time_out"].sum())
    assert covered >= 20 and timed_out >= 1, (covered, timed_out)


def test_null_episode_info_changes_no_other_field():
    n, L = 300, 7
    base = PostState(n, TaskConfig(grid_size=4), L, seed=8)
    off = base.clone()
    off.with_info = False
    a, b = _PostRun(base), _PostRun(off)
    rs = np.random.RandomState(9)
    resets = 0
    for s in range(20):
        grow = rs.randint(0, 40, n)
        contact = ((rs.rand(n) < 0.1) * rs.randint(1, 8, n)).astype(np.uint8)
        for run in (a, b):
            run.advance(grow)
        resets += a.post(contact)["count"]
        b.post(contact)
        ha, hb = a.st.host(), b.st.host()
        for k in PostState.NAMES:
            if k not in ("episode_info", "episode_state"):
                assert ha[k].tobytes() == hb[k].tobytes(), (s, k)
        assert not hb["episode_info"].any() and not hb["episode_state"].any()
    assert resets > n


def test_ring_total_above_2_pow_33():
    """64-bit ring positions: ring_state = 2^33 + 5 on a full, consistently laid-out ring, then one mass reset."""
    n, L, ring_len = 257, 5, 100
    st = PostState(n, TaskConfig(grid_size=4), L, seed=10, ring_len=ring_len)
    rs = np.random.RandomState(11)
    st.ring_reward.copy_(torch.from_numpy(rs.randn(ring_len).astype(f32)).to(DEV))
    st.ring_length.copy_(torch.from_numpy(rs.randint(1, 40, ring_len).astype(f32)).to(DEV))
    st.ring_state.fill_(2 ** 33 + 5)
    st.episode_length_buf.fill_(L - 2)
    run = _PostRun(st)
    assert len(run.ref.ring_r.dq) == ring_len and run.ref.ring_r.dq[-1] == run.ref.ring_reward[(2 ** 33 + 4) % ring_len]
    _preload_env_ids(run)
    counts = []
    for s in range(2):
        run.advance(rs.randint(0, 8, n))
        counts.append(run.post()["count"])
    assert counts == [0, n]
    assert int(run.st.ring_state.item()) == 2 ** 33 + 5 + n


# ---------------------------------------------------------------------------
# observe
# ---------------------------------------------------------------------------
SENTINEL = -7.25e8
LAT = R.Lattice(clip_low=[-3, 0, 2, 0, 0, -5], clip_up=[80, 80, 50, 0, 12, 12], init_action=[40, 40, 50, 0, 12, 0],
                action_unit=TaskConfig().action_unit, pose_low=TaskConfig().clip_pose_low, init_pose=TaskConfig().init_pose_buf)


def _c_lattice(lat):
    L, _ = _lib()
    c = L.GnbvLattice()
    for i in range(6):
        c.clip_low[i], c.clip_up[i], c.init_action[i] = int(lat.clip_low[i]), int(lat.clip_up[i]), int(lat.init_action[i])
        c.action_unit[i], c.pose_low[i], c.init_pose[i] = float(lat.action_unit[i]), float(lat.pose_low[i]), float(lat.init_pose[i])
    return c


def _actions(rs, n):
    """In range, with rows on both bounds, one past them, negative and at +-2^40 (as many of them as n has rows)."""
    a = np.stack([rs.randint(lo, up + 1, n) for lo, up in zip(LAT.clip_low, LAT.clip_up)], -1).astype(np.int64)
    special = [LAT.clip_low, LAT.clip_up, LAT.clip_low - 1, LAT.clip_up + 1, np.full(6, -7), np.full(6, 2 ** 40), np.full(6, -2 ** 40),
               np.array([2 ** 40, -2 ** 40, 3, -1, 2 ** 40, 0])]
    rows = rs.permutation(n)[:len(special)]
    for e, i in zip(rows, rs.permutation(len(special))):
        a[e] = special[i]
    return a


class _ObsState:
    """Host copy of what the observe entry points read and write; dev() uploads a fresh clone."""
    OUT = ("actions_out", "poses_out", "episode_length_buf", "pose_hist", "gray_prev", "obs")

    def __init__(self, n, stack, oh, ow, seed, alloc_stack=None):
        rs = np.random.RandomState(seed)
        self.n, self.stack, self.oh, self.ow = n, stack, oh, ow
        per = oh * ow
        self.rgb_off = stack * 6 + 5  # a gap between the slices and a tail after them: the sentinel must survive there
        self.row = self.rgb_off + 2 * per + 3
        self.episode_length_buf = (rs.randint(0, 2, n) * rs.randint(1, 9, n)).astype(np.int64)  # zero and nonzero
        if n >= 2:
            self.episode_length_buf[0], self.episode_length_buf[-1] = 0, 4
        self.pose_hist = rs.randn(n, alloc_stack or stack, 6).astype(f32)
        self.gray_prev = rs.randint(0, 256, (n, per)).astype(f32)
        self.actions_out = np.full((n, 6), -99, np.int64)
        self.poses_out = np.full((n, 6), SENTINEL, f32)
        self.obs = np.full((n, self.row), SENTINEL, f32)

    def dev(self):
        return {k: torch.from_numpy(getattr(self, k).copy()).to(DEV) for k in self.OUT}

    def ref_step(self, actions, rgba, mask):
        hist = self.pose_hist[:, :self.stack]
        a, p, s_state, s_rgb = R.observe(actions, LAT, self.episode_length_buf, hist, self.gray_prev, rgba, mask, self.oh, self.ow)
        self.pose_hist[:, :self.stack] = hist
        self.actions_out, self.poses_out = a, p
        self.obs[:, :self.stack * 6] = s_state
        self.obs[:, self.rgb_off:self.rgb_off + 2 * self.oh * self.ow] = s_rgb


def _call_fused(d, s, actions, rgba, mask, h, w, stack=None, stride=None, n=None):
    L, lib = _lib()
    return lib.gnbv_env_observe(actions.data_ptr(), C.byref(_c_lattice(LAT)), d["episode_length_buf"].data_ptr(), s.n if n is None else n,
                                d["actions_out"].data_ptr(), d["poses_out"].data_ptr(), d["pose_hist"].data_ptr(), L.ptr(mask),
                                s.stack if stack is None else stack, d["obs"].data_ptr(), s.row if stride is None else stride, rgba.data_ptr(),
                                d["gray_prev"].data_ptr(), h, w, s.oh, s.ow, d["obs"].data_ptr() + 4 * s.rgb_off, None)


def _call_three(d, s, actions, rgba, mask, h, w):
    L, lib = _lib()
    lat = _c_lattice(LAT)
    L.check(lib.gnbv_env_pre_step(actions.data_ptr(), C.byref(lat), d["episode_length_buf"].data_ptr(), s.n, d["actions_out"].data_ptr(),
                                  d["poses_out"].data_ptr(), None), "gnbv_env_pre_step")
    L.check(lib.gnbv_env_obs_state(d["pose_hist"].data_ptr(), d["poses_out"].data_ptr(), L.ptr(mask), C.byref(lat), s.n, s.stack,
                                   d["obs"].data_ptr(), s.row, None), "gnbv_env_obs_state")
    L.check(lib.gnbv_env_obs_rgb(rgba.data_ptr(), d["gray_prev"].data_ptr(), L.ptr(mask), s.n, h, w, s.oh, s.ow,
                                 d["obs"].data_ptr() + 4 * s.rgb_off, s.row, None), "gnbv_env_obs_rgb")


def _rgba(rs, n, h, w):
    """Random RGBA with 0 and 255 in every channel at a pixel every nearest resize samples (the first one)."""
    x = rs.randint(0, 256, (n, h, w, 4)).astype(np.uint8)
    x[0, 0, 0, :] = 0
    if n > 1:
        x[-1, 0, 0, :] = 255
    return x


def _observe_case(n, stack, h, w, oh, ow, mask_mode, seed):
    L, _ = _lib()
    rs = np.random.RandomState(seed)
    s = _ObsState(n, stack, oh, ow, seed)
    fused, three = s.dev(), s.dev()
    for step in range(2):  # two consecutive steps: the history and the previous gray frame carry over
        actions, rgba = _actions(rs, n), _rgba(rs, n, h, w)
        mask = None
        if mask_mode == "mixed":
            mask = (rs.rand(n) < 0.5).astype(np.uint8) * rs.randint(1, 256, n).astype(np.uint8)
            if n >= 2:
                mask[0], mask[-1] = (0, 200) if step == 0 else (1, 0)
        a_d, r_d = torch.from_numpy(actions).to(DEV), torch.from_numpy(rgba).to(DEV)
        m_d = None if mask is None else torch.from_numpy(mask).to(DEV)
        L.check(_call_fused(fused, s, a_d, r_d, m_d, h, w), "gnbv_env_observe")
        _call_three(three, s, a_d, r_d, m_d, h, w)
        s.ref_step(actions, rgba, mask)
        for k in s.OUT:
            want = np.ascontiguousarray(getattr(s, k)).tobytes()
            gf, gt = fused[k].cpu().numpy().tobytes(), three[k].cpu().numpy().tobytes()
            assert gf == want, f"step {step}: gnbv_env_observe {k}"
            assert gt == want, f"step {step}: three entry points {k}"
            assert gf == gt
        assert a_d.cpu().numpy().tobytes() == actions.tobytes() and r_d.cpu().numpy().tobytes() == rgba.tobytes()  # inputs untouched


@pytest.mark.parametrize("mask_mode", ["null", "mixed"])
@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("stack", [1, 2, 100, 170])
def test_observe_pose_history_depths(stack, n, mask_mode):
    _observe_case(n, stack, 7, 5, 3, 2, mask_mode, seed=stack * 100 + n)


@pytest.mark.parametrize("mask_mode", ["null", "mixed"])
@pytest.mark.parametrize("h,w,oh,ow", [(64, 64, 64, 64), (48, 64, 64, 64), (100, 75, 64, 64), (7, 5, 3, 2), (1, 1, 2, 2)])
def test_observe_resize_shapes(h, w, oh, ow, mask_mode):
    _observe_case(3, 2, h, w, oh, ow, mask_mode, seed=h * 7 + w)


def test_observe_gray_frames_past_the_block_cap():
    """n * oh * ow > 2048 * 256: the gray-frame blocks are capped and every thread strides over several pixels."""
    n, oh, ow = 130, 64, 64
    assert n * oh * ow > 2048 * 256
    _observe_case(n, 2, 48, 64, oh, ow, "mixed", seed=130)


@pytest.mark.parametrize("what", ["stack 171", "stride below stack * 6", "stride below 2 * oh * ow", "n = 0"])
def test_observe_refuses_bad_arguments_and_touches_nothing(what):
    L, lib = _lib()
    n, h, w, oh, ow = 3, 7, 5, 3, 2
    stack = {"stack 171": 170, "stride below stack * 6": 100, "stride below 2 * oh * ow": 1, "n = 0": 2}[what]
    s = _ObsState(n, stack, oh, ow, seed=1, alloc_stack=171)  # (every buffer large enough for the refused arguments)
    if what == "stack 171":
        s.obs = np.full((n, 171 * 6 + 5 + 2 * oh * ow + 3), SENTINEL, f32)
    rs = np.random.RandomState(2)
    a_d, r_d = torch.from_numpy(_actions(rs, n)).to(DEV), torch.from_numpy(_rgba(rs, n, h, w)).to(DEV)
    m_d = torch.ones(n, dtype=torch.uint8, device=DEV)
    kw = {"stack 171": dict(stack=171), "stride below stack * 6": dict(stride=stack * 6 - 1),
          "stride below 2 * oh * ow": dict(stride=2 * oh * ow - 1), "n = 0": dict(n=0)}[what]
    assert kw.get("stride", 10 ** 9) >= min(stack * 6, 2 * oh * ow)  # (only the named check can refuse)
    d = s.dev()
    before = {k: t.cpu().numpy().tobytes() for k, t in d.items()}
    lat = _c_lattice(LAT)
    rets = [_call_fused(d, s, a_d, r_d, m_d, h, w, **kw)]
    st_, stride_, n_ = kw.get("stack", stack), kw.get("stride", s.row), kw.get("n", n)
    if what != "stride below 2 * oh * ow":
        rets.append(lib.gnbv_env_obs_state(d["pose_hist"].data_ptr(), d["poses_out"].data_ptr(), m_d.data_ptr(), C.byref(lat), n_, st_,
                                           d["obs"].data_ptr(), stride_, None))
    if what in ("stride below 2 * oh * ow", "n = 0"):
        rets.append(lib.gnbv_env_obs_rgb(r_d.data_ptr(), d["gray_prev"].data_ptr(), m_d.data_ptr(), n_, h, w, oh, ow,
                                         d["obs"].data_ptr() + 4 * s.rgb_off, stride_, None))
    if what == "n = 0":
        rets.append(lib.gnbv_env_pre_step(a_d.data_ptr(), C.byref(lat), d["episode_length_buf"].data_ptr(), 0, d["actions_out"].data_ptr(),
                                          d["poses_out"].data_ptr(), None))
    assert rets == [INVALID] * len(rets), rets
    torch.cuda.synchronize()
    assert {k: t.cpu().numpy().tobytes() for k, t in d.items()} == before
