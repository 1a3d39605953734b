"""CPU: the numpy reference of the env-step kernels (tests/envstep_ref.py) against what is already pinned -- a plain deque,
the C oracle's gray frames and the oracle env's reward / termination."""
from collections import deque

import numpy as np
import pytest

from gennbv_amd.env.config import TaskConfig
from tests import envstep_ref as R
from tests.envstep_util import contact_oracle_cls

f32 = np.float32
RESIZE_SHAPES = [(64, 64, 64, 64), (48, 64, 64, 64), (100, 75, 64, 64), (7, 5, 3, 2), (1, 1, 2, 2)]


@pytest.mark.parametrize("ring_len", [1, 7, 100])
def test_ring_model_equals_a_deque_and_sequential_slot_stores(ring_len):
    rs = np.random.RandomState(ring_len)
    ring, dq, total = R.RingModel(ring_len), deque(maxlen=ring_len), 0
    slots = np.zeros(ring_len, f32)  # the obvious semantics: one store per append, in order
    big = 0
    for it in range(60):
        k = int(rs.choice([0, 1, 3, ring_len - 1, ring_len, ring_len + 1, 2 * ring_len + 5, 1024]))
        vals = rs.randn(k).astype(f32)
        big += k > ring_len
        ring.extend(vals)
        dq.extend(vals)
        for v in vals:
            slots[total % ring_len] = v
            total += 1
        assert ring.total == total and list(ring.dq) == list(dq)
        assert ring.slots.tobytes() == slots.tobytes()
        kk = len(dq)
        assert [ring.slots[p % ring_len] for p in range(total - kk, total)] == list(dq)
        m, s_abs = ring.mean()
        if kk:
            assert abs(m - float(np.mean(np.array(dq, np.float64)))) <= 2.0 ** -52 * s_abs
        # rebuilt from (slots, total): the same deque
        assert list(R.RingModel(ring_len, total, ring.slots).dq) == list(dq)
    assert big >= 5


@pytest.mark.parametrize("h,w,oh,ow", RESIZE_SHAPES)
def test_gray_frames_equal_the_c_oracle(h, w, oh, ow):
    from oracle import oracle as orc
    rs = np.random.RandomState(h * 100 + w)
    rgba = rs.randint(0, 256, (3, h, w, 4)).astype(np.uint8)
    rgba[0, 0, 0, :] = 0
    rgba[-1, -1, -1, :] = 255
    got = R.gray_resized(rgba, oh, ow)
    want = orc.rgb_to_gray64(rgba, oh, ow).reshape(3, oh * ow)
    assert got.tobytes() == want.tobytes()
    src = R.resize_source_index(h, w, oh, ow)
    assert src.shape == (oh * ow,) and src.min() >= 0 and src.max() < h * w


@pytest.mark.parametrize("only_positive", [False, True])
def test_post_step_equals_the_oracle_env_reward_and_termination(only_positive):
    n, L = 300, 34
    cfg = TaskConfig(grid_size=4, only_positive_rewards=only_positive)
    rs = np.random.RandomState(3)
    num_valid = (200 + rs.randint(0, 100, n)).astype(f32)
    o = contact_oracle_cls()(cfg, np.eye(3, dtype=f32), np.zeros((n, 6), f32), np.ones((n, 3), f32), np.zeros((n, 4, 4, 4), f32),
                             num_valid, max_episode_length=L)
    o.episode_length_buf = rs.randint(0, L, n).astype(np.int64)
    z = lambda *s, dt=f32: np.zeros(s, dt)  # noqa: E731
    arrays = dict(coverage_count=z(n, dt=np.int32), num_valid=num_valid, prev_ratio=z(n), episode_length_buf=o.episode_length_buf.copy(),
                  rewards=z(n), dones=z(n, dt=np.uint8), reset_mask=z(n, dt=np.uint8), step_time_out=z(n, dt=np.uint8),
                  extras_time_outs=z(n, dt=np.uint8), coverage_ratio=z(n), episode_sums=z(3, n), cur_reward_sum=z(n),
                  cur_episode_length=z(n), ring_reward=z(100), ring_length=z(100), ring_state=z(1, dt=np.int64),
                  episode_info=z(6, dt=np.float64), episode_state=z(4, dt=np.float64))
    st = R.PostRef(arrays, only_positive=only_positive, max_episode_length=L, scale_cov=f32(cfg.scale_surface_coverage * cfg.dt),
                   scale_short=f32(cfg.scale_short_path * cfg.dt), scale_term=f32(cfg.scale_termination * cfg.dt),
                   coverage_threshold=f32(cfg.coverage_threshold), ring_len=100, max_episode_length_s=f32(cfg.episode_length_s))
    rew_dq, len_dq = deque(maxlen=100), deque(maxlen=100)
    cur_r, cur_l = np.zeros(n, f32), np.zeros(n, f32)
    short, contacts, covered = 0, 0, 0
    for s in range(80):
        grow = rs.randint(0, 25, n).astype(np.int32)
        st.coverage_count = np.minimum(np.where(st.reset_mask != 0, grow, st.coverage_count + grow), num_valid.astype(np.int32))
        st.episode_length_buf += 1
        o.episode_length_buf += 1
        contact = ((rs.rand(n) < 0.05) * rs.randint(1, 8, n)).astype(np.uint8)
        o.contact = contact
        rew, reset, time_out, ratio = o._reward_done(st.coverage_count)
        o.prev_ratio = np.where(reset, f32(0), ratio).astype(f32)
        o.episode_length_buf[reset] = 0
        info = R.post_step(st, contact)
        assert st.rewards.tobytes() == rew.tobytes(), f"step {s}"
        assert np.array_equal(st.dones.astype(bool), reset) and np.array_equal(st.reset_mask.astype(bool), reset)
        assert np.array_equal(st.step_time_out.astype(bool), time_out)
        assert st.coverage_ratio.tobytes() == ratio.tobytes() and st.prev_ratio.tobytes() == o.prev_ratio.tobytes()
        assert np.array_equal(st.episode_length_buf, o.episode_length_buf)
        assert info["r_term"].tobytes() == o.term.tobytes()
        # the episode ring against the style of the env-level host recomputation
        cur_r, cur_l = (cur_r + rew).astype(f32), (cur_l + f32(1)).astype(f32)
        for e in np.nonzero(reset)[0]:
            rew_dq.append(cur_r[e]); len_dq.append(cur_l[e]); cur_r[e] = 0; cur_l[e] = 0
        assert list(st.ring_r.dq) == list(rew_dq) and list(st.ring_l.dq) == list(len_dq)
        assert int(st.ring_state[0]) == st.ring_r.total
        assert st.cur_reward_sum.tobytes() == cur_r.tobytes() and st.cur_episode_length.tobytes() == cur_l.tobytes()
        if rew_dq:
            np.testing.assert_allclose(st.episode_info[1:3], [np.mean(rew_dq), np.mean(len_dq)], rtol=1e-6)
        short += int((info["r_short"] != 0).sum())
        contacts += int((reset & ~time_out & (contact != 0)).sum())
        covered += int((reset & ~time_out & (contact == 0)).sum())
    assert short > 20 and contacts > 20 and covered > 20, (short, contacts, covered)
