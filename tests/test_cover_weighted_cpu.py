"""CPU: the numpy reference of gnbv_cover_greedy_w -- its lazy form equals its exhaustive form, one plane of weight 1 is
gnbv_cover_greedy's reference, the weights change a plan on random planes and on the view-gain oracle's masks; the entry point
is declared, exported and bound and refuses bad arguments before any launch; plan_weighted's and MapCoverPolicy(mask="mixed")'s
refusals, and the policy's keep / adopt / cursor logic on the stubs of tests/test_gain_masks_cpu.py's kind."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import cover_greedy_oracle as CG
from tests import cover_weighted_oracle as CW
from tests import gain_masks_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # hipErrorInvalidValue


def _random_case(rng, trial, planes=None, k_min=1, all_contact_every=3):
    k, words, waves = int(rng.integers(k_min, 40)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
    planes = int(rng.integers(1, 5)) if planes is None else planes
    rounds = int(rng.integers(1, k + 4))
    masks = [CG.random_masks(rng, k, words, rng.choice([0.02, 0.2, 0.5])) for _ in range(planes)]
    if k > 3:
        for m in masks:  # duplicated and empty rows, per plane
            m[rng.integers(k)] = m[rng.integers(k)]
            m[rng.integers(k)] = 0
        a, b = rng.integers(k), rng.integers(k)  # one candidate equal to another in every plane: an exact tie of the scores
        for m in masks:
            m[a] = m[b]
    weights = [int(w) for w in rng.integers(0, 17, planes)]
    if trial % 5 == 0:
        weights[int(rng.integers(planes))] = 0
    if trial % 41 == 0:
        weights = [0] * planes
    cov = [CG.random_masks(rng, 1, words, 0.3)[0] for _ in range(planes)]
    contact = np.zeros(k, np.uint8)
    if trial % all_contact_every == all_contact_every - 1:
        contact[:] = 1
    elif trial % 2 == 1:
        contact = (rng.random(k) < 0.3).astype(np.uint8)
    return masks, cov, weights, contact, rounds, waves


def test_lazy_reference_equals_exhaustive_reference():
    """400 seeded cases, 1..4 independent planes, weights 0..16 with zeros, ties, duplicated and empty rows, no / random / all
    contacts, 1..8 evaluations per pass: the same choices, scores, plane gains and covered sets; the bounds at exit are upper
    bounds of the scores against the final sets; rounds split over two calls carrying `ub` equal one call."""
    rng = np.random.default_rng(0)
    evals = total = 0
    for trial in range(400):
        masks, cov, weights, contact, rounds, waves = _random_case(rng, trial)
        k = masks[0].shape[0]
        a = CW.exhaustive(masks, cov, weights, contact, rounds)
        b = CW.lazy(masks, cov, weights, contact, rounds, waves=waves)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), trial
        assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])), trial
        assert np.array_equal(a[1], (a[2] * np.asarray(weights)).sum(1)), trial  # the score is the weighted sum of the plane gains
        assert (b[4] >= CW.scores(masks, b[3], weights)).all(), trial
        r1 = rounds // 2
        if r1 >= 1:
            c = CW.lazy(masks, cov, weights, contact, r1, waves=waves)
            d = CW.lazy(masks, c[3], weights, contact, rounds - r1, ub=c[4], waves=waves)
            assert np.array_equal(np.concatenate([c[0], d[0]]), a[0]) and np.array_equal(np.concatenate([c[1], d[1]]), a[1]), trial
            assert np.array_equal(np.concatenate([c[2], d[2]]), a[2]) and all(np.array_equal(x, y) for x, y in zip(d[3], a[3])), trial
        evals += b[5]
        total += k * rounds
    print("lazy evaluations", evals, "of", total)
    assert evals < total


def test_the_weights_change_the_plan_on_random_planes():
    """A condition on the inputs: in at least half of the two-plane cases with both weights positive the weighted choice
    sequence differs from the sequence of either plane alone -- otherwise a kernel that ignored a plane would pass.  (Cases
    with all candidates in contact or with k < 3 cannot differ: this test draws fewer of them than the one above.)"""
    rng = np.random.default_rng(1)
    cases = differ = 0
    for trial in range(300):
        masks, cov, weights, contact, rounds, _ = _random_case(rng, trial, planes=2, k_min=3, all_contact_every=10)
        if min(weights) == 0:
            continue
        cases += 1
        both = CW.exhaustive(masks, cov, weights, contact, rounds)[0]
        only0 = CW.exhaustive(masks, cov, [1, 0], contact, rounds)[0]
        only1 = CW.exhaustive(masks, cov, [0, 1], contact, rounds)[0]
        differ += (not np.array_equal(both, only0)) and (not np.array_equal(both, only1))
    print("two-plane cases with both weights positive", cases, "whose plan differs from both single-plane plans", differ)
    assert cases >= 150 and 2 * differ >= cases


def test_one_plane_is_the_unweighted_reference():
    rng = np.random.default_rng(2)
    for trial in range(60):
        masks, cov, _, contact, rounds, _ = _random_case(rng, trial, planes=1)
        ref = CG.exhaustive(masks[0], cov[0], contact, rounds)
        one = CW.exhaustive(masks, cov, [1], contact, rounds)
        assert np.array_equal(one[0], ref[0]) and np.array_equal(one[1], ref[1]) and np.array_equal(one[2][:, 0], ref[1])
        assert np.array_equal(one[3][0], ref[2]) and np.array_equal(one[4], ref[3])
        w = int(rng.integers(2, 17))
        many = CW.exhaustive(masks, cov, [w], contact, rounds)
        assert np.array_equal(many[0], ref[0]) and np.array_equal(many[1], w * ref[1]) and np.array_equal(many[2][:, 0], ref[1])
        assert np.array_equal(many[4], w * ref[3])


def test_a_tie_across_planes_goes_to_the_lower_index():
    """A: 4 bits in plane 0, B: 1 bit in plane 1, weights (1, 4): both score 4."""
    zero, none = [np.zeros(1, np.uint32)] * 2, np.zeros(2, np.uint8)
    a_first = [np.array([[0b1111], [0]], np.uint32), np.array([[0], [0b1]], np.uint32)]
    ch, gn, pg, cov, g0 = CW.exhaustive(a_first, zero, [1, 4], none, 3)
    assert g0.tolist() == [4, 4] and ch.tolist() == [0, 1, 0] and gn.tolist() == [4, 4, 0] and pg.tolist() == [[4, 0], [0, 1], [0, 0]]
    assert cov[0].tolist() == [0b1111] and cov[1].tolist() == [0b1]
    b_first = [m[::-1].copy() for m in a_first]
    ch, gn, pg, _, _ = CW.exhaustive(b_first, zero, [1, 4], none, 2)
    assert ch.tolist() == [0, 1] and gn.tolist() == [4, 4] and pg.tolist() == [[0, 1], [4, 0]]
    assert CW.lazy(a_first, zero, [1, 4], none, 3, waves=1)[0].tolist() == [0, 1, 0]
    assert CW.exhaustive(a_first, zero, [1, 5], none, 1)[0].tolist() == [1]  # (and the weight decides where there is no tie)
    ch, gn, _, _, _ = CW.exhaustive(a_first, zero, [0, 0], np.array([1, 0], np.uint8), 2)  # all weights 0: the lowest not in contact
    assert ch.tolist() == [1, 1] and gn.tolist() == [0, 0]


G, H, W, K, STRIDE, RANGE = 20, 60, 80, 8, 4, 50.0
CFG = TaskConfig(camera_width=W, camera_height=H, grid_size=G)


def test_the_weights_change_a_plan_on_view_gain_masks():
    """One env at 20^3, occupied density 0.1, 8 lattice candidates (tests/test_gain_masks_cpu.py's case at the denser grid)."""
    from gennbv_amd.eval.baselines import LatticeCandidates
    sc = S.make_scenes(1, G, seed=2)
    tri = MO.random_tri(1, G, 0.1, seed=21).numpy()
    lc = LatticeCandidates(CFG, K, 20)
    poses = lc.poses(lc.sample(1))
    c2w = S.camera_to_world(poses.view(-1, 6)).float().view(1, K, 4, 4).numpy()
    kinv = S.inverse_intrinsics(H, W, CFG.horizontal_fov).numpy()
    ub, hb = MO.masks(tri, c2w, sc.range_gt.numpy(), sc.voxel_size.numpy(), kinv, H, W, STRIDE, RANGE, words=MO.min_words(G))
    masks, zero, none = [ub[0], hb[0]], [np.zeros(ub.shape[-1], np.uint32)] * 2, np.zeros(K, np.uint8)
    plans = {w: CW.exhaustive(masks, zero, list(w), none, 4) for w in ((1, 0), (0, 1), (1, 4), (1, 16))}
    for w, p in plans.items():
        print("weights", w, "choice", p[0].tolist(), "gain", p[1].tolist(), "plane gains", p[2].tolist())
    assert plans[(1, 4)][0].tolist() == [5, 3, 1, 0] and plans[(1, 4)][1].tolist() == [2388, 1550, 403, 391]
    assert plans[(1, 16)][0].tolist() == [5, 3, 0, 1]
    assert plans[(1, 0)][0].tolist() == [5, 3, 1, 0] and plans[(0, 1)][0].tolist() == [5, 3, 0, 1]
    for w in ((1, 4), (1, 16)):
        choice, gain, pg, cov, g0 = plans[w]
        seen = [np.zeros_like(m[0]) for m in masks]
        for t, j in enumerate(choice):
            assert pg[t].tolist() == [int(CG.popcount(m[j] & ~s)) for m, s in zip(masks, seen)]
            seen = [s | m[j] for m, s in zip(masks, seen)]
        assert np.array_equal(g0, w[0] * CG.popcount(ub[0]) + w[1] * CG.popcount(hb[0]))
        assert [int(CG.popcount(c)) for c in cov] == pg.sum(0).tolist()


def test_header_declares_and_library_exports_the_entry_point():
    from gennbv_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gennbv_hip.h")).read()
    assert re.search(r"\bint\s+gnbv_cover_greedy_w\s*\(\s*const\s+GnbvCoverGreedyW\s*\*", hdr)
    assert _lib.SIGNATURES["gnbv_cover_greedy_w"] == (C.c_int, [C.c_void_p, C.c_void_p])
    lib = _lib.load()
    assert lib.gnbv_cover_greedy_w is not None and lib.gnbv_abi_version() == 5
    body = re.search(r"typedef struct GnbvCoverGreedyW \{(.*?)\} GnbvCoverGreedyW;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
    names = [re.sub(r"\[4\]$", "", re.split(r"[\s\*]+", n)[-1]) for n in names]
    assert names == [f[0] for f in _lib.GnbvCoverGreedyW._fields_]
    arrays = {f[0] for f in _lib.GnbvCoverGreedyW._fields_ if hasattr(f[1], "_length_")}
    assert arrays == {"weight", "mask_bits", "covered_in", "covered_out"} == set(re.findall(r"(\w+)\[4\]", body))
    assert C.sizeof(_lib.GnbvCoverGreedyW) == 5 * 4 + 4 * 4 + 4 + 12 * 8 + 6 * 8 + 8  # (one pad int before the pointers)


def _args(**kw):
    """A GnbvCoverGreedyW the entry point accepts, on made-up aligned pointers (never dereferenced: a refusal comes first).
    A keyword names a scalar field, or `field_p` for entry p of an array field."""
    from gennbv_amd import _lib
    c = _lib.GnbvCoverGreedyW()
    c.n, c.k, c.words, c.rounds, c.lazy, c.planes = 2, 3, 8, 2, 1, 2
    for p in range(2):
        c.weight[p], c.mask_bits[p], c.covered_out[p] = 1 + 3 * p, 0x1000 * (p + 1), 0x10000 * (p + 1)
    c.choice = c.gain = 0x100000
    for f, v in kw.items():
        m = re.fullmatch(r"(\w+)_(\d)", f)
        if m:
            getattr(c, m.group(1))[int(m.group(2))] = v
        else:
            setattr(c, f, v)
    return c


def test_invalid_arguments_are_refused_before_any_launch():
    from gennbv_amd import _lib
    lib = _lib.load()
    assert lib.gnbv_cover_greedy_w(None, None) == INVALID
    bad = [dict(n=0), dict(n=65536), dict(k=0), dict(k=4097), dict(rounds=0), dict(rounds=4097), dict(words=0), dict(words=6),
           dict(words=-4), dict(lazy=2), dict(lazy=-1), dict(choice=None), dict(gain=None),  # gnbv_cover_greedy's
           dict(planes=0), dict(planes=5), dict(planes=-1)]
    for p in (0, 1):  # ... and applied to each used plane
        bad += [{f"mask_bits_{p}": None}, {f"covered_out_{p}": None}, {f"mask_bits_{p}": 0x1004}, {f"covered_in_{p}": 0x2008},
                {f"covered_out_{p}": 0x3001}, {f"weight_{p}": -1}]
    bad += [dict(planes=3), dict(planes=4),                      # plane 2 is now used: its mask_bits is NULL
            dict(covered_out_1=0x10000),                         # two planes sharing one covered_out
            dict(planes=3, mask_bits_2=0x3000, covered_out_2=0x20000, weight_2=2),
            dict(weight_0=2 ** 31 - 1, weight_1=1),              # the weights' sum alone is past int32
            dict(words=1 << 20, weight_0=32, weight_1=32),       # 64 * 32 * 2^20 = 2^31
            dict(weight_0=(2 ** 31 - 1) // 256 + 1, weight_1=0),  # one past the largest sum that fits at words = 8
            dict(words=1 << 26)]
    for kw in bad:
        assert lib.gnbv_cover_greedy_w(C.byref(_args(**kw)), None) == INVALID, kw


def test_operator_refuses_weights_missing_masks_and_bad_arguments():
    from gennbv_amd import _lib
    from gennbv_amd.ops import gain_masks as GM
    assert GM.plan_weights((1, 4), 252) == (1, 4) and GM.plan_weights([0, 0], 252) == (0, 0)
    assert GM.plan_weights((np.int64(3), 2.0), 252) == (3, 2)
    top = (2 ** 31 - 1) // (32 * 252)
    assert GM.plan_weights((top, 0), 252) == (top, 0)
    for weights, why in (((1, -1), ">= 0"), ((-4, 1), ">= 0"), ((1,), "two integers"), ((1, 2, 3), "two integers"), ((1.5, 2), "two integers"),
                         (3, "two integers"), (("a", 1), "two integers"), ((top, 1), "int32"), ((1, top), "int32")):
        with pytest.raises(_lib.GennbvHipError, match=why):
            GM.plan_weights(weights, 252)
    # the method's own refusals come before anything touches the device: an instance that never saw the GPU shows them
    op = object.__new__(GM.ViewGainMasks)
    op.words, op.num_envs, op.k = 252, 2, 3
    op.unknown_bits, op.hit_bits = torch.zeros(2, 3, 252, dtype=torch.int32), None
    with pytest.raises(_lib.GennbvHipError, match="the hit mask is not kept"):
        op.plan_weighted(2)
    op.unknown_bits, op.hit_bits = None, torch.zeros(2, 3, 252, dtype=torch.int32)
    with pytest.raises(_lib.GennbvHipError, match="the unknown mask is not kept"):
        op.plan_weighted(2)
    op.unknown_bits = op.hit_bits
    for rounds in (0, 4097):
        with pytest.raises(_lib.GennbvHipError, match="rounds"):
            op.plan_weighted(rounds)
    with pytest.raises(_lib.GennbvHipError, match=">= 0"):
        op.plan_weighted(2, weights=(1, -4))
    with pytest.raises(_lib.GennbvHipError, match="no CPU fallback"):
        op.plan_weighted(2, contact=torch.zeros(2, 3, dtype=torch.uint8))
    with pytest.raises(_lib.GennbvHipError, match="pair"):
        op.plan_weighted(2, covered_bits=torch.zeros(2, 252, dtype=torch.int32))
    with pytest.raises(_lib.GennbvHipError, match="no CPU fallback"):
        op.plan_weighted(2, covered_bits=(torch.zeros(2, 252, dtype=torch.int32),) * 2)


# ---------------------------------------------------------------------------
# MapCoverPolicy(mask="mixed") on stubs
# ---------------------------------------------------------------------------
N, KP = 2, 6
OBS = torch.zeros(N, CFG.obs_dim)
ROWS = torch.arange(N)


class _Masks:
    """ViewGainMasks' protocol with plan_weighted; hands out the scripted (choice, gain, plane_gain) of each decision in turn."""

    def __init__(self, script):
        self.script, self.i, self.asked, self.plane_gain = script, 0, [], None

    def __call__(self, tri, poses):
        return torch.zeros(N, KP, 3, dtype=torch.int32)

    def plan(self, rounds, which="hit", contact=None, covered_bits=None, lazy=True):
        raise AssertionError("mask='mixed' plans with plan_weighted")

    def plan_weighted(self, rounds, weights=(1, 4), contact=None, covered_bits=None, lazy=True):
        choice, gain = self.script[self.i]
        self.i += 1
        self.asked.append((rounds, tuple(weights), contact.clone()))
        assert covered_bits is None
        self.plane_gain = torch.full((N, rounds, 2), self.i, dtype=torch.int32)
        return torch.tensor(choice, dtype=torch.int32), torch.tensor(gain, dtype=torch.int32), (None, None)


class _Flight:
    belief, shortcut = True, False

    def __init__(self):
        self.ok = torch.ones(N, KP, dtype=torch.bool)

    def reachable(self, poses):
        return self.ok.clone()


def _policy(script, seed=3, **kw):
    from gennbv_amd.eval.baselines import LatticeCandidates, MapCoverPolicy
    env = types.SimpleNamespace(cfg=CFG, num_envs=N, device="cpu", collision=None, flight=_Flight(), poses=torch.zeros(N, 6),
                                episode_length_buf=torch.full((N,), 5, dtype=torch.int64))
    pol = MapCoverPolicy(env, k=KP, seed=seed, masks_backend=_Masks(script), **kw)
    return env, pol, LatticeCandidates(CFG, KP, seed)  # the twin draws what the policy draws, decision by decision


def _pick(cand, idx):
    return cand[ROWS, torch.tensor(idx)]


@pytest.mark.parametrize("kw", [dict(mask="hit", weights=(1, 4)), dict(mask="unknown", weights=(1, 0)), dict(mask="hit", weights=(0, 1)),
                                dict(mask="mixed", weights=(1, -4)), dict(mask="mixed", weights=(1, 2, 3)), dict(mask="mixed", weights=(1.5, 1)),
                                dict(mask="both", weights=(1, 4)), dict(mask="both")])
def test_policy_refuses_weights_without_mixed_and_bad_weights(kw):
    with pytest.raises(ValueError):
        _policy([], **kw)


def test_signature_ends_with_weights_and_the_single_mask_modes_keep_their_weights():
    import inspect
    from gennbv_amd.eval.baselines import MapCoverPolicy
    params = list(inspect.signature(MapCoverPolicy.__init__).parameters)
    assert params[-1] == "weights" and params[-3:-1] == ["masks_backend", "tour_backend"]
    assert _policy([], mask="mixed")[1].weights == (1, 4) and _policy([], mask="mixed", weights=[2, 0])[1].weights == (2, 0)
    assert _policy([], mask="hit")[1].weights == (0, 1) and _policy([], mask="unknown")[1].weights == (1, 0)
    assert _policy([], mask="hit")[1].last_plane_gain is None


def test_mixed_weights_reach_the_backend_and_commit_adopt_and_cursor_are_unchanged():
    """tests/test_gain_masks_cpu.py's commit and restart scripts, flown through plan_weighted."""
    plan = ([[1, 2, 3], [4, 5, 0]], [[9, 5, 2], [7, 3, 1]])
    other = ([[0, 1, 2], [3, 2, 1]], [[8, 4, 2], [6, 5, 4]])
    env, pol, twin = _policy([plan, other, other, other, other], horizon=3, commit=2, mask="mixed", weights=(2, 7))
    c = [twin.sample(N) for _ in range(5)]
    a0 = pol(OBS)[0]
    assert a0.dtype == torch.int64 and a0.shape == (N, 6)
    assert bool(pol.adopted.all()) and pol.last_views.tolist() == [3, 3] and pol.last_length_mm.tolist() == [-1, -1]
    assert torch.equal(a0, _pick(c[0], [1, 4])) and pol.last_plane_gain is pol.gain_backend.plane_gain
    a1 = pol(OBS)[0]  # the stored plan continues; the new one is computed all the same
    assert not bool(pol.adopted.any()) and torch.equal(a1, _pick(c[0], [2, 5]))
    assert torch.equal(pol.last_choice, torch.tensor(other[0], dtype=torch.int32)) and torch.equal(pol.last_actions[:, 0], _pick(c[1], [0, 3]))
    assert bool((pol.last_plane_gain == 2).all())  # the second decision's
    a2 = pol(OBS)[0]  # cursor == commit: the third view is never flown
    assert bool(pol.adopted.all()) and torch.equal(a2, _pick(c[2], [0, 3]))
    assert torch.equal(pol.predict(OBS)[0], _pick(c[2], [1, 2]))
    assert torch.equal(pol(OBS)[0], _pick(c[4], [0, 3]))
    assert pol.gain_backend.i == 5 and all(r == 3 and w == (2, 7) for r, w, _ in pol.gain_backend.asked)
    # a restart adopts per env, and a refused choice is dropped from the kept views
    env, pol, twin = _policy([plan, other, other], horizon=3, commit=3, mask="mixed")
    c = [twin.sample(N) for _ in range(3)]
    env.flight.ok[0, 2] = False
    assert torch.equal(pol(OBS)[0], _pick(c[0], [1, 4])) and pol.last_views.tolist() == [2, 3]
    assert pol.gain_backend.asked[0][1] == (1, 4) and pol.gain_backend.asked[0][2].tolist() == [[0, 0, 1, 0, 0, 0], [0] * 6]
    env.flight.ok[0, 2] = True
    env.episode_length_buf[0] = 1
    a1 = pol(OBS)[0]
    assert pol.adopted.tolist() == [True, False] and pol.cursor.tolist() == [1, 2]
    assert torch.equal(a1[0], c[1][0, 0]) and torch.equal(a1[1], c[0][1, 5])


def test_mixed_horizon_one_is_the_greedy_choice():
    from gennbv_amd.eval.baselines import choose
    gain3 = torch.tensor([[[3, 1, 0], [7, 0, 0], [6, 2, 0], [0, 0, 0], [1, 3, 0], [2, 0, 0]]] * 2, dtype=torch.int32)
    picks = set()
    for w in ((1, 4), (4, 1), (1, 0), (0, 1)):
        best = choose(gain3, w)
        score = [int(w[0] * gain3[e, best[e], 0] + w[1] * gain3[e, best[e], 1]) for e in range(N)]
        env, pol, twin = _policy([([[int(best[0])], [int(best[1])]], [[score[0]], [score[1]]])] * 2, horizon=1, mask="mixed", weights=w)
        for _ in range(2):
            cand = twin.sample(N)
            assert torch.equal(pol(OBS)[0], cand[ROWS, best]) and bool(pol.adopted.all())
        picks.add(int(best[0]))
    assert len(picks) >= 3  # (the weights matter on this gain table)
