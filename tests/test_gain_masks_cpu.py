"""CPU: the view-gain masks' oracle against the view-gain oracle, a set-cover plan on its masks that top-T would not make, the new
entry point's export and its refusals (all made before any launch, so they need no GPU), and MapCoverPolicy's keep / order / adopt
logic on CPU tensors with stubs for the masks op, the flight field and the tour (the injection points exist for tests; the product
path has no CPU fallback)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import cover_greedy_oracle as CO
from tests import gain_masks_oracle as MO
from tests import view_gain_oracle as VO

G, H, W, K, STRIDE, RANGE = 20, 60, 80, 8, 4, 50.0
CFG = TaskConfig(camera_width=W, camera_height=H, grid_size=G)
INVALID = 1  # hipErrorInvalidValue


@pytest.fixture(scope="module")
def case():
    """One env at 20^3, occupied density 0.05, 8 lattice candidates: the masks and the gains of both oracles, computed once."""
    from gennbv_amd.eval.baselines import LatticeCandidates
    sc = S.make_scenes(1, G, seed=2)
    tri = MO.random_tri(1, G, 0.05, seed=21).numpy()
    lc = LatticeCandidates(CFG, K, 20)
    poses = lc.poses(lc.sample(1))
    c2w = S.camera_to_world(poses.view(-1, 6)).float().view(1, K, 4, 4).numpy()
    kinv = S.inverse_intrinsics(H, W, CFG.horizontal_fov).numpy()
    args = (tri, c2w, sc.range_gt.numpy(), sc.voxel_size.numpy(), kinv, H, W, STRIDE, RANGE)
    ub, hb = MO.masks(*args, words=MO.min_words(G) + 4)
    return dict(tri=tri, ub=ub, hb=hb, gain=VO.view_gain(*args))


def test_oracle_popcounts_subsets_and_bounds(case):
    tri, ub, hb, gain = case["tri"], case["ub"], case["hb"], case["gain"]
    assert ub.shape == hb.shape == (1, K, MO.min_words(G) + 4) and MO.min_words(G) == 252 and MO.min_words(33) == 1124
    assert np.array_equal(CO.popcount(ub), gain[..., 0]) and np.array_equal(CO.popcount(hb), gain[..., 1])
    assert gain[..., 0].min() > 0 and gain[..., 1].max() > 0
    assert not (hb & ~ub).any()  # H is a subset of U
    bits = MO.unpack(ub)
    assert not bits[..., G ** 3:].any()  # no bit at or past G^3
    assert not (bits[0, :, :G ** 3] & (tri[0] != 0)[None]).any()  # only unknown voxels


def test_bits_of_layout():
    w = MO.bits_of([0, 31, 32, 33, 33, 95], 4)
    assert w.tolist() == [0x80000001, 0x3, 0x80000000, 0]
    assert MO.unpack(w).nonzero()[0].tolist() == [0, 31, 32, 33, 95]


@pytest.mark.parametrize("which", ["ub", "hb"])
def test_set_cover_on_the_masks_is_not_top_t(case, which):
    """Some later round's gain is below what its candidate would add alone: the plan saw the overlap."""
    masks = case[which][0]
    choice, gain, covered, gains0 = CO.exhaustive(masks, np.zeros(masks.shape[1], np.uint32), np.zeros(K, np.uint8), 4)
    print(which, "plan", choice.tolist(), "gains", gain.tolist(), "gains0", gains0.tolist())
    assert gain[0] == gains0[choice[0]] == gains0.max()
    assert any(gain[t] < gains0[choice[t]] for t in range(1, 4))
    assert len(set(choice.tolist())) == 4 and (gain > 0).all()
    assert CO.popcount(covered) == gain.sum()


def test_library_exports_the_entry_point_and_binds_it():
    from gennbv_amd import _lib
    assert _lib.SIGNATURES["gnbv_view_gain_masks"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    lib = _lib.load()
    assert hasattr(lib, "gnbv_view_gain_masks") and lib.gnbv_abi_version() == 5


def _args(**kw):
    """A GnbvViewGain the entry point accepts, on made-up non-NULL pointers: every call below is refused before any is read."""
    from gennbv_amd import _lib
    a = _lib.GnbvViewGain()
    a.n, a.k, a.g, a.h, a.w, a.stride, a.range, a.chunk, a.ablate = 2, 3, 20, 60, 80, 4, 50.0, 0, 0
    a.tri_i8 = a.poses = a.range_gt = a.voxel_size = a.inv_intri = a.gain = 0x1000
    a.tri_row_stride = 20 ** 3
    for f, v in kw.items():
        setattr(a, f, v)
    return a


def test_refusals_before_any_launch():
    from gennbv_amd import _lib
    lib = _lib.load()
    call = lambda a, words=252, ub=0x2000, hb=0x3000: lib.gnbv_view_gain_masks(C.byref(a), words, ub, hb, None)  # noqa: E731
    assert lib.gnbv_view_gain_masks(None, 252, 0x2000, 0x3000, None) == INVALID
    # everything gnbv_view_gain refuses
    for kw in (dict(stride=0), dict(range=0.0), dict(range=float("inf")), dict(k=0), dict(n=0), dict(g=1), dict(g=65, tri_row_stride=65 ** 3),
               dict(g=128, tri_row_stride=128 ** 3), dict(gain=None), dict(poses=None), dict(tri_row_stride=7999), dict(chunk=-1)):
        assert call(_args(**kw), words=gnbv_words(128)) == INVALID, kw
        assert lib.gnbv_view_gain(C.byref(_args(**kw)), None) == INVALID, kw
    assert call(_args(), ub=None, hb=None) == INVALID                       # both outputs NULL
    for words in (0, -4, 248, 250, 251, 253, 254):                          # not a multiple of 4, or < ceil(8000 / 32) = 250
        assert call(_args(), words=words) == INVALID, words
    assert call(_args(g=33, tri_row_stride=33 ** 3), words=1120) == INVALID  # ceil(35937 / 32) = 1124
    for ub, hb in ((0x2004, 0x3000), (0x2000, 0x3008), (0x2001, None), (None, 0x300c)):
        assert call(_args(), ub=ub, hb=hb) == INVALID, (ub, hb)             # not 16-byte aligned
    assert call(_args(n=65536, k=4096, g=2, tri_row_stride=8), words=8) == INVALID  # n k words = 2^31
    for ablate in (1, 2, 3):
        assert call(_args(ablate=ablate)) == INVALID, ablate


def gnbv_words(g):
    from gennbv_amd import _lib
    return int(_lib.load().gnbv_grid_bit_words(g))


def test_operator_refuses_cpu_large_grids_and_large_masks():
    from gennbv_amd import _lib
    from gennbv_amd.ops.gain_masks import ViewGainMasks
    sc = S.make_scenes(2, G, seed=1)
    with pytest.raises(_lib.GennbvHipError, match="GPU only"):
        ViewGainMasks(2, 4, CFG, sc.range_gt, sc.voxel_size, device="cpu")
    with pytest.raises(_lib.GennbvHipError, match="slab"):
        ViewGainMasks(2, 4, TaskConfig(camera_width=W, camera_height=H, grid_size=65), sc.range_gt, sc.voxel_size, device="cuda:0")
    with pytest.raises(_lib.GennbvHipError, match="above max_bytes = 1000"):
        ViewGainMasks(2, 4, CFG, sc.range_gt, sc.voxel_size, device="cuda:0", max_bytes=1000)
    for kw in (dict(words=250), dict(words=248), dict(hit=False, unknown=False)):
        with pytest.raises(_lib.GennbvHipError):
            ViewGainMasks(2, 4, CFG, sc.range_gt, sc.voxel_size, device="cuda:0", **kw)


# ---------------------------------------------------------------------------
# MapCoverPolicy on stubs
# ---------------------------------------------------------------------------
N, KP = 2, 6


class _Masks:
    """ViewGainMasks' protocol; plan() hands out the scripted (choice, gain) of each decision in turn."""

    def __init__(self, script):
        self.script, self.i, self.asked = script, 0, []

    def __call__(self, tri, poses):
        return torch.zeros(N, KP, 3, dtype=torch.int32)

    def plan(self, rounds, which="hit", contact=None, covered_bits=None, lazy=True):
        choice, gain = self.script[self.i]
        self.i += 1
        self.asked.append((rounds, which, contact.clone()))
        assert covered_bits is None
        return torch.tensor(choice, dtype=torch.int32), torch.tensor(gain, dtype=torch.int32), None


class _Flight:
    belief, shortcut = True, False

    def __init__(self):
        self.ok = torch.ones(N, KP, dtype=torch.bool)

    def reachable(self, poses):
        return self.ok.clone()

    def pairwise_mm(self, points, count):
        from gennbv_amd.ops.tour import euclid_mm
        return euclid_mm(points, count)


def _env():
    return types.SimpleNamespace(cfg=CFG, num_envs=N, device="cpu", collision=None, flight=_Flight(), poses=torch.zeros(N, 6),
                                 episode_length_buf=torch.full((N,), 5, dtype=torch.int64))


def _policy(script, seed=3, **kw):
    from gennbv_amd.eval.baselines import LatticeCandidates, MapCoverPolicy
    env = _env()
    pol = MapCoverPolicy(env, k=KP, seed=seed, masks_backend=_Masks(script), **kw)
    return env, pol, LatticeCandidates(CFG, KP, seed)  # the twin draws what the policy draws, decision by decision


OBS = torch.zeros(N, CFG.obs_dim)
ROWS = torch.arange(N)


def _pick(cand, idx):
    return cand[ROWS, torch.tensor(idx)]


@pytest.mark.parametrize("kw", [dict(horizon=0), dict(horizon=17), dict(horizon=3, commit=0), dict(horizon=3, commit=4), dict(horizon=1, commit=2),
                                dict(mask="both")])
def test_policy_refuses_bad_horizon_commit_and_mask(kw):
    with pytest.raises(ValueError):
        _policy([], **kw)


def test_policy_needs_a_belief_field():
    from gennbv_amd import _lib
    from gennbv_amd.eval.baselines import MapCoverPolicy, MapGreedyPolicy
    assert issubclass(MapCoverPolicy, MapGreedyPolicy) and MapCoverPolicy.contact is MapGreedyPolicy.contact
    env = _env()
    env.flight = None
    with pytest.raises(_lib.GennbvHipError):
        MapCoverPolicy(env, k=KP, masks_backend=_Masks([]))


def test_commit_is_honoured_and_the_plan_is_computed_at_every_decision():
    plan = ([[1, 2, 3], [4, 5, 0]], [[9, 5, 2], [7, 3, 1]])
    other = ([[0, 1, 2], [3, 2, 1]], [[8, 4, 2], [6, 5, 4]])
    env, pol, twin = _policy([plan, other, other, other, other], horizon=3, commit=2, mask="unknown")
    assert pol.policy is pol
    c = [twin.sample(N) for _ in range(5)]
    a0 = pol(OBS)[0]
    assert a0.dtype == torch.int64 and a0.shape == (N, 6)
    assert bool(pol.adopted.all()) and pol.last_views.tolist() == [3, 3] and pol.last_length_mm.tolist() == [-1, -1]
    assert torch.equal(a0, _pick(c[0], [1, 4]))
    a1 = pol(OBS)[0]  # the stored plan continues; the new one is computed all the same
    assert not bool(pol.adopted.any()) and torch.equal(a1, _pick(c[0], [2, 5]))
    assert torch.equal(pol.last_choice, torch.tensor(other[0], dtype=torch.int32)) and torch.equal(pol.last_actions[:, 0], _pick(c[1], [0, 3]))
    a2 = pol(OBS)[0]  # cursor == commit: the third view is never flown
    assert bool(pol.adopted.all()) and torch.equal(a2, _pick(c[2], [0, 3]))
    a3 = pol.predict(OBS)[0]
    assert torch.equal(a3, _pick(c[2], [1, 2]))
    assert torch.equal(pol(OBS)[0], _pick(c[4], [0, 3]))
    assert pol.gain_backend.i == 5 and all(r == 3 and w == "unknown" for r, w, _ in pol.gain_backend.asked)


def test_adoption_on_restart_is_per_env():
    plan = ([[1, 2, 3], [4, 5, 0]], [[9, 5, 2], [7, 3, 1]])
    other = ([[0, 1, 2], [3, 2, 1]], [[8, 4, 2], [6, 5, 4]])
    env, pol, twin = _policy([plan, other, other, other], horizon=3, commit=3)
    c = [twin.sample(N) for _ in range(4)]
    assert torch.equal(pol(OBS)[0], _pick(c[0], [1, 4]))
    env.episode_length_buf[0] = 1  # env 0 has just restarted: it must not fly the old plan's second view
    a1 = pol(OBS)[0]
    assert pol.adopted.tolist() == [True, False]
    assert torch.equal(a1[0], c[1][0, 0]) and torch.equal(a1[1], c[0][1, 5])
    env.episode_length_buf[0] = 2
    a2 = pol(OBS)[0]
    assert pol.adopted.tolist() == [False, False]
    assert torch.equal(a2[0], c[1][0, 1]) and torch.equal(a2[1], c[0][1, 0])
    assert pol.cursor.tolist() == [2, 3]
    env.episode_length_buf[1] = 0  # the done step itself: adopted too (the env forces the init action whatever is chosen)
    pol(OBS)
    assert pol.adopted.tolist() == [False, True]


def test_adoption_when_the_cursor_runs_out_of_views():
    short = ([[1, 2, 3], [4, 5, 0]], [[9, 0, 0], [7, 3, 0]])  # one view and two views, commit 3
    other = ([[0, 1, 2], [3, 2, 1]], [[8, 4, 2], [6, 5, 4]])
    env, pol, twin = _policy([short, other, other], horizon=3, commit=3)
    c = [twin.sample(N) for _ in range(3)]
    assert torch.equal(pol(OBS)[0], _pick(c[0], [1, 4])) and pol.plan_views.tolist() == [1, 2]
    assert torch.equal(pol.last_actions[0], c[0][0, [1, 1, 1]])  # the tail repeats the last view
    a1 = pol(OBS)[0]
    assert pol.adopted.tolist() == [True, False]
    assert torch.equal(a1[0], c[1][0, 0]) and torch.equal(a1[1], c[0][1, 5])
    pol(OBS)
    assert pol.adopted.tolist() == [False, True]


def test_refused_choices_are_dropped_and_an_empty_plan_takes_round_zero():
    script = [([[1, 2, 3], [4, 5, 0]], [[9, 5, 2], [0, 0, 0]]),   # env 0: candidate 2 is refused -> views 1, 3; env 1: nothing to gain
              ([[0, 0, 0], [2, 1, 3]], [[4, 0, 0], [5, 4, 3]])]   # env 0: every candidate refused -> candidate 0, though its gain is 4
    env, pol, twin = _policy(script, horizon=3, commit=3)
    c = [twin.sample(N) for _ in range(2)]
    env.flight.ok[0, 2] = False
    a0 = pol(OBS)[0]
    assert pol.last_views.tolist() == [2, 0]
    assert torch.equal(pol.last_actions[0], c[0][0, [1, 3, 3]])
    assert torch.equal(a0, _pick(c[0], [1, 4]))  # env 1: round 0's choice
    assert pol.gain_backend.asked[0][2].tolist() == [[0, 0, 1, 0, 0, 0], [0] * 6]
    env.flight.ok[0, :] = False
    a1 = pol(OBS)[0]
    assert pol.adopted.tolist() == [False, True]  # an empty plan is replaced at once; env 0 goes on to its second view
    assert torch.equal(a1[0], c[0][0, 3]) and torch.equal(a1[1], c[1][1, 2])
    assert pol.last_views.tolist() == [0, 3] and torch.equal(pol.last_actions[0], c[1][0, [0, 0, 0]])


def test_horizon_one_is_the_greedy_choice():
    from gennbv_amd.eval.baselines import choose
    gain3 = torch.tensor([[[3, 1, 0], [7, 0, 0], [7, 2, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0]]] * 2, dtype=torch.int32)
    for mask, w, col in (("unknown", (1, 0), 0), ("hit", (0, 1), 1)):
        best = choose(gain3, w)
        script = [([[int(best[0])], [int(best[1])]], [[int(gain3[0, best[0], col])], [int(gain3[1, best[1], col])]])] * 3
        env, pol, twin = _policy(script, horizon=1, mask=mask)
        assert pol.weights == w
        for _ in range(3):
            cand = twin.sample(N)
            assert torch.equal(pol(OBS)[0], cand[ROWS, best]) and bool(pol.adopted.all())


def test_route_orders_the_kept_views_and_leaves_the_unrouted_out():
    from gennbv_amd.ops.tour import TourResult
    seen = {}

    def tour(dist, count):
        # env 0: three kept views flown 3, 1, 2; env 1: two kept views of which the tour reaches only point 2
        seen["count"], seen["dist"] = count.clone(), dist.clone()
        return TourResult(torch.tensor([[0, 3, 1, 2], [0, 2, 1, 3]], dtype=torch.int32), torch.tensor([4, 2], dtype=torch.int32),
                          torch.tensor([1234, 77]), torch.zeros(2, dtype=torch.int32))
    script = [([[1, 2, 3], [4, 5, 0]], [[9, 5, 2], [7, 3, 0]])]
    env, pol, twin = _policy(script, horizon=3, commit=3, route=True, tour_backend=tour)
    env.poses = torch.tensor([[1.0, 2.0, 3.0, 0, 0, 0], [4.0, 5.0, 6.0, 0, 0, 0]])
    cand = twin.sample(N)
    a0 = pol(OBS)[0]
    assert seen["count"].tolist() == [4, 3] and seen["count"].dtype == torch.int32 and seen["dist"].shape == (N, 4, 4)
    pos = twin.poses(cand)[..., :3]
    d = seen["dist"][0].long() & 0xFFFFFFFF
    assert int(d[0, 1]) == round(1000 * float((env.poses[0, :3].double() - pos[0, 1].double()).norm()))  # point 0 the start, 1 the first kept view
    assert pol.last_views.tolist() == [3, 1] and pol.last_length_mm.tolist() == [1234, 77]
    assert torch.equal(pol.last_actions[0], cand[0, [3, 1, 2]]) and torch.equal(pol.last_actions[1], cand[1, [5, 5, 5]])
    assert torch.equal(a0, _pick(cand, [3, 5]))
