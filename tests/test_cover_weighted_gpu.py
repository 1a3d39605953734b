"""GPU: gnbv_cover_greedy_w (csrc/covergreedy.hip) on random planes against the numpy reference
(tests/cover_weighted_oracle.py), one plane of weight 1 against gnbv_cover_greedy byte for byte, ViewGainMasks.plan_weighted
against `choose`, `plan` and the reference on the view-gain oracle's masks, and MapCoverPolicy(mask="mixed") on a real closed-loop
env.  Every comparison is `==` on integers; every output is pre-filled with 0xFF bytes and followed by a tail that must keep them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gennbv_amd.env import synthetic as S
from gennbv_amd.env.config import TaskConfig
from tests import cover_greedy_oracle as CG
from tests import cover_weighted_oracle as CW
from tests import gain_masks_oracle as MO
from tests.test_view_gain_gpu import _lattice_poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 8  # int32 elements after every output that the entry point must leave alone


def _filled(*shape, dtype=torch.int32):
    """A tensor of `shape` viewed from a flat 0xFF-filled buffer with TAIL more elements behind it -> (view, whole buffer)"""
    count = int(np.prod(shape))
    buf = torch.empty(count + TAIL, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    return buf[:count].view(*shape), buf


def _dev_u32(a):
    """uint32 numpy -> int32 device tensor behind a 16-byte aligned pointer (torch allocations are)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def _planes_case(seed, n, k, words, planes, density, contact_kind):
    """masks P x uint32 [n, k, words] (independent planes; a duplicated and an all-zero row per env and plane, and one candidate
    equal to another in every plane, where k allows), covered P x [n, words], contact u8 [n, k]"""
    rng = np.random.default_rng(seed)
    masks = [np.stack([CG.random_masks(rng, k, words, density) for _ in range(n)]) for _ in range(planes)]
    if k > 3:
        for e in range(n):
            for m in masks:
                m[e, rng.integers(k)] = m[e, rng.integers(k)]
                m[e, rng.integers(k)] = 0
            a, b = rng.integers(k), rng.integers(k)
            for m in masks:
                m[e, a] = m[e, b]
    cov = [np.stack([CG.random_masks(rng, 1, words, 0.3)[0] for _ in range(n)]) for _ in range(planes)]
    contact = {"none": np.zeros((n, k), np.uint8), "random": (rng.random((n, k)) < 0.3).astype(np.uint8), "all": np.ones((n, k), np.uint8)}[contact_kind]
    return masks, cov, contact


class _Call:
    """One gnbv_cover_greedy_w call on device copies.  cov_kind: "null" | "given" | "alias" (covered_out is covered_in)."""

    def __init__(self, masks, cov, weights, contact, rounds, lazy, cov_kind="given", gains0=True, plane_gain=True, ub=None, covered_out=True):
        from gennbv_amd import _lib
        self.lib = _lib.load()
        planes = len(masks)
        n, k, words = masks[0].shape
        self.masks = [_dev_u32(m) for m in masks]
        self.contact = None if contact is None else torch.from_numpy(contact).to(DEV)
        self.choice, self.choice_buf = _filled(n, rounds)
        self.gain, self.gain_buf = _filled(n, rounds)
        self.cov_in, self.cov_out, self.cov_bufs = [], [], []
        for p in range(planes):
            if cov_kind == "alias":
                view, buf = _filled(n, words)
                view.copy_(_dev_u32(cov[p]))
                self.cov_in.append(view), self.cov_out.append(view), self.cov_bufs.append(buf)
            else:
                self.cov_in.append(None if cov_kind == "null" else _dev_u32(cov[p]))
                view, buf = _filled(n, words) if covered_out else (None, None)
                self.cov_out.append(view), self.cov_bufs.append(buf)
        self.gains0, self.gains0_buf = _filled(n, k) if gains0 else (None, None)
        self.plane_gain, self.plane_gain_buf = _filled(n, rounds, planes) if plane_gain else (None, None)
        self.ub = ub
        a = _lib.GnbvCoverGreedyW()
        a.n, a.k, a.words, a.rounds, a.lazy, a.planes = n, k, words, rounds, lazy, planes
        for p in range(planes):
            a.weight[p], a.mask_bits[p] = int(weights[p]), self.masks[p].data_ptr()
            a.covered_in[p], a.covered_out[p] = _lib.ptr(self.cov_in[p]), _lib.ptr(self.cov_out[p])
        a.contact, a.choice, a.gain = _lib.ptr(self.contact), self.choice.data_ptr(), self.gain.data_ptr()
        a.plane_gain, a.gains0, a.ub = _lib.ptr(self.plane_gain), _lib.ptr(self.gains0), _lib.ptr(self.ub)
        self.args = a

    def run(self):
        from gennbv_amd import _lib
        return self.lib.gnbv_cover_greedy_w(C.byref(self.args), _lib.stream_ptr(torch.device(DEV)))

    def tails_untouched(self):
        bufs = [self.choice_buf, self.gain_buf, self.gains0_buf, self.plane_gain_buf] + self.cov_bufs
        return all(bool((b[-TAIL:] == -1).all()) for b in bufs if b is not None)

    def outputs(self):
        host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return (host(self.choice), host(self.gain), host(self.plane_gain),
                [None if c is None else c.cpu().numpy().view(np.uint32) for c in self.cov_out], host(self.gains0))


def _covered_after(masks, cov, choice):
    """P x [n, words]: cov | the chosen rows"""
    out = [c.copy() for c in cov]
    for p, m in enumerate(masks):
        for e in range(m.shape[0]):
            for j in choice[e]:
                out[p][e] |= m[e, j]
    return out


def _scores(masks, cov, weights):
    """int64 [n, k]: the weighted score of every candidate against cov"""
    return sum(int(w) * CG.popcount(m & ~c[:, None, :]) for m, c, w in zip(masks, cov, weights))


# words: 4 = one 16-byte group, 252 = 63 groups (a partial wave), 260 = 65 (a second trip with one lane), 1124; k: 1, 3, 16, 17 (a
# wave owns two candidates), 40, 1030 (the second trip of the per-lane key scan); n: 1, 9 (the XCD mapping pads 9 envs to 16
# slots); planes 1..3 with zero weights; contact none / random / all.  Pairwise over the dimensions, not their product.
KERNEL_CASES = [  # words, k, n, weights, density, contact
    (4, 1, 1, [3], 0.3, "none"),
    (4, 1030, 9, [1, 4], 0.3, "random"),
    (4, 3, 1, [0, 0], 0.3, "random"),
    (4, 17, 9, [5, 0, 2], 0.3, "all"),
    (252, 3, 9, [2, 0, 5], 0.02, "none"),
    (252, 17, 1, [1, 16], 0.3, "all"),
    (252, 40, 9, [4, 1], 0.3, "random"),
    (260, 16, 9, [0, 1], 0.02, "random"),
    (260, 40, 1, [1, 4, 0], 0.3, "none"),
    (260, 1, 9, [1, 1, 1], 0.3, "all"),
    (1124, 17, 9, [1, 4], 0.02, "none"),
    (1124, 40, 1, [7], 0.3, "random"),
    (1124, 3, 1, [1, 2, 3], 0.3, "random"),
    (1124, 16, 1, [16, 1], 0.3, "all"),
]


@pytest.mark.parametrize("words,k,n,weights,density,contact_kind", KERNEL_CASES)
def test_equals_the_reference(words, k, n, weights, density, contact_kind):
    planes = len(weights)
    masks, cov, contact = _planes_case(7 * words + 13 * k + n, n, k, words, planes, density, contact_kind)
    zero = [np.zeros_like(c) for c in cov]
    t_max = min(k + 3, 20)
    full = {kind: CW.batch_exhaustive(masks, zero if kind == "null" else cov, weights, contact, max(5, t_max)) for kind in ("null", "given")}
    full["alias"] = full["given"]
    idx = 0
    for rounds in (1, 5, t_max):
        for lazy in (0, 1):
            # the three ways round 0 is reached: the wide pass into gains0; inside the workgroup; from a row of unknown bounds
            for mode in ("gains0", "plain", "ub"):
                cov_kind = ("null", "given", "alias")[idx % 3]
                idx += 1
                start = zero if cov_kind == "null" else cov
                ref = full[cov_kind]
                want_choice, want_gain, want_pg = ref[0][:, :rounds], ref[1][:, :rounds], ref[2][:, :rounds]
                want_cov = _covered_after(masks, start, want_choice)
                ub = torch.full((n, k), CG.UNKNOWN, dtype=torch.int32, device=DEV) if mode == "ub" else None
                bare = mode == "plain" and rounds == 1 and cov_kind != "alias"  # rounds == 1 goes without covered_out
                call = _Call(masks, cov, weights, None if contact_kind == "none" and lazy else contact, rounds, lazy, cov_kind=cov_kind,
                             gains0=mode == "gains0", plane_gain=mode != "plain" or lazy == 1, ub=ub, covered_out=not bare)
                assert call.run() == 0
                choice, gain, pg, cov_out, gains0 = call.outputs()
                tag = (rounds, lazy, mode, cov_kind)
                assert np.array_equal(choice, want_choice), tag
                assert np.array_equal(gain, want_gain), tag
                assert call.tails_untouched(), tag
                if pg is not None:
                    assert np.array_equal(pg, want_pg), tag
                for p in range(planes):
                    if cov_out[p] is not None:
                        assert np.array_equal(cov_out[p], want_cov[p]), tag + (p,)
                if gains0 is not None:
                    assert np.array_equal(gains0, ref[4]), tag
                if ub is not None:  # bounds at exit: upper bounds of the scores against covered_out, none left as garbage
                    got = ub.cpu().numpy()
                    assert (got >= _scores(masks, want_cov, weights)).all() and (got != CG.UNKNOWN).any(), tag
                    if lazy == 0:  # exhaustive: the exact scores of the last round
                        assert np.array_equal(got, _scores(masks, _covered_after(masks, start, want_choice[:, :rounds - 1]), weights)), tag
    assert idx == 18
    if min(weights) > 0 and contact_kind != "all" and k >= 16:
        assert (full["given"][1] > 0).any()


def test_the_weights_change_the_plan_on_these_inputs():
    """A condition on the inputs of the test above: with both planes weighted the plan is neither plane's own."""
    words, k, n, weights, density, contact_kind = KERNEL_CASES[6]
    masks, cov, contact = _planes_case(7 * words + 13 * k + n, n, k, words, 2, density, contact_kind)
    both, only0, only1 = (CW.batch_exhaustive(masks, cov, w, contact, 5)[0] for w in (weights, [1, 0], [0, 1]))
    assert not np.array_equal(both, only0) and not np.array_equal(both, only1)


@pytest.mark.parametrize("contact_kind", ["none", "random"])
def test_split_calls_carrying_bounds_equal_one_call(contact_kind):
    n, k, words, weights = 3, 70, 252, [1, 4]
    masks, cov, contact = _planes_case(7, n, k, words, 2, 0.02, contact_kind)
    ref = CW.batch_exhaustive(masks, cov, weights, contact, 5)
    one = _Call(masks, cov, weights, contact, 5, 1)
    assert one.run() == 0
    want = one.outputs()
    assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1]) and np.array_equal(want[2], ref[2])
    assert all(np.array_equal(want[3][p], ref[3][p]) for p in range(2)) and np.array_equal(want[4], ref[4])
    ub = torch.full((n, k), CG.UNKNOWN, dtype=torch.int32, device=DEV)
    a = _Call(masks, cov, weights, contact, 3, 1, gains0=False, ub=ub)
    assert a.run() == 0
    ca, ga, pa, cova, _ = a.outputs()
    assert bool((ub != CG.UNKNOWN).any())  # the bounds were written
    b = _Call(masks, cova, weights, contact, 2, 1, cov_kind="alias", gains0=False, ub=ub)  # covered_out aliases covered_in
    assert b.run() == 0
    cb, gb, pb, covb, _ = b.outputs()
    assert np.array_equal(np.concatenate([ca, cb], 1), want[0]) and np.array_equal(np.concatenate([ga, gb], 1), want[1])
    assert np.array_equal(np.concatenate([pa, pb], 1), want[2]) and all(np.array_equal(covb[p], want[3][p]) for p in range(2))
    assert a.tails_untouched() and b.tails_untouched()
    # two runs of one call are bit-identical and overwrite every output element
    for t in (one.choice, one.gain, one.plane_gain, one.gains0, *one.cov_out):
        t.fill_(-777)
    assert one.run() == 0
    again = one.outputs()
    assert all(np.array_equal(x, y) for x, y in zip(again[:3] + (again[4],) + tuple(again[3]), want[:3] + (want[4],) + tuple(want[3])))


@pytest.mark.parametrize("words,k,n,contact_kind", [(4, 1030, 2, "random"), (252, 17, 9, "none"), (260, 70, 3, "random"), (1124, 40, 1, "all")])
def test_one_plane_of_weight_one_is_byte_equal_to_cover_greedy(words, k, n, contact_kind):
    from gennbv_amd import _lib
    masks, cov, contact = _planes_case(3 * words + k, n, k, words, 1, 0.3 if k < 1000 else 0.5, contact_kind)
    lib = _lib.load()
    for rounds in (1, 6):
        for lazy in (0, 1):
            for mode in ("gains0", "ub", "gains0+ub"):
                for cov_kind in ("null", "given"):
                    ub_w = torch.full((n, k), CG.UNKNOWN, dtype=torch.int32, device=DEV) if "ub" in mode else None
                    ub_o = None if ub_w is None else ub_w.clone()
                    w = _Call(masks, cov, [1], contact, rounds, lazy, cov_kind=cov_kind, gains0="gains0" in mode, ub=ub_w)
                    assert w.run() == 0
                    o = _lib.GnbvCoverGreedy()
                    o.n, o.k, o.words, o.rounds, o.lazy = n, k, words, rounds, lazy
                    choice, gain, covered, gains0 = _filled(n, rounds)[0], _filled(n, rounds)[0], _filled(n, words)[0], _filled(n, k)[0]
                    o.mask_bits, o.covered_in, o.contact = w.masks[0].data_ptr(), _lib.ptr(w.cov_in[0]), _lib.ptr(w.contact)
                    o.choice, o.gain, o.covered_out = choice.data_ptr(), gain.data_ptr(), covered.data_ptr()
                    o.gains0, o.ub = (gains0.data_ptr() if "gains0" in mode else None), _lib.ptr(ub_o)
                    assert lib.gnbv_cover_greedy(C.byref(o), _lib.stream_ptr(torch.device(DEV))) == 0
                    tag = (rounds, lazy, mode, cov_kind)
                    assert torch.equal(w.choice, choice) and torch.equal(w.gain, gain) and torch.equal(w.cov_out[0], covered), tag
                    assert torch.equal(w.plane_gain[..., 0], gain), tag
                    if "gains0" in mode:
                        assert torch.equal(w.gains0, gains0), tag
                    if ub_w is not None:
                        assert torch.equal(ub_w, ub_o) and bool((ub_w != CG.UNKNOWN).any()), tag


def test_refusals_launch_nothing():
    masks, cov, contact = _planes_case(3, 2, 7, 252, 2, 0.3, "random")
    bad = [dict(planes=0), dict(planes=5), dict(planes=3), dict(words=254), dict(rounds=0), dict(lazy=2), dict(choice=None), dict(gain=None),
           dict(weight=(0, -1)), dict(weight=(1, 2 ** 31 - 1)), dict(weight=(2 ** 31 - 1) // (32 * 252), bump=1),
           dict(mask_bits=(1, None)), dict(covered_out=(0, None)), dict(covered_out=(1, "share")), dict(mask_bits=(0, "+4")),
           dict(covered_in=(1, "+4")), dict(covered_out=(0, "+8"))]
    for kw in bad:
        call = _Call(masks, cov, [1, 4], contact, 2, 1, ub=torch.full((2, 7), -1, dtype=torch.int32, device=DEV))
        a = call.args
        for f, v in kw.items():
            if f == "bump":
                a.weight[1] = a.weight[1] + v
            elif f == "weight" and isinstance(v, int):
                a.weight[0], a.weight[1] = v, 0  # the largest sum that fits; `bump` takes it one past
            elif isinstance(v, tuple):
                p, x = v
                arr = getattr(a, f)
                arr[p] = (a.covered_out[0] if x == "share" else arr[p] + int(x) if isinstance(x, str) else x)
            else:
                setattr(a, f, v)
        assert call.run() == 1, kw  # hipErrorInvalidValue
        torch.cuda.synchronize()
        for t in (call.choice_buf, call.gain_buf, call.gains0_buf, call.plane_gain_buf, call.ub, *call.cov_bufs):
            assert bool((t == -1).all()), kw
    ok = _Call(masks, cov, [(2 ** 31 - 1) // (32 * 252), 0], contact, 2, 1)  # the largest weight sum that fits is accepted
    assert ok.run() == 0
    ref = CW.batch_exhaustive(masks, cov, [(2 ** 31 - 1) // (32 * 252), 0], contact, 2)
    assert np.array_equal(ok.outputs()[0], ref[0]) and np.array_equal(ok.outputs()[1], ref[1])


# ---------------------------------------------------------------------------
# ViewGainMasks.plan_weighted
# ---------------------------------------------------------------------------
def _cfg(h, w, g):
    return TaskConfig(camera_width=w, camera_height=h, grid_size=g)


@functools.lru_cache(maxsize=None)
def _plan_case():
    """tests/test_gain_masks_gpu.py's plan case at occupied density 0.1 and 8 candidates: 5 envs at 20^3, the operator after one
    call, the oracle's masks of the same cameras (computed once), and a contact table whose env 0 is all refused."""
    from gennbv_amd.ops.gain_masks import ViewGainMasks
    g, n, k = 20, 5, 8
    cfg = _cfg(60, 80, g)
    scene = S.make_scenes(n, g, seed=2)
    tri = MO.random_tri(n, g, 0.1, seed=21)
    poses = _lattice_poses(cfg, n, k, seed=20, extremes=False).to(DEV)
    op = ViewGainMasks(n, k, cfg, scene.range_gt, scene.voxel_size, stride=4, range_m=50.0, device=DEV, with_c2w=True)
    gain = op(tri.to(DEV), poses).clone()
    kinv = S.inverse_intrinsics(60, 80, cfg.horizontal_fov).numpy()
    want = MO.masks(tri.numpy(), op.c2w.cpu().numpy(), scene.range_gt.numpy(), scene.voxel_size.numpy(), kinv, 60, 80, 4, 50.0, words=op.words)
    gen = torch.Generator().manual_seed(11)
    contact = (torch.rand(n, k, generator=gen) < 0.4).to(torch.uint8)
    contact[0] = 1
    return op, gain, want, contact


@pytest.mark.parametrize("with_contact", [False, True])
def test_plan_weighted_is_choose_at_one_round_and_the_reference_at_four(with_contact):
    from gennbv_amd.eval.baselines import choose
    op, gain, want, contact = _plan_case()
    n, k = gain.shape[:2]
    assert np.array_equal(op.unknown_bits.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(op.hit_bits.cpu().numpy().view(np.uint32), want[1])
    con = contact if with_contact else torch.zeros_like(contact)
    con_d = con.to(DEV) if with_contact else None
    zero = [np.zeros((n, op.words), np.uint32)] * 2
    firsts = {}
    for w in ((1, 4), (4, 1), (1, 0), (0, 1)):
        for lazy in (True, False):
            choice, g, covered = op.plan_weighted(1, weights=w, contact=con_d, lazy=lazy)
            best = choose(gain, w, con_d)
            assert torch.equal(choice[:, 0].long(), best), (w, lazy)
            score = w[0] * gain[..., 0] + w[1] * gain[..., 1]
            assert torch.equal(op.gains0, score) and torch.equal(g[:, 0], score.gather(1, best[:, None])[:, 0])
            assert torch.equal(op.plane_gain[:, 0], gain[..., :2].gather(1, best[:, None, None].expand(-1, 1, 2))[:, 0])
        firsts[w] = choice[:, 0].tolist()
    plans = {}
    for w in ((1, 4), (1, 16), (1, 0), (0, 1)):
        ref = CW.batch_exhaustive(list(want), zero, list(w), con.numpy(), 4)
        for lazy in (True, False):
            choice, g, covered = op.plan_weighted(4, weights=w, contact=con_d, lazy=lazy)
            assert np.array_equal(choice.cpu().numpy(), ref[0]) and np.array_equal(g.cpu().numpy(), ref[1]), (w, lazy)
            assert np.array_equal(op.plane_gain.cpu().numpy(), ref[2]) and np.array_equal(op.gains0.cpu().numpy(), ref[4])
            assert all(np.array_equal(covered[p].cpu().numpy().view(np.uint32), ref[3][p]) for p in range(2))
            assert op.plan_weighted(4, weights=w, contact=con_d)[0] is choice  # cached per `rounds`
        plans[w] = (choice.clone(), g.clone())
    kept = op.plan(4, which="hit", contact=con_d)
    hit = (kept[0].clone(), kept[1].clone())
    unknown = op.plan(4, which="unknown", contact=con_d)
    assert unknown[0] is kept[0] and op.plan_weighted(4, weights=(1, 4), contact=con_d)[0] is not kept[0]  # caches of their own
    assert torch.equal(plans[(0, 1)][0], hit[0]) and torch.equal(plans[(0, 1)][1], hit[1])
    assert torch.equal(plans[(1, 0)][0], unknown[0]) and torch.equal(plans[(1, 0)][1], unknown[1])
    if not with_contact:  # a condition on the inputs: the weights change this plan, not only its first view
        assert not torch.equal(plans[(1, 4)][0], plans[(1, 16)][0]) and firsts[(1, 4)] != firsts[(1, 0)]
        assert not torch.equal(plans[(1, 4)][0], plans[(1, 0)][0]) and not torch.equal(plans[(1, 4)][0], plans[(0, 1)][0])
    # covered_bits: the second half of a plan from the first half's covered sets
    a = op.plan_weighted(2, weights=(1, 4), contact=con_d)
    first, cov2 = (a[0].clone(), a[1].clone()), tuple(c.clone() for c in a[2])
    b = op.plan_weighted(2, weights=(1, 4), contact=con_d, covered_bits=cov2)
    assert torch.equal(torch.cat([first[0], b[0]], 1), plans[(1, 4)][0]) and torch.equal(torch.cat([first[1], b[1]], 1), plans[(1, 4)][1])


def test_plan_weighted_refusals_and_no_synchronisation():
    from gennbv_amd import _lib
    from gennbv_amd.ops.gain_masks import ViewGainMasks
    op, gain, _, contact = _plan_case()
    n, k = gain.shape[:2]
    for kw in (dict(rounds=0), dict(rounds=2, weights=(1, -1)), dict(rounds=2, weights=(2 ** 31 - 1, 1)), dict(rounds=2, weights=(1, 2, 3)),
               dict(rounds=2, contact=torch.zeros(n, k, dtype=torch.uint8)), dict(rounds=2, contact=torch.zeros(n, k + 1, dtype=torch.uint8, device=DEV)),
               dict(rounds=2, covered_bits=torch.zeros(n, op.words, dtype=torch.int32, device=DEV)),
               dict(rounds=2, covered_bits=(torch.zeros(n, op.words, dtype=torch.int64, device=DEV),) * 2)):
        with pytest.raises(_lib.GennbvHipError):
            op.plan_weighted(**kw)
    scene = S.make_scenes(n, 20, seed=2)
    only_hit = ViewGainMasks(n, k, _cfg(60, 80, 20), scene.range_gt, scene.voxel_size, device=DEV, unknown=False)
    with pytest.raises(_lib.GennbvHipError, match="unknown mask is not kept"):
        only_hit.plan_weighted(2)
    con = contact.to(DEV)
    want = tuple(t.clone() for t in op.plan_weighted(3, weights=(1, 4), contact=con)[:2])  # (warm-up: the first use allocates the outputs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        plan = op.plan_weighted(3, weights=(1, 4), contact=con)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(plan[0], want[0]) and torch.equal(plan[1], want[1]) and op.plane_gain.shape == (n, 3, 2)


# ---------------------------------------------------------------------------
# MapCoverPolicy(mask="mixed") on a real closed-loop env (tests/test_gain_masks_gpu.py's env: 8 envs, 20^3, 20-step episodes)
# ---------------------------------------------------------------------------
def test_mixed_horizon_one_flies_what_map_greedy_flies():
    from gennbv_amd.eval.baselines import MapCoverPolicy, MapGreedyPolicy
    from tests.test_gain_masks_gpu import EP_LEN, _env
    env_a, cfg = _env()
    env_b, _ = _env()
    pa = MapCoverPolicy(env_a, k=8, horizon=1, mask="mixed", weights=(1, 4), seed=7, stride=4)
    pb = MapGreedyPolicy(env_b, k=8, weights=(1, 4), seed=7, stride=4)
    oa, ob = env_a.reset(), env_b.reset()
    for step in range(EP_LEN + 2):  # a whole episode and its restart
        a, b = pa(oa)[0], pb(ob)[0]
        assert torch.equal(a, b), step
        assert torch.equal(pa.last_gain3, pb.last_gain) and bool(pa.adopted.all())
        assert torch.equal(pa.last_gain[:, 0], pa.last_plane_gain[:, 0, 0] + 4 * pa.last_plane_gain[:, 0, 1])
        oa, ob = env_a.step(a)[0], env_b.step(b)[0]
        assert torch.equal(oa, ob)


def test_committed_mixed_plans_are_flown_in_order_and_dropped_on_reset():
    """horizon = commit = 3: tests/test_gain_masks_gpu.py's host mirror of the stored plans, fed only with what the policy exposes."""
    from gennbv_amd.eval.baselines import MapCoverPolicy
    from tests.test_gain_masks_gpu import ENV_N, EP_LEN, _env
    env, cfg = _env()
    pol = MapCoverPolicy(env, k=8, horizon=3, commit=3, mask="mixed", weights=(1, 4), seed=5)
    obs = env.reset()
    plan, views, cursor = [None] * ENV_N, [0] * ENV_N, [0] * ENV_N
    multi = resets_mid_plan = 0
    for step in range(2 * EP_LEN + 5):
        ep_len = env.episode_length_buf.cpu().tolist()
        act = pol(obs)[0]
        adopted, new_plan, new_views = pol.adopted.cpu().tolist(), pol.last_actions.cpu(), pol.last_views.cpu().tolist()
        choice, gain, pg = pol.last_choice.cpu(), pol.last_gain.cpu(), pol.last_plane_gain.cpu()
        assert choice.shape == gain.shape == (ENV_N, 3) and pg.shape == (ENV_N, 3, 2)
        assert torch.equal(gain, pg[..., 0] + 4 * pg[..., 1]) and bool((pg >= 0).all())
        for e in range(ENV_N):
            restart = ep_len[e] <= 1
            mid = 0 < cursor[e] < min(3, views[e])
            assert adopted[e] == (restart or cursor[e] >= min(3, views[e])), (step, e)
            if restart and mid:
                resets_mid_plan += 1  # the rest of the old plan is dropped: the action below comes from a plan made after the reset
            if adopted[e]:
                plan[e], views[e], cursor[e] = new_plan[e], new_views[e], 0
                assert 0 <= views[e] <= int((gain[e] > 0).sum())
                multi += views[e] > 1
            assert torch.equal(act[e].cpu(), plan[e][cursor[e]]), (step, e, cursor[e])
            cursor[e] += 1
        assert pol.cursor.cpu().tolist() == cursor and pol.plan_views.cpu().tolist() == views
        obs = env.step(act)[0]
    print("plans with more than one view", multi, "resets in mid-plan", resets_mid_plan)
    assert multi > 0 and resets_mid_plan > 0
