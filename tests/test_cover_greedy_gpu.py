"""GPU: gnbv_cover_greedy (csrc/covergreedy.hip) alone, on random masks, against the numpy reference
(tests/cover_greedy_oracle.py).  Every comparison is `==` on integers."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import cover_greedy_oracle as CG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 3
GARBAGE = -12345


def _words(g):
    from gennbv_amd import _lib
    return int(_lib.load().gnbv_grid_bit_words(g))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype) if a.dtype != dtype else np.ascontiguousarray(a)).to(DEV)


def _case(seed, k, words, density, cov_kind, contact_kind, n=N):
    """masks uint32 [n, k, words] with a duplicated and an all-zero row per env where k allows, covered [n, words] or None,
    contact u8 [n, k] or None"""
    rng = np.random.default_rng(seed)
    m = np.stack([CG.random_masks(rng, k, words, density) for _ in range(n)])
    if k > 3:
        for e in range(n):
            m[e, rng.integers(k)] = m[e, rng.integers(k)]
            m[e, rng.integers(k)] = 0
    cov = None if cov_kind == "null" else np.stack([CG.random_masks(rng, 1, words, 0.3)[0] for _ in range(n)])
    contact = {"none": None, "random": (rng.random((n, k)) < 0.3).astype(np.uint8), "all": np.ones((n, k), np.uint8)}[contact_kind]
    return m, cov, contact


def _reference(m, cov, contact, rounds):
    n, k, words = m.shape
    return CG.batch_exhaustive(m, np.zeros((n, words), np.uint32) if cov is None else cov,
                               np.zeros((n, k), np.uint8) if contact is None else contact, rounds)


def _covered_after(m, cov, choice):
    out = np.zeros((m.shape[0], m.shape[2]), np.uint32) if cov is None else cov.copy()
    for e in range(m.shape[0]):
        for j in choice[e]:
            out[e] |= m[e, j]
    return out


class _Call:
    """One gnbv_cover_greedy call on device copies; outputs prefilled with garbage."""

    def __init__(self, m, cov, contact, rounds, lazy, gains0=True, ub=None, covered_out=True, alias=False):
        from gennbv_amd import _lib
        self.lib = _lib.load()
        n, k, words = m.shape
        self.mask = _dev(m, np.int32)
        self.cov = None if cov is None else _dev(cov, np.int32)
        self.contact = None if contact is None else _dev(contact, np.uint8)
        self.choice = torch.full((n, rounds), GARBAGE, dtype=torch.int32, device=DEV)
        self.gain = torch.full((n, rounds), GARBAGE, dtype=torch.int32, device=DEV)
        self.cov_out = self.cov if alias else (torch.full((n, words), GARBAGE, dtype=torch.int32, device=DEV) if covered_out else None)
        self.gains0 = torch.full((n, k), GARBAGE, dtype=torch.int32, device=DEV) if gains0 else None
        self.ub = ub
        a = _lib.GnbvCoverGreedy()
        a.n, a.k, a.words, a.rounds, a.lazy = n, k, words, rounds, lazy
        a.mask_bits, a.covered_in, a.contact = self.mask.data_ptr(), _lib.ptr(self.cov), _lib.ptr(self.contact)
        a.choice, a.gain, a.covered_out = self.choice.data_ptr(), self.gain.data_ptr(), _lib.ptr(self.cov_out)
        a.gains0, a.ub = _lib.ptr(self.gains0), _lib.ptr(self.ub)
        self.args = a

    def run(self):
        from gennbv_amd import _lib
        return self.lib.gnbv_cover_greedy(C.byref(self.args), _lib.stream_ptr(torch.device(DEV)))

    def outputs(self):
        u32 = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)
        return (self.choice.cpu().numpy(), self.gain.cpu().numpy(), u32(self.cov_out),
                None if self.gains0 is None else self.gains0.cpu().numpy())


def _compare_with_the_reference(seed, n, k, words, densities, rounds_list):
    """Every (density, covered_in, contact) kind x rounds x lazy x the three ways round 0 is reached, outputs prefilled with
    garbage, `==` against the reference -> the reference of the last kind at the most rounds, and per kind (density, round-0 top
    shared by two candidates in some env, a last round at gain 0 in some env)."""
    kinds = list(itertools.product(densities, ("null", "random"), ("none", "random", "all")))
    checked, seen = 0, []
    for idx, (density, cov_kind, contact_kind) in enumerate(kinds):
        m, cov, contact = _case(seed + idx, k, words, density, cov_kind, contact_kind, n)
        full = _reference(m, cov, contact, max(rounds_list))
        seen.append((density, bool(((full[3] == full[3].max(1, keepdims=True)).sum(1) > 1).any()), bool((full[1][:, -1] == 0).any())))
        for rounds in rounds_list:
            want_choice, want_gain = full[0][:, :rounds], full[1][:, :rounds]
            want_cov = _covered_after(m, cov, want_choice)
            for lazy in (0, 1):
                # the three ways round 0 is reached: wide pass into gains0; inside the workgroup; from a row of unknown bounds
                for mode in ("gains0", "plain", "ub"):
                    ub = torch.full((n, k), CG.UNKNOWN, dtype=torch.int32, device=DEV) if mode == "ub" else None
                    call = _Call(m, cov, contact, rounds, lazy, gains0=mode == "gains0", ub=ub, covered_out=not (rounds == 1 and mode == "plain"))
                    assert call.run() == 0
                    choice, gain, cov_out, gains0 = call.outputs()
                    tag = (n, k, words, density, cov_kind, contact_kind, rounds, lazy, mode)
                    assert np.array_equal(choice, want_choice), tag
                    assert np.array_equal(gain, want_gain), tag
                    if cov_out is not None:
                        assert np.array_equal(cov_out, want_cov), tag
                    if gains0 is not None:
                        assert np.array_equal(gains0, full[3]), tag
                    if ub is not None:  # bounds at exit: upper bounds of the gains against covered_out, none left as garbage
                        left = CG.popcount(m & ~want_cov[:, None, :])
                        assert (ub.cpu().numpy() >= left).all(), tag
                        if lazy == 0:
                            assert np.array_equal(ub.cpu().numpy(), CG.popcount(m & ~_covered_after(m, cov, want_choice[:, :rounds - 1])[:, None, :])), tag
                    checked += 1
    assert checked == len(kinds) * len(rounds_list) * 2 * 3
    return full, seen


@pytest.mark.parametrize("g", [20, 33])
@pytest.mark.parametrize("k", [1, 7, 70])
def test_equals_the_reference(k, g):
    full, _ = _compare_with_the_reference(1000 * k + 10 * g, N, k, _words(g), (0.02, 0.5), (1, 5, k + 3))  # k = 1: 5 rounds are more than k + 3
    if k == 70:
        assert (full[1] > 0).any() and (full[1][:, -1] == 0).all()  # k + 3 rounds: the last ones repeat a view at gain 0


# The regimes the sizes above stop short of:
#   n = 9        a second group of 8 envs in the gains kernel's block -> (env, candidates) mapping, e = (slot / per_env) * 8 + xcd;
#   k = 1030     more than 16 waves x 64 lanes of candidates: the key scan j = wave + waves * lane takes a second trip, and the
#                lazy passes have stale tops in every wave;
#   words = 4    one 16-byte group per row: 63 lanes of a wave read nothing.
# The sparse density leaves about four set bits among all of an env's rows: round 0's top is shared and five rounds run out of gain.
@pytest.mark.parametrize("n,k,words", [(9, 7, 252), (N, 1030, 4), (N, 1030, 252), (N, 70, 4)])
def test_equals_the_reference_in_a_second_env_group_a_second_key_trip_and_one_group_rows(n, k, words):
    sparse = 4.0 / (k * words * 32)
    _, seen = _compare_with_the_reference(100000 * n + 10 * k + words, n, k, words, (sparse, 0.5), (1, 5))
    assert any(tie for _, tie, _ in seen) and any(zero for d, _, zero in seen if d == sparse)


@pytest.mark.parametrize("contact_kind", ["none", "random"])
def test_split_calls_carrying_bounds_equal_one_call_and_aliasing_works(contact_kind):
    k, words = 70, _words(20)
    m, cov, contact = _case(7, k, words, 0.02, "random", contact_kind)
    one = _Call(m, cov, contact, 5, 1)
    assert one.run() == 0
    want = one.outputs()
    ref = _reference(m, cov, contact, 5)
    assert np.array_equal(want[0], ref[0]) and np.array_equal(want[1], ref[1]) and np.array_equal(want[2], ref[2])
    ub = torch.full((N, k), CG.UNKNOWN, dtype=torch.int32, device=DEV)
    a = _Call(m, cov, contact, 3, 1, gains0=False, ub=ub)
    assert a.run() == 0
    ca, ga, cova, _ = a.outputs()
    assert bool((ub != CG.UNKNOWN).any())  # the bounds were written
    b = _Call(m, cova, contact, 2, 1, gains0=False, ub=ub, alias=True)  # covered_out aliases covered_in
    assert b.run() == 0
    cb, gb, covb, _ = b.outputs()
    assert np.array_equal(np.concatenate([ca, cb], 1), want[0]) and np.array_equal(np.concatenate([ga, gb], 1), want[1])
    assert np.array_equal(covb, want[2])
    # one call whose covered_out aliases covered_in, lazy and exhaustive, with the wide round 0 reading the row first
    for lazy in (0, 1):
        c = _Call(m, cov, contact, 5, lazy, alias=True)
        assert c.run() == 0
        got = c.outputs()
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), lazy


def test_two_runs_are_bit_identical_and_outputs_are_fully_overwritten():
    k, words = 70, _words(33)
    m, cov, contact = _case(11, k, words, 0.5, "random", "random")
    for lazy in (0, 1):
        a = _Call(m, cov, contact, 9, lazy)
        assert a.run() == 0
        first = a.outputs()
        for t in (a.choice, a.gain, a.cov_out, a.gains0):
            t.fill_(-777)
        assert a.run() == 0
        second = a.outputs()
        assert all(np.array_equal(x, y) for x, y in zip(first, second))
        assert not (first[0] == GARBAGE).any() and not (second[0] == -777).any()
        assert (first[0] >= 0).all() and (first[0] < k).all() and (first[1] >= 0).all() and (first[3] >= 0).all()


def test_every_refusal_returns_an_error_and_launches_nothing():
    k, words = 7, _words(20)
    m, cov, contact = _case(3, k, words, 0.5, "random", "random")
    bad = [dict(n=0), dict(n=65536), dict(k=0), dict(k=4097), dict(rounds=0), dict(rounds=4097), dict(words=0), dict(words=words + 2),
           dict(lazy=2), dict(lazy=-1), dict(mask_bits=None), dict(choice=None), dict(gain=None), dict(covered_out=None)]
    for kw in bad:
        call = _Call(m, cov, contact, 2, 1, ub=torch.full((N, k), GARBAGE, dtype=torch.int32, device=DEV))
        for f, v in kw.items():
            setattr(call.args, f, v)
        assert call.run() == 1, kw  # hipErrorInvalidValue
        torch.cuda.synchronize()
        for t in (call.choice, call.gain, call.cov_out, call.gains0, call.ub):
            assert bool((t == GARBAGE).all()), kw
    for field in ("mask_bits", "covered_in", "covered_out"):  # rows off the 16-byte grid
        call = _Call(m, cov, contact, 2, 1)
        setattr(call.args, field, getattr(call.args, field) + 4)
        assert call.run() == 1, field
        torch.cuda.synchronize()
        assert bool((call.choice == GARBAGE).all()) and bool((call.cov_out == GARBAGE).all())
    assert _Call(m, cov, contact, 2, 1).lib.gnbv_cover_greedy(None, None) == 1
    ok = _Call(m, cov, contact, 1, 1, covered_out=False)  # rounds == 1 goes without covered_out
    assert ok.run() == 0
    assert np.array_equal(ok.outputs()[0], _reference(m, cov, contact, 1)[0])
