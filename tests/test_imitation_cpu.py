"""CPU: the imitation pieces that need no GPU -- soft_targets against its fp64 formula, the Demonstrations ring on CPU tensors,
the loss oracle (tests/imitation_oracle.py) against itself, and the refusals of gnbv_imitation_loss (its argument checks precede any
HIP call, so the library can be asked without a device)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import imitation_oracle as orc

F64 = torch.float64
SIX = [81, 81, 51, 1, 13, 13]
INVALID = 1  # hipErrorInvalidValue


# ---------------------------------------------------------------------------------------------------------------------------------
def _soft_ref(score, temperature):
    out = np.zeros(score.shape, dtype=np.float64)
    for i, row in enumerate(score.tolist()):
        ok = [j for j, s in enumerate(row) if s >= 0]
        if not ok:
            continue
        smax = max(row[j] for j in ok)
        e = {j: math.exp((row[j] - smax) / (temperature * max(1, smax))) for j in ok}
        tot = sum(e.values())
        for j in ok:
            out[i, j] = e[j] / tot
    return out.astype(np.float32)


def test_soft_targets_is_the_fp64_formula_rounded_once():
    from gennbv_amd.eval.baselines import soft_targets
    gen = torch.Generator().manual_seed(0)
    score = torch.randint(-1, 400, (64, 8), generator=gen)
    score[3] = -1                                        # every candidate refused
    score[4] = torch.tensor([7, 7, -1, 7, 0, 7, -1, 3])  # ties
    score[5] = torch.tensor([0, 0, -1, 0, 0, 0, 0, 0])   # nothing to gain anywhere: uniform over the admitted
    score[6] = torch.tensor([-1, -1, -1, -1, -1, 250, -1, -1])
    for temp in (0.05, 0.5, 3.0):
        q = soft_targets(score, temp)
        assert q.dtype == torch.float32 and q.shape == score.shape
        assert np.array_equal(q.numpy(), _soft_ref(score, temp)), temp
        assert bool((q[score < 0] == 0).all()) and bool((q[3] == 0).all())
        live = torch.arange(64) != 3
        assert float((q[live].double().sum(1) - 1).abs().max()) < 1e-6
        assert q[4, 0] == q[4, 1] == q[4, 3] == q[4, 5] and float(q[6, 5]) == 1.0
    assert torch.equal(soft_targets(score, 0.5)[5], torch.tensor([1, 1, 0, 1, 1, 1, 1, 1]) / 7)


def test_soft_targets_at_a_very_small_temperature_is_one_hot_on_the_first_best():
    from gennbv_amd.eval.baselines import choose, soft_targets
    gen = torch.Generator().manual_seed(1)
    score = torch.randint(0, 300, (32, 8), generator=gen)
    score[:, 2] = -1
    score[0, 5] = score[0].max() + 1  # (an untied row)
    q = soft_targets(score, 1e-6)
    tied = (score == score.amax(1, keepdim=True))
    # all mass on the best candidates, shared evenly among ties; the FIRST arg-max of the weights is the candidate `choose` picks
    assert float((q * (~tied)).abs().max()) == 0.0
    assert torch.allclose(q.double().sum(1), torch.ones(32, dtype=F64), atol=1e-6)
    gain = torch.stack([score.clamp(min=0), torch.zeros_like(score), torch.zeros_like(score)], -1)
    best = choose(gain, (1, 0), contact=(score < 0).to(torch.uint8))
    assert torch.equal(q.argmax(1), best)
    assert float(q[0, 5]) == 1.0
    with pytest.raises(ValueError):
        soft_targets(score, 0.0)
    with pytest.raises(TypeError):
        soft_targets(score)  # no default temperature


def test_choose_scored_returns_what_choose_ranked():
    from gennbv_amd.eval.baselines import candidate_score, choose, choose_scored
    gen = torch.Generator().manual_seed(2)
    gain = torch.randint(0, 50, (16, 8, 3), generator=gen, dtype=torch.int32)
    contact = (torch.rand(16, 8, generator=gen) < 0.3).to(torch.uint8)
    contact[1] = 1
    best, score = choose_scored(gain, (1, 4), contact)
    assert torch.equal(best, choose(gain, (1, 4), contact)) and torch.equal(score, candidate_score(gain, (1, 4), contact))
    want = gain[..., 0].long() + 4 * gain[..., 1].long()
    assert torch.equal(score, torch.where(contact != 0, torch.full_like(want, -1), want)) and score.dtype == torch.int64
    assert torch.equal(best, torch.tensor([int(np.argmax(r)) for r in score.tolist()]))  # (numpy: the first of the largest)


# ---------------------------------------------------------------------------------------------------------------------------------
def _block(r, s, g3, rgb, k, fill):
    gen = torch.Generator().manual_seed(fill)
    obs = torch.randn(r, s + g3 + rgb, generator=gen)
    obs[:, s:s + g3] = torch.randint(-1, 2, (r, g3), generator=gen).float()
    return dict(obs=obs, cand=torch.randint(0, 13, (r, k, 6), generator=gen), cand_w=torch.rand(r, k, generator=gen),
                sample_w=torch.rand(r, generator=gen), rewards=torch.randn(r, generator=gen), values=torch.randn(r, generator=gen),
                returns=torch.randn(r, generator=gen), episode_starts=(torch.rand(r, generator=gen) < 0.2).to(torch.uint8))


def test_demonstrations_append_blocks_and_overwrite_the_oldest():
    from gennbv_amd.sb3.imitation import Demonstrations
    r, s, g3, rgb, k = 6, 12, 27, 5, 3
    d = Demonstrations(3 * r, r, s, g3, rgb, k, 6, "cpu")
    assert d.grid_i8.dtype == torch.int8 and d.small.shape == (18, s + rgb) and d.cand.dtype == torch.int64 and d.filled == 0
    blocks = [_block(r, s, g3, rgb, k, i) for i in range(5)]
    where = []
    for i, b in enumerate(blocks):
        where.append(d.append(**b))
        assert d.blocks == i + 1 and d.filled == min(18, (i + 1) * r)
    assert [w.start for w in where] == [0, 6, 12, 0, 6]  # blocks 3 and 4 overwrote blocks 0 and 1
    for i, slot in ((3, 0), (4, 1), (2, 2)):
        sl, b = slice(slot * r, (slot + 1) * r), blocks[i]
        rows = torch.arange(sl.start, sl.stop)
        assert torch.equal(d.dense_rows(rows), b["obs"]), "observations are not bit-equal after the int8 round trip"
        for name in ("cand", "cand_w", "sample_w", "rewards", "values", "returns", "episode_starts"):
            assert torch.equal(getattr(d, name)[sl], b[name]), name
    with pytest.raises(ValueError):
        d.append(**_block(r + 1, s, g3, rgb, k, 9))
    with pytest.raises(ValueError):
        Demonstrations(20, 6, s, g3, rgb, k)


# ---------------------------------------------------------------------------------------------------------------------------------
def _case(dims, B, k, seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(logits=torch.randn(B, sum(dims), generator=gen) * 2, values=torch.randn(B, generator=gen), returns=torch.randn(B, generator=gen),
                cand=torch.stack([torch.randint(0, d, (B, k), generator=gen) for d in dims], 2), cand_w=torch.rand(B, k, generator=gen) + 0.05,
                sample_w=torch.rand(B, generator=gen) + 0.1)


def _ref(dims, x, **kw):
    return orc.reference(dims, x["logits"], x["values"], x["cand"], x["cand_w"], x["sample_w"], x["returns"], **kw)


def test_oracle_hard_label_is_the_sum_of_per_head_cross_entropies():
    dims, B = SIX, 7
    x = _case(dims, B, 1, 0)
    x["cand_w"], x["sample_w"] = None, None
    ref = _ref(dims, x)
    lg = x["logits"].double().requires_grad_()
    off, ce = 0, 0.0
    for h, n in enumerate(dims):
        ce = ce + torch.nn.functional.cross_entropy(lg[:, off:off + n], x["cand"][:, 0, h], reduction="sum")
        off += n
    (ce / B).backward()
    ce = ce.detach()
    assert abs(float(ref["stats"][0]) - float(ce) / B) < 1e-12 and abs(float(ref["stats"][5]) - float(ce) / B) < 1e-12
    assert float((ref["d_logits"] - lg.grad).abs().max()) < 1e-14
    assert abs(float(ref["stats"][4]) - float(ce) / B) < 1e-12  # hard nll of j* = the cross-entropy itself
    assert float(ref["stats"][6]) == B and ref["flags"] == 0


def test_oracle_gradient_is_the_closed_form_of_the_header():
    """d_logits = (w/W)((p - m) + c_e p (lp + H)), d_values = (w/W) 2 c_v (v - R): the formula the kernel implements, against autograd."""
    dims, B, k = [7, 5, 3, 1, 4, 2], 9, 4
    x = _case(dims, B, k, 3)
    x["sample_w"][2] = 0.0
    eps, ec, vf = 0.1, 0.01, 0.5
    ref = _ref(dims, x, label_smoothing=eps, ent_coef=ec, vf_coef=vf)
    eps, ec, vf = orc.f32(eps), orc.f32(ec), orc.f32(vf)
    w, W = ref["wl"], ref["W"]
    want = []
    for st, m in zip(orc.head_stats(x["logits"], dims), ref["ms"]):
        want.append((w / W)[:, None] * ((st["p"] - m) + ec * st["p"] * (st["lp"] + st["H"][:, None])))
    assert float((torch.cat(want, 1) - ref["d_logits"]).abs().max()) < 1e-14
    assert float(((w / W) * 2 * vf * (x["values"].double() - x["returns"].double()) - ref["d_values"]).abs().max()) < 1e-14
    assert bool((ref["d_logits"][2] == 0).all()) and float(ref["stats"][6]) == B - 1


def test_oracle_duplicate_candidates_equal_one_with_the_summed_weight_and_scaling_changes_nothing():
    dims, B = SIX, 6
    x = _case(dims, B, 3, 5)
    x["cand"][:, 2] = x["cand"][:, 0]
    kw = dict(label_smoothing=0.1, ent_coef=0.01, vf_coef=0.5)
    a = _ref(dims, x, **kw)
    y = dict(x, cand=x["cand"][:, :2].contiguous(), cand_w=torch.stack([x["cand_w"][:, 0].double() + x["cand_w"][:, 2].double(), x["cand_w"][:, 1].double()], 1))
    b = _ref(dims, y, **kw)
    assert float((a["d_logits"] - b["d_logits"]).abs().max()) < 1e-15 and float((a["stats"][:3] - b["stats"][:3]).abs().max()) < 1e-13
    z = dict(x, cand_w=x["cand_w"] * torch.tensor([0.5, 2.0, 4.0, 8.0, 0.25, 16.0])[:, None])  # (powers of two: exact)
    c = _ref(dims, z, **kw)
    assert torch.equal(a["d_logits"], c["d_logits"]) and torch.equal(a["stats"], c["stats"])


def test_oracle_liveness_rules():
    dims, B, k = SIX, 8, 3
    x = _case(dims, B, k, 7)
    x["sample_w"][0] = 0.0               # dead
    x["cand_w"][1] = 0.0                 # Q = 0: dead
    x["cand"][2, 1, 0] = 81              # out of range with weight: dead, bit 0
    x["cand_w"][3, 2] = -1.0             # dead, bit 1
    x["cand"][4, 0, 2], x["cand_w"][4, 0] = 99, 0.0  # out of range without weight: live, no flag
    x["cand"][0, 0, 0] = -5              # a sample that weighs nothing is not judged
    live, flags, _, _ = orc.liveness(dims, x["cand"], x["cand_w"], x["sample_w"])
    assert live.tolist() == [False, False, False, False, True, True, True, True] and flags == 3
    ref = _ref(dims, x)
    assert bool((ref["d_logits"][:4] == 0).all()) and float(ref["stats"][6]) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
def _args(dims=SIX, B=4, k=2):
    from gennbv_amd import _lib
    a = _lib.GnbvImitationLoss()
    a.batch, a.n_logits, a.n_heads, a.k = B, sum(dims), len(dims), k
    for h, d in enumerate(dims):
        a.head_dims[h] = d
    a.label_smoothing, a.ent_coef, a.vf_coef = 0.1, 0.01, 0.5
    fake = 0x1000  # (never dereferenced: every call below is refused before a launch)
    for name in ("logits", "values", "cand", "cand_w", "sample_w", "returns", "rows", "d_logits", "d_values", "stats", "stats_row", "flags", "scratch"):
        setattr(a, name, fake)
    return a


BAD = [
    ("batch 0", lambda a: setattr(a, "batch", 0)), ("k 0", lambda a: setattr(a, "k", 0)),
    ("no heads", lambda a: setattr(a, "n_heads", 0)), ("nine heads", lambda a: setattr(a, "n_heads", 9)),
    ("head of 0", lambda a: a.head_dims.__setitem__(3, 0)), ("head of 1025", lambda a: a.head_dims.__setitem__(0, 1025)),
    ("sum != n_logits", lambda a: setattr(a, "n_logits", a.n_logits + 1)),
    ("smoothing 1", lambda a: setattr(a, "label_smoothing", 1.0)), ("smoothing < 0", lambda a: setattr(a, "label_smoothing", -0.1)),
    ("smoothing nan", lambda a: setattr(a, "label_smoothing", float("nan"))),
    ("ent_coef < 0", lambda a: setattr(a, "ent_coef", -1.0)), ("vf_coef < 0", lambda a: setattr(a, "vf_coef", -1.0)),
    ("no logits", lambda a: setattr(a, "logits", None)), ("no cand", lambda a: setattr(a, "cand", None)),
    ("no d_logits", lambda a: setattr(a, "d_logits", None)), ("no stats", lambda a: setattr(a, "stats", None)),
    ("no stats_row", lambda a: setattr(a, "stats_row", None)), ("no flags", lambda a: setattr(a, "flags", None)),
    ("no scratch", lambda a: setattr(a, "scratch", None)),
    ("values without d_values", lambda a: setattr(a, "d_values", None)),
    ("values and vf_coef without returns", lambda a: setattr(a, "returns", None)),
]


@pytest.mark.parametrize("name,spoil", BAD, ids=[b[0] for b in BAD])
def test_imitation_loss_refuses_before_any_launch(name, spoil):
    from gennbv_amd import _lib
    from gennbv_amd.csrc import build
    build.build(verbose=False)
    lib = _lib.load()
    a = _args()
    spoil(a)
    assert lib.gnbv_imitation_loss(C.byref(a), None) == INVALID
    assert lib.gnbv_imitation_loss(None, None) == INVALID


def test_imitation_struct_matches_the_header():
    """Field order and types of the ctypes struct against the header's declaration (the call reads the struct by offset)."""
    import os
    import re
    from gennbv_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "gennbv_hip.h")).read()
    body = re.search(r"typedef struct GnbvImitationLoss \{(.*?)\} GnbvImitationLoss;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            names.append(re.findall(r"(\w+)\s*(?:\[\d+\])?$", part.strip())[0])
    assert names == [f[0] for f in _lib.GnbvImitationLoss._fields_]
