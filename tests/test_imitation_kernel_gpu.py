"""GPU: csrc/imitation.hip's soft-target imitation loss (gnbv_imitation_loss), called through the C ABI and compared with fp64 torch
on the GPU (tests/imitation_oracle.py: the reference and the error model, which extends the one of tests/test_ppo_kernels_gpu.py by
the marginals' and W's rounding).  Outputs are NaN-prefilled and followed by a sentinel tail that must stay untouched.  Every bound
is carried elementwise in fp64 from the reference's own magnitudes and doubled (SAFETY); every case prints its largest err / bound
ratio and asserts it is <= 1.  A workgroup takes four samples (one wave each): batches of 1, 3, 4, 5 and 9 lie on both sides of one
and of two workgroups; 300 passes the 256 threads of the last workgroup's strided sums; k = 65 passes the 64 candidates a wave
stages in LDS."""
import ctypes as C
import math

import pytest
import torch

from gennbv_amd import _lib
from tests import imitation_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAFETY = 2.0
TAIL, SENTINEL = 64, 1234.5
F64 = torch.float64

SIX = [81, 81, 51, 1, 13, 13]  # the reference's action lattice
SMALL6 = [7, 5, 3, 1, 4, 2]
FIVE = [128, 65, 1, 64, 3]
EIGHT = [3, 1, 128, 7, 64, 2, 13, 5]
BIG3 = [129, 1, 1000]


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _out(*shape, dtype=torch.float32, fill=float("nan")):
    n = math.prod(shape)
    buf = torch.full((n + TAIL,), fill, dtype=dtype, device=DEV)
    buf[n:] = SENTINEL
    return buf[:n].view(*shape), buf


def _check_written(name, body, buf):
    n = body.numel()
    bad = int((~torch.isfinite(body)).sum())
    assert bad == 0, f"{name}: {bad} of {n} elements not written or not finite"
    assert bool((buf[n:] == SENTINEL).all()), f"{name}: the {TAIL} elements past the output were written"


def _ratio(got, want, bound):
    err = (got.double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=F64, device=err.device).expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


def _report(what, ratios):
    line = f"[err/bound] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
    print(line)
    assert max(ratios.values()) <= 1.0, line


def _inputs(dims, B, k, seed, weights=True, sample_w=True, dup=False, peaked=False):
    """fp32 / int64 inputs of one minibatch: random logits, values, returns, candidate tuples and positive weights.  dup: candidate 1
    repeats candidate 0's tuple (k >= 2)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    logits = (torch.randn(B, sum(dims), generator=gen, device=DEV, dtype=F64) * (40.0 if peaked else 2.0)).float().contiguous()
    values = torch.randn(B, generator=gen, device=DEV)
    returns = torch.randn(B, generator=gen, device=DEV)
    cand = torch.stack([torch.randint(0, d, (B, k), generator=gen, device=DEV) for d in dims], 2).contiguous()
    if dup and k >= 2:
        cand[:, 1] = cand[:, 0]
    cw = (torch.rand(B, k, generator=gen, device=DEV) + 0.05).contiguous() if weights else None
    sw = (torch.rand(B, generator=gen, device=DEV) * 2 + 0.1).contiguous() if sample_w else None
    return dict(logits=logits, values=values, returns=returns, cand=cand, cand_w=cw, sample_w=sw)


def _struct(dims, B, k, x, eps=0.0, ec=0.0, vf=0.0, rows=None, stats_rows=4, o=None):
    """A GnbvImitationLoss over fresh NaN-prefilled outputs (or the outputs `o` of an earlier call): (struct, outputs)."""
    if o is None:
        o = dict(d_logits=_out(B, sum(dims)), d_values=_out(B), stats=_out(stats_rows, 8),
                 stats_row=torch.zeros(1, dtype=torch.int64, device=DEV), flags=torch.zeros(1, dtype=torch.int32, device=DEV),
                 scratch=torch.zeros(8 * B + 64, dtype=torch.float32, device=DEV))
    a = _lib.GnbvImitationLoss()
    a.batch, a.n_logits, a.n_heads, a.k = B, sum(dims), len(dims), k
    for h, d in enumerate(dims):
        a.head_dims[h] = d
    a.label_smoothing, a.ent_coef, a.vf_coef = eps, ec, vf
    for name in ("logits", "values", "cand", "cand_w", "sample_w", "returns"):
        setattr(a, name, _lib.ptr(x.get(name)))
    a.rows = _lib.ptr(rows)
    a.d_logits, a.d_values = o["d_logits"][0].data_ptr(), o["d_values"][0].data_ptr()
    a.stats, a.stats_row, a.flags, a.scratch = o["stats"][0].data_ptr(), o["stats_row"].data_ptr(), o["flags"].data_ptr(), o["scratch"].data_ptr()
    return a, o


def _run(a):
    _lib.check(_lib.load().gnbv_imitation_loss(C.byref(a), _stream()), "gnbv_imitation_loss")
    torch.cuda.synchronize()


def _compare(what, dims, x, o, eps, ec, vf, row=0, flags=0):
    """Outputs of one call against the oracle within the doubled error model; returns the reference."""
    _check_written("d_logits", *o["d_logits"])
    _check_written("d_values", *o["d_values"])
    st, sbuf = o["stats"]
    assert bool(torch.isfinite(st[row]).all()), st[row]
    assert bool(torch.isnan(st[row + 1:]).all()), "statistics rows behind the current one were written"
    assert bool((sbuf[st.numel():] == SENTINEL).all())
    assert int(o["stats_row"]) == row + 1
    ref = orc.reference(dims, x["logits"], x.get("values"), x["cand"], x.get("cand_w"), x.get("sample_w"), x.get("returns"), eps, ec, vf)
    assert int(o["flags"]) == flags == ref["flags"], (int(o["flags"]), flags, ref["flags"])
    dead = ~ref["live"]
    assert bool((o["d_logits"][0][dead] == 0).all()) and bool((o["d_values"][0][dead] == 0).all()), "a dead sample's gradient is not zero"
    assert float(st[row, 6]) == float(ref["live"].sum()) and float(st[row, 7]) == 0.0
    if int(ref["live"].sum()) == 0:
        assert bool((o["d_logits"][0] == 0).all()) and bool((o["d_values"][0] == 0).all()) and bool((st[row] == 0).all())
        return ref
    bd = orc.bounds(dims, x["logits"], x["cand"], ref, eps, ec, vf)
    ratios = {k: _ratio(o[k][0], ref[k], SAFETY * bd[k]) for k in ("d_logits", "d_values")}
    ratios["stats"] = _ratio(st[row, :6], ref["stats"][:6], SAFETY * bd["stats"][:6])
    _report(what, ratios)
    return ref


CASES = [
    # name, dims, B, k, kwargs of _inputs, (eps, ent_coef, vf_coef)
    ("six-B1-k1", SIX, 1, 1, {}, (0.0, 0.0, 0.0)),
    ("six-B3-k2", SIX, 3, 2, dict(dup=True), (0.1, 0.01, 0.5)),
    ("six-B4-k33", SIX, 4, 33, {}, (0.0, 0.01, 0.0)),
    ("six-B5-k33", SIX, 5, 33, dict(dup=True), (0.1, 0.0, 0.5)),
    ("six-B128-k33", SIX, 128, 33, {}, (0.1, 0.01, 0.5)),
    ("six-B128-k1-hard", SIX, 128, 1, dict(weights=False, sample_w=False), (0.0, 0.0, 0.5)),
    ("six-B300-k2-peaked", SIX, 300, 2, dict(peaked=True), (0.1, 0.01, 0.5)),
    ("six-B9-k65", SIX, 9, 65, dict(dup=True), (0.1, 0.01, 0.5)),
    ("small6-B1-k2", SMALL6, 1, 2, {}, (0.1, 0.01, 0.5)),
    ("small6-B9-k33", SMALL6, 9, 33, dict(dup=True), (0.0, 0.0, 0.0)),
    ("small6-B300-k1", SMALL6, 300, 1, {}, (0.1, 0.01, 0.5)),
    ("five-B5-k2", FIVE, 5, 2, {}, (0.0, 0.01, 0.5)),
    ("five-B128-k33", FIVE, 128, 33, {}, (0.1, 0.0, 0.0)),
    ("eight-B4-k33", EIGHT, 4, 33, dict(dup=True), (0.1, 0.01, 0.5)),
    ("eight-B300-k2", EIGHT, 300, 2, {}, (0.0, 0.0, 0.5)),
    ("big3-B1-k1", BIG3, 1, 1, {}, (0.1, 0.01, 0.5)),
    ("big3-B5-k33", BIG3, 5, 33, dict(dup=True), (0.0, 0.01, 0.0)),
    ("big3-B128-k2-peaked", BIG3, 128, 2, dict(peaked=True), (0.1, 0.0, 0.5)),
    ("big3-B3-k65", BIG3, 3, 65, {}, (0.1, 0.01, 0.5)),
]


@pytest.mark.parametrize("name,dims,B,k,kw,hyper", CASES, ids=[c[0] for c in CASES])
def test_imitation_loss_vs_fp64_autograd(name, dims, B, k, kw, hyper):
    """d loss / d logits, d loss / d values and the statistics row against fp64 autograd of the loss written with torch."""
    x = _inputs(dims, B, k, seed=B * 31 + sum(dims) + k, **kw)
    a, o = _struct(dims, B, k, x, *hyper)
    _run(a)
    ref = _compare(f"imitation {name}", dims, x, o, *hyper)
    assert int(ref["live"].sum()) == B


@pytest.mark.parametrize("dims", [SIX, BIG3], ids=["six", "big3"])
def test_values_null_means_no_value_term(dims):
    B, k = 9, 2
    x = _inputs(dims, B, k, seed=5)
    x["values"] = None
    a, o = _struct(dims, B, k, x, 0.1, 0.01, 0.5)
    a.d_values = None
    _run(a)
    assert bool(torch.isnan(o["d_values"][0]).all()), "d_values was written without values"
    o["d_values"][0].zero_()
    x["returns"] = None
    ref = _compare("values NULL", dims, x, o, 0.1, 0.01, 0.5)
    assert float(o["stats"][0][0, 1]) == 0.0 and float(ref["stats"][1]) == 0.0


DEAD = ["sample_w0", "q0", "bad_index", "neg_weight", "nan_weight", "inf_sample_w"]


def _kill(x, dims, b, how):
    """Makes sample b dead; returns the flag bits it must raise."""
    if how == "sample_w0":
        x["sample_w"][b] = 0.0
        return 0
    if how == "q0":
        x["cand_w"][b] = 0.0
        return 0
    if how == "bad_index":
        x["cand"][b, -1, 1] = dims[1]
        return 1
    if how == "neg_weight":
        x["cand_w"][b, 0] = -0.5
        return 2
    if how == "nan_weight":
        x["cand_w"][b, -1] = float("nan")
        return 2
    x["sample_w"][b] = float("inf")
    return 2


@pytest.mark.parametrize("how", DEAD)
@pytest.mark.parametrize("dims,k", [(SIX, 33), (BIG3, 2)], ids=["six-k33", "big3-k2"])
def test_dead_samples_among_live_ones(dims, k, how):
    """Two dead samples (one in the first workgroup, one in the last) in a batch of nine: zero gradient rows, no share in any sum,
    the flag bits of the cause and no other."""
    B = 9
    x = _inputs(dims, B, k, seed=11 + k)
    flags = 0
    for b in (2, 8):
        flags |= _kill(x, dims, b, how)
    a, o = _struct(dims, B, k, x, 0.1, 0.01, 0.5)
    _run(a)
    ref = _compare(f"dead {how}", dims, x, o, 0.1, 0.01, 0.5, flags=flags)
    assert ref["live"].tolist() == [b not in (2, 8) for b in range(B)]


def test_zero_weight_candidate_out_of_range_does_not_flag():
    """A candidate of weight 0 takes part in nothing: its index may lie anywhere (a refused candidate's tuple is never judged)."""
    dims, B, k = SIX, 9, 33
    x = _inputs(dims, B, k, seed=3)
    for b, j, v in ((0, 5, 81), (4, 0, -1), (8, 32, 2 ** 40)):
        x["cand_w"][b, j] = 0.0
        x["cand"][b, j, 0] = v
    a, o = _struct(dims, B, k, x, 0.1, 0.01, 0.5)
    _run(a)
    ref = _compare("zero-weight out of range", dims, x, o, 0.1, 0.01, 0.5)
    assert int(ref["live"].sum()) == B


@pytest.mark.parametrize("how", ["sample_w0", "q0", "bad_index", "neg_weight"])
def test_all_dead_batch(how):
    dims, B, k = SIX, 9, 2
    x = _inputs(dims, B, k, seed=7)
    flags = 0
    for b in range(B):
        flags |= _kill(x, dims, b, how)
    a, o = _struct(dims, B, k, x, 0.1, 0.01, 0.5)
    _run(a)
    _compare(f"all dead {how}", dims, x, o, 0.1, 0.01, 0.5, flags=flags)


@pytest.mark.parametrize("dims,k", [(SIX, 33), (BIG3, 65)], ids=["six-k33", "big3-k65"])
def test_rows_is_bit_identical_to_gathered_arrays(dims, k):
    B, M = 9, 40
    src = _inputs(dims, M, k, seed=21)
    src["sample_w"][5] = 0.0
    rows = torch.tensor([39, 0, 5, 17, 17, 3, 22, 1, 38], dtype=torch.int64, device=DEV)
    x = dict(src, logits=src["logits"][:B].contiguous(), values=src["values"][:B].contiguous())
    a, o = _struct(dims, B, k, x, 0.1, 0.01, 0.5, rows=rows)
    _run(a)
    g = dict(x, **{n: src[n][rows].contiguous() for n in ("cand", "cand_w", "sample_w", "returns")})
    a2, o2 = _struct(dims, B, k, g, 0.1, 0.01, 0.5)
    _run(a2)
    for n in ("d_logits", "d_values", "stats"):
        assert torch.equal(o[n][0][:1] if n == "stats" else o[n][0], o2[n][0][:1] if n == "stats" else o2[n][0]), n
    _compare("rows", dims, g, o, 0.1, 0.01, 0.5)


def test_two_calls_advance_stats_row_and_reuse_scratch():
    dims, B, k = SIX, 9, 2
    x = _inputs(dims, B, k, seed=31)
    a, o = _struct(dims, B, k, x, 0.1, 0.01, 0.5)
    _run(a)
    first = {n: o[n][0].clone() for n in ("d_logits", "d_values", "stats")}
    counter = o["scratch"][8 * B:].view(torch.int32)
    assert int(counter.abs().sum()) == 0, "the completion counter was not left at zero"
    y = _inputs(dims, B, k, seed=32)
    o["d_logits"][0].fill_(float("nan"))
    o["d_values"][0].fill_(float("nan"))
    a2, _ = _struct(dims, B, k, y, 0.1, 0.01, 0.5, o=o)
    _run(a2)
    assert torch.equal(o["stats"][0][0], first["stats"][0]), "the first statistics row changed"
    _compare("second call", dims, y, o, 0.1, 0.01, 0.5, row=1)
    # and the first inputs again give the first call's bits (deterministic, scratch reusable)
    a3, _ = _struct(dims, B, k, x, 0.1, 0.01, 0.5, o=o)
    _run(a3)
    assert int(o["stats_row"]) == 3
    assert torch.equal(o["d_logits"][0], first["d_logits"]) and torch.equal(o["d_values"][0], first["d_values"])
    assert torch.equal(o["stats"][0][2], first["stats"][0])


@pytest.mark.parametrize("dims", [SIX, BIG3], ids=["six", "big3"])
def test_agreement_counts_exactly_the_samples_whose_argmax_is_the_best_candidate(dims):
    """Logits built so that the arg-max is j*'s tuple on the even samples and differs from it on exactly one head (in turn) on the
    odd ones; j* is the FIRST candidate of the largest weight (candidates 1 and 2 tie)."""
    B, k = 10, 3
    x = _inputs(dims, B, k, seed=41)
    x["cand_w"][:, 0], x["cand_w"][:, 1], x["cand_w"][:, 2] = 0.25, 0.75, 0.75
    multi = [h for h, d in enumerate(dims) if d > 1]
    off = [sum(dims[:h]) for h in range(len(dims))]
    for b in range(B):
        for h in multi:
            c = int(x["cand"][b, 1, h])
            if b % 2 == 1 and h == multi[(b // 2) % len(multi)]:
                c = (c + 1) % dims[h]
            x["logits"][b, off[h] + c] = 30.0
    x["cand"][:, 2] = (x["cand"][:, 1] + 1) % torch.tensor(dims, device=DEV)  # the later tie differs on every head of more than one category
    a, o = _struct(dims, B, k, x)
    _run(a)
    ref = _compare("agreement", dims, x, o, 0.0, 0.0, 0.0)
    assert float(ref["stats"][3]) == 0.5 and abs(float(o["stats"][0][0, 3]) - 0.5) < 1e-6
    # an even tie of the logits resolves to the first arg-max
    h = multi[0]
    x["logits"][0, off[h]:off[h] + dims[h]] = 0.0
    c = int(x["cand"][0, 1, h])
    a, o = _struct(dims, B, k, x)
    _run(a)
    assert abs(float(o["stats"][0][0, 3]) - (0.5 if c == 0 else 0.4)) < 1e-6
