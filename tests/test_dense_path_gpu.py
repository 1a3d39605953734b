"""GPU: the policy's dense path through the C ABI against fp64 torch of the same operation, element by element --
  1. gnbv_policy_head_forward / _backward (csrc/head.hip), stage by stage,
  2. gnbv_linear_forward (csrc/linear.hip: the fp32-MFMA and the split-f16 stage 1, 4 and 8 waves, and the reduce),
  3. gnbv_pose_encode (csrc/linear.hip).
Outputs are prefilled with NaN and followed by a sentinel tail (tests/abi_check.py); every case prints its largest err / bound ratio.

Error models (u = 2^-24, gamma(n) = n u / (1 - n u)):
  fp32 MFMA   v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain with one rounding per product, so a contraction of length L plus one
              bias add is within gamma(L + 1) (|A| |B| + |bias|) of the exact value; a plain fp32 sum of M terms within gamma(M) sum |a|.
              For gnbv_linear_forward the chain of a chunk has at most Lc = 32 (ceil(ceil(K / 32) / nchunks) + 1) terms and is followed
              by nchunks partial sums and the bias: gamma(Lc + nchunks + 1).
  split f16   the model of tests/test_linear_gpu.py with the forward's fixed scalings (x by 2^6, W by 2^12):
              C_REL (|x| |W|^T) + 2^-25 / 2^12 sum_k |x| + 2^-25 / 2^6 sum_k |W| + u |bias|.
An element whose bound is 0 must be exact."""
import math

import pytest
import torch

from gennbv_amd import _lib
from tests.abi_check import DEV, SENTINEL, TAIL, _check_written, _out, _ratio, _report, _stream

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
C_REL = 1e-6
X_SCALE, W_SCALE = 2.0 ** 6, 2.0 ** 12  # (kLinXScale, kLinWScale)
X_CLAMP, W_CLAMP = 65000.0 / 64.0, 65000.0 / 4096.0  # (kLinMax / scale)


def gamma(n):
    return n * U / (1.0 - n * U)


def _ceil_div(a, b):
    return -(-a // b)


@pytest.fixture(autouse=True)
def _kernel_choice_by_flag_word_only(monkeypatch):
    """Nothing here depends on GENNBV_CONV_SPLIT: the tests pick the arithmetic through the flag word."""
    monkeypatch.delenv("GENNBV_CONV_SPLIT", raising=False)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _padded(t):
    """A copy of t followed by TAIL zeros (a pointer 4 bytes off still reads inside the allocation)."""
    buf = torch.zeros(t.numel() + TAIL, dtype=t.dtype, device=DEV)
    buf[:t.numel()] = t.flatten()
    return buf[:t.numel()].view(t.shape)


def _untouched(r, bufs):
    torch.cuda.synchronize()
    for name in r:
        n = r[name].numel()
        assert bool(torch.isnan(r[name]).all()), f"{name} was written by a refused call"
        assert bool((bufs[name][n:] == SENTINEL).all()), name


# =================================================================================================================================
# 1. policy head
# =================================================================================================================================
HEAD_REAL = [(128, 256, 256, 256, 240), (256, 256, 256, 256, 240), (128, 256, 512, 256, 240)]  # minibatch, rollout, semantic branch
HEAD_SHAPES = (HEAD_REAL
               + [(m, 256, 256, 256, 240) for m in (1, 15, 16, 17, 129, 1000)]
               # K = 32: one round trip, 14 of 16 groups dead; K = 512 from 16 + 496; the fa | fg seam inside a round trip; K = 528: a
               # third round trip with one live group
               + [(37, 16, 16, 256, 17), (37, 16, 496, 256, 17), (37, 272, 240, 256, 17), (37, 256, 272, 256, 17)]
               + [(37, 64, 64, f, 17) for f in (16, 48, 144)]  # kind 0's clamp; one F tile; F / 16 not a power of two
               + [(37, 256, 256, 256, a) for a in (1, 15, 16, 31, 32, 241)])  # where the value head sits in the action tiles
HEAD_IDS = ["M{}_K{}+{}_F{}_A{}".format(*s) for s in HEAD_SHAPES]
FWD_ORDER = ["fa", "fg", "M", "K1", "K2", "W_out", "b_out", "F", "W_act", "b_act", "A", "W_val", "b_val", "feat", "logits", "values"]
FWD_OUT = ["feat", "logits", "values"]
BWD_ORDER = ["fa", "fg", "M", "K1", "K2", "feat", "d_logits", "d_values", "W_out", "F", "W_act", "A", "W_val", "dH", "d_fa", "d_fg", "gW_out",
             "gb_out", "gW_act", "gb_act", "gW_val", "gb_val"]
BWD_OUT = BWD_ORDER[13:]
DIMS = ("M", "K1", "K2", "F", "A")


def _head_inputs(m, k1, k2, f, a, seed, pad=False):
    """Inputs like the real ones: fa, fg ReLU outputs (half of them exactly 0); weights randn / sqrt(fan_in); b_out shifted so that
    roughly 40 % of feat is exactly 0; d_logits / d_values with rows spread over 1e-6 .. 1 and (from 4 rows on) two rows exactly 0."""
    gen = _gen(seed)

    def rn(*s):
        return torch.randn(*s, generator=gen, device=DEV)

    p = {"fa": torch.relu(rn(m, k1)), "fg": torch.relu(rn(m, k2)),
         "W_out": rn(f, k1 + k2) / math.sqrt(k1 + k2), "W_act": rn(a, f) / math.sqrt(f), "b_act": 0.1 * rn(a),
         "W_val": rn(1, f) / math.sqrt(f), "b_val": 0.1 * rn(1)}
    pre = torch.cat((p["fa"], p["fg"]), 1).double() @ p["W_out"].double().t()
    p["b_out"] = 0.05 * rn(f) - float(torch.quantile(pre.flatten(), 0.4))
    rs = 10.0 ** (-6.0 * torch.rand(m, 1, generator=gen, device=DEV))
    if m >= 4:
        rs[1], rs[m // 2] = 0.0, 0.0
    p["d_logits"] = rn(m, a) * rs
    p["d_values"] = rn(m) * rs[:, 0]
    if pad:
        p = {k: _padded(v) for k, v in p.items()}
    p.update(M=m, K1=k1, K2=k2, F=f, A=a)
    return p


def _head_call(fn, order, p, r, **over):
    vals = []
    for k in order:
        v = over[k] if k in over else (r[k] if k in r else p[k])
        vals.append(v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return fn(*vals, _stream())


def _head_outputs(p, names):
    m, k1, k2, f, a = (p[k] for k in DIMS)
    shapes = {"feat": (m, f), "logits": (m, a), "values": (m,), "dH": (m, f), "d_fa": (m, k1), "d_fg": (m, k2), "gW_out": (f, k1 + k2),
              "gb_out": (f,), "gW_act": (a, f), "gb_act": (a,), "gW_val": (1, f), "gb_val": (1,)}
    r, bufs = {}, {}
    for name in names:
        r[name], bufs[name] = _out(*shapes[name])
    return r, bufs


def _head_forward(p):
    """gnbv_policy_head_forward on fresh NaN-prefilled outputs; every element written and finite, nothing past them."""
    lib = _lib.load()
    r, bufs = _head_outputs(p, FWD_OUT)
    _lib.check(_head_call(lib.gnbv_policy_head_forward, FWD_ORDER, p, r), "gnbv_policy_head_forward")
    torch.cuda.synchronize()
    for name in r:
        _check_written(name, r[name], bufs[name])
    return r


def _head_backward(p, feat):
    lib = _lib.load()
    r, bufs = _head_outputs(p, BWD_OUT)
    _lib.check(_head_call(lib.gnbv_policy_head_backward, BWD_ORDER, p, r, feat=feat), "gnbv_policy_head_backward")
    torch.cuda.synchronize()
    for name in r:
        _check_written(name, r[name], bufs[name])
    return r


def _mm_ratio(got, a, b, length, bias=None, relu=False):
    """got against the fp64 product a b (+ bias) within gamma(length + 1) (|a| |b| + |bias|)."""
    want, mag = a @ b, a.abs() @ b.abs()
    if bias is not None:
        want, mag = want + bias, mag + bias.abs()
    if relu:
        want = torch.relu(want)  # (1-Lipschitz: the bound of the pre-activation holds)
    return _ratio(got, want.view(got.shape), (gamma(length + 1) * mag).view(got.shape))


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=HEAD_IDS)
def test_policy_head_stages_vs_fp64(shape):
    """Forward and backward through the C ABI, each stage against fp64 of the kernel's own input to that stage (no ReLU-mask
    disagreement near 0 enters a bound): feat; logits, values from the kernel's feat; dH from the kernel's feat; d_fa | d_fg, gW_out,
    gb_out from the kernel's dH; gW_act, gb_act, gW_val, gb_val from the kernel's feat.  feat == 0 gives dH == 0 exactly.  A second
    call gives the same bits."""
    m, k1, k2, f, a = shape
    p = _head_inputs(m, k1, k2, f, a, seed=m * 7 + k1 * 3 + k2 * 5 + f * 11 + a * 13)
    d = {k: v.double() for k, v in p.items() if isinstance(v, torch.Tensor)}
    cat = torch.cat((d["fa"], d["fg"]), 1)
    fw = _head_forward(p)
    zeros = float((fw["feat"] == 0).double().mean())
    assert 0.2 < zeros < 0.6, zeros
    featd = fw["feat"].double()
    ratios = {"feat": _mm_ratio(fw["feat"], cat, d["W_out"].t(), k1 + k2, d["b_out"], relu=True),
              "logits": _mm_ratio(fw["logits"], featd, d["W_act"].t(), f, d["b_act"]),
              "values": _mm_ratio(fw["values"], featd, d["W_val"].t(), f, d["b_val"])}
    bw = _head_backward(p, fw["feat"])
    dead = fw["feat"] == 0
    assert bool((bw["dH"][dead] == 0).all()), "dH is not 0 where feat is 0"
    # dH: one contraction over the A + 1 entries [d_logits | d_values] x [W_act ; W_val], masked
    dcat, wcat = torch.cat((d["d_logits"], d["d_values"][:, None]), 1), torch.cat((d["W_act"], d["W_val"]), 0)
    live = (~dead).double()
    ratios["dH"] = _ratio(bw["dH"], live * (dcat @ wcat), gamma(a + 2) * live * (dcat.abs() @ wcat.abs()))
    dhd = bw["dH"].double()
    ratios["d_in"] = _mm_ratio(torch.cat((bw["d_fa"], bw["d_fg"]), 1), dhd, d["W_out"], f)
    ratios["gW_out"] = _mm_ratio(bw["gW_out"], dhd.t(), cat, m)
    ratios["gb_out"] = _ratio(bw["gb_out"], dhd.sum(0), gamma(m) * dhd.abs().sum(0))
    ratios["gW_act"] = _mm_ratio(bw["gW_act"], d["d_logits"].t(), featd, m)
    ratios["gb_act"] = _ratio(bw["gb_act"], d["d_logits"].sum(0), gamma(m) * d["d_logits"].abs().sum(0))
    ratios["gW_val"] = _mm_ratio(bw["gW_val"], d["d_values"][None, :], featd, m)
    ratios["gb_val"] = _ratio(bw["gb_val"], d["d_values"].sum().view(1), gamma(m) * d["d_values"].abs().sum().view(1))
    line = _report("head M{} K{}+{} F{} A{}".format(*shape), ratios)
    assert max(ratios.values()) <= 1.0, line
    fw2 = _head_forward(p)
    bw2 = _head_backward(p, fw["feat"])
    for name in FWD_OUT:
        assert torch.equal(fw[name], fw2[name]), name
    for name in BWD_OUT:
        assert torch.equal(bw[name], bw2[name]), name


class _Enc:
    def __init__(self, lo):
        self.output_layer = torch.nn.Sequential(lo, torch.nn.ReLU())


def _head_modules(p, write_through):
    k, f, a = p["K1"] + p["K2"], p["F"], p["A"]
    mods = [torch.nn.Linear(k, f).to(DEV), torch.nn.Linear(f, a).to(DEV), torch.nn.Linear(f, 1).to(DEV)]
    with torch.no_grad():
        for mod, w, b in zip(mods, ("W_out", "W_act", "W_val"), ("b_out", "b_act", "b_val")):
            mod.weight.copy_(p[w])
            mod.bias.copy_(p[b])
    for mod in mods:
        mod._grad_write_through = write_through
        if write_through:  # (the kernels write straight into .grad: ops/direct_grad.py)
            mod.weight.grad = torch.full_like(mod.weight, float("nan"))
            mod.bias.grad = torch.full_like(mod.bias, float("nan"))
    return mods


def _head_autograd_vs_fp64(p, write_through):
    """policy_head through autograd against fp64 autograd of the three linears, at test_fused_policy_head_vs_fp64's tolerances."""
    from gennbv_amd.ops import encoder_ops as eo
    lo, la, lv = _head_modules(p, write_through)
    assert eo.policy_head_supported(_Enc(lo), la, lv)
    fa, fg = p["fa"].clone().requires_grad_(True), p["fg"].clone().requires_grad_(True)
    logits, values, feat = eo.policy_head(_Enc(lo), la, lv, fa, fg)
    cat = torch.cat((fa, fg), -1).detach().double().requires_grad_(True)
    wd = [t.detach().double().requires_grad_(True) for t in (lo.weight, lo.bias, la.weight, la.bias, lv.weight, lv.bias)]
    feat_ref = torch.relu(cat @ wd[0].t() + wd[1])
    logits_ref, values_ref = feat_ref @ wd[2].t() + wd[3], (feat_ref @ wd[4].t() + wd[5]).flatten()
    for got, ref in ((feat, feat_ref), (logits, logits_ref), (values, values_ref)):
        assert got.shape == ref.shape
        assert torch.allclose(got.double(), ref, rtol=1e-5, atol=1e-5), float((got.double() - ref).abs().max())
    torch.autograd.backward([logits, values], [p["d_logits"], p["d_values"]])
    torch.autograd.backward([logits_ref, values_ref], [p["d_logits"].double(), p["d_values"].double()])
    torch.cuda.synchronize()
    got = [fa.grad, fg.grad, lo.weight.grad, lo.bias.grad, la.weight.grad, la.bias.grad, lv.weight.grad, lv.bias.grad]
    ref = [cat.grad[:, :p["K1"]], cat.grad[:, p["K1"]:]] + [t.grad for t in wd]
    for g, r in zip(got, ref):
        assert g.shape == r.shape
        assert torch.allclose(g.double(), r, rtol=1e-4, atol=1e-4 * float(r.abs().max()) + 1e-7), float((g.double() - r).abs().max())


@pytest.mark.parametrize("write_through", [False, True], ids=["autograd", "write_through"])
@pytest.mark.parametrize("shape", HEAD_REAL, ids=HEAD_IDS[:len(HEAD_REAL)])
def test_policy_head_end_to_end_vs_fp64_autograd(shape, write_through):
    """The real shapes through encoder_ops.policy_head, gradients returned to autograd and written through into .grad."""
    _head_autograd_vs_fp64(_head_inputs(*shape, seed=sum(shape) + 1), write_through)


def test_policy_head_wrapper_on_an_uneven_split():
    """An output_layer with in_features = 64 fed as K1 = 48, K2 = 16 passes policy_head_supported (64 % 32 == 0) and both widths are
    multiples of 16, which is what the C entry needs: it must compute correctly.  Fed as 40 + 24 (also admitted by
    policy_head_supported, which sees modules and not the split) the C entry refuses and the wrapper raises: never garbage."""
    from gennbv_amd.ops import encoder_ops as eo
    _head_autograd_vs_fp64(_head_inputs(37, 48, 16, 64, 17, seed=4816), False)
    p = _head_inputs(37, 40, 24, 64, 17, seed=4024)
    lo, la, lv = _head_modules(p, False)
    with pytest.raises(_lib.GennbvHipError):
        eo.policy_head(_Enc(lo), la, lv, p["fa"], p["fg"])


def _refusal_cases(p, r, checked_aligned, pointers):
    cases = [("K1=24", {"K1": 24}), ("K2=8", {"K2": 8}), ("F=40", {"F": 40}), ("M=0", {"M": 0}), ("A=0", {"A": 0})]
    for name in checked_aligned:
        t = r[name] if name in r else p[name]
        cases.append((f"{name}+4", {name: t.data_ptr() + 4}))
    for name in pointers:
        cases.append((f"{name}=NULL", {name: None}))
    return cases


def test_policy_head_forward_refusals():
    """Unsupported widths, empty shapes, a pointer 4 bytes off (each one the entry checks) and a NULL (each pointer): a nonzero
    return code and no output touched.  (The bad values only shrink the shape: an entry that launched would still stay in bounds.)"""
    lib = _lib.load()
    p = _head_inputs(37, 32, 32, 48, 17, seed=1, pad=True)
    r, bufs = _head_outputs(p, FWD_OUT)
    pointers = [k for k in FWD_ORDER if k not in DIMS]
    for what, over in _refusal_cases(p, r, ["fa", "fg", "W_out", "W_act", "W_val", "feat"], pointers):
        assert _head_call(lib.gnbv_policy_head_forward, FWD_ORDER, p, r, **over) != 0, what
        _untouched(r, bufs)
    _lib.check(_head_call(lib.gnbv_policy_head_forward, FWD_ORDER, p, r), "gnbv_policy_head_forward")  # (the same arguments, unaltered, run)
    torch.cuda.synchronize()
    for name in r:
        _check_written(name, r[name], bufs[name])


def test_policy_head_backward_refusals():
    """The same for the backward entry (the one pointer it checks for alignment is dH_scratch)."""
    lib = _lib.load()
    p = _head_inputs(37, 32, 32, 48, 17, seed=2, pad=True)
    feat = _padded(_head_forward(p)["feat"])
    r, bufs = _head_outputs(p, BWD_OUT)
    pointers = [k for k in BWD_ORDER if k not in DIMS]
    for what, over in _refusal_cases(p, r, ["dH"], pointers):
        over.setdefault("feat", feat)
        assert _head_call(lib.gnbv_policy_head_backward, BWD_ORDER, p, r, **over) != 0, what
        _untouched(r, bufs)
    _lib.check(_head_call(lib.gnbv_policy_head_backward, BWD_ORDER, p, r, feat=feat), "gnbv_policy_head_backward")
    torch.cuda.synchronize()
    for name in r:
        _check_written(name, r[name], bufs[name])


# =================================================================================================================================
# 2. gnbv_linear_forward
# =================================================================================================================================
LIN_SHAPES = list(dict.fromkeys(
    [(128, 256, 54000), (256, 256, 54000), (128, 256, 1024), (128, 256, 2400), (128, 256, 256), (128, 256, 4096)]  # the real layers
    + [(m, 256, 1000) for m in (1, 16, 127, 128, 129, 200, 255, 256, 257, 600)]  # 4- and 8-wave workgroups, partial and several slabs
    + [(48, n, 1000) for n in (64, 128, 192)]  # column-tile decode
    + [(48, 64, k) for k in (4, 60, 64, 68, 72, 104, 1000, 1032)]  # fp32 only (4, 60, 68); a partial last 32-k trip
    + [(48, 64, k) for k in (128, 256, 512, 8192)]))  # with 64: the 1 -> 2 -> 4 -> 8 -> 128 chunk counts
LIN_IDS = [f"{m}x{n}x{k}" for m, n, k in LIN_SHAPES]


def _nchunks(lib, m, n, k):
    """Read back from the ABI: the workspace is nchunks partial [M][N] fp32 slabs + 256 bytes."""
    body = lib.gnbv_linear_workspace_bytes(m, n, k) - 256
    assert body > 0 and body % (4 * m * n) == 0
    return body // (4 * m * n)


def _lin_inputs(m, n, k, seed, variant="pos"):
    """x = 10^U(-3, 1) (variant "zeros": 30 % exact zeros; "signed": random signs -- the pose branch's first layer sees sin / cos);
    W randn / sqrt(K); bias 0.1 randn."""
    gen = _gen(seed)
    x = 10.0 ** (torch.rand(m, k, generator=gen, device=DEV) * 4.0 - 3.0)
    if variant == "zeros":
        x = x * (torch.rand(m, k, generator=gen, device=DEV) >= 0.3)
    elif variant == "signed":
        x = x * torch.sign(torch.randn(m, k, generator=gen, device=DEV))
    w = torch.randn(n, k, generator=gen, device=DEV) / math.sqrt(k)
    b = 0.1 * torch.randn(n, generator=gen, device=DEV)
    return x.contiguous(), w, b


def _lin_forward(lib, x, w, b, flag):
    """gnbv_linear_forward with flag word `flag` (bit 0: ReLU, bit 1: fp32 arithmetic) on a NaN-prefilled output and a workspace of
    NaN bytes: every partial the reduce reads must have been written by stage 1."""
    m, k = x.shape
    n = w.shape[0]
    ws = torch.full((lib.gnbv_linear_workspace_bytes(m, n, k),), 0xFF, dtype=torch.uint8, device=DEV)
    out, buf = _out(m, n)
    _lib.check(lib.gnbv_linear_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), m, n, k, flag, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
               "gnbv_linear_forward")
    torch.cuda.synchronize()
    _check_written(f"linear_forward flag {flag}", out, buf)
    return out


def _lin_bounds(lib, xd, wd, bd):
    """(fp64 x W^T + b, the fp32-path bound, the split-path bound) for fp64 copies of the operands as the kernel uses them."""
    m, k = xd.shape
    n = wd.shape[0]
    mag = xd.abs() @ wd.abs().t()
    nchunks = _nchunks(lib, m, n, k)
    lc = 32 * (_ceil_div(_ceil_div(k, 32), nchunks) + 1)
    fp32 = gamma(lc + nchunks + 1) * (mag + bd.abs())
    split = (C_REL * mag + (2.0 ** -25 / W_SCALE) * xd.abs().sum(1, keepdim=True) + (2.0 ** -25 / X_SCALE) * wd.abs().sum(1)[None, :]
             + U * bd.abs())
    return xd @ wd.t() + bd, fp32, split


def _split_eligible(k):
    return k % 8 == 0 and k >= 64


def _lin_check(what, m, n, k, seed, variant="pos"):
    lib = _lib.load()
    x, w, b = _lin_inputs(m, n, k, seed, variant)
    o = [_lin_forward(lib, x, w, b, flag) for flag in range(4)]
    assert torch.equal(o[1], torch.relu(o[0])), "split: relu = 1 is not max(relu = 0, 0)"
    assert torch.equal(o[3], torch.relu(o[2])), "fp32: relu = 1 is not max(relu = 0, 0)"
    want, fp32, split = _lin_bounds(lib, x.double(), w.double(), b.double())
    ratios = {"fp32": _ratio(o[2], want, fp32)}
    if _split_eligible(k):
        ratios["split"] = _ratio(o[0], want, split)
        assert not torch.equal(o[0], o[2]), "flag 0 and flag 2 gave the same bits: the split kernel did not run"
    else:
        assert torch.equal(o[0], o[2]), "K not eligible for the split kernels: flag 0 must give the fp32 kernel's bits"
    line = _report(f"linear {what}", ratios)
    assert max(ratios.values()) <= 1.0, line
    for flag in (0, 2):
        assert torch.equal(_lin_forward(lib, x, w, b, flag), o[flag]), f"flag {flag}: a second call gave other bits"


@pytest.mark.parametrize("m,n,k", LIN_SHAPES, ids=LIN_IDS)
def test_linear_forward_vs_fp64(m, n, k):
    """Every shape as split (flag 0 / 1) where eligible and as fp32 (flag 2 / 3), relu off and on, against fp64 within the two models."""
    _lin_check(f"{m}x{n}x{k}", m, n, k, seed=m * 7 + n * 131 + k)


@pytest.mark.parametrize("variant", ["zeros", "signed"])
@pytest.mark.parametrize("m,n,k", [(128, 256, 2400), (128, 256, 1024), (200, 256, 1000), (48, 64, 72)])
def test_linear_forward_zero_and_signed_inputs(m, n, k, variant):
    """x with 30 % exact zeros, and x of both signs."""
    _lin_check(f"{m}x{n}x{k} {variant}", m, n, k, seed=m + n + k, variant=variant)


@pytest.mark.parametrize("m", [129, 200, 256, 257, 600])
def test_linear_forward_rows_do_not_depend_on_their_slab(m):
    """Above 128 rows the split path runs 256-row workgroups (one staged W tile for both halves), several of them above 256: the
    output equals the concatenation of 128-row calls, bit for bit."""
    lib = _lib.load()
    n, k = 256, 1000
    x, w, b = _lin_inputs(m, n, k, seed=m)
    for flag in (0, 1):
        whole = _lin_forward(lib, x, w, b, flag)
        parts = torch.cat([_lin_forward(lib, x[i:i + 128].contiguous(), w, b, flag) for i in range(0, m, 128)])
        assert torch.equal(whole, parts), flag


@pytest.mark.parametrize("m", [48, 200])
def test_linear_forward_operand_clamps(m):
    """include/gennbv_hip.h: the split path clamps |x| at 65000 / 64 (1015.6) and |w| at 65000 / 4096 (15.87).  With x entries at 1014
    and 2000 and w entries at 15.7 and 40: the split output is the product of the CLAMPED operands within the split model (1014 and
    15.7 pass unchanged), the fp32 flag's output the product of the operands as given within the fp32 model."""
    lib = _lib.load()
    n, k = 64, 1000
    x, w, b = _lin_inputs(m, n, k, seed=m + 1)
    x[3, 5], x[7, 100], x[0, 999], x[m - 1, 0] = 1014.0, 2000.0, -2000.0, -1014.0
    w[2, 5], w[9, 100], w[11, 7], w[n - 1, 999] = 15.7, 40.0, -40.0, -15.7
    xc, wc = x.double().clamp(-X_CLAMP, X_CLAMP), w.double().clamp(-W_CLAMP, W_CLAMP)
    assert int((xc != x.double()).sum()) == 2 and int((wc != w.double()).sum()) == 2
    got_split, got_fp32 = _lin_forward(lib, x, w, b, 0), _lin_forward(lib, x, w, b, 2)
    want_c, _, split_c = _lin_bounds(lib, xc, wc, b.double())
    want, fp32, split = _lin_bounds(lib, x.double(), w.double(), b.double())
    ratios = {"split vs clamped": _ratio(got_split, want_c, split_c), "fp32 vs given": _ratio(got_fp32, want, fp32)}
    line = _report(f"linear clamps M{m}", ratios)
    assert max(ratios.values()) <= 1.0, line
    assert _ratio(got_split, want, split) > 100.0, "the clamped and the given product are too close for this test to tell them apart"


def test_linear_workspace_bytes_and_chunk_counts():
    """gnbv_linear_workspace_bytes is monotone in each argument; K = 64, 128, 256, 512, 8192 take 1, 2, 4, 8, 128 chunks; a
    workspace one byte short is refused."""
    lib = _lib.load()
    ms, ns, ks = [1, 16, 48, 128, 129, 256, 257, 600], [64, 128, 192, 256], [4, 60, 64, 68, 128, 256, 512, 1000, 1024, 2400, 4096, 8192, 54000]
    size = {(m, n, k): lib.gnbv_linear_workspace_bytes(m, n, k) for m in ms for n in ns for k in ks}
    assert min(size.values()) > 0
    for n in ns:
        for k in ks:
            by = [size[m, n, k] for m in ms]
            assert by == sorted(by), ("M", n, k)
    for m in ms:
        for k in ks:
            by = [size[m, n, k] for n in ns]
            assert by == sorted(by), ("N", m, k)
        for n in ns:
            by = [size[m, n, k] for k in ks]
            assert by == sorted(by), ("K", m, n)
    assert [_nchunks(lib, 48, 64, k) for k in (64, 128, 256, 512, 8192)] == [1, 2, 4, 8, 128]
    m, n, k = 48, 64, 512
    x, w, b = _lin_inputs(m, n, k, seed=5)
    need = lib.gnbv_linear_workspace_bytes(m, n, k)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    out, buf = _out(m, n)
    err = lib.gnbv_linear_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), m, n, k, 1, out.data_ptr(), ws.data_ptr(), need - 1, _stream())
    assert err != 0
    _untouched({"out": out}, {"out": buf})


def test_linear_forward_refusals():
    """N = 32, K = 6, M = 0, a pointer 4 bytes off and a NULL for each pointer: a nonzero return code, the output untouched."""
    lib = _lib.load()
    m, n, k = 48, 64, 72
    x, w, b = (_padded(t) for t in _lin_inputs(m, n, k, seed=6))
    ws = torch.full((lib.gnbv_linear_workspace_bytes(m, n, k) + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    out, buf = _out(m, n)
    good = {"x": x.data_ptr(), "w": w.data_ptr(), "bias": b.data_ptr(), "M": m, "N": n, "K": k, "relu": 1, "out": out.data_ptr(),
            "ws": ws.data_ptr(), "ws_bytes": ws.numel() - 256}
    order = list(good)
    cases = [("N=32", {"N": 32}), ("K=6", {"K": 6}), ("M=0", {"M": 0})]
    for name in ("x", "w", "bias", "out", "ws"):
        cases.append((f"{name}+4", {name: good[name] + 4}))
        cases.append((f"{name}=NULL", {name: None}))
    for what, over in cases:
        args = dict(good, **over)
        assert lib.gnbv_linear_forward(*[args[kk] for kk in order], _stream()) != 0, what
        _untouched({"out": out}, {"out": buf})
    _lib.check(lib.gnbv_linear_forward(*[good[kk] for kk in order], _stream()), "gnbv_linear_forward")
    torch.cuda.synchronize()
    _check_written("linear_forward", out, buf)


# =================================================================================================================================
# 3. gnbv_pose_encode
# =================================================================================================================================
# (batch, n_pose, row_stride, rows of the base when gathered through int64 `rows`, else None)
POSE_CASES = [(256, 100, 600 + 8000, None),  # the 20^3 observation row
              (128, 100, 4699, None),  # a stride that is not a multiple of 4: rows are not 16-byte aligned
              (128, 100, 4699, 300),  # int64 rows drawn with repeats from a 300-row base
              (1, 1, 6, None), (7, 3, 18, None), (5, 100, 600, 300)]
POSE_IDS = ["b{}_p{}_s{}_{}".format(b, p, s, "rows" if r else "dense") for b, p, s, r in POSE_CASES]
POSE_TOL = 4.0  # units of 2^-24, absolute


def _pose_base(batch, n_pose, row_stride, base_rows, seed):
    """(base, rows or None): pose values uniform in [-16, 16], the last pose of a history of 3 or more uniform in [-1000, 1000], and
    in every row exact 0, +-pi/2, +-pi (as fp32), 1e-30 and -0.0; columns past 6 n_pose and rows that `rows` does not name are NaN."""
    gen = torch.Generator().manual_seed(seed)
    nrow, cols = base_rows or batch, 6 * n_pose
    v = torch.rand(nrow, cols, generator=gen) * 32.0 - 16.0
    if n_pose >= 3:
        v[:, cols - 6:] = torch.rand(nrow, 6, generator=gen) * 2000.0 - 1000.0
    special = torch.tensor([0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi, 1e-30, -0.0, 0.0], dtype=torch.float32)
    cnt = min(len(special), cols)
    for r in range(nrow):
        at = ((5 * r) % cols + torch.arange(cnt)) % cols
        v[r, at] = special[(r + torch.arange(cnt)) % len(special)]
    base = torch.full((nrow, row_stride), float("nan"))
    base[:, :cols] = v
    rows = None
    if base_rows:
        rows = torch.randint(0, nrow, (batch,), generator=gen, dtype=torch.int64)
        rows[batch - 1] = rows[0]  # (a repeat in any case)
        unnamed = torch.ones(nrow, dtype=torch.bool)
        unnamed[rows] = False
        assert bool(unnamed.any())
        base[unnamed] = float("nan")
    return base.to(DEV), (rows.to(DEV) if rows is not None else None)


@pytest.mark.parametrize("batch,n_pose,row_stride,base_rows", POSE_CASES, ids=POSE_IDS)
def test_pose_encode_vs_fp64(batch, n_pose, row_stride, base_rows):
    """The reference's Hybrid_Encoder.positional_encoding in fp64: pts = x[..., None] * [1, 2] flattened, cat(sin, cos), per pose of 6
    -- output column 24 p + i is sin and 24 p + 12 + i is cos of x[6 p + i // 2] * (1 + i % 2).  The products are exact in fp32, so the
    only error is the device's sinf / cosf: 4 * 2^-24 absolute per element (torch's own fp32 sin / cos on the CPU are within
    0.60 * 2^-24 of fp64 over these ranges; GPU math libraries commonly specify 1 to 2 ulp; the consumer is a linear layer, which
    sees absolute error).  sin(0) == 0 and cos(0) == 1 exactly.
    Observed on an MI355X: at most 1.134 * 2^-24 (cos of -3.9036350250244141), 0.76 to 1.12 in the other cases; printed per case."""
    lib = _lib.load()
    base, rows = _pose_base(batch, n_pose, row_stride, base_rows, seed=batch * 3 + n_pose + row_stride)
    out, buf = _out(batch, 24 * n_pose)
    _lib.check(lib.gnbv_pose_encode(base.data_ptr(), _lib.ptr(rows), row_stride, batch, n_pose, out.data_ptr(), _stream()), "gnbv_pose_encode")
    torch.cuda.synchronize()
    _check_written("pose_encode", out, buf)
    x = (base if rows is None else base[rows])[:, :6 * n_pose].double().view(batch, n_pose, 6)
    assert bool(torch.isfinite(x).all())
    pts = (x[..., None] * torch.tensor([1.0, 2.0], dtype=torch.float64, device=DEV)).reshape(batch, n_pose, 12)
    want = torch.cat((torch.sin(pts), torch.cos(pts)), -1).reshape(batch, 24 * n_pose)
    err = (out.double() - want).abs() / U
    worst = int(err.argmax())
    arg = float(torch.cat((pts, pts), -1).reshape(-1)[worst])
    print(f"[pose] b{batch} p{n_pose} stride {row_stride} {'rows' if base_rows else 'dense'}: max err {float(err.max()):.3f} x 2^-24 "
          f"({'sin' if (worst % 24) < 12 else 'cos'} of {arg!r})")
    assert float(err.max()) <= POSE_TOL, (float(err.max()), arg)
    got = out.view(batch, n_pose, 24)
    zero = pts == 0
    assert int(zero.sum()) >= 2
    assert bool((got[..., :12][zero] == 0).all()) and bool((got[..., 12:][zero] == 1).all())
    out2, _ = _out(batch, 24 * n_pose)
    _lib.check(lib.gnbv_pose_encode(base.data_ptr(), _lib.ptr(rows), row_stride, batch, n_pose, out2.data_ptr(), _stream()), "gnbv_pose_encode")
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


def test_pose_encode_refusals():
    """row_stride < 6 n_pose, batch = 0, n_pose = 0, a NULL base or output: a nonzero return code, the output untouched (`rows` may be NULL)."""
    lib = _lib.load()
    batch, n_pose, stride = 7, 3, 18
    base, _ = _pose_base(batch, n_pose, stride, None, seed=9)
    out, buf = _out(batch, 24 * n_pose)
    good = {"base": base.data_ptr(), "rows": None, "row_stride": stride, "batch": batch, "n_pose": n_pose, "out": out.data_ptr()}
    order = list(good)
    for what, over in [("stride 17", {"row_stride": 17}), ("batch 0", {"batch": 0}), ("n_pose 0", {"n_pose": 0}), ("base NULL", {"base": None}),
                       ("out NULL", {"out": None})]:
        args = dict(good, **over)
        assert lib.gnbv_pose_encode(*[args[kk] for kk in order], _stream()) != 0, what
        _untouched({"out": out}, {"out": buf})
