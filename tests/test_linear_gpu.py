"""GPU: the fc layers' hand-written split-f16 backward (csrc/linear.hip: gnbv_linear_bwd_prep / _dx / _dw / _dw_sq) and the
BatchNorm-fold entry points (gnbv_linear_forward_fold / gnbv_linear_bwd_dw_fold), called through the C ABI and compared with fp64
torch on the GPU; and linear_relu's backward modes (write-through, deferred dW, sum(dW^2) partials), which must agree bit for bit.

Error model of a split product C = A B (A row-scaled by a power of two per row, B scaled by `bscale`; both split into f16 hi + lo):
    |err[i, k]| <= c (|A| |B|)[i, k] + 2^-25 / bscale (|A| 1)[i] + 2^-37 amax_i (1 |B|)[k]
-- fp32 round-off of the products and sums, then the absolute resolution of the two f16 splits (lo's half ulp at f16's smallest
subnormal).  Every case prints its largest err / bound ratio."""
import math

import pytest
import torch

from gennbv_amd import _lib
from tests.abi_check import DEV, SENTINEL, TAIL, _check_written, _out, _ratio, _report, _stream

pytestmark = pytest.mark.gpu
C_REL = 1e-6
X_SCALE, W_SCALE = 2.0 ** 6, 2.0 ** 12  # (kLinXScale, kLinWScale)

# (M, N, K): the real layers (fc_grid at 64^3 / 20^3, the pose branch, output_layer_rgb), then M in {16, 48, 112} (dx runs 1, 3 or 7
# of its 8 row tiles, dW pads its contraction), N in {16, 48, 208} (dW runs a partial set of its 16 row tiles, dx pads its
# contraction), K in {64, 68, 100, 1000} (a partial last 64-column slab, clamped staging columns)
SHAPES = [(128, 256, 256), (128, 256, 2400), (128, 256, 1024), (128, 256, 4096), (128, 256, 54000),
          (16, 256, 1000), (48, 128, 68), (112, 208, 100), (128, 16, 64), (128, 48, 1000), (16, 16, 64), (48, 208, 4096),
          (112, 48, 68), (128, 208, 100)]
IDS = [f"{m}x{n}x{k}" for m, n, k in SHAPES]


def _inputs(m, n, k, seed):
    """out: a ReLU output with ~40 % exact zeros; d_out: normal noise; W: a trained layer's range; x: activations in [1e-3, 10]."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    out = torch.relu(torch.randn(m, n, generator=gen, device=DEV) + 0.25)
    d_out = torch.randn(m, n, generator=gen, device=DEV)
    w = torch.randn(n, k, generator=gen, device=DEV) / math.sqrt(k)
    x = 10.0 ** (torch.rand(m, k, generator=gen, device=DEV) * 4.0 - 3.0)
    return d_out, out, w, x


def _bwd(d_out, out, w, x):
    """prep + dx + dw + dw_sq through the C ABI on fresh NaN-prefilled outputs (the workspace too: every f16 the products read must
    have been written by prep).  Checks that every output element was written and nothing past it."""
    lib = _lib.load()
    m, n = d_out.shape
    k = w.shape[1]
    ws = torch.full((lib.gnbv_linear_bwd_workspace_bytes(m, n, k),), 0xFF, dtype=torch.uint8, device=DEV)
    parts = int(lib.gnbv_linear_bwd_dw_sq_parts(k))
    assert parts == (k + 63) // 64
    r, bufs = {}, {}
    for name, shape, dt in (("db", (n,), torch.float32), ("dx", (m, k), torch.float32), ("dw", (n, k), torch.float32),
                            ("dw_sq", (n, k), torch.float32), ("sq", (parts,), torch.float64)):
        r[name], bufs[name] = _out(*shape, dtype=dt)
    st = _stream()
    _lib.check(lib.gnbv_linear_bwd_prep(d_out.data_ptr(), out.data_ptr(), m, n, r["db"].data_ptr(), ws.data_ptr(), ws.numel(), st),
               "gnbv_linear_bwd_prep")
    _lib.check(lib.gnbv_linear_bwd_dx(ws.data_ptr(), w.data_ptr(), m, n, k, r["dx"].data_ptr(), st), "gnbv_linear_bwd_dx")
    _lib.check(lib.gnbv_linear_bwd_dw(ws.data_ptr(), x.data_ptr(), m, n, k, r["dw"].data_ptr(), st), "gnbv_linear_bwd_dw")
    _lib.check(lib.gnbv_linear_bwd_dw_sq(ws.data_ptr(), x.data_ptr(), m, n, k, r["dw_sq"].data_ptr(), r["sq"].data_ptr(), st),
               "gnbv_linear_bwd_dw_sq")
    torch.cuda.synchronize()
    for name in r:
        _check_written(name, r[name], bufs[name])
    return r


def _bound(a, b, bscale, floor=0.0):
    """The error model above for C = a b (fp64 operands), plus an absolute `floor` per element."""
    aa, ba = a.abs(), b.abs()
    amax = aa.amax(1, keepdim=True)
    return (C_REL * (aa @ ba) + (2.0 ** -25 / bscale) * aa.sum(1, keepdim=True) + 2.0 ** -37 * amax * ba.sum(0, keepdim=True)) + floor


def _check_vs_fp64(what, r, d_out, out, w, x, floor=0.0):
    """dx, dW, db of g = d_out (out > 0) against fp64 within the error model; `floor` is an absolute allowance per unit of
    contraction length (see test_bwd_tiny_gradient_rows)."""
    g = d_out.double() * (out > 0)
    wd, xd = w.double(), x.double()
    m, n = g.shape
    fx = floor * (n + wd.abs().sum(0, keepdim=True)) if floor else 0.0
    fw = floor * (m + xd.abs().sum(0, keepdim=True)) if floor else 0.0
    ratios = {"dx": _ratio(r["dx"], g @ wd, _bound(g, wd, W_SCALE, fx)),
              "dw": _ratio(r["dw"], g.t() @ xd, _bound(g.t(), xd, X_SCALE, fw)),
              "db": _ratio(r["db"], g.sum(0), 1e-6 * g.abs().sum(0) + (floor * m if floor else 0.0))}
    line = _report(what, ratios)
    assert max(ratios.values()) <= 1.0, line


@pytest.mark.parametrize("m,n,k", SHAPES, ids=IDS)
def test_bwd_vs_fp64(m, n, k):
    """prep + dx + dw + db against fp64 g W, g^T x, sum_m g, elementwise within the error model."""
    d_out, out, w, x = _inputs(m, n, k, seed=m * 7 + n * 131 + k)
    r = _bwd(d_out, out, w, x)
    _check_vs_fp64(f"bwd {m}x{n}x{k}", r, d_out, out, w, x)


@pytest.mark.parametrize("m,n,k", SHAPES, ids=IDS)
def test_dw_sq_partials_match_the_returned_dw(m, n, k):
    """gnbv_linear_bwd_dw_sq: the same dW bits as gnbv_linear_bwd_dw, and gnbv_linear_bwd_dw_sq_parts(K) fp64 partials (every slot
    written: _bwd) whose sum is sum(dW^2) of that dW in fp64."""
    d_out, out, w, x = _inputs(m, n, k, seed=m * 7 + n * 131 + k + 1)
    r = _bwd(d_out, out, w, x)
    assert torch.equal(r["dw_sq"], r["dw"])
    want = float((r["dw"].double() ** 2).sum())
    got = float(r["sq"].sum())
    assert want > 0 and abs(got - want) <= 1e-12 * want, (got, want)


@pytest.mark.parametrize("m,n,k", SHAPES, ids=IDS)
def test_bwd_pow2_equivariance_is_bit_exact(m, n, k):
    """prep normalises every row to [2^13, 2^14): d_out 2^j must give dx, dW, db 2^j and every sum(dW^2) partial 2^2j, bit for bit."""
    d_out, out, w, x = _inputs(m, n, k, seed=m * 7 + n * 131 + k + 2)
    base = _bwd(d_out, out, w, x)
    for j in (-60, -13, 13, 60):
        for name in ("dx", "dw", "db"):  # (no result is subnormal: a power-of-two scaling of it is exact)
            v = base[name].abs() * 2.0 ** j
            assert bool(((v == 0) | (v >= 2.0 ** -100)).all()), (name, j)
        r = _bwd(d_out * 2.0 ** j, out, w, x)
        for name in ("dx", "dw", "db", "dw_sq"):
            assert torch.equal(r[name], base[name] * 2.0 ** j), (name, j)
        assert torch.equal(r["sq"], base["sq"] * 2.0 ** (2 * j)), j


@pytest.mark.parametrize("m,n,k", SHAPES, ids=IDS)
def test_bwd_tiny_gradient_rows(m, n, k):
    """d_out 2^-118, and some rows / columns down to the smallest normal float: prep's per-row scale must stay finite (it was
    2^(14 - e): +inf below 2^-114, a NaN dx / dW row).  Every output finite and within the error model, plus an absolute 2^-149
    per term of the contraction and per unit of sum |B|: results in the subnormal range, and rows whose scale is capped at 2^126
    split with a coarser absolute resolution."""
    d_out, out, w, x = _inputs(m, n, k, seed=m * 7 + n * 131 + k + 3)
    rs = torch.ones(m, 1, dtype=torch.float64, device=DEV)
    cs = torch.ones(1, n, dtype=torch.float64, device=DEV)
    rs[1], rs[m // 2], rs[m - 1] = 2.0 ** -8, 2.0 ** -4, 2.0 ** -8
    cs[0, 0], cs[0, n // 2], cs[0, n - 1] = 2.0 ** -8, 2.0 ** -5, 2.0 ** -7
    d = (d_out.double() * 2.0 ** -118 * rs * cs).float()
    assert float(d.abs().max()) < 2.0 ** -112 and 0 < float(d[m - 1].abs().max()) < 2.0 ** -122
    r = _bwd(d, out, w, x)
    _check_vs_fp64(f"tiny {m}x{n}x{k}", r, d, out, w, x, floor=2.0 ** -149)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm fold: the operand is relu(scale[c] y + shift[c]), c = column / P
# ---------------------------------------------------------------------------------------------------------------------------------
FOLD = [(512, 2), (512, 16), (1331, 8), (3375, 8), (3375, 16)]  # (P, channels); P = 3375 is odd: channels meet inside quads / trips
FOLD_IDS = [f"P{p}xC{c}" for p, c in FOLD]


def _fold_data(m, p, c, seed, exact):
    """y [m][c p] and per-channel (scale, shift): negative, zero and positive scales; shifts that put some activations exactly on 0.
    exact: y on a 2^-12 grid, scales with at most 11 significant bits and shift = -scale v (v a power of two, planted in y) -- then
    scale y + shift is exact in fp64, so relu of it rounded to fp32 is the kernels' fmaf + max."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    k = c * p
    y = torch.randn(m, k, generator=gen, device=DEV)
    sc = torch.randn(c, generator=gen, device=DEV)
    sh = torch.randn(c, generator=gen, device=DEV) * 0.5
    sc[0], sc[1] = 0.0, -abs(float(sc[1])) - 0.1
    sh[0] = 0.25
    if exact:
        y = torch.round(y * 2 ** 12) / 2 ** 12
        sc = torch.round(sc.clamp(-1.99, 1.99) * 2 ** 10) / 2 ** 10
        v = 2.0 ** torch.randint(-3, 2, (c,), generator=gen, device=DEV).float() * torch.sign(torch.randn(c, generator=gen, device=DEV))
        sh = torch.where(sc != 0, -sc * v, sh)
        plant = torch.rand(m, k, generator=gen, device=DEV) < 0.05
        y = torch.where(plant, v.repeat_interleave(p).view(1, k).expand(m, k), y)
    act = torch.relu(sc.double().repeat_interleave(p) * y.double() + sh.double().repeat_interleave(p)) + 0.0
    return y.contiguous(), sc.contiguous(), sh.contiguous(), act


def _lin_params(n, k, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, k, generator=gen, device=DEV) / math.sqrt(k), torch.randn(n, generator=gen, device=DEV) * 0.1


def _forward(lib, x, w, b, fold=None, flag=None):
    m, k = x.shape
    n = w.shape[0]
    ws = torch.empty(lib.gnbv_linear_workspace_bytes(m, n, k), dtype=torch.uint8, device=DEV)
    out, buf = _out(m, n)
    if fold is None:
        err = lib.gnbv_linear_forward(x.data_ptr(), w.data_ptr(), b.data_ptr(), m, n, k, 1, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    else:
        sc, sh, p = fold
        err = lib.gnbv_linear_forward_fold(x.data_ptr(), sc.data_ptr(), sh.data_ptr(), p, _lib.ptr(flag), w.data_ptr(), b.data_ptr(), m, n, k, 1,
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    return err, out, buf


def _dw(lib, d_out, relu_out, x, fold=None):
    """prep, then dW (folded or not) on NaN-prefilled outputs."""
    m, n = d_out.shape
    k = x.shape[1]
    ws = torch.empty(lib.gnbv_linear_bwd_workspace_bytes(m, n, k), dtype=torch.uint8, device=DEV)
    dw, buf = _out(n, k)
    _lib.check(lib.gnbv_linear_bwd_prep(d_out.data_ptr(), relu_out.data_ptr(), m, n, None, ws.data_ptr(), ws.numel(), _stream()), "gnbv_linear_bwd_prep")
    if fold is None:
        err = lib.gnbv_linear_bwd_dw(ws.data_ptr(), x.data_ptr(), m, n, k, dw.data_ptr(), _stream())
    else:
        sc, sh, p = fold
        err = lib.gnbv_linear_bwd_dw_fold(ws.data_ptr(), x.data_ptr(), sc.data_ptr(), sh.data_ptr(), p, m, n, k, dw.data_ptr(), None, _stream())
    torch.cuda.synchronize()
    return err, dw, buf


@pytest.mark.parametrize("p,c", FOLD, ids=FOLD_IDS)
def test_fold_is_bit_identical_to_materialised_activations(p, c):
    """On exactly representable (scale, shift, y): gnbv_linear_forward_fold == gnbv_linear_forward on relu(scale y + shift) for
    M in {16, 128, 130, 256} (above 128 rows the 8-wave kernel), gnbv_linear_bwd_dw_fold == gnbv_linear_bwd_dw for M in {16, 128, 256}."""
    lib = _lib.load()
    n, k = 256, c * p
    w, b = _lin_params(n, k, seed=p + c)
    for m in (16, 128, 130, 256):
        assert lib.gnbv_linear_fold_ok(m, n, k, p) == 1
        y, sc, sh, act = _fold_data(m, p, c, seed=p * 3 + c + m, exact=True)
        assert float((act == 0).double().mean()) > 0.1 and float(act.max()) < 1000
        xm = act.float()
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        e1, o1, b1 = _forward(lib, y, w, b, fold=(sc, sh, p), flag=flag)
        e2, o2, b2 = _forward(lib, xm, w, b)
        assert e1 == 0 and e2 == 0
        _check_written("forward_fold", o1, b1)
        _check_written("forward", o2, b2)
        assert torch.equal(o1, o2), m
        assert int(flag.item()) == 0
        if m % 16:
            continue
        gen = torch.Generator(device=DEV).manual_seed(m + k)
        d_out = torch.randn(m, n, generator=gen, device=DEV)
        relu_out = torch.relu(torch.randn(m, n, generator=gen, device=DEV) + 0.25)
        e1, d1, b1 = _dw(lib, d_out, relu_out, y, fold=(sc, sh, p))
        e2, d2, b2 = _dw(lib, d_out, relu_out, xm)
        assert e1 == 0 and e2 == 0
        _check_written("bwd_dw_fold", d1, b1)
        _check_written("bwd_dw", d2, b2)
        assert torch.equal(d1, d2), m


@pytest.mark.parametrize("p,c", FOLD, ids=FOLD_IDS)
def test_fold_vs_fp64(p, c):
    """Arbitrary fp32 scales, shifts and y: the folded forward and weight gradient against fp64 relu(scale y + shift) within the
    error model (forward: x split at 2^6, W at 2^12, no row scaling; the fp32 rounding of an activation is inside c)."""
    lib = _lib.load()
    n, k = 256, c * p
    w, b = _lin_params(n, k, seed=p + c + 1)
    ratios = {}
    for m in (16, 128, 256):
        y, sc, sh, act = _fold_data(m, p, c, seed=p * 5 + c + m, exact=False)
        e, o, buf = _forward(lib, y, w, b, fold=(sc, sh, p))
        assert e == 0
        _check_written("forward_fold", o, buf)
        wt = w.double().t()
        pre = act @ wt + b.double()
        bound = (C_REL * (act @ wt.abs() + b.double().abs()) + (2.0 ** -25 / W_SCALE) * act.sum(1, keepdim=True)
                 + (2.0 ** -25 / X_SCALE) * wt.abs().sum(0, keepdim=True))
        ratios[f"fwd M{m}"] = _ratio(o, torch.relu(pre), bound)
        gen = torch.Generator(device=DEV).manual_seed(m + k + 1)
        d_out = torch.randn(m, n, generator=gen, device=DEV)
        relu_out = torch.relu(torch.randn(m, n, generator=gen, device=DEV) + 0.25)
        e, dw, buf = _dw(lib, d_out, relu_out, y, fold=(sc, sh, p))
        assert e == 0
        _check_written("bwd_dw_fold", dw, buf)
        g = d_out.double() * (relu_out > 0)
        ratios[f"dw M{m}"] = _ratio(dw, g.t() @ act, _bound(g.t(), act, X_SCALE))
    line = _report(f"fold P{p} C{c}", ratios)
    assert max(ratios.values()) <= 1.0, line


@pytest.mark.parametrize("top,flag_want", [(1000.5, 4), (999.0, 0)])
def test_fold_range_flag(top, flag_want):
    """Bit 4 of *range_flag once an operand passes 1000 (the x split clamps at 1015): 1000.5 sets it, a largest operand of 999 does not."""
    lib = _lib.load()
    m, n, p, c = 16, 256, 512, 2
    k = p * c
    w, b = _lin_params(n, k, seed=11)
    gen = torch.Generator(device=DEV).manual_seed(12)
    y = torch.rand(m, k, generator=gen, device=DEV) * 900.0
    y[5, 700] = top
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    e, o, buf = _forward(lib, y, w, b, fold=(sc, sh, p), flag=flag)
    assert e == 0
    _check_written("forward_fold", o, buf)
    assert int(flag.item()) == flag_want


@pytest.mark.parametrize("entry", ["forward_fold", "bwd_dw_fold"])
@pytest.mark.parametrize("p,k", [(511, 511 * 8), (512, 1000)])
def test_fold_entry_points_refuse_what_fold_ok_refuses(entry, p, k):
    """Where gnbv_linear_fold_ok says no (P < 512, K % P != 0) both entry points return an error and launch nothing."""
    lib = _lib.load()
    m, n = 16, 256
    assert lib.gnbv_linear_fold_ok(m, n, k, p) == 0
    c = (k + p - 1) // p
    w, b = _lin_params(n, k, seed=13)
    y = torch.rand(m, k, device=DEV)
    sc, sh = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    if entry == "forward_fold":
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        e, o, buf = _forward(lib, y, w, b, fold=(sc, sh, p), flag=flag)
        assert int(flag.item()) == 0
    else:
        e, o, buf = _dw(lib, torch.randn(m, n, device=DEV), torch.rand(m, n, device=DEV), y, fold=(sc, sh, p))
    assert e != 0
    assert bool(torch.isnan(o).all()) and bool((buf[o.numel():] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# linear_relu's backward modes
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = ["write_through", "write_through_sq", "deferred", "write_through_unaligned", "deferred_unaligned"]


def _linear_relu_grads(lin, x, d, mode):
    """One forward + backward of linear_relu in `mode` ("plain": autograd's own .grad; otherwise write-through into a flat NaN-filled
    gradient buffer as FlatAdam lays it out, the weight's slice 16-byte aligned or 1 float past a boundary)."""
    from gennbv_amd.ops import encoder_ops as eo
    n, k = lin.weight.shape
    lin._dw_sq_partial, lin._async_wgrad, lin._defer_wgrad = None, False, False
    flat = None
    if mode == "plain":
        lin._grad_write_through = False
        lin.weight.grad = lin.bias.grad = None
    else:
        off = 1 if mode.endswith("unaligned") else 0
        flat = torch.full((off + n * k + n + TAIL,), float("nan"), device=DEV)
        flat[off + n * k + n:] = SENTINEL
        lin.weight.grad = flat[off:off + n * k].view(n, k)
        lin.bias.grad = flat[off + n * k:off + n * k + n]
        assert (lin.weight.grad.data_ptr() % 16 == 4) == bool(off)
        lin._grad_write_through = True
        if mode.endswith("_sq"):
            lin._dw_sq_partial = torch.full((int(_lib.load().gnbv_linear_bwd_dw_sq_parts(k)),), float("nan"), dtype=torch.float64, device=DEV)
        if mode.startswith("deferred"):
            lin._async_wgrad = lin._defer_wgrad = True
    xx = x.clone().requires_grad_(True)
    out = eo.linear_relu(xx, lin)
    out.backward(d)
    lin._defer_wgrad = False
    eo.join_async_wgrads(torch.device(DEV))
    torch.cuda.synchronize()
    if flat is not None:
        assert bool((flat[flat.numel() - TAIL:] == SENTINEL).all())
    res = (out.detach().clone(), xx.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone(), lin._dw_sq_partial)
    lin._grad_write_through, lin._dw_sq_partial, lin._async_wgrad = False, None, False
    return res


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [54000, 2400])
def test_linear_relu_backward_modes_agree_bitwise(k, mode, monkeypatch):
    """(128, 256, K) through linear_relu: write-through, write-through + sum(dW^2) partials, the dW launch deferred to the second
    stream (+ join_async_wgrads), and write-through into a gradient slice that is not 16-byte aligned must all give the dx, dW and db
    bits of the plain backward -- the hand-written kernels in every mode (an unaligned target goes through a temporary)."""
    monkeypatch.setenv("GENNBV_CONV_SPLIT", "1")
    m, n = 128, 256
    gen = torch.Generator(device=DEV).manual_seed(k)
    lin = torch.nn.Linear(k, n).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, generator=gen, device=DEV) / math.sqrt(k))
        lin.bias.copy_(torch.randn(n, generator=gen, device=DEV) * 0.1)
    x = 10.0 ** (torch.rand(m, k, generator=gen, device=DEV) * 4.0 - 3.0) * (torch.rand(m, k, generator=gen, device=DEV) < 0.6)
    d = torch.randn(m, n, generator=gen, device=DEV)
    ref = _linear_relu_grads(lin, x, d, "plain")
    got = _linear_relu_grads(lin, x, d, mode)
    for name, a, b in zip(("out", "dx", "dW", "db"), ref[:4], got[:4]):
        assert bool(torch.isfinite(b).all()), name
        assert torch.equal(a, b), name
    if mode.endswith("_sq"):
        want = float((got[2].double() ** 2).sum())
        assert abs(float(got[4].sum()) - want) <= 1e-12 * want
