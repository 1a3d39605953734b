"""GPU: the encoder grid branch (csrc/encoder.hip, conv_split.h, conv_splitx.h) called through its C ABI --
gnbv_encoder_grid_forward / _backward, gnbv_encoder_eval_prepare, gnbv_input_autocorr -- on every kernel path the dispatcher
selects, against a layered fp64 reference (tests/encoder_abi_ref.py).

Buffers.  Every output and scratch buffer is NaN-prefilled and followed by a sentinel tail; the workspace is exactly
gnbv_encoder_workspace_bytes long, 0xFF-filled, with a tail of its own.  Each documented output must be written in full and
finite, no tail may change, and the read-only inputs must be bit-unchanged.  The same call on a zero-filled workspace and zero-filled
outputs / scratch must give bit-identical results (no read of memory this call did not write).

Layered reference.  Each stage is recomputed in fp64 from the kernel's own output of the stage before (y1 and bn_state for conv2,
y2 and bn_state for the BN-2 backward, dy2 for the conv2 gradients, ...), so each contraction is checked on its own and the ReLU
masks agree by construction.  The fused inference kernel stores no y1: there conv2 is fed by the exact conv1, and the ReLU's
Lipschitz bound carries conv1's error bound |scale1| e(y1) into conv2's.

Error model (elementwise, fp64; u = 2^-24, c = C_REL):
* a convolution / weight gradient / data gradient computed in fp32: c (|W| (*) |x| + |b|), the same contraction on magnitudes;
* where a split-f16 kernel runs (conv_split.h), plus the absolute resolution of each operand's hi + lo halves under its
  power-of-two scaling, 2^-25 / scale: kZScale = 2^8 for z1, kWScale = 2^10 for W2, gs = 2^(14 - e) (max |dy2| = f 2^e) for dy2,
  and in the fused data gradient the layer-1 gradient's 2^-24 max_ci sum |W2| / gs: e.g. 2^-25/kWScale (1 (*) |z1|) for conv2;
* BatchNorm statistics: C_STAT E|y| for the mean and C_STAT E[y^2] for the variance (one pass over fp32 partial sums: on a batch
  of equal values the round-off of every partial has the same sign), propagated by interval into rstd (+ 2^-22 rstd), scale
  and shift (+ 2^-23 of their terms); the running statistics add 2^-22 of their terms;
* the BN backward means S1 = sum g, S2 = sum g xhat carry c of their magnitude sums plus the propagated errors of g and xhat; the
  conv1 weight gradient carries |scale1| (e(g) + e(S1)/N + |xhat| e(S2)/N + e(xhat) |S2|/N) and c |scale1| (|g| + |S1|/N +
  |xhat| |S2|/N) through |x|;
* features = relu(fma(scale2, y2, shift2)): within one fp32 ulp.
Every case prints its worst err / bound per output and asserts it is <= 1."""
import ctypes as C
import math
import zlib

import pytest
import torch

from gennbv_amd import _lib
from tests import encoder_abi_ref as R
from tests.encoder_abi_cases import CASES, K, KNOBS, _paths

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_REL = 2e-6
C_STAT = 4e-6  # (BatchNorm statistics: one-pass sums of fp32 partials, whose round-off is systematic when the values are all equal)
U = 2.0 ** -24
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))
MOM32 = float(torch.tensor(0.1, dtype=torch.float32))
Z_SCALE, W_SCALE = 2.0 ** 8, 2.0 ** 10  # (conv_split.h: kZScale, kWScale)
TAIL, SENTINEL = 64, 1234.5
WS_TAIL = 256
STATE_DIM = 600  # (the grid slice of an observation row starts here: policy_util.obs_dim)


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _buf(n, dtype=torch.float32, fill=float("nan")):
    """(view of n elements, whole buffer): prefilled with `fill`, followed by TAIL sentinel elements."""
    b = torch.full((n + TAIL,), fill, dtype=dtype, device=DEV)
    b[n:] = SENTINEL if dtype.is_floating_point else -7
    return b[:n], b


def _tail_ok(name, view, buf):
    n = view.numel()
    s = SENTINEL if buf.dtype.is_floating_point else -7
    assert bool((buf[n:] == s).all()), f"{name}: the {TAIL} elements past the buffer were written"


def _finite(name, t):
    bad = int((~torch.isfinite(t)).sum())
    assert bad == 0, f"{name}: {bad} of {t.numel()} elements not written or not finite"


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.dtype.is_floating_point else torch.equal(a, b)


class Setup:
    """Inputs and parameters of one case (seeded from its id)."""

    def __init__(self, cs, seed):
        g, b = cs["g"], cs["b"]
        gen = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=gen, device=DEV)  # noqa: E731
        nrows = b + 3
        if cs["fill"] == "zeros":
            x = torch.zeros(nrows, g ** 3, device=DEV)
        elif cs["fill"] == "ones":
            x = torch.ones(nrows, g ** 3, device=DEV)
        else:
            x = (torch.randint(-1, 2, (nrows, g ** 3), generator=gen, device=DEV)
                 * (torch.rand(nrows, g ** 3, generator=gen, device=DEV) < 0.4)).float()
        rows = list(range(nrows - 1, -1, -1))[:b]  # reversed order ...
        if b >= 3:
            rows[2] = rows[0]  # ... with a repeat
        self.rows = torch.tensor(rows, dtype=torch.int64, device=DEV)
        self.x = x
        # fp32 observation rows [state | grid | rest] at the policy's row stride (+ 1 column: the grid slice 4 bytes off alignment)
        off = STATE_DIM + (1 if cs["inp"] == "unaligned" else 0)
        d = STATE_DIM + g ** 3 + 8192 + (1 if cs["inp"] == "unaligned" else 0)
        self.base = rn(nrows, d)
        self.base[:, off:off + g ** 3] = x
        self.obs_off, self.row_stride = off, d
        self.obs_ptr = None if cs["inp"] == "compact" else self.base.data_ptr() + 4 * off
        # int8 rows: stride a multiple of 16 past G^3, the bytes behind a row's grid hold 85 (never read as data)
        self.i8 = None
        if cs["inp"] in ("i8", "compact"):
            s = (g ** 3 + 31) // 16 * 16
            self.i8 = torch.full((nrows, s), 85, dtype=torch.int8, device=DEV)
            self.i8[:, :g ** 3] = x.to(torch.int8)
        self.ac = self.ac_total = None
        self.exact_ac = None
        if cs["ac"]:
            self.exact_ac = R.autocorr_rows(x.view(nrows, g, g, g))
            lib = _lib.load()
            stride = R.AC_ROW + 16
            acb = torch.full((nrows * stride + TAIL,), -7, dtype=torch.int32, device=DEV)
            self.ac = acb[:nrows * stride].view(nrows, stride)
            _lib.check(lib.gnbv_input_autocorr(self.i8.data_ptr(), self.i8.stride(0), nrows, g, self.ac.data_ptr(), stride, _stream()),
                       "gnbv_input_autocorr")
            torch.cuda.synchronize()
            assert torch.equal(self.ac[:, :R.AC_ROW].long(), self.exact_ac), "gnbv_input_autocorr rows differ from the exact ones"
            assert bool((self.ac[:, R.AC_ROW:] == -7).all()) and bool((acb[nrows * stride:] == -7).all()), "autocorr: padding written"
            if cs["ac"] == "total":
                self.ac_total = self.exact_ac[self.rows].sum(0).to(torch.int32).contiguous()
        # parameters (torch layouts), running statistics with sentinel tails
        self.w1 = rn(16, 1, 3, 3, 3) * 0.25
        self.b1 = rn(16) * 0.1
        self.g1 = 1.0 + 0.2 * rn(16)
        self.be1 = 0.2 * rn(16)
        self.w2 = rn(16, 16, 3, 3, 3) * (1.5 / math.sqrt(432))
        self.b2 = rn(16) * 0.1
        self.g2 = 1.0 + 0.2 * rn(16)
        self.be2 = 0.2 * rn(16)
        if cs["big"]:  # just inside the split kernels' operand ranges: |W2| < 63.4, z1 = relu(bn1(y1)) <= 253.9
            self.w2[3, 5, 1, 1, 1], self.w2[7, 0, 2, 0, 1] = 62.5, -62.0
            self.g1[2], self.be1[2] = 36.0, 20.0
        self.rm1, self.rm1_buf = _buf(16, fill=0.0)
        self.rv1, self.rv1_buf = _buf(16, fill=0.0)
        self.rm2, self.rm2_buf = _buf(16, fill=0.0)
        self.rv2, self.rv2_buf = _buf(16, fill=0.0)
        self.rm1.copy_(0.1 * rn(16))
        self.rv1.copy_(0.5 + torch.rand(16, generator=gen, device=DEV))
        self.rm2.copy_(0.1 * rn(16))
        self.rv2.copy_(0.5 + torch.rand(16, generator=gen, device=DEV))
        self.nbt1, self.nbt1_buf = _buf(1, torch.int64, 5)
        self.nbt2, self.nbt2_buf = _buf(1, torch.int64, 5)
        self.flag, self.flag_buf = _buf(1, torch.int32, 0)
        self.skip = torch.tensor([1 if cs["skip"] else 0], dtype=torch.int32, device=DEV)
        self.running0 = [t.clone() for t in (self.rm1, self.rv1, self.nbt1, self.rm2, self.rv2, self.nbt2)]
        self.readonly = {"obs rows": self.base, "rows": self.rows, "w1": self.w1, "b1": self.b1, "bn1_w": self.g1, "bn1_b": self.be1,
                         "w2": self.w2, "b2": self.b2, "bn2_w": self.g2, "bn2_b": self.be2, "skip_flag": self.skip}
        if self.i8 is not None:
            self.readonly["int8 rows"] = self.i8
        if self.ac is not None:
            self.readonly["autocorr rows"] = acb
        if self.ac_total is not None:
            self.readonly["autocorr_total"] = self.ac_total
        self.readonly0 = {k: v.clone() for k, v in self.readonly.items()}

    def restore_running(self):
        for t, t0 in zip((self.rm1, self.rv1, self.nbt1, self.rm2, self.rv2, self.nbt2), self.running0):
            t.copy_(t0)
        self.flag.zero_()

    def params(self, cs, eval_prepared=0):
        p = _lib.GnbvEncoderParams()
        p.w1, p.b1, p.bn1_w, p.bn1_b = self.w1.data_ptr(), self.b1.data_ptr(), self.g1.data_ptr(), self.be1.data_ptr()
        p.bn1_rm, p.bn1_rv, p.bn1_nbt = self.rm1.data_ptr(), self.rv1.data_ptr(), self.nbt1.data_ptr()
        p.w2, p.b2, p.bn2_w, p.bn2_b = self.w2.data_ptr(), self.b2.data_ptr(), self.g2.data_ptr(), self.be2.data_ptr()
        p.bn2_rm, p.bn2_rv, p.bn2_nbt = self.rm2.data_ptr(), self.rv2.data_ptr(), self.nbt2.data_ptr()
        p.eps, p.momentum = 1e-5, 0.1
        p.grid_i8 = None if self.i8 is None else self.i8.data_ptr()
        p.grid_i8_row_stride = 0 if self.i8 is None else self.i8.stride(0)
        p.autocorr = None if self.ac is None else self.ac.data_ptr()
        p.autocorr_row_stride = 0 if self.ac is None else self.ac.stride(0)
        p.world = 0
        p.autocorr_total = None if self.ac_total is None else self.ac_total.data_ptr()
        p.force_fp32 = int(cs["force"])
        p.range_flag = self.flag.data_ptr()
        p.eval_prepared = eval_prepared
        return p


def _run(cs, st, fill):
    """One forward (+ backward when training) through the C ABI on buffers prefilled with `fill` (NaN: outputs, 0xFF: workspace;
    or 0 for both).  Returns every buffer."""
    lib = _lib.load()
    g, b = cs["g"], cs["b"]
    o2 = R.out_size(R.out_size(g))
    n1, n2 = lib.gnbv_encoder_y1_elems(b, g), b * 16 * o2 ** 3
    nan = fill == "nan"
    v = float("nan") if nan else 0.0
    out = {}
    for name, n in (("y1", n1), ("y2", n2), ("bn_state", R.BN_STATE), ("features", n2), ("dy2", n2), ("dz1", n1)):
        out[name] = _buf(n, fill=v)
    for name, t in (("dw1", st.w1), ("db1", st.b1), ("dg1", st.g1), ("dbe1", st.be1), ("dw2", st.w2), ("db2", st.b2), ("dg2", st.g2),
                    ("dbe2", st.be2)):
        out[name] = _buf(t.numel(), fill=v)
    wsn = lib.gnbv_encoder_workspace_bytes(b, g)
    ws = torch.full((wsn + WS_TAIL,), 0xFF if nan else 0, dtype=torch.uint8, device=DEV)
    ws[wsn:] = 0xA5
    assert ws.data_ptr() % 256 == 0
    out["ws"] = (ws[:wsn], ws)
    p = st.params(cs, eval_prepared=cs["prep"])
    s = _stream()
    feats = out["features"][0] if cs["feats"] else None
    if cs["prep"]:
        _lib.check(lib.gnbv_encoder_eval_prepare(b, g, C.byref(p), out["bn_state"][0].data_ptr(), ws.data_ptr(), wsn, s),
                   "gnbv_encoder_eval_prepare")
    _lib.check(lib.gnbv_encoder_grid_forward(st.obs_ptr, st.rows.data_ptr(), st.row_stride, b, g, C.byref(p), int(cs["train"]),
                                             st.skip.data_ptr(), out["y1"][0].data_ptr(), out["y2"][0].data_ptr(),
                                             out["bn_state"][0].data_ptr(), _lib.ptr(feats), ws.data_ptr(), wsn, s),
               "gnbv_encoder_grid_forward")
    if cs["train"]:
        d = torch.zeros(b, n2 // b, device=DEV)
        if cs["dfeat"] == "randn":
            d = torch.randn(b, n2 // b, generator=torch.Generator(device=DEV).manual_seed(7), device=DEV)
        elif cs["dfeat"] == "onehot":
            d[b - 1, (n2 // b) // 3] = 1.0
        out["d_features"] = d
        gs = _lib.GnbvEncoderGrads()
        for name, key in (("w1", "dw1"), ("b1", "db1"), ("bn1_w", "dg1"), ("bn1_b", "dbe1"), ("w2", "dw2"), ("b2", "db2"),
                          ("bn2_w", "dg2"), ("bn2_b", "dbe2")):
            setattr(gs, name, out[key][0].data_ptr())
        _lib.check(lib.gnbv_encoder_grid_backward(st.obs_ptr, st.rows.data_ptr(), st.row_stride, b, g, C.byref(p),
                                                  out["y1"][0].data_ptr(), out["y2"][0].data_ptr(), out["bn_state"][0].data_ptr(),
                                                  d.data_ptr(), out["dy2"][0].data_ptr(), out["dz1"][0].data_ptr(), C.byref(gs),
                                                  ws.data_ptr(), wsn, s), "gnbv_encoder_grid_backward")
    torch.cuda.synchronize()
    return out


def _bn_ref(y, e_rel, gamma, beta, train, rm0, rv0):
    """BatchNorm statistics of y [B, 16, ...] (fp64; train) or the running ones, with their error bounds (module docstring)."""
    if train:
        dims = [0] + list(range(2, y.dim()))
        mean = y.mean(dims)
        var = ((y - mean.view(1, -1, *([1] * (y.dim() - 2)))) ** 2).mean(dims)
        e_mean = e_rel * y.abs().mean(dims)
        e_var = e_rel * (y * y).mean(dims)
    else:
        mean, var = rm0.double(), rv0.double()
        e_mean = e_var = torch.zeros_like(mean)
    rstd = 1.0 / torch.sqrt(var + EPS32)
    # (the kernel's variance lies in [max(var - e_var, 0), var + e_var]: it clamps a negative one-pass variance at 0)
    e_rstd = torch.maximum(1.0 / torch.sqrt((var - e_var).clamp_min(0.0) + EPS32) - rstd, rstd - 1.0 / torch.sqrt(var + e_var + EPS32))
    e_rstd = e_rstd + 2.0 ** -22 * rstd
    scale = gamma.double() * rstd
    e_scale = gamma.double().abs() * e_rstd + 2 * U * scale.abs()
    shift = beta.double() - mean * scale
    e_shift = scale.abs() * e_mean + mean.abs() * e_scale + 2 * U * (beta.double().abs() + (mean * scale).abs())
    return dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, e_mean=e_mean + U * mean.abs(), e_var=e_var,
                e_rstd=e_rstd, e_scale=e_scale, e_shift=e_shift)


def _check_bn(tag, bn_k, ref, ratios):
    for i, k in enumerate(("scale", "shift", "mean", "rstd")):
        ratios[f"{tag}.{k}"] = R.ratio(bn_k[16 * i:16 * i + 16], ref[k], ref["e_" + k])


def _check_running(tag, st, cs, idx, ref, n, ratios):
    rm, rv, nbt = [(st.rm1, st.rv1, st.nbt1), (st.rm2, st.rv2, st.nbt2)][idx]
    rm0, rv0, nbt0 = st.running0[3 * idx:3 * idx + 3]
    if not cs["train"] or cs["skip"]:
        assert _same_bits(rm, rm0) and _same_bits(rv, rv0) and torch.equal(nbt, nbt0), f"{tag}: running statistics changed"
        return
    m = MOM32
    f = n / (n - 1) if n > 1 else 1.0
    want_m = (1 - m) * rm0.double() + m * ref["mean"]
    want_v = (1 - m) * rv0.double() + m * f * ref["var"]
    ratios[f"{tag}.running_mean"] = R.ratio(rm, want_m, m * ref["e_mean"] + 2.0 ** -22 * ((1 - m) * rm0.double().abs() + m * ref["mean"].abs()))
    ratios[f"{tag}.running_var"] = R.ratio(rv, want_v, m * f * ref["e_var"] + 2.0 ** -22 * ((1 - m) * rv0.double().abs() + m * f * ref["var"]))
    assert int(nbt) == int(nbt0) + 1, f"{tag}: num_batches_tracked"


def _check(cs, st, out, pth):
    """Every documented output of one run against the layered fp64 reference; returns {output: worst err / bound}."""
    g, b = cs["g"], cs["b"]
    o1 = R.out_size(g)
    o2 = R.out_size(o1)
    p2 = o2 ** 3
    ratios = {}
    for name, vb in out.items():
        if name not in ("ws", "d_features"):
            _tail_ok(name, *vb)
    ws, wsb = out["ws"]
    assert bool((wsb[ws.numel():] == 0xA5).all()), "workspace: bytes past gnbv_encoder_workspace_bytes were written"
    for k, t in st.readonly.items():
        assert _same_bits(t, st.readonly0[k]), f"read-only input changed: {k}"
    x = st.x[st.rows].double().view(b, 1, g, g, g)
    w1, w2 = st.w1.double(), st.w2.double()
    # ---- conv1 ----
    y1_ex = R.conv(x, w1, st.b1.double())
    e_y1 = C_REL * R.conv(x.abs(), w1.abs(), st.b1.double().abs())
    y1v = out["y1"][0]
    if pth["fused_eval"]:
        assert bool(torch.isnan(y1v).all()) or bool((y1v == 0).all()), "fused inference forward wrote y1"
        y1k = None
    else:
        y1k = R.decode_l1(y1v, b, o1).double()
        _finite("y1", y1k)
        ratios["y1"] = R.ratio(y1k, y1_ex, e_y1)
    # ---- BatchNorm 1 ----
    bnk = out["bn_state"][0]
    _finite("bn_state", bnk[:128])
    y_stats = y1_ex if (pth["analytic"] or y1k is None) else y1k
    ref1 = _bn_ref(y_stats, C_STAT, st.g1, st.be1, cs["train"], *st.running0[0:2])
    _check_bn("bn1", bnk[:64], ref1, ratios)
    _check_running("bn1", st, cs, 0, ref1, b * o1 ** 3, ratios)
    tail = bnk[128:].view(torch.int32)
    if pth["analytic"]:
        assert torch.equal(tail.long(), st.exact_ac[st.rows].sum(0)), "bn_state: autocorrelation total"
    else:
        assert bool(torch.isnan(bnk[128:]).all()) or bool((tail == 0).all()), "bn_state: the autocorrelation tail was written"
    sc1, sh1 = bnk[0:16].double().view(1, 16, 1, 1, 1), bnk[16:32].double().view(1, 16, 1, 1, 1)
    mu1, rs1 = bnk[32:48].double().view(1, 16, 1, 1, 1), bnk[48:64].double().view(1, 16, 1, 1, 1)
    # range guard: bit 2 when |scale| sum |W1| + |scale b1 + shift| > 253 for some channel
    l1b = sc1.view(16).abs() * w1.abs().view(16, 27).sum(1) + (sc1.view(16) * st.b1.double() + sh1.view(16)).abs()
    flag = int(st.flag)
    if float(l1b.max()) > 253.0 * 1.001:
        assert flag & 2, f"range_flag {flag}: layer-1 bound {float(l1b.max()):.1f} > 253 not flagged"
    elif float(l1b.max()) < 253.0 * 0.999:
        assert not flag & 2, f"range_flag {flag}: layer-1 bound {float(l1b.max()):.1f} flagged"
    # ---- conv2 (fed by the kernel's y1 and scale / shift; the fused inference kernel by the exact conv1) ----
    if y1k is None:
        z1 = torch.relu(sc1 * y1_ex + sh1)
        e_z1 = sc1.abs() * e_y1
    else:
        z1 = torch.relu(sc1 * y1k + sh1)
        e_z1 = None
    if cs["big"]:  # (the case is meant to approach the clamp of the split kernels, not to pass it)
        print(f"[range] max z1 {float(z1.max()):.1f}, max |W2| {float(w2.abs().max()):.1f}")
        assert float(z1.max()) < 253.9 and float(z1.max()) > 100.0
    y2_ex = R.conv(z1, w2, st.b2.double())
    e_y2 = C_REL * R.conv(z1.abs(), w2.abs(), st.b2.double().abs())
    if e_z1 is not None:
        e_y2 += R.conv(e_z1, w2.abs())
    if pth["split_fwd"]:
        e_y2 += 2.0 ** -25 / Z_SCALE * R.conv(torch.ones_like(z1), w2.abs()) + 2.0 ** -25 / W_SCALE * R.conv(z1.abs(), torch.ones_like(w2))
    y2k = out["y2"][0].double().view(b, 16, o2, o2, o2)
    _finite("y2", y2k)
    ratios["y2"] = R.ratio(y2k, y2_ex, e_y2)
    ref2 = _bn_ref(y2k, C_STAT, st.g2, st.be2, cs["train"], *st.running0[3:5])
    _check_bn("bn2", bnk[64:128], ref2, ratios)
    _check_running("bn2", st, cs, 1, ref2, b * p2, ratios)
    sc2, sh2 = bnk[64:80].double().view(1, 16, 1), bnk[80:96].double().view(1, 16, 1)
    mu2, rs2 = bnk[96:112].double().view(1, 16, 1), bnk[112:128].double().view(1, 16, 1)
    y2f = y2k.view(b, 16, p2)
    feat_ex = torch.relu(sc2 * y2f + sh2)
    if cs["feats"]:
        fk = out["features"][0].view(b, 16, p2)
        _finite("features", fk)
        ratios["features"] = R.ratio(fk, feat_ex, R.ulp32(feat_ex))
        fmax = float(feat_ex.max())
        if fmax > 1001.0:
            assert flag & 4, "range_flag: a feature above 1000 not flagged"
        elif fmax < 999.0:
            assert not flag & 4, "range_flag: features flagged"
    else:
        assert bool(torch.isnan(out["features"][0]).all()) or bool((out["features"][0] == 0).all()), "features written although NULL"
        assert not flag & 4
    if not cs["train"]:
        return ratios
    # ---- BN2 + ReLU backward -> dy2 [B, P2, 16] ----
    df = out["d_features"].double().view(b, 16, p2)
    g2 = df * ((sc2 * y2f + sh2) > 0)
    xh2 = (y2f - mu2) * rs2
    m2 = b * p2
    s1 = g2.sum((0, 2))
    s2 = (g2 * xh2).sum((0, 2))
    a1 = g2.abs().sum((0, 2)).view(1, 16, 1)
    a2 = (g2 * xh2).abs().sum((0, 2)).view(1, 16, 1)
    dy2_ex = sc2 * (g2 - s1.view(1, 16, 1) / m2 - xh2 * s2.view(1, 16, 1) / m2)
    e_dy2 = C_REL * sc2.abs() * (g2.abs() + a1 / m2 + 2 * xh2.abs() * a2 / m2)
    dy2k = out["dy2"][0].view(b, p2, 16).permute(0, 2, 1).double()
    _finite("dy2", dy2k)
    ratios["dy2"] = R.ratio(dy2k, dy2_ex, e_dy2)
    ratios["dbn2_w"] = R.ratio(out["dg2"][0], s2, 2 * C_REL * a2.view(16))
    ratios["dbn2_b"] = R.ratio(out["dbe2"][0], s1, C_REL * a1.view(16))
    # ---- conv2 weight gradient, from the kernel's dy2 and z1 ----
    d5 = dy2k.reshape(b, 16, o2, o2, o2)
    amax = float(dy2k.abs().max())
    gsc = 2.0 ** min(14 - math.frexp(amax)[1], 126) if 0.0 < amax < 3.0e38 else 1.0
    res_dy2 = 2.0 ** -25 / gsc
    dw2_ex = R.weight_grad(d5, z1)
    e_dw2 = C_REL * R.weight_grad(d5.abs(), z1.abs())
    db2_ex = d5.sum((0, 2, 3, 4))
    e_db2 = C_REL * d5.abs().sum((0, 2, 3, 4))
    if pth["split_wg"]:
        e_dw2 += 2.0 ** -25 / Z_SCALE * d5.abs().sum((0, 2, 3, 4)).view(16, 1, 1, 1, 1)
        e_dw2 += res_dy2 * R.patches(z1.abs()).sum(0).view(1, 16, 3, 3, 3)
        e_db2 += res_dy2 * b * p2
    ratios["dw2"] = R.ratio(out["dw2"][0].view(16, 16, 3, 3, 3), dw2_ex, e_dw2)
    ratios["db2"] = R.ratio(out["db2"][0], db2_ex, e_db2)
    # ---- conv2 data gradient + ReLU-1 mask: dz1' ----
    mask1 = (sc1 * y1k + sh1) > 0
    gz = R.conv_t(d5, w2, o1) * mask1
    e_g = C_REL * R.conv_t(d5.abs(), w2.abs(), o1)
    if pth["split_dg"]:
        e_g += res_dy2 * R.conv_t(torch.ones_like(d5), w2.abs(), o1) + 2.0 ** -25 / W_SCALE * R.conv_t(d5.abs(), torch.ones_like(w2), o1)
        e_g += 2.0 ** -24 * float(w2.abs().sum((0, 2, 3, 4)).max()) / gsc
    e_g = e_g * mask1
    if pth["fused_bwd"]:
        assert bool(torch.isnan(out["dz1"][0]).all()) or bool((out["dz1"][0] == 0).all()), "the fused backward wrote dz1_scratch"
    else:
        dz1k = R.decode_l1(out["dz1"][0], b, o1).double()
        _finite("dz1", dz1k)
        ratios["dz1"] = R.ratio(dz1k, gz, e_g)
    # ---- BatchNorm-1 backward and the conv1 weight gradient ----
    n1 = b * o1 ** 3
    xh1 = (y1k - mu1) * rs1
    e_xh = C_REL * (y1k.abs() + mu1.abs()) * rs1 + (rs1 * e_y1 if pth["fused_bwd"] else 0.0)
    dims = (0, 2, 3, 4)
    t1, t2 = gz.sum(dims), (gz * xh1).sum(dims)
    e_t1 = e_g.sum(dims) + C_REL * gz.abs().sum(dims)
    e_t2 = (e_g * xh1.abs() + gz.abs() * e_xh).sum(dims) + C_REL * (gz * xh1).abs().sum(dims)
    ratios["dbn1_b"] = R.ratio(out["dbe1"][0], t1, e_t1)
    ratios["dbn1_w"] = R.ratio(out["dg1"][0], t2, e_t2)
    v = lambda t: t.view(1, 16, 1, 1, 1)  # noqa: E731
    dy1 = sc1 * (gz - v(t1) / n1 - xh1 * v(t2) / n1)
    e_dy1 = sc1.abs() * (e_g + v(e_t1) / n1 + xh1.abs() * v(e_t2) / n1 + e_xh * v(t2).abs() / n1)
    e_dy1 += C_REL * sc1.abs() * (gz.abs() + v(t1).abs() / n1 + xh1.abs() * v(t2).abs() / n1)
    ratios["dw1"] = R.ratio(out["dw1"][0].view(16, 1, 3, 3, 3), R.weight_grad(dy1, x), R.weight_grad(e_dy1, x.abs()))
    ratios["db1"] = R.ratio(out["db1"][0], dy1.sum(dims), e_dy1.sum(dims))
    for k in ("dw1", "db1", "dg1", "dbe1", "dw2", "db2", "dg2", "dbe2"):
        _finite(k, out[k][0])
    return ratios


def _documented(cs, pth, out):
    """The buffers whose every element is a documented output of this case (compared bit for bit across prefills)."""
    names = ["y2", "features" if cs["feats"] else None]
    if not pth["fused_eval"]:
        names.append("y1")
    if cs["train"]:
        names += ["dy2", "dw1", "db1", "dg1", "dbe1", "dw2", "db2", "dg2", "dbe2"] + ([] if pth["fused_bwd"] else ["dz1"])
    res = {k: out[k][0] for k in names if k}
    res["bn_state"] = out["bn_state"][0] if pth["analytic"] else out["bn_state"][0][:128]
    if "y1" in res or "dz1" in res:  # (layer-1 buffers: their padding slots are not documented)
        o1 = R.out_size(cs["g"])
        for k in ("y1", "dz1"):
            if k in res:
                res[k] = R.decode_l1(res[k], cs["b"], o1)
    return res


def _run_case(cs, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, val in cs["env"].items():
        monkeypatch.setenv(k, val)
    pth = _paths(cs)
    st = Setup(cs, zlib.crc32(repr(sorted((k, v) for k, v in cs.items() if k != "prep")).encode()))
    out = _run(cs, st, "nan")
    ratios = _check(cs, st, out, pth)
    worst = max(ratios, key=ratios.get) if ratios else None
    print(f"[err/bound] {worst} {ratios.get(worst, 0.0):.3f} | " + ", ".join(f"{k} {r:.3f}" for k, r in ratios.items()))
    running = [t.clone() for t in (st.rm1, st.rv1, st.nbt1, st.rm2, st.rv2, st.nbt2)]
    flag = int(st.flag)
    # the same call on zero-filled workspace / outputs / scratch: bit-identical documented outputs
    st.restore_running()
    out0 = _run(cs, st, "zero")
    a, z = _documented(cs, pth, out), _documented(cs, pth, out0)
    for k in a:
        assert _same_bits(a[k], z[k]), f"{k}: differs between a 0xFF / NaN-filled and a zero-filled workspace and outputs"
    for t, t0 in zip((st.rm1, st.rv1, st.nbt1, st.rm2, st.rv2, st.nbt2), running):
        assert _same_bits(t, t0), "running statistics differ between the two prefills"
    assert int(st.flag) == flag
    return out, ratios


@pytest.mark.parametrize("cs", CASES)
def test_encoder_abi_vs_fp64(cs, monkeypatch):
    """One forward (+ backward) per case on its kernel path; every documented output against the layered fp64 reference."""
    _, ratios = _run_case(cs, monkeypatch)
    bad = {k: r for k, r in ratios.items() if not r <= 1.0}
    assert not bad, f"outside the error model: {bad}"


def test_zero_upstream_gradient_gives_exact_zeros(monkeypatch):
    """d_features = 0 through the split kernels' max |dy2| scaling (gs = 1 there): every gradient exactly 0 and finite."""
    for g, inp in ((64, "i8"), (128, "i8"), (20, "rows")):
        cs = K(g, 2, inp, ac="rows" if inp == "i8" else None, dfeat="zero").values[0]
        out, _ = _run_case(cs, monkeypatch)
        for k in ("dy2", "dw1", "db1", "dg1", "dbe1", "dw2", "db2", "dg2", "dbe2"):
            assert bool((out[k][0] == 0).all()), f"G = {g}: {k} not exactly zero"


def test_fused_eval_prepared_is_bit_identical(monkeypatch):
    """The fused inference forward at G = 64 with eval_prepared 0 and 1 (gnbv_encoder_eval_prepare first): same bits."""
    outs = []
    for prep in (0, 1):
        cs = K(64, 3, "i8", train=False, prep=prep).values[0]
        assert _paths(cs)["fused_eval"]
        out, _ = _run_case(cs, monkeypatch)
        outs.append(out)
    for k in ("y2", "features", "bn_state"):
        assert _same_bits(outs[0][k][0], outs[1][k][0]), k


def test_eval_prepare_not_applicable_launches_nothing(monkeypatch):
    """gnbv_encoder_eval_prepare where the inference forward is not the one-launch kernel: GNBV_ERR_NOT_APPLICABLE, nothing written."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    cs = K(20, 2, train=False).values[0]
    st = Setup(cs, 3)
    bn, bnb = _buf(R.BN_STATE)
    wsn = lib.gnbv_encoder_workspace_bytes(2, 20)
    ws = torch.full((wsn,), 0xFF, dtype=torch.uint8, device=DEV)
    p = st.params(cs)
    assert lib.gnbv_encoder_eval_prepare(2, 20, C.byref(p), bn.data_ptr(), ws.data_ptr(), wsn, _stream()) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(bnb[:R.BN_STATE]).all()) and bool((ws == 0xFF).all())


def test_refused_arguments_launch_nothing(monkeypatch):
    """Each invalid argument returns an error before anything is launched: every output still NaN, the workspace untouched.
    The buffers are large enough for the call to run safely, so a missing check fails an assertion rather than memory."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    lib = _lib.load()
    g, b = 64, 2
    cs = K(g, b, "i8", ac="rows").values[0]
    st = Setup(cs, 11)
    n1, n2 = lib.gnbv_encoder_y1_elems(b, g), b * 16 * 15 ** 3
    wsn = lib.gnbv_encoder_workspace_bytes(b, g)
    s = _stream()

    def bufs():
        r = {k: _buf(n)[1] for k, n in (("y1", n1), ("y2", n2), ("bn", R.BN_STATE), ("f", n2), ("dy2", n2), ("dz1", n1))}
        r.update({k: _buf(432)[1] for k in ("dw1", "db1", "dg1", "dbe1", "dw2", "db2", "dg2", "dbe2")})
        r["ws"] = torch.full((wsn + 1024,), 0xFF, dtype=torch.uint8, device=DEV)
        return r

    def fwd(p, bb=b, gg=g, ws_off=0, ws_n=wsn):
        r = bufs()
        e = lib.gnbv_encoder_grid_forward(st.obs_ptr, st.rows.data_ptr(), st.row_stride, bb, gg, C.byref(p), 1, None, r["y1"].data_ptr(),
                                          r["y2"].data_ptr(), r["bn"].data_ptr(), r["f"].data_ptr(), r["ws"].data_ptr() + ws_off, ws_n, s)
        return e, r

    def bwd(p, bb=b, gg=g, ws_off=0, ws_n=wsn):
        r = bufs()
        d = torch.zeros(n2, device=DEV)
        y1, y2, bn = _buf(n1, fill=0.0)[1], _buf(n2, fill=0.0)[1], _buf(R.BN_STATE, fill=1.0)[1]
        gs = _lib.GnbvEncoderGrads()
        for name, key in (("w1", "dw1"), ("b1", "db1"), ("bn1_w", "dg1"), ("bn1_b", "dbe1"), ("w2", "dw2"), ("b2", "db2"),
                          ("bn2_w", "dg2"), ("bn2_b", "dbe2")):
            setattr(gs, name, r[key].data_ptr())
        e = lib.gnbv_encoder_grid_backward(st.obs_ptr, st.rows.data_ptr(), st.row_stride, bb, gg, C.byref(p), y1.data_ptr(), y2.data_ptr(),
                                           bn.data_ptr(), d.data_ptr(), r["dy2"].data_ptr(), r["dz1"].data_ptr(), C.byref(gs),
                                           r["ws"].data_ptr() + ws_off, ws_n, s)
        return e, r

    def untouched(what, e, r):
        torch.cuda.synchronize()
        assert e != 0, f"{what}: accepted"
        for k, t in r.items():
            if k == "ws":
                assert bool((t == 0xFF).all()), f"{what}: workspace written"
            else:
                assert bool(torch.isnan(t[:t.numel() - TAIL]).all()), f"{what}: {k} written"

    p = st.params(cs)
    bad_ac = st.params(cs)
    bad_ac.autocorr = st.ac.data_ptr() + 4  # (4-byte aligned: the rows are read with 16-byte loads)
    short_ac = st.params(cs)
    short_ac.autocorr_row_stride = R.AC_ROW - 4
    for name, call in (("grid 6", lambda f: f(p, gg=6)), ("batch 0", lambda f: f(p, bb=0)),
                       ("workspace one byte short", lambda f: f(p, ws_n=wsn - 1)),
                       ("workspace not 256-byte aligned", lambda f: f(p, ws_off=64)),
                       ("misaligned autocorr", lambda f: f(bad_ac)), ("autocorr row stride < 768", lambda f: f(short_ac))):
        for what, f in (("forward", fwd), ("backward", bwd)):
            untouched(f"{what}, {name}", *call(f))
    r = bufs()
    e = lib.gnbv_encoder_eval_prepare(b, 6, C.byref(p), r["bn"].data_ptr(), r["ws"].data_ptr(), wsn, s)
    untouched("eval_prepare, grid 6", e, r)
    r = bufs()
    e = lib.gnbv_encoder_eval_prepare(b, g, C.byref(p), r["bn"].data_ptr(), r["ws"].data_ptr() + 64, wsn, s)
    untouched("eval_prepare, workspace not 256-byte aligned", e, r)
    # gnbv_input_autocorr: G % 16 != 0, a short output row
    out = torch.full((4, 800), -7, dtype=torch.int32, device=DEV)
    assert lib.gnbv_input_autocorr(st.i8.data_ptr(), st.i8.stride(0), 2, 20, out.data_ptr(), 800, s) != 0
    assert lib.gnbv_input_autocorr(st.i8.data_ptr(), st.i8.stride(0), 2, g, out.data_ptr(), 700, s) != 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())
