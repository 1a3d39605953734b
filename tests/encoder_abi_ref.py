"""fp64 reference of the encoder grid branch for tests/test_encoder_abi_gpu.py, written from the operator definitions of
include/gennbv_hip.h section B1: Conv3d(1, 16, 3, s2), BatchNorm, ReLU, Conv3d(16, 16, 3, s2), BatchNorm, ReLU.

Convolutions are an explicit unfold followed by a matmul (no fp64 conv3d), the transposed convolution is 27 strided slice-adds.
Every function works on fp64 tensors on whatever device they live on.  The same functions applied to absolute values give the
magnitude sums |W| (*) |x| of the error model."""
from __future__ import annotations

import math

import torch

C = 16          # channels of both layers
TAPS = 27
AC_ROW = 768    # ints of one autocorrelation row (gnbv_input_autocorr_row_ints)
BN_STATE = 2 * 4 * C + AC_ROW


def out_size(g: int) -> int:
    return (g - 3) // 2 + 1


def patches(v: torch.Tensor) -> torch.Tensor:
    """v [B, Cin, D, D, D] -> [B * O^3, Cin * 27] (column = cin * 27 + (dz * 3 + dy) * 3 + dx: torch's weight layout)."""
    b, cin = v.shape[:2]
    u = v.unfold(2, 3, 2).unfold(3, 3, 2).unfold(4, 3, 2)  # [B, Cin, O, O, O, 3, 3, 3]
    o = u.shape[2]
    return u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(b * o ** 3, cin * TAPS)


def conv(v: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """Valid stride-2 3x3x3 convolution: v [B, Cin, D, D, D], w [16, Cin, 3, 3, 3] -> [B, 16, O, O, O]."""
    b = v.shape[0]
    o = out_size(v.shape[2])
    y = patches(v) @ w.reshape(w.shape[0], -1).t()
    if bias is not None:
        y = y + bias
    return y.view(b, o, o, o, -1).permute(0, 4, 1, 2, 3)


def conv_t(d: torch.Tensor, w: torch.Tensor, o_in: int) -> torch.Tensor:
    """Transposed (data-gradient) convolution: d [B, 16, O, O, O], w [16, Cin, 3, 3, 3] -> [B, Cin, o_in, o_in, o_in]."""
    b, _, o = d.shape[:3]
    out = torch.zeros(b, w.shape[1], o_in, o_in, o_in, dtype=d.dtype, device=d.device)
    e = 2 * (o - 1) + 1
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out[:, :, kz:kz + e:2, ky:ky + e:2, kx:kx + e:2] += torch.einsum("bnzyx,nc->bczyx", d, w[:, :, kz, ky, kx])
    return out


def weight_grad(d: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """sum over samples and output positions of d [B, 16, O, O, O] (x) patches of v [B, Cin, D, D, D] -> [16, Cin, 3, 3, 3]."""
    n = d.shape[1]
    g = d.permute(0, 2, 3, 4, 1).reshape(-1, n).t() @ patches(v)
    return g.view(n, v.shape[1], 3, 3, 3)


def decode_l1(buf: torch.Tensor, b: int, o1: int) -> torch.Tensor:
    """A layer-1 buffer (y1 / dz1': channels-last, split by x parity, vox1() in csrc/encoder.hip) -> [B, 16, O1, O1, O1].
    The padding slot of the odd half row (odd O1) is dropped."""
    xh = (o1 + 1) // 2
    v = buf[:b * o1 * o1 * 2 * xh * C].view(b, o1, o1, 2, xh, C)
    out = torch.empty(b, o1, o1, o1, C, dtype=buf.dtype, device=buf.device)
    out[:, :, :, 0::2] = v[:, :, :, 0, :(o1 + 1) // 2]
    out[:, :, :, 1::2] = v[:, :, :, 1, :o1 // 2]
    return out.permute(0, 4, 1, 2, 3)


def autocorr_rows(x: torch.Tensor) -> torch.Tensor:
    """Exact input autocorrelation rows (gnbv_input_autocorr) of int grids x [n, G, G, G] -> [n, 768] int64."""
    n = x.shape[0]
    pat = patches(x.unsqueeze(1).double())  # (integers below 2^53 throughout: exact in fp64)
    o3 = pat.shape[0] // n
    pat = pat.view(n, o3, TAPS)
    pat = torch.cat((pat, torch.ones(n, o3, 1, dtype=pat.dtype, device=x.device),
                     torch.zeros(n, o3, 4, dtype=pat.dtype, device=x.device)), dim=2)
    r = torch.einsum("npt,npu->ntu", pat, pat).round().to(torch.int64)
    return torch.stack((r[:, :16, :16], r[:, :16, 16:], r[:, 16:, 16:]), dim=1).reshape(n, AC_ROW)


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """One fp32 ulp at |x| (fp64 in, fp64 out; the smallest normal's ulp below it)."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def ratio(got: torch.Tensor, want: torch.Tensor, bound) -> float:
    """Largest |got - want| / bound over the elements (an element whose bound is 0 must be exact; a non-finite value is inf)."""
    got = got.double()
    err = (got - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=got.device).expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(torch.isfinite(got), r, math.inf)
    return float(r.max()) if r.numel() else 0.0
