"""GPU: the G = 64 conv kernels that walk several items per workgroup on one continuous ring (csrc/conv_split.h:
k_conv12_fwd_split<TRAIN>, k_conv2_wgrad_split_dma) must not depend on how many workgroups share the items.

GENNBV_CONV_MAXWG = 512 gives every item its own workgroup (the one-item kernels); 16 and 8 make a workgroup walk two to five items, the
next item's first rows entering the ring while the last rows of the current one are still being read.  Everything the forward writes is the
same arithmetic in the same order, so it must be BIT-identical; the weight gradient's fp32 partial rows sum several items before the fp64
reduction, which legitimately regroups conv2's weight / bias gradient (tolerances of tests/test_encoder_gpu.py::
test_wgrad_lds_dma_transport_is_bit_identical, whose modules and inputs are used here: int8 rows plus autocorrelation rows)."""
import pytest
import torch

from tests import policy_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 64


def _obs(b, zero_rows, seed=7):
    gen = torch.Generator().manual_seed(seed)
    o = torch.zeros(b, pu.obs_dim(G))
    o[:, :600] = torch.randn(b, 600, generator=gen)
    o[:, 600:600 + G ** 3] = torch.randint(-1, 2, (b, G ** 3), generator=gen).float() * (torch.rand(b, G ** 3, generator=gen) < 0.4).float()
    o[zero_rows, 600:600 + G ** 3] = 0
    return o.to(DEV)


# batch 3: 12 items in 32 slots (non-live items, workgroups without any); batch 9: a second round of samples, the three-plane last group
# of a sample inside and at the end of a walk; "zeros": samples 0 .. 7 are empty grids and sample 8 is random -- at 8 workgroups every
# walk with two samples passes from an all-zero one to a random one, so a row of the neighbouring item left in the ring cannot cancel
@pytest.mark.parametrize("b,zeros", [(3, False), (9, False), (9, True)])
def test_item_walk_is_independent_of_the_grid(b, zeros, monkeypatch):
    from gennbv_amd.ops import encoder_ops
    from gennbv_amd.ops.encoder_ops import RowGather, input_autocorr
    hip, _, _ = pu.make_policy(g=G, device=DEV, backend="hip", det_weights=True)
    enc = hip.features_extractor
    rows = torch.randperm(b + 2, generator=torch.Generator().manual_seed(5))[:b]
    base = _obs(b + 2, rows[:8] if zeros else [])
    rows = rows.to(DEV)
    grid_i8 = base[:, 600:600 + G ** 3].to(torch.int8).contiguous()
    ac = input_autocorr(grid_i8, G)
    w = torch.linspace(0.5, 1.5, 256).to(DEV)
    seen = {}
    conv_stack = encoder_ops.grid_encoder

    def recording(*a, **k):  # the conv stack's own output (y2 / the features in front of fc_grid) and what it saved for the backward
        r = conv_stack(*a, **k)
        t = r[0] if isinstance(r, tuple) else r
        seen["out"] = t.detach().clone()
        if t.grad_fn is not None:
            seen["y2"] = t.grad_fn.saved_tensors[3].detach().clone()
        return r
    monkeypatch.setattr(encoder_ops, "grid_encoder", recording)
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    res = {}
    for maxwg in ("512", "512 again", "16", "8"):
        monkeypatch.setenv("GENNBV_CONV_MAXWG", maxwg.split()[0])
        enc.load_state_dict(state)
        enc.train()
        hip.zero_grad()
        f = enc(RowGather(base, rows, grid_i8, autocorr=ac))
        (f * w).sum().backward()
        cur = dict(f=f.detach().clone(), out=seen.pop("out"), y2=seen.pop("y2"),
                   stats={k: v.clone() for k, v in enc.state_dict().items() if "running" in k},
                   grads={k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None})
        enc.eval()
        with torch.no_grad():
            cur["eval_f"] = enc(RowGather(base, rows, grid_i8)).clone()
        cur["eval_out"] = seen.pop("out")
        torch.cuda.synchronize()
        res[maxwg] = cur
    ref = res["512"]
    k2w, k2b = "naive_encoder_grid.3.weight", "naive_encoder_grid.3.bias"
    assert float(ref["y2"].abs().max()) > 0 and float(ref["grads"][k2w].abs().max()) > 0 and float(ref["eval_out"].abs().max()) > 0
    assert any("naive_encoder_grid" in k for k in ref["stats"]) and k2b in ref["grads"]
    for maxwg in ("512 again", "16", "8"):
        cur = res[maxwg]
        for k in ("f", "out", "y2", "eval_f", "eval_out"):
            assert torch.equal(cur[k], ref[k]), (maxwg, k, float((cur[k] - ref[k]).abs().max()))
        for k, v in ref["stats"].items():
            assert torch.equal(cur["stats"][k], v), (maxwg, k)
        for k, a in ref["grads"].items():
            c = cur["grads"][k]
            if k in (k2w, k2b) and maxwg != "512 again":
                # conv2's weight and bias gradient: a partial row sums a walk's items in fp32 before the fp64 reduction (the bias in front of
                # BatchNorm has an analytically zero gradient: what it holds is the rounding noise of a sum of B * O^3 terms)
                floor = 1e-4 * max(1.0, b / 8) if k == k2b else 1e-9
                err = float((a - c).abs().max())
                print(f"b={b} zeros={zeros} maxwg={maxwg} {k}: max |delta| {err:.3e}, max |grad| {float(a.abs().max()):.3e}")
                assert err <= 2e-6 * float(a.abs().max()) + floor, (maxwg, k)
            else:
                assert torch.equal(a, c), (maxwg, k, float((a - c).abs().max()))
