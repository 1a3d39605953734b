"""GPU: hand-written conv3d/BN/ReLU encoder kernels (fwd + bwd) vs the torch fp32 reference of
the same op and vs the golden produced by the reference's Hybrid_Encoder (F7)."""
import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import policy_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(g, seed=0):
    torch.manual_seed(seed)
    a, _, _ = pu.make_policy(g=g, device=DEV, backend="torch", det_weights=True)
    b, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    return a, b


def _obs(b, g, seed=0):
    gen = torch.Generator().manual_seed(seed)
    o = torch.zeros(b, pu.obs_dim(g))
    o[:, :600] = torch.randn(b, 600, generator=gen)
    grid = torch.randint(-1, 2, (b, g ** 3), generator=gen).float() * (torch.rand(b, g ** 3, generator=gen) < 0.4).float()
    o[:, 600:600 + g ** 3] = grid
    return o.to(DEV)


def _obs_clear_of_the_relu_threshold(ref, b, g):
    """The seeded observation batch, re-drawn (seed + 1, ...) until no BatchNorm-2 output of the fp64 reference lies within
    1e-5 of the ReLU threshold.  Such a knife-edge element flips its mask on ANY fp32 rounding difference (two correct fp32
    kernels land on opposite sides) and, at a batch of 4, one flip moves the conv / BN gradients by 1e-3 of their scale --
    measured at seed 64: element (3, 5, 2, 13, 1) sits at +-6e-8."""
    seen = {}
    bn2 = ref.features_extractor.naive_encoder_grid[4]
    h = bn2.register_forward_hook(lambda mod, inp, out: seen.__setitem__("min", float(out.detach().abs().min())))
    try:
        for seed in range(g, g + 16):
            obs = _obs(b, g, seed=seed)
            ref.set_training_mode(True)
            stats = {k: v.clone() for k, v in ref.state_dict().items() if "running" in k or "num_batches" in k}
            with torch.no_grad():
                ref.features_extractor(obs.cpu().double())
            ref.load_state_dict(stats, strict=False)  # (the probe must not advance the running statistics)
            if seen["min"] >= 1e-5 or b > 16 or g > 64:  # (large batches / grids always hold such elements and dilute them)
                return obs
    finally:
        h.remove()
    raise AssertionError("no clean seed")


@pytest.mark.parametrize("conv2", ["fp32", "split", "splitx"])
@pytest.mark.parametrize("g,b", [(20, 8), (16, 5), (33, 3), (64, 4), (128, 1), (128, 3), (64, 128)])  # last: the bench's minibatch
def test_encoder_forward_backward_vs_torch_reference(g, b, conv2, monkeypatch):
    """Reference = the same torch modules in fp64 on the CPU (ground truth), tolerance = fp32 round-off.
    (torch-GPU fp32 is NOT used as the reference: MIOpen's conv/BN backward is off by 0.7-4.6 % at
    G=64 against fp64, tools/check_conv_grads.py; the hand-written kernels are within 1e-6.)
    conv2 = "split": the conv2 kernels on the f16 matrix pipe with split (hi + lo) operands (csrc/conv_split.h; G = 64, the
    default there) -- SAME tolerances as the fp32-MFMA kernels, which conv2 = "fp32" (GENNBV_CONV_SPLIT=0) keeps covered.
    conv2 = "splitx": the x-tiled kernels of csrc/conv_splitx.h (17-voxel ring rows) -- what G = 128 runs by default (there "split" and
    "splitx" are the same path), and at G = 64 the same kernels with one tile per row (GENNBV_SPLITX=1).
    Every case runs what its setting selects at its size: below G = 64 the conv kernels are the fp32-MFMA ones under every setting, and
    "split" / "splitx" there keep the default split-f16 fc-layer kernels that "fp32" (GENNBV_CONV_SPLIT=0) switches off."""
    monkeypatch.setenv("GENNBV_CONV_SPLIT", "0" if conv2 == "fp32" else "1")
    monkeypatch.setenv("GENNBV_SPLITX", "1" if conv2 == "splitx" else "")
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    ref, _, _ = pu.make_policy(g=g, device="cpu", backend="torch", det_weights=True)
    ref = ref.double()
    ref.extract_features = lambda x: ref.features_extractor(x)  # keep fp64 (no .float() cast)
    obs = _obs_clear_of_the_relu_threshold(ref, b, g)
    actions = torch.stack([torch.randint(0, n, (b,)) for n in pu.NVEC], -1).float()
    w = torch.linspace(0.5, 1.5, b)
    outs = []
    for pol, dev, dt in ((ref, "cpu", torch.float64), (hip, DEV, torch.float32)):
        pol.set_training_mode(True)
        pol.zero_grad()
        values, log_prob, entropy = pol.evaluate_actions(obs.to(dev, dt), actions.to(dev))
        ww = w.to(dev, dt)
        loss = (values.flatten() * ww).sum() + (log_prob * ww.flip(0)).sum() + 0.3 * (entropy * ww).sum()
        loss.backward()
        outs.append([t.detach().double().cpu() for t in (values, log_prob, entropy)])
    for x, y in zip(*outs):
        assert float((x - y).abs().max()) <= 2e-5 * float(x.abs().max()) + 1e-6
    for (n1, p1), (n2, p2) in zip(ref.named_parameters(), hip.named_parameters()):
        r = p1.grad.double()
        scale = float(r.abs().max())
        err = float((r - p2.grad.double().cpu()).abs().max())
        if scale < 1e-9:  # conv bias in front of BatchNorm: analytically zero gradient (rounding noise, grows with the batch)
            assert err < 1e-4 * max(1.0, b / 8), (n1, err)
        else:
            assert err <= 2e-5 * scale, (n1, err, scale)
    for (k1, v1), (k2, v2) in zip(ref.state_dict().items(), hip.state_dict().items()):
        if "running" in k1:
            torch.testing.assert_close(v2.double().cpu(), v1.double(), rtol=1e-5, atol=1e-6)
        if "num_batches" in k1:
            assert int(v1) == int(v2) == 1
    for pol in (ref, hip):
        pol.set_training_mode(False)
    with torch.no_grad():
        a = hip.extract_features(obs).double().cpu()
        r = ref.extract_features(obs.cpu().double())
    assert float((a - r).abs().max()) <= 2e-5 * float(r.abs().max()) + 1e-6


@pytest.mark.parametrize("conv2", ["split", "splitx"])
def test_encoder_backward_of_a_tiny_gradient(conv2, monkeypatch):
    """d_feats 2^-118 backpropagated through the HIP encoder (G = 64, the split-f16 conv2 kernels): their gradient scale puts max |dy2|
    into [2^13, 2^14) and was 2^(14 - e), +inf (and its inverse -inf) once max |dy2| fell below 2^-114.  Every gradient must be finite
    and, rescaled by 2^118, within the tolerances of test_encoder_forward_backward_vs_torch_reference against fp64."""
    g, b = 64, 4
    monkeypatch.setenv("GENNBV_CONV_SPLIT", "1")
    monkeypatch.setenv("GENNBV_SPLITX", "1" if conv2 == "splitx" else "")
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    ref, _, _ = pu.make_policy(g=g, device="cpu", backend="torch", det_weights=True)
    ref = ref.double()
    obs = _obs_clear_of_the_relu_threshold(ref, b, g)
    d = torch.randn(b, 256, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    for pol, dev, dt, scale in ((ref, "cpu", torch.float64, 1.0), (hip, DEV, torch.float32, 2.0 ** -118)):
        pol.set_training_mode(True)
        pol.zero_grad()
        f = pol.features_extractor(obs.to(dev, dt))
        assert f.shape == d.shape
        f.backward((d * scale).to(dev, dt))
    for (n1, p1), (n2, p2) in zip(ref.features_extractor.named_parameters(), hip.features_extractor.named_parameters()):
        assert n1 == n2
        got = p2.grad.double().cpu()
        assert bool(torch.isfinite(got).all()), n2
        got = got * 2.0 ** 118
        r = p1.grad.double()
        scale = float(r.abs().max())
        err = float((r - got).abs().max())
        if scale < 1e-9:  # (conv bias in front of BatchNorm: analytically zero gradient, as in the test above)
            assert err < 1e-4 * max(1.0, b / 8), (n1, err)
        else:
            assert err <= 2e-5 * scale, (n1, err, scale)


@pytest.mark.parametrize("z1",["0", "fp32", "splitx"])  # "fp32": GENNBV_CONV_SPLIT=0, the fp32-MFMA conv2 kernels ("0" runs the split-f16 ones at G = 64 / 128)
@pytest.mark.parametrize("g,b", [(16, 5), (32, 3), (48, 2), (64, 4), (128, 1), (128, 2), (64, 128)])  # last: the bench's minibatch
# ((128, 3) with these seeds holds a layer-1 pre-activation on the ReLU knife edge: the fp32-MFMA and the split kernels then miss the fp64
# conv1 weight gradient by the same 2.8e-4 of its scale -- 0.0024914 and 0.0024921 --, a property of the sample, not of a kernel)
def test_fused_dgrad_conv1_wgrad_vs_fp64_reference(g, b, z1, monkeypatch):
    """With the int8 grid rows present (G % 16 == 0) the backward runs k_conv2_dgrad_c1w: conv2 data gradient and conv1
    weight gradient in one launch, BN1 backward applied to fp64 sums afterwards (dz1' is never stored).  All conv / BN
    gradients against the fp64 torch reference, tolerance = fp32 round-off; rows are gathered (RowGather)."""
    monkeypatch.setenv("GENNBV_CONV_SPLIT", "0" if z1 == "fp32" else "1")
    # The comparison "analytic vs measured BN1 statistics" below needs bit-identical y1 in both runs: the split conv1 kernel only
    # runs where no partial sums are asked for (the analytic run), the fp32 one in the measured run, and two of the 61 M layer-1
    # pre-activations of the (64, 128) case sit within 2e-8 of the ReLU threshold -- a flipped mask moves the bias gradient, a sum
    # of 3.8 M terms of mixed sign per channel, by 7e-4 of its value.  k_conv1_fwd_split has its own test below.
    monkeypatch.setenv("GENNBV_CONV1_SPLIT", "0")
    # Every case runs what its setting selects at its size.  Below G = 64 the conv kernels are the fp32-MFMA ones under every setting
    # ("fp32" also switches the split-f16 fc-layer kernels off); GENNBV_SPLITX=1 selects the x-tiled kernels at G = 64, which are
    # G = 128's default -- there "splitx" differs from "0" by the small workgroup cap below (several items per workgroup).
    monkeypatch.setenv("GENNBV_SPLITX", "1" if z1 == "splitx" else "")
    if z1 == "splitx":
        monkeypatch.setenv("GENNBV_FUSED_TRAIN", "0")  # (the one-launch training forward would bypass the x-tiled conv2 forward)
        monkeypatch.setenv("GENNBV_SPLITX_MAXWG", "8")  # (32 / 512 items over 8 workgroups: the several-items-per-workgroup loops)
    from gennbv_amd.ops.encoder_ops import RowGather, input_autocorr
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    ref, _, _ = pu.make_policy(g=g, device="cpu", backend="torch", det_weights=True)
    ref = ref.double()
    base = _obs(2 * b + 1, g, seed=g + 1)
    # fixed row subset: with an unseeded permutation one run in ~5 hit a batch in which a layer-1 pre-activation lies within
    # fp32 round-off of zero, where the fp32 kernels and the fp64 reference take different sides of the ReLU
    rows = torch.randperm(2 * b + 1, generator=torch.Generator().manual_seed(100 + g))[:b].to(DEV)
    grid_i8 = base[:, 600:600 + g ** 3].to(torch.int8).contiguous()
    w = torch.linspace(0.5, 1.5, 256)
    # the input autocorrelation is either computed by the backward call (minibatch total) or gathered from per-row
    # results stored with the observations (exact integers both ways)
    hip.train()
    for _ in range(2):  # (first pass: warm-up, the library GEMMs of the fc layer may be auto-tuned on their first call)
        hip.zero_grad()
        f = hip.features_extractor(RowGather(base, rows, grid_i8, autocorr=input_autocorr(grid_i8, g)))
        (f * w.to(DEV)).sum().backward()
    stored = [p.grad.clone() for p in hip.features_extractor.parameters()]
    outs = []
    for pol, obs, dev, dt in ((ref, base[rows].cpu().double(), "cpu", torch.float64), (hip, RowGather(base, rows, grid_i8), DEV, torch.float32)):
        pol.train()
        pol.zero_grad()
        f = pol.features_extractor(obs)
        (f * w.to(dev, dt)).sum().backward()
        outs.append(f.detach().double().cpu())
    # (with stored rows BatchNorm-1's batch statistics come analytically from the autocorrelation, without them from the
    # activations: equal to fp32 round-off, not bit for bit)
    for a, c in zip(stored, hip.features_extractor.parameters()):
        # (+ the noise floor of the analytically zero conv-bias gradients: a sum of B*O^3 rounded terms, it grows with the batch)
        assert float((a - c.grad).abs().max()) <= 1e-5 * float(a.abs().max()) + 1e-5 * max(1.0, b / 4)
    assert float((outs[0] - outs[1]).abs().max()) <= 2e-5 * float(outs[0].abs().max()) + 1e-6
    for (n1, p1), (n2, p2) in zip(ref.features_extractor.named_parameters(), hip.features_extractor.named_parameters()):
        r = p1.grad.double()
        scale = float(r.abs().max())
        err = float((r - p2.grad.double().cpu()).abs().max())
        if scale < 1e-9:  # conv bias in front of BatchNorm: analytically zero gradient (rounding noise, grows with the batch)
            assert err < 1e-4 * max(1.0, b / 8), (n1, err)
        else:
            assert err <= 2e-5 * scale, (n1, err, scale)
    # BatchNorm running statistics (z1 mode, G <= 64: analytic batch statistics from the input autocorrelation; three training
    # forwards on the GPU side, so compare after bringing the reference to the same count) and the eval-mode forward
    # (conv1 with the BN + ReLU epilogue on the running statistics)
    for _ in range(2):
        ref.features_extractor(base[rows].cpu().double())
    for (k1, v1), (k2, v2) in zip(ref.state_dict().items(), hip.state_dict().items()):
        if "running" in k1:
            torch.testing.assert_close(v2.double().cpu(), v1.double(), rtol=2e-5, atol=1e-6)
        if "num_batches" in k1:
            assert int(v1) == int(v2) == 3
    ref.eval()
    hip.eval()
    with torch.no_grad():
        a = hip.features_extractor(RowGather(base, rows, grid_i8)).double().cpu()
        r = ref.features_extractor(base[rows].cpu().double())
    assert float((a - r).abs().max()) <= 2e-5 * float(r.abs().max()) + 1e-6


@pytest.mark.parametrize("g,n", [(16, 3), (32, 2), (48, 2), (64, 3), (128, 1)])
def test_input_autocorrelation_rows_exact(g, n):
    """gnbv_input_autocorr: R[t][t'] = sum over conv1 output positions of x[pos,t] x[pos,t'] per row (t = 27: ones),
    exact integers, vs torch unfold on the CPU."""
    from gennbv_amd.ops.encoder_ops import input_autocorr
    gen = torch.Generator().manual_seed(g)
    x = (torch.randint(-1, 2, (n, g ** 3), generator=gen) * (torch.rand(n, g ** 3, generator=gen) < 0.6)).to(torch.int8)
    rows = input_autocorr(x.to(DEV), g).cpu()
    assert rows.shape == (n, 768)
    o1 = (g - 3) // 2 + 1
    v = x.view(n, g, g, g).to(torch.int64)
    pat = v.unfold(1, 3, 2).unfold(2, 3, 2).unfold(3, 3, 2).reshape(n, o1 ** 3, 27)  # [n, pos, tap = (dz, dy, dx)]
    pat = torch.cat((pat, torch.ones(n, o1 ** 3, 1, dtype=torch.int64), torch.zeros(n, o1 ** 3, 4, dtype=torch.int64)), dim=2)
    R = torch.einsum("npt,npu->ntu", pat, pat)  # [n, 32, 32]
    tiles = torch.stack((R[:, :16, :16], R[:, :16, 16:], R[:, 16:, 16:]), dim=1).reshape(n, 768)
    assert torch.equal(rows.to(torch.int64), tiles)
    assert int(rows[0, 512 + 11 * 16 + 11]) == o1 ** 3  # R[27][27] = number of positions


def test_encoder_matches_reference_golden_f7():
    fx = gu.load("F7_policy")
    pol, _, _ = pu.make_policy(g=20, device=DEV, backend="hip", det_weights=True)
    obs, actions = pu.unpack_obs(fx).to(DEV), torch.from_numpy(fx["actions"]).to(DEV)
    pol.set_training_mode(False)
    with torch.no_grad():
        feats = pol.extract_features(obs)
        values, log_prob, entropy = pol.evaluate_actions(obs, actions)
    np.testing.assert_allclose(feats.cpu().numpy(), fx["eval_features"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(values.cpu().numpy(), fx["eval_values"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(log_prob.cpu().numpy(), fx["eval_log_prob"], rtol=1e-4, atol=1e-5)
    pol.set_training_mode(True)
    pol.zero_grad()
    values, log_prob, entropy = pol.evaluate_actions(obs, actions)
    w = torch.linspace(0.5, 1.5, obs.shape[0], device=DEV)
    loss = (values.flatten() * w).sum() + (log_prob * w.flip(0)).sum() + 0.3 * (entropy * w).sum()
    loss.backward()
    np.testing.assert_allclose(values.detach().cpu().numpy(), fx["train_values"], rtol=1e-4, atol=1e-5)
    for name, p in pol.named_parameters():
        g = p.grad.cpu().numpy()
        mine = g if g.size <= 70000 else g.reshape(-1)[::97]
        ref = fx["grad/" + name]
        assert np.abs(mine - ref).max() <= 2e-4 * (np.abs(ref).max() + 1e-6) + 2e-6, name
    for k, v in pol.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), fx["bn_after/" + k], rtol=1e-5, atol=1e-6)


def test_row_gather_equals_materialised_batch():
    from gennbv_amd.ops.encoder_ops import RowGather
    g, n = 20, 12
    pol, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    base = _obs(n, g, seed=3)
    rows = torch.tensor([7, 0, 3, 3, 11], device=DEV)
    pol.set_training_mode(False)
    with torch.no_grad():
        a = pol.extract_features(RowGather(base, rows))
        b = pol.extract_features(base[rows])
    assert torch.equal(a, b)


def test_reduced_precision_storage_is_refused():
    """The bf16 activation-storage mode of rounds 1-3 was removed (slower than the fp32-accurate split-f16 kernels, 1e-3-class loss
    deltas: DESIGN.md section 5): asking for it fails loudly instead of silently computing in another precision."""
    with pytest.raises(ValueError, match="fp32"):
        pu.make_policy(g=20, device=DEV, backend="hip", det_weights=True, compute_dtype=torch.bfloat16)


@pytest.mark.parametrize("arith", ["split", "fp32"])
@pytest.mark.parametrize("m,n,k", [(128, 256, 54000), (256, 256, 54000), (7, 64, 1024), (130, 128, 1000), (1, 64, 4)])
def test_splitk_linear_relu_vs_fp64(m, n, k, arith, monkeypatch):
    """fc_grid (hybrid_encoder.py:39-42): relu(x W^T + b) on the split-K MFMA kernel vs an fp64 reference;
    tolerance = fp32 accumulation round-off over K terms.  Backward = library GEMMs on the same mask.
    arith = "split": k_linear_splitk_split (f16 matrix pipe, split fp32 operands; K % 8 == 0 and K >= 64, else the fp32
    kernel runs); "fp32": GENNBV_CONV_SPLIT=0, k_linear_splitk (fp32 MFMA).  Same tolerance."""
    monkeypatch.setenv("GENNBV_CONV_SPLIT", "1" if arith == "split" else "0")
    from gennbv_amd.ops.encoder_ops import linear_relu
    gen = torch.Generator().manual_seed(m + n + k)
    x = (torch.rand(m, k, generator=gen) * (torch.rand(m, k, generator=gen) < 0.5)).to(DEV).requires_grad_(True)
    lin = torch.nn.Linear(k, n).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(n, k, generator=gen) / k ** 0.5)
        lin.bias.copy_(torch.randn(n, generator=gen) * 0.1)
    out = linear_relu(x, lin)
    ref = torch.relu(x.detach().double() @ lin.weight.detach().double().t() + lin.bias.detach().double())
    assert out.shape == (m, n)
    assert torch.allclose(out.double(), ref, rtol=1e-5, atol=2e-6), float((out.double() - ref).abs().max())
    # deterministic: identical bits on a second call
    assert torch.equal(out, linear_relu(x, lin))
    if m > 128 and arith == "split":
        # round 5: more than 128 rows go through 256-row workgroups (one staged W tile for both halves); the rows' arithmetic is that
        # of the 128-row workgroups, bit for bit
        with torch.no_grad():
            halves = torch.cat([linear_relu(x[i:i + 128].detach().contiguous(), lin) for i in range(0, m, 128)])
        assert torch.equal(out.detach(), halves)
    d = torch.randn(m, n, generator=gen).to(DEV)
    out.backward(d)
    g = d.double() * (ref > 0)
    assert torch.allclose(x.grad.double(), g @ lin.weight.detach().double(), rtol=1e-4, atol=1e-6)
    assert torch.allclose(lin.weight.grad.double(), g.t() @ x.detach().double(), rtol=1e-4, atol=1e-5)
    assert torch.allclose(lin.bias.grad.double(), g.sum(0), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("m,a", [(128, 241), (37, 241), (256, 17), (5, 3)])
def test_fused_policy_head_vs_fp64(m, a):
    """output_layer + action_net + value_net (hybrid_encoder.py:51-54,:89; sb3 policies.py:975-979) fused in
    csrc/head.hip, forward and backward, against fp64 torch; tolerance = fp32 round-off of K <= 512 sums."""
    from gennbv_amd.ops import encoder_ops as eo
    gen = torch.Generator().manual_seed(m * 1000 + a)
    k1 = k2 = f = 256

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, generator=gen) * scale).to(DEV)

    fa, fg = rnd(m, k1).abs().requires_grad_(True), rnd(m, k2).abs().requires_grad_(True)
    lo, la, lv = torch.nn.Linear(k1 + k2, f).to(DEV), torch.nn.Linear(f, a).to(DEV), torch.nn.Linear(f, 1).to(DEV)

    class Enc:
        output_layer = torch.nn.Sequential(lo, torch.nn.ReLU())

    logits, values, feat = eo.policy_head(Enc, la, lv, fa, fg)
    cat = torch.cat((fa, fg), -1).detach().double().requires_grad_(True)
    wd = [t.detach().double().requires_grad_(True) for t in (lo.weight, lo.bias, la.weight, la.bias, lv.weight, lv.bias)]
    feat_ref = torch.relu(cat @ wd[0].t() + wd[1])
    logits_ref, values_ref = feat_ref @ wd[2].t() + wd[3], (feat_ref @ wd[4].t() + wd[5]).flatten()
    assert torch.allclose(feat.double(), feat_ref, rtol=1e-5, atol=1e-5)
    assert torch.allclose(logits.double(), logits_ref, rtol=1e-5, atol=1e-5)
    assert torch.allclose(values.double(), values_ref, rtol=1e-5, atol=1e-5)
    dl, dv = rnd(m, a), rnd(m)
    torch.autograd.backward([logits, values], [dl, dv])
    torch.autograd.backward([logits_ref, values_ref], [dl.double(), dv.double()])
    got = [fa.grad, fg.grad, lo.weight.grad, lo.bias.grad, la.weight.grad, la.bias.grad, lv.weight.grad, lv.bias.grad]
    ref = [cat.grad[:, :k1], cat.grad[:, k1:]] + [t.grad for t in wd]
    for g, r in zip(got, ref):
        assert g.shape == r.shape
        assert torch.allclose(g.double(), r, rtol=1e-4, atol=1e-4 * float(r.abs().max()) + 1e-7), float((g.double() - r).abs().max())


@pytest.mark.parametrize("g,b", [(64, 6), (16, 5), (32, 3)])
def test_int8_grid_copy_gives_identical_results(g, b, monkeypatch):
    """GnbvEncoderParams.grid_i8: conv1 forward / weight gradient reading the compact int8 copy of the tri-class grid
    ({-1,0,1}: exact conversion) produce the same bits as reading the fp32 observation slice (separate backward
    kernels; the fused data-gradient + weight-gradient kernel sums in another order)."""
    from gennbv_amd.ops.encoder_ops import RowGather
    monkeypatch.setenv("GENNBV_FUSED_BWD", "0")
    _, hip = _pair(g)
    hip.train()
    base = _obs(2 * b, g, seed=3)
    rows = torch.randperm(2 * b, generator=torch.Generator().manual_seed(7 + g))[:b].to(DEV)  # (fixed subset: reproducible)
    grid_i8 = base[:, 600:600 + g ** 3].to(torch.int8).contiguous()
    outs = []
    for gi in (None, grid_i8):
        hip.zero_grad()
        f = hip.features_extractor(RowGather(base, rows, gi))
        f.backward(torch.ones_like(f) * 0.01)
        outs.append((f.detach().clone(), [p.grad.clone() for p in hip.features_extractor.naive_encoder_grid.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, c in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, c)


@pytest.mark.parametrize("g,b,train", [(20, 5, True), (20, 8, False), (33, 3, True), (64, 4, True), (128, 2, True)])
def test_compact_observation_rows_match_flat_rows(g, b, train, monkeypatch):
    """Compact rows ([state | state_rgb] fp32 + the grid as int8 only, obs pointer NULL at the C-ABI): features and
    gradients equal those of the flat fp32 rows -- bit for bit where both take the LDS-staged kernels (G % 16 == 0 and
    the slab fits), to fp32 round-off where the compact rows take the direct int8 kernels (other summation order)."""
    from gennbv_amd.ops.encoder_ops import RowGather, DenseObs
    monkeypatch.setenv("GENNBV_FUSED_BWD", "0")
    _, hip = _pair(g)
    hip.train(train)
    base = _obs(2 * b, g, seed=5)
    rows = torch.randperm(2 * b, generator=torch.Generator().manual_seed(7 + g))[:b].to(DEV)  # (fixed subset: reproducible)
    s0 = 600
    grid_i8 = base[:, s0:s0 + g ** 3].to(torch.int8).contiguous()
    small = torch.cat((base[:, :s0], base[:, s0 + g ** 3:]), dim=1).contiguous()
    compact = RowGather(small, rows, grid_i8, compact_state_dim=s0)
    assert torch.equal(compact.materialize(), base[rows])
    assert torch.equal(DenseObs(small, grid_i8, s0).materialize(), base)
    outs = []
    for obs in (RowGather(base, rows), compact):
        hip.zero_grad()
        with torch.set_grad_enabled(train):
            f = hip.features_extractor(obs)
        if train:
            f.backward(torch.ones_like(f) * 0.01)
        outs.append((f.detach().clone(), [p.grad.clone() for p in hip.features_extractor.naive_encoder_grid.parameters()] if train else []))
    exact = g == 64
    if exact:
        assert torch.equal(outs[0][0], outs[1][0])
    else:
        assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-6), float((outs[0][0] - outs[1][0]).abs().max())
    for a, c in zip(outs[0][1], outs[1][1]):
        if exact:
            assert torch.equal(a, c)
        else:
            assert torch.allclose(a, c, rtol=1e-4, atol=1e-6), float((a - c).abs().max())


@pytest.mark.parametrize("b", [3, 128])
def test_fused_eval_conv1_conv2_vs_fp64_and_the_two_kernel_path(b, monkeypatch):
    """Inference at G = 64 with the grid as int8 rows: k_conv12_fwd_split<false> (conv1 + BN1 + ReLU + conv2 in one launch, the
    layer-1 activations never stored; csrc/conv_split.h) against the fp64 torch modules in eval mode (running statistics) and
    against the two-kernel path (GENNBV_FUSED_EVAL=0: k_conv1_fwd_lds + k_conv2_fwd_split)."""
    from gennbv_amd.ops import encoder_ops
    g = 64
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    seq = hip.features_extractor.naive_encoder_grid
    gen = torch.Generator().manual_seed(7 + b)
    with torch.no_grad():  # non-trivial running statistics
        for bn in (seq[1], seq[4]):
            bn.running_mean.copy_(torch.randn(16, generator=gen) * 0.2)
            bn.running_var.copy_(torch.rand(16, generator=gen) + 0.5)
    n = 2 * b + 1
    grid_i8 = (torch.randint(-1, 2, (n, g ** 3), generator=gen) * (torch.rand(n, g ** 3, generator=gen) < 0.4)).to(torch.int8).to(DEV)
    small = torch.randn(n, 600 + 8192, generator=gen).to(DEV)
    rows = torch.randperm(n, generator=gen)[:b].to(DEV)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GENNBV_FUSED_EVAL", mode)
        with torch.no_grad():
            outs[mode] = encoder_ops.grid_encoder(small, rows, 600, g, seq, False, grid_i8=grid_i8, compact=True).double().cpu()
    import copy
    ref = copy.deepcopy(seq).double().cpu().eval()
    with torch.no_grad():
        want = ref(grid_i8[rows].double().cpu().view(b, 1, g, g, g)).reshape(b, -1)
    scale = float(want.abs().max())
    for mode in ("1", "0"):
        assert float((outs[mode] - want).abs().max()) <= 2e-5 * scale + 1e-6, (mode, float((outs[mode] - want).abs().max()), scale)
    assert float((outs["1"] - outs["0"]).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("b", [2, 128])
def test_conv1_split_kernel_y1_vs_fp64(b, fused, monkeypatch):
    """k_conv1_fwd_split (training-mode conv1 at G = 64 on the f16 pipe: W1 split, int8 input exact; fused = "0") and the y1
    store of k_conv12_fwd_split<true> (fused = "1") against conv3d in fp64: every stored y1 element (the x-parity-split layout,
    padding slot excluded), and against the fp32-MFMA kernel's accuracy."""
    import torch.nn.functional as F
    from gennbv_amd.ops import encoder_ops
    g = 64
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    seq = hip.features_extractor.naive_encoder_grid
    gen = torch.Generator().manual_seed(11 + b)
    n = 2 * b
    grid_i8 = (torch.randint(-1, 2, (n, g ** 3), generator=gen) * (torch.rand(n, g ** 3, generator=gen) < 0.4)).to(torch.int8).to(DEV)
    small = torch.randn(n, 600 + 8192, generator=gen).to(DEV)
    ac = encoder_ops.input_autocorr(grid_i8, g)
    rows = torch.randperm(n, generator=gen)[:b].to(DEV)
    hip.train()
    c1 = seq[0]
    ref = F.conv3d(grid_i8[rows].double().cpu().view(b, 1, g, g, g), c1.weight.double().cpu(), c1.bias.double().cpu(), stride=2)
    errs = {}
    monkeypatch.setenv("GENNBV_FUSED_TRAIN", fused)
    for mode in ("1", "0"):
        monkeypatch.setenv("GENNBV_CONV1_SPLIT", mode)
        f = encoder_ops.grid_encoder(small, rows, 600, g, seq, True, grid_i8=grid_i8, compact=True, autocorr=ac)
        y = f.grad_fn.saved_tensors[2].detach().cpu().view(b, 31, 31, 2, 16, 16)
        full = torch.zeros(b, 31, 31, 32, 16)
        full[:, :, :, 0::2] = y[:, :, :, 0]
        full[:, :, :, 1::2] = y[:, :, :, 1]
        errs[mode] = float((full[:, :, :, :31].permute(0, 4, 1, 2, 3).double() - ref).abs().max())
    scale = float(ref.abs().max())
    assert errs["1"] <= 2e-6 * scale and errs["1"] <= 2.0 * errs["0"] + 1e-7, (errs, scale)


@pytest.mark.parametrize("b", [3, 128])
def test_fused_train_forward_vs_the_two_kernel_path(b, monkeypatch):
    """Training forward at G = 64 with BN1's statistics known beforehand (input autocorrelation): k_conv12_fwd_split<true>
    (conv1 + BN1 + ReLU + conv2 in one launch that also stores y1 and the BN2 partial sums; csrc/conv_split.h) against
    GENNBV_FUSED_TRAIN=0 (k_conv1_fwd_split + k_conv2_fwd_split): y1 wherever a voxel exists, y2, the BatchNorm
    state (scale / shift / mean / rstd of both layers), the running statistics and the features within fp32 round-off; then the
    gradients of a random cotangent through both (same backward kernels, fed by either forward)."""
    import copy
    from gennbv_amd.ops import encoder_ops
    g = 64
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    gen = torch.Generator().manual_seed(23 + b)
    n = 2 * b + 1
    grid_i8 = (torch.randint(-1, 2, (n, g ** 3), generator=gen) * (torch.rand(n, g ** 3, generator=gen) < 0.4)).to(torch.int8).to(DEV)
    small = torch.randn(n, 600 + 8192, generator=gen).to(DEV)
    ac = encoder_ops.input_autocorr(grid_i8, g)
    rows = torch.randperm(n, generator=gen)[:b].to(DEV)
    cot = torch.randn(b, 16 * 15 ** 3, generator=gen).to(DEV)
    hip.train()
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GENNBV_FUSED_TRAIN", mode)
        seq = copy.deepcopy(hip.features_extractor.naive_encoder_grid)
        f = encoder_ops.grid_encoder(small, rows, 600, g, seq, True, grid_i8=grid_i8, compact=True, autocorr=ac)
        _, _, y1, y2, bn_state, _, _ = f.grad_fn.saved_tensors
        y1 = y1.detach().clone().view(b, 31, 31, 2, 16, 16)[:, :, :, :, :, :]
        y1[:, :, :, 1, 15] = 0  # x = 31 does not exist (padding slot of the odd-x half row)
        (f * cot).sum().backward()
        res[mode] = dict(f=f.detach().clone(), y1=y1, y2=y2.detach().clone(), bn=bn_state.detach().clone()[:128],
                         rm=[seq[1].running_mean.clone(), seq[1].running_var.clone(), seq[4].running_mean.clone(), seq[4].running_var.clone()],
                         grads=[q.grad.clone() for q in seq.parameters()])
    a, c = res["1"], res["0"]
    # (the fused kernel contracts the 27 taps in another order than k_conv1_fwd_split: last-bit differences)
    assert float((a["y1"] - c["y1"]).abs().max()) <= 1e-6 * float(c["y1"].abs().max()), float((a["y1"] - c["y1"]).abs().max())
    s2 = float(c["y2"].abs().max())
    assert float((a["y2"] - c["y2"]).abs().max()) <= 2e-6 * s2, float((a["y2"] - c["y2"]).abs().max()) / s2
    assert torch.allclose(a["bn"], c["bn"], rtol=1e-5, atol=1e-6)
    for u, v in zip(a["rm"], c["rm"]):
        assert torch.allclose(u, v, rtol=1e-5, atol=1e-7)
    assert float((a["f"] - c["f"]).abs().max()) <= 1e-5 * float(c["f"].abs().max())
    # the two forwards' y2 differ in the last bit, so a BN2 output within round-off of zero may sit on different sides of the ReLU
    # (a knife-edge element: |feature| ~ 1e-7) and moves the small per-channel sums by its whole cotangent -- such elements are
    # counted and must be few and tiny; the gradients are compared when there are none
    flips = (a["f"] > 0) != (c["f"] > 0)
    nflip = int(flips.sum())
    assert nflip <= 4 and (nflip == 0 or float(torch.maximum(a["f"], c["f"])[flips].max()) <= 1e-5 * float(c["f"].abs().max())), nflip
    if nflip == 0:
        # (the conv biases sit in front of a training-mode BatchNorm: their gradients are analytically zero, what is computed is
        # round-off of sums of the size of the other gradients -- hence the absolute term on the global scale)
        top = max(float(v.abs().max()) for v in c["grads"])
        for u, v in zip(a["grads"], c["grads"]):
            assert float((u - v).abs().max()) <= 2e-4 * float(v.abs().max()) + 2e-6 * top, (u.shape, float((u - v).abs().max()), float(v.abs().max()), top)



@pytest.mark.parametrize("g,b", [(16, 8), (64, 4)])
def test_semantic_branch_forward_backward_vs_fp64(g, b):
    """SURVEY 8f.4 / BASELINE configs[2] (opt-in, build-defined: the released reference never reads obs["state_rgb"]): the two
    64 x 64 gray frames -> 8 x 8 patch embeddings -> 256 features in front of output_layer (768 inputs), on the split-K linear
    kernels and the fused policy head with K2 = 512.  Reference = the same modules in fp64 on the CPU; flat rows and gathered
    compact rows; the default (branch off) keeps the reference's state_dict."""
    from gennbv_amd.ops.encoder_ops import RowGather, input_autocorr
    torch.manual_seed(1000 + g)  # (random initialisation: seeded, so that the ReLU-threshold probe below sees the same weights every run)
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=False, semantic_branch=True)
    ref, _, _ = pu.make_policy(g=g, device="cpu", backend="torch", det_weights=False, semantic_branch=True)
    plain, _, _ = pu.make_policy(g=g, device="cpu", backend="torch", det_weights=False)
    extra = set(ref.state_dict()) - set(plain.state_dict())
    assert extra == {f"features_extractor.{k}" for k in ("naive_encoder_rgb.0.weight", "naive_encoder_rgb.0.bias", "output_layer_rgb.0.weight", "output_layer_rgb.0.bias")}
    hip.load_state_dict({k: v.to(DEV) for k, v in ref.state_dict().items()})
    ref = ref.double()
    ref.extract_features = lambda x: ref.features_extractor(x)
    obs = _obs_clear_of_the_relu_threshold(ref, b, g)  # (the grid branch does not see the gray frames: the probe stays valid)
    gen = torch.Generator().manual_seed(g)
    obs[:, 600 + g ** 3:] = (torch.rand(b, 8192, generator=gen) * 255.0).round().to(DEV)  # gray values as the env writes them
    rows = torch.randperm(b, generator=gen).to(DEV)
    actions = torch.stack([torch.randint(0, n, (b,), generator=gen) for n in pu.NVEC], -1).float()
    w = torch.linspace(0.5, 1.5, b)
    grid_i8 = obs[:, 600:600 + g ** 3].to(torch.int8).contiguous()
    small = torch.cat((obs[:, :600], obs[:, 600 + g ** 3:]), 1).contiguous()
    inputs = {"flat": obs[rows], "compact": RowGather(small, rows, grid_i8, 600, input_autocorr(grid_i8, g) if g % 16 == 0 else None)}
    res = {}
    for name, (pol, x, dev, dt) in {"ref": (ref, obs[rows].cpu().double(), "cpu", torch.float64), "flat": (hip, inputs["flat"], DEV, torch.float32),
                                     "compact": (hip, inputs["compact"], DEV, torch.float32)}.items():
        pol.set_training_mode(True)
        pol.zero_grad()
        values, log_prob, entropy = pol.evaluate_actions(x, actions.to(dev))
        ww = w.to(dev, dt)
        ((values.flatten() * ww).sum() + (log_prob * ww.flip(0)).sum() + 0.3 * (entropy * ww).sum()).backward()
        res[name] = ([t.detach().double().cpu() for t in (values, log_prob, entropy)],
                     {k: p.grad.detach().double().cpu().clone() for k, p in pol.named_parameters() if p.grad is not None})
    for name in ("flat", "compact"):
        for x, y in zip(res["ref"][0], res[name][0]):
            assert float((x - y).abs().max()) <= 2e-5 * float(x.abs().max()) + 1e-6, name
        for k, r in res["ref"][1].items():
            scale = float(r.abs().max())
            if scale > 1e-9 and ("rgb" in k or "output_layer." in k or "action_net" in k or "value_net" in k):
                err = float((r - res[name][1][k]).abs().max())
                assert err <= 2e-5 * scale, (name, k, err, scale)
    assert float(res["ref"][1]["features_extractor.naive_encoder_rgb.0.weight"].abs().max()) > 0


@pytest.mark.parametrize("g,b,train", [(64, 4, True), (64, 128, True), (64, 37, False), (128, 1, True)])
def test_bn2_relu_folded_into_fc_grid_is_bit_identical(g, b, train, monkeypatch):
    """Round 3: fc_grid's kernels form relu(bn2(y2)) in their operand loads (gnbv_linear_forward_fold / gnbv_linear_bwd_dw_fold)
    instead of reading a materialised feature tensor (`lin._no_fold`: k_bn_relu_apply + the plain entry points).  Same fp32
    fma + max, same split-f16 product: every output and every gradient must be IDENTICAL, bit for bit.  (One exception: batches the
    hand-written backward does not take -- M % 16 != 0 -- form the activations in torch for the library GEMM, a multiply and an add
    instead of one fma: fc_grid's weight gradient then agrees to an ulp of its operands.)"""
    from gennbv_amd.ops import encoder_ops as eo
    outs = []
    for fold in ("1", "0"):
        hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
        enc = hip.features_extractor
        enc.output_layer_grid[0]._no_fold = fold == "0"
        assert eo.linear_fold_ok(enc.output_layer_grid[0], b, eo.conv_out(eo.conv_out(g)) ** 3, False) == (fold == "1")
        obs = _obs(b, g, seed=5)
        hip.set_training_mode(train)
        if train:
            hip.zero_grad()
            f = enc(obs)
            (f * torch.linspace(0.5, 1.5, f.shape[1], device=DEV)).sum().backward()
            names = ["features"] + [n for n, _ in enc.named_parameters()] + [k for k in enc.state_dict() if "running" in k]
            outs.append([f.detach().clone()] + [p.grad.detach().clone() for p in enc.parameters()]
                        + [v.clone() for k, v in enc.state_dict().items() if "running" in k])
        else:
            names = ["features"]
            with torch.no_grad():
                outs.append([enc(obs).clone()])
        assert int(enc._range_flag.item()) == 0
    assert len(outs[0]) == len(outs[1]) == len(names)
    for n, a, r in zip(names, *outs):
        if n == "output_layer_grid.0.weight" and b % 16:
            assert float((a - r).abs().max()) <= 2e-7 * float(r.abs().max()), n
        else:
            assert torch.equal(a, r), n


@pytest.mark.parametrize("b", [3, 128])
def test_wgrad_lds_dma_transport_is_bit_identical(b, monkeypatch):
    """k_conv2_wgrad_split_dma (round 6): y1 / dy2 reach the ring by LDS-DMA requests and are converted in place -- the same arithmetic in the
    same order as the register-staged k_conv2_wgrad_split, so every conv / BN gradient must be BIT-identical (b = 3: a sample's last
    plane group has three planes; 128: the bench's minibatch, two full rounds of workgroups)."""
    from gennbv_amd.ops.encoder_ops import RowGather, input_autocorr
    g = 64
    hip, _, _ = pu.make_policy(g=g, device=DEV, backend="hip", det_weights=True)
    base = _obs(b + 2, g, seed=7)
    rows = torch.randperm(b + 2, generator=torch.Generator().manual_seed(5))[:b].to(DEV)
    grid_i8 = base[:, 600:600 + g ** 3].to(torch.int8).contiguous()
    ac = input_autocorr(grid_i8, g)
    w = torch.linspace(0.5, 1.5, 256).to(DEV)
    hip.train()
    grads = {}
    monkeypatch.setenv("GENNBV_CONV_MAXWG", "512")  # one item per workgroup, as the register-staged kernel has them: same grouping of the sums
    for mode in ("0", "1", "0", "1 with two items per workgroup"):
        monkeypatch.setenv("GENNBV_WGRAD_DMA", mode[0])
        if len(mode) > 1:
            monkeypatch.setenv("GENNBV_CONV_MAXWG", "")  # the default: 256 workgroups walk the 512 items of the bench's minibatch
        hip.zero_grad()
        f = hip.features_extractor(RowGather(base, rows, grid_i8, autocorr=ac))
        (f * w).sum().backward()
        torch.cuda.synchronize()
        cur = [p.grad.detach().clone() for p in hip.features_extractor.naive_encoder_grid.parameters()]
        if mode in grads:  # (the register-staged kernel reproduces itself: the comparison below is meaningful)
            assert all(torch.equal(a, c) for a, c in zip(grads[mode], cur))
        grads[mode] = cur
    assert float(grads["0"][2].abs().max()) > 0  # conv2.weight's gradient
    for a, c in zip(grads["0"], grads["1"]):
        assert torch.equal(a, c)
    # two items per workgroup: a partial row then sums two items in fp32 before the fp64 reduction -- fp32 round-off of ONE extra addition
    # (the conv biases in front of BatchNorm have an analytically zero gradient: what they hold is the rounding noise of a sum of B * O^3 terms,
    # ~2e-4 at this batch, and regrouping the sum moves it by a tenth of that -- the same floor the fp64 comparisons above grant them)
    for (name, _), a, c in zip(hip.features_extractor.naive_encoder_grid.named_parameters(), grads["0"], grads["1 with two items per workgroup"]):
        floor = 1e-4 * max(1.0, b / 8) if name in ("0.bias", "3.bias") else 1e-9
        assert float((a - c).abs().max()) <= 2e-6 * float(a.abs().max()) + floor, name
