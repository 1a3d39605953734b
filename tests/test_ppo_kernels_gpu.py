"""GPU: csrc/ppo.hip's minibatch loss (gnbv_ppo_loss / _finish, gnbv_gather_minibatch), clip + Adam step (gnbv_clip_adam_step_ex,
gnbv_adam_shard_step, gnbv_sq_partials) and rollout sampler (gnbv_multicategorical_sample), called through the C ABI and compared
with fp64 torch on the GPU.  Outputs are NaN-prefilled and followed by a sentinel tail that must stay untouched.

Error model (u = 2^-24; every bound is carried elementwise in fp64 from the magnitudes of the reference's own terms, and the
derived part is doubled, SAFETY).  Every case prints its largest err / bound ratio and asserts it is <= 1.
* Loss.  Per head of n categories, lse = mx + log(sum exp(x - mx)) is off by
      d_lse <= u (|lse| + |mx| + 2 sum p |x - mx| + ceil(n/64) + 12)
  (the shifted logits, each off by u |x - mx|, weighted by their share of the sum; expf / logf; the lane-serial sums and the
  6-stage butterfly); lp = x - lse: d_lp <= d_lse + u |lp|;
  p = exp(lp): d_p <= p (d_lp + 2u) + 2^-126 (underflow); H = -sum p lp: d_H <= sum(d_p |lp| + p d_lp) + (ceil(n/64) + 8) u
  sum p |lp|.  The log-ratio, the ratio, the normalised advantage (its mean / std add (ceil(B/64) + 8) u of their sums) and the
  surrogate's factor gl carry these forward to first order; d logits = gl (onehot - p) + (c_e/B) p (lp + H) then is off by
  |d gl| |onehot - p| + |gl| d_p + (c_e/B)(d_p |lp + H| + p (d_lp + d_H)) + 4u of each term.  A logged statistic adds the
  mean per-sample error plus (ceil(B/256) + 10) u of the mean |term|.  Random inputs stay >= 1e-3 away from every clip boundary,
  where the reference's gradient is discontinuous; the cases built exactly on a boundary check torch's clamp semantics there.
* Clip + Adam.  Before every step the reference copies the kernel's fp32 state and takes ONE fp64 step with the fp32 values of
  the hyperparameters.  norm_out[0] (fp64 sum, one rounding) is within 1 ulp of the fp64 norm, the factor norm_out[1] within
  3 ulp; exp_avg within 8u (|m'| + (1 - b1)(|g c| + |m|)), exp_avg_sq within 16u v' (a sum of non-negative terms); a parameter
  within 2 ulp(p) + 16u lr/(1 - b1^t) (|m'| + (1 - b1)(|g c| + |m|)) / (sqrt(v')/sqrt(1 - b2^t) + eps) -- the magnitude of the
  update's terms: its relative sensitivity to v is at most 1/2, so this holds where sqrt(v') is near eps too.
* Sampler.  The kernel's prefix sums of exp(x - mx) and their total are off by (2 ceil(n/64) + 16) u of the total: an action
  is accepted when it has non-zero mass and u lies in [CDF_(a-1), CDF_a) widened by that margin (fp64 CDF).  The row's
  log-prob (sum of x_a - lse per head) is off by sum_h (d_lse + u |lp_a|) + n_heads u sum |lp_a|.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from gennbv_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TINY = 2.0 ** -126
SAFETY = 2.0
TAIL, SENTINEL = 64, 1234.5
F64 = torch.float64

SIX = [81, 81, 51, 1, 13, 13]  # the reference's action lattice
SMALL6 = [7, 5, 3, 1, 4, 2]
FIVE = [128, 65, 1, 64, 3]
EIGHT = [3, 1, 128, 7, 64, 2, 13, 5]  # kMaxHeads


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _out(*shape, dtype=torch.float32, fill=float("nan")):
    """An output buffer prefilled with `fill` and followed by a TAIL-element sentinel: (the output view, the whole buffer)."""
    n = math.prod(shape)
    buf = torch.full((n + TAIL,), fill, dtype=dtype, device=DEV)
    buf[n:] = SENTINEL
    return buf[:n].view(*shape), buf


def _check_written(name, body, buf):
    n = body.numel()
    bad = int((~torch.isfinite(body)).sum()) if body.is_floating_point() else 0
    assert bad == 0, f"{name}: {bad} of {n} elements not written or not finite"
    assert bool((buf[n:] == SENTINEL).all()), f"{name}: the {TAIL} elements past the output were written"


def _ratio(got, want, bound):
    """Largest |got - want| / bound (an element whose bound is 0 must be exact)."""
    err = (got.double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=F64, device=err.device).expand_as(err)
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


def _report(what, ratios):
    line = f"[err/bound] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
    print(line)
    assert max(ratios.values()) <= 1.0, line
    return line


def _ulp(x):
    """Spacing of fp32 numbers at |x| (fp64 tensor in, fp64 tensor out; 2^-149 at 0)."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23.0)


def _heads(x, dims):
    """fp64 statistics of every head of the logits x [B, sum(dims)]: list of (off, n, mx, lse, lp, p, H, d_lse, d_lp, d_p, d_H)."""
    out, off = [], 0
    for n in dims:
        xs = x[:, off:off + n].double()
        mx = xs.amax(1)
        lse = torch.logsumexp(xs, 1)
        lp = xs - lse[:, None]
        p = lp.exp()
        H = -(p * lp).sum(1)
        k = math.ceil(n / 64)
        d_lse = U * (lse.abs() + mx.abs() + 2 * (p * (xs - mx[:, None]).abs()).sum(1) + k + 12)
        d_lp = d_lse[:, None] + U * lp.abs()
        d_p = p * (d_lp + 2 * U) + TINY
        d_H = (d_p * lp.abs() + p * d_lp).sum(1) + (k + 8) * U * (p * lp.abs()).sum(1)
        out.append(dict(off=off, n=n, mx=mx, lse=lse, lp=lp, p=p, H=H, d_lse=d_lse, d_lp=d_lp, d_p=d_p, d_H=d_H))
        off += n
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the fused loss
# ---------------------------------------------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, norm=True, adv_norm=False, clip=0.2, clip_vf=0.2, ent_coef=0.01, vf_coef=0.8, policy_scale=10.0,
                 target_kl=-1.0, heads_out=True, generic=False, peaked=False, edges=False):
        self.norm, self.adv_norm, self.heads_out, self.generic, self.peaked, self.edges = norm, adv_norm, heads_out, generic, peaked, edges
        self.clip, self.clip_vf, self.ent_coef = _f32(clip), _f32(clip_vf), _f32(ent_coef)
        self.vf_coef, self.policy_scale, self.target_kl = _f32(vf_coef), _f32(policy_scale), _f32(target_kl)
        one = torch.tensor(1.0, dtype=torch.float32)
        self.lo = float(one - torch.tensor(self.clip, dtype=torch.float32))  # the kernel's 1.0f - clip_range
        self.hi = float(one + torch.tensor(self.clip, dtype=torch.float32))


def _away(x, edges, margin=2e-3):
    """x moved >= margin / 2 away from every value in `edges` (the reference's gradient is discontinuous there)."""
    for e in edges:
        near = (x - e).abs() < margin
        x = torch.where(near, e + torch.where(x >= e, 1.0, -1.0) * 2 * margin, x)
    return x


def _loss_inputs(dims, B, cfg, seed):
    """fp32 inputs of one minibatch; log-ratios and value differences placed away from the clip boundaries (cfg.edges: the
    extremes -- log-ratios of +-5, zero advantages, value differences exactly on the value clip)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    n = sum(dims)
    scale = 40.0 if cfg.peaked else 2.0
    logits = (torch.randn(B, n, generator=gen, device=DEV, dtype=F64) * scale).float()
    values = torch.randn(B, generator=gen, device=DEV).float()
    actions = torch.stack([torch.randint(0, d, (B,), generator=gen, device=DEV) for d in dims], 1).float()
    adv = (torch.randn(B, generator=gen, device=DEV) * 2 + 0.5).float()
    ret = torch.randn(B, generator=gen, device=DEV).float()
    logp = sum(h["lp"].gather(1, actions[:, i:i + 1].long()).squeeze(1) for i, h in enumerate(_heads(logits, dims)))
    lr = torch.rand(B, generator=gen, device=DEV, dtype=F64) - 0.5
    lr = _away(lr, [math.log(cfg.lo), math.log(cfg.hi)], 2e-2 if cfg.peaked else 2e-3)
    dv = torch.rand(B, generator=gen, device=DEV, dtype=F64) * 0.8 - 0.4
    if cfg.clip_vf > 0:
        dv = _away(dv, [-cfg.clip_vf, cfg.clip_vf])
    adv_norm = None
    if cfg.adv_norm:
        adv_norm = torch.tensor([0.25, _f32(1.0 / (1.7 + 1e-8))], dtype=torch.float32, device=DEV)
    if cfg.edges:
        lr[0::5] = 5.0
        lr[1::5] = -5.0
        if not cfg.norm:
            adv[2::5] = 0.0
        elif cfg.adv_norm:
            adv[2::5] = 0.25  # (A - mean) == 0 exactly
    old_lp = (logp - lr).float()
    old_values = (values.double() - dv).float()
    if cfg.edges and cfg.clip_vf > 0:
        # exactly on the value clip (both signs): torch's clamp passes the gradient there
        b = cfg.clip_vf
        values[3::5], old_values[3::5] = 1.0 + b, 1.0
        values[4::5], old_values[4::5] = 1.0 - b, 1.0
        assert float(torch.tensor(1.0 + b, dtype=torch.float32) - 1.0) == b
    return dict(logits=logits.contiguous(), values=values.contiguous(), actions=actions.contiguous(), old_values=old_values.contiguous(),
                old_log_prob=old_lp.contiguous(), advantages=adv.contiguous(), returns=ret.contiguous(), adv_norm=adv_norm)


def _loss_struct(dims, B, cfg, x, rows=None, defer=0, kl_out=None, stats_rows=4, stop=None, stats=None, stats_row=None):
    """A GnbvPpoLoss over fresh NaN-prefilled outputs; returns (struct, outputs dict, keepalive)."""
    nh = len(dims)
    o = {}
    o["d_logits"] = _out(B, sum(dims))
    o["d_values"] = _out(B)
    if cfg.heads_out:
        o["head_entropy"] = _out(B, nh)
        o["head_lse"] = _out(B, nh)
    o["stats"] = stats if stats is not None else _out(stats_rows, 8)
    o["stats_row"] = stats_row if stats_row is not None else torch.zeros(1, dtype=torch.int64, device=DEV)
    o["stop_flag"] = stop if stop is not None else torch.zeros(1, dtype=torch.int32, device=DEV)
    o["scratch"] = torch.zeros(8 * B + 64, dtype=torch.float32, device=DEV)
    a = _lib.GnbvPpoLoss()
    a.batch, a.n_logits, a.n_heads = B, sum(dims), nh
    for h, d in enumerate(dims):
        a.head_dims[h] = d
    a.normalize_advantage = int(cfg.norm)
    a.clip_range, a.clip_range_vf, a.ent_coef = cfg.clip, cfg.clip_vf, cfg.ent_coef
    a.vf_coef, a.policy_scale, a.target_kl = cfg.vf_coef, cfg.policy_scale, cfg.target_kl
    for k in ("logits", "values", "actions", "old_values", "old_log_prob", "advantages", "returns"):
        setattr(a, k, x[k].data_ptr())
    a.d_logits, a.d_values = o["d_logits"][0].data_ptr(), o["d_values"][0].data_ptr()
    a.head_entropy = o["head_entropy"][0].data_ptr() if cfg.heads_out else None
    a.head_lse = o["head_lse"][0].data_ptr() if cfg.heads_out else None
    a.stats, a.stats_row = o["stats"][0].data_ptr(), o["stats_row"].data_ptr()
    a.stop_flag = o["stop_flag"].data_ptr()
    a.scratch = o["scratch"].data_ptr()
    a.kl_out = _lib.ptr(kl_out)
    a.rows = _lib.ptr(rows)
    a.adv_norm = _lib.ptr(x["adv_norm"]) if cfg.norm else None
    a.defer_stats = int(defer)
    return a, o


def _run_loss(a, monkeypatch=None, generic=False):
    lib = _lib.load()
    if monkeypatch is not None:
        monkeypatch.setenv("GENNBV_PPO_GENERIC", "1" if generic else "0")
    _lib.check(lib.gnbv_ppo_loss(C.byref(a), _stream()), "gnbv_ppo_loss")
    torch.cuda.synchronize()


def _loss_ref(dims, cfg, x):
    """The reference's loss (ppo_grid_obs.py:209-262) in fp64, its gradients by autograd, the six statistics, and the error model's
    bounds for each of them."""
    from gennbv_amd.sb3.distributions import MultiCategoricalDistribution
    B = x["logits"].shape[0]
    logits = x["logits"].double().requires_grad_()
    values = x["values"].double().requires_grad_()
    acts, old_lp, old_v = x["actions"].double(), x["old_log_prob"].double(), x["old_values"].double()
    A, ret = x["advantages"].double(), x["returns"].double()
    dist = MultiCategoricalDistribution(dims).proba_distribution(logits)
    log_prob, entropy = dist.log_prob(acts), dist.entropy()
    if cfg.norm and x["adv_norm"] is not None:
        m, inv = (float(v) for v in x["adv_norm"].double())
        adv = (A - m) * inv
    elif cfg.norm:
        adv = (A - A.mean()) / (A.std() + 1e-8)
    else:
        adv = A
    ratio = torch.exp(log_prob - old_lp)
    pg = -torch.min(adv * ratio, adv * torch.clamp(ratio, cfg.lo, cfg.hi)).mean()
    vp = old_v + torch.clamp(values - old_v, -cfg.clip_vf, cfg.clip_vf) if cfg.clip_vf > 0 else values
    vl = torch.nn.functional.mse_loss(ret, vp)
    el = -entropy.mean()
    loss = cfg.policy_scale * pg + cfg.ent_coef * el + cfg.vf_coef * vl
    loss.backward()
    lr = (log_prob - old_lp).detach()
    ratio = ratio.detach()
    kl = ((torch.exp(lr) - 1) - lr).mean()
    cf = ((ratio - 1).abs() > cfg.clip).double().mean()
    ref = dict(d_logits=logits.grad, d_values=values.grad,
               stats=torch.stack([pg.detach(), vl.detach(), el.detach(), kl, cf, loss.detach()]))

    # ---- the error model ----
    hs = _heads(x["logits"], dims)
    ref["head_entropy"] = torch.stack([h["H"] for h in hs], 1)
    ref["head_lse"] = torch.stack([h["lse"] for h in hs], 1)
    nh = len(dims)
    lp_a = [h["lp"].gather(1, acts[:, i:i + 1].long()).squeeze(1) for i, h in enumerate(hs)]
    d_logp = sum(h["d_lse"] for h in hs) + (nh + 1) * U * sum(v.abs() for v in lp_a)
    ent = sum(h["H"] for h in hs)
    d_ent = sum(h["d_H"] for h in hs) + nh * U * sum(h["H"].abs() for h in hs)
    d_lr = d_logp + U * lr.abs()
    d_ratio = ratio * (d_lr + 2 * U)
    adv = adv.detach()
    if not cfg.norm:
        d_adv = torch.zeros_like(A)
    elif x["adv_norm"] is not None:
        d_adv = 2 * U * adv.abs()
    else:
        kb = math.ceil(B / 64) + 8
        mean = A.mean()
        d_mean = kb * U * A.abs().mean() + U * mean.abs()
        q = ((A - mean) ** 2).sum()
        d_q = 2 * kb * U * q + 2 * d_mean * (A - mean).abs().sum()
        inv = 1.0 / (torch.sqrt(q / max(B - 1, 1)) + 1e-8)
        d_inv = d_q / (2 * q) + 4 * U
        d_adv = d_mean * inv + U * (A - mean).abs() * inv + adv.abs() * (d_inv + U)
    rc = ratio.clamp(cfg.lo, cfg.hi)
    s1, s2 = adv * ratio, adv * rc
    g1 = (s1 < s2).double() + 0.5 * (s1 == s2).double()
    inrange = ((ratio >= cfg.lo) & (ratio <= cfg.hi)).double()
    w = g1 + (1 - g1) * inrange
    ps, e = cfg.policy_scale, cfg.ent_coef / B
    gl = -(ps / B) * adv * ratio * w
    d_gl = (ps / B) * w * (adv.abs() * d_ratio + ratio * d_adv) + 6 * U * gl.abs()
    bl = []
    for i, h in enumerate(hs):
        oh = torch.nn.functional.one_hot(acts[:, i].long(), h["n"]).double()
        lpH = h["lp"] + h["H"][:, None]
        t1, t2 = gl[:, None] * (oh - h["p"]), e * h["p"] * lpH
        bl.append(d_gl[:, None] * (oh - h["p"]).abs() + gl.abs()[:, None] * h["d_p"]
                  + e * (h["d_p"] * lpH.abs() + h["p"] * (h["d_lp"] + h["d_H"][:, None])) + 4 * U * (t1.abs() + t2.abs()))
    bound = dict(d_logits=torch.cat(bl, 1), head_entropy=torch.stack([h["d_H"] for h in hs], 1),
                 head_lse=torch.stack([h["d_lse"] for h in hs], 1))
    v, vo = x["values"].double(), old_v
    if cfg.clip_vf > 0:
        dv = v - vo
        vpx = vo + dv.clamp(-cfg.clip_vf, cfg.clip_vf)
        err = vpx - ret
        d_err = U * (dv.abs() + vpx.abs() + err.abs())
        dvp = ((dv >= -cfg.clip_vf) & (dv <= cfg.clip_vf)).double()
    else:
        err = v - ret
        d_err = U * err.abs()
        dvp = torch.ones_like(v)
    kv = cfg.vf_coef * 2.0 / B
    bound["d_values"] = kv * dvp * d_err + 5 * U * (kv * err * dvp).abs()
    t = [-torch.min(s1, s2), err * err, -ent, (ratio - 1) - lr]
    dt = [adv.abs() * d_ratio + torch.maximum(ratio, rc) * d_adv + U * t[0].abs(), 2 * err.abs() * d_err + U * t[1],
          d_ent, d_ratio + d_lr + U * ((ratio - 1).abs() + t[3].abs())]
    S = math.ceil(B / 256) + 10
    sb = [dt[k].mean() + S * U * t[k].abs().mean() + U * t[k].mean().abs() for k in range(4)]
    sb.append(2 * U * cf)
    sb.append(ps * sb[0] + cfg.ent_coef * sb[2] + cfg.vf_coef * sb[1]
              + 3 * U * (abs(ps * pg.detach()) + abs(cfg.ent_coef * el.detach()) + abs(cfg.vf_coef * vl.detach())))
    bound["stats"] = torch.stack([torch.as_tensor(s, dtype=F64, device=DEV) for s in sb])
    # the inputs must keep their distance from the clip boundaries (cases built on one on purpose excepted)
    far = (ratio - cfg.lo).abs().minimum((ratio - cfg.hi).abs()) > 10 * d_ratio
    assert bool(far.all()), "a sample's ratio is within the error model of a clip boundary"
    return ref, bound


LOSS_CASES = [
    ("six-B2", SIX, 2, {}), ("six-B3", SIX, 3, {}), ("six-B5", SIX, 5, {}), ("six-B128", SIX, 128, {}),
    ("six-B300", SIX, 300, {}), ("six-B1030", SIX, 1030, {}),
    ("six-B128-runtime", SIX, 128, dict(generic=True)),
    ("six-B128-nonorm-novf", SIX, 128, dict(norm=False, clip_vf=-1.0)),
    ("six-B128-advnorm", SIX, 128, dict(adv_norm=True)),
    ("six-B128-peaked-edges", SIX, 128, dict(peaked=True, edges=True, norm=False, clip_vf=0.25)),
    ("six-B300-edges-advnorm", SIX, 300, dict(edges=True, adv_norm=True, clip_vf=0.25)),
    ("six-B5-noheads", SIX, 5, dict(heads_out=False)),
    ("small6-B3-runtime", SMALL6, 3, dict(generic=True)), ("small6-B300", SMALL6, 300, dict(norm=False)),
    ("small6-B128-runtime-novf", SMALL6, 128, dict(generic=True, clip_vf=-1.0)),
    ("five-B5", FIVE, 5, {}), ("five-B128-advnorm-novf", FIVE, 128, dict(adv_norm=True, clip_vf=-1.0)),
    ("five-B1030-peaked-edges", FIVE, 1030, dict(peaked=True, edges=True, norm=False, clip_vf=0.25)),
    ("mem3-B5", [200, 1, 65], 5, {}), ("mem3-B128", [200, 1, 65], 128, dict(norm=False)),
    ("mem3-B300-peaked-edges", [200, 1, 65], 300, dict(peaked=True, edges=True, adv_norm=True, clip_vf=0.25)),
    ("mem1-B2", [129], 2, {}), ("mem1-B1030", [129], 1030, dict(clip_vf=-1.0)),
    ("eight-B128", EIGHT, 128, {}), ("eight-B1030-advnorm", EIGHT, 1030, dict(adv_norm=True)),
    ("eight-B300-peaked-edges", EIGHT, 300, dict(peaked=True, edges=True, norm=False, clip_vf=0.25)),
    ("one-B2", [13], 2, {}), ("one-B300-peaked", [81], 300, dict(peaked=True, norm=False)),
    ("one-B5-single", [1], 5, {}),
]


@pytest.mark.parametrize("name,dims,B,kw", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_ppo_loss_vs_fp64_autograd(name, dims, B, kw, monkeypatch):
    """gnbv_ppo_loss's d loss / d logits, d loss / d values, per-head entropy / log-sum-exp and statistics row against fp64 autograd
    of the reference's expressions, elementwise within the error model."""
    cfg = Cfg(**kw)
    x = _loss_inputs(dims, B, cfg, seed=B * 31 + sum(dims) + len(name))
    a, o = _loss_struct(dims, B, cfg, x)
    _run_loss(a, monkeypatch, cfg.generic)
    for k in ("d_logits", "d_values") + (("head_entropy", "head_lse") if cfg.heads_out else ()):
        _check_written(k, *o[k])
    st, sbuf = o["stats"]
    assert bool(torch.isfinite(st[0]).all()), st[0]
    assert bool(torch.isnan(st[1:]).all()), "statistics rows behind the current one were written"
    assert bool((sbuf[st.numel():] == SENTINEL).all())
    assert int(o["stats_row"]) == 1 and int(o["stop_flag"]) == 0
    assert float(st[0, 6]) == 1.0 and float(st[0, 7]) == 0.0
    ref, bound = _loss_ref(dims, cfg, x)
    ratios = {k: _ratio(o[k][0], ref[k], SAFETY * bound[k]) for k in ("d_logits", "d_values")}
    if cfg.heads_out:
        ratios.update({k: _ratio(o[k][0], ref[k], SAFETY * bound[k]) for k in ("head_entropy", "head_lse")})
    ratios["stats"] = _ratio(st[0, :6], ref["stats"], SAFETY * bound["stats"])
    _report(f"loss {name}", ratios)


@pytest.mark.parametrize("dims", [SIX, [200, 1, 65]], ids=["six", "mem3"])
def test_fused_gather_rows_is_bit_identical_to_gather_then_loss(dims, monkeypatch):
    """`rows` over whole rollout arrays with a permutation == gnbv_gather_minibatch (which must equal torch indexing exactly) followed
    by the call without `rows`: the same gradient, per-head and statistics bits."""
    lib = _lib.load()
    B, T = 128, 5
    cfg = Cfg()
    gen = torch.Generator(device=DEV).manual_seed(7)
    roll = _loss_inputs(dims, B * T, cfg, seed=11)
    rows = torch.randperm(B * T, generator=gen, device=DEV)[:B].contiguous()
    mb = dict(logits=roll["logits"][:B].contiguous(), values=roll["values"][:B].contiguous(), adv_norm=None)
    # gather
    g = {k: _out(*s) for k, s in (("actions", (B, len(dims))), ("old_values", (B,)), ("old_log_prob", (B,)), ("advantages", (B,)),
                                  ("returns", (B,)))}
    _lib.check(lib.gnbv_gather_minibatch(rows.data_ptr(), B, len(dims), roll["actions"].data_ptr(), roll["old_values"].data_ptr(),
                                         roll["old_log_prob"].data_ptr(), roll["advantages"].data_ptr(), roll["returns"].data_ptr(),
                                         *(g[k][0].data_ptr() for k in ("actions", "old_values", "old_log_prob", "advantages", "returns")),
                                         _stream()), "gnbv_gather_minibatch")
    torch.cuda.synchronize()
    for k in g:
        _check_written(k, *g[k])
        assert torch.equal(g[k][0], roll[k][rows]), k
    gathered = dict(mb, **{k: g[k][0] for k in g})
    fused = dict(mb, **{k: roll[k] for k in g})
    outs = []
    for x, r in ((gathered, None), (fused, rows)):
        a, o = _loss_struct(dims, B, cfg, x, rows=r)
        _run_loss(a, monkeypatch)
        outs.append(o)
    for k in ("d_logits", "d_values", "head_entropy", "head_lse"):
        assert torch.equal(outs[0][k][0], outs[1][k][0]), k
    assert torch.equal(outs[0]["stats"][0][0], outs[1]["stats"][0][0]) and int(outs[0]["stats_row"]) == int(outs[1]["stats_row"]) == 1
    assert torch.equal(outs[0]["scratch"][:8 * B], outs[1]["scratch"][:8 * B])


def test_deferred_statistics_and_kl_out(monkeypatch):
    """defer_stats = 1 + gnbv_ppo_loss_finish writes the statistics row defer_stats = 0 writes, bit for bit; with kl_out the row's KL
    lands there and stop_flag is left alone even when the KL is far above the target."""
    lib = _lib.load()
    B = 300
    cfg = Cfg(target_kl=1e-9)  # (every KL trips it)
    x = _loss_inputs(SIX, B, cfg, seed=5)
    a0, o0 = _loss_struct(SIX, B, cfg, x)
    _run_loss(a0, monkeypatch)
    assert int(o0["stop_flag"]) == 1
    for with_kl in (False, True):
        kl = _out(1) if with_kl else None
        a1, o1 = _loss_struct(SIX, B, cfg, x, defer=1, kl_out=kl[0] if with_kl else None)
        _run_loss(a1, monkeypatch)
        assert bool(torch.isnan(o1["stats"][0]).all()) and int(o1["stats_row"]) == 0, "defer_stats = 1 wrote the statistics"
        _lib.check(lib.gnbv_ppo_loss_finish(C.byref(a1), _stream()), "gnbv_ppo_loss_finish")
        torch.cuda.synchronize()
        assert torch.equal(o1["stats"][0][0], o0["stats"][0][0]), (o1["stats"][0][0], o0["stats"][0][0])
        assert torch.equal(o1["d_logits"][0], o0["d_logits"][0]) and torch.equal(o1["d_values"][0], o0["d_values"][0])
        assert int(o1["stats_row"]) == 1
        if with_kl:
            _check_written("kl_out", *kl)
            assert float(kl[0]) == float(o0["stats"][0][0, 3])
            assert int(o1["stop_flag"]) == 0, "kl_out must leave the stop decision to the caller"
        else:
            assert int(o1["stop_flag"]) == 1


@pytest.mark.parametrize("defer", [0, 1])
def test_stop_flag_is_sticky_and_the_threshold_strict(defer, monkeypatch):
    """A sequence of calls on one statistics table: stats_row counts up; the call whose KL exceeds 1.5 target_kl sets stop_flag and
    its row is live ([6] = 1); every later row has [6] = 0 and the flag stays set.  KL == 1.5 target_kl (fp32) does not stop."""
    lib = _lib.load()
    B = 128
    x = _loss_inputs(SIX, B, Cfg(), seed=9)
    a, o = _loss_struct(SIX, B, Cfg(), x)
    _run_loss(a, monkeypatch)
    kl = torch.tensor(float(o["stats"][0][0, 3]), dtype=torch.float32)
    assert float(kl) > 0
    # target_kl values around kl / 1.5 whose fp32 product 1.5f * t is just below (stops), at or just above kl (does not stop)
    prod = lambda t: float(torch.tensor(1.5, dtype=torch.float32) * torch.tensor(t, dtype=torch.float32))
    ts = [torch.tensor(float(kl) / 1.5, dtype=torch.float32)]
    for _ in range(4):
        ts = [torch.nextafter(ts[0], torch.tensor(0.0))] + ts + [torch.nextafter(ts[-1], torch.tensor(1.0))]
    ts = [float(t) for t in ts]
    t_stop = max(t for t in ts if prod(t) < float(kl))
    t_go = min(t for t in ts if prod(t) >= float(kl))
    seq = [(t_go, False)]
    if prod(t_go) == float(kl):  # KL == 1.5 t exactly: strict, no stop; then the next t up
        seq.append((min(t for t in ts if prod(t) > float(kl)), False))
    seq += [(t_stop, True), (t_go, True), (t_stop, True)]
    stats, stats_row = _out(len(seq) + 1, 8), torch.zeros(1, dtype=torch.int64, device=DEV)
    stop = torch.zeros(1, dtype=torch.int32, device=DEV)
    tripped = False
    for k, (tk, stop_after) in enumerate(seq):
        cfg = Cfg(target_kl=tk)
        a, o = _loss_struct(SIX, B, cfg, x, defer=defer, stop=stop, stats=stats, stats_row=stats_row)
        _run_loss(a, monkeypatch)
        if defer:
            _lib.check(lib.gnbv_ppo_loss_finish(C.byref(a), _stream()), "gnbv_ppo_loss_finish")
            torch.cuda.synchronize()
        row = stats[0][k]
        assert int(stats_row) == k + 1
        assert float(row[3]) == float(kl)
        assert float(row[6]) == (0.0 if tripped else 1.0), (k, row)
        assert int(stop) == int(stop_after), (k, tk, float(kl))
        tripped = tripped or stop_after
    assert bool(torch.isfinite(stats[0][:len(seq)]).all()) and bool(torch.isnan(stats[0][len(seq)]).all())
    assert bool((stats[1][stats[0].numel():] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. clip + Adam over the flat buffer
# ---------------------------------------------------------------------------------------------------------------------------------
LR, B1, B2, EPS = 3e-4, 0.9, 0.999, 1e-5
STREAMS = ("p", "g", "m", "v")


@functools.lru_cache(maxsize=None)
def _policy_n(g):
    """Length of the flat parameter buffer of the real policy at grid size g (FlatAdam over policy_util.make_policy)."""
    from gennbv_amd.ops.ppo_ops import FlatAdam
    from tests import policy_util
    pol = policy_util.make_policy(g=g, device=DEV, det_weights=False)[0]
    n = FlatAdam(pol, lr=LR, eps=EPS).n
    del pol
    torch.cuda.empty_cache()
    return n


def _adam_data(n, seed):
    """fp32 state + gradient over many magnitudes: parameters ~0.05, gradients 1e-7..1 (some exactly 0), exp_avg 1e-8..1e-2 of both
    signs, exp_avg_sq 1e-14..1e-4 (sqrt(v) from far below eps to far above)."""
    gen = torch.Generator(device=DEV).manual_seed(seed)

    def mag(lo, hi):
        return torch.pow(10.0, torch.rand(n, generator=gen, device=DEV) * (hi - lo) + lo)

    sign = lambda: torch.where(torch.rand(n, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
    p = torch.randn(n, generator=gen, device=DEV) * 0.05
    g = mag(-7, 0) * sign() * (torch.rand(n, generator=gen, device=DEV) > 0.05)
    m = mag(-8, -2) * sign()
    v = mag(-14, -4)
    return {"p": p, "g": g.float(), "m": m, "v": v}


class Flat:
    """The four streams, each at its own float offset inside a buffer whose head and tail hold SENTINEL."""

    def __init__(self, data, offs=(0, 0, 0, 0)):
        self.offs, self.bufs, self.views = dict(zip(STREAMS, offs)), {}, {}
        n = data["p"].numel()
        for k in STREAMS:
            o = self.offs[k]
            buf = torch.full((o + n + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
            buf[o:o + n] = data[k]
            self.bufs[k], self.views[k] = buf, buf[o:o + n]
        self.n = n
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.stop = torch.zeros(1, dtype=torch.int32, device=DEV)

    def __getitem__(self, k):
        return self.views[k]

    def state(self):
        return {k: self.views[k].clone() for k in STREAMS}

    def check_pads(self):
        for k in STREAMS:
            o = self.offs[k]
            assert bool((self.bufs[k][:o] == SENTINEL).all()) and bool((self.bufs[k][o + self.n:] == SENTINEL).all()), \
                f"{k}: written outside its {self.n} elements"


def _adam_step(f, max_norm, gs=1.0, kl=None, target_kl=-1.0, sq=None, skip=None, loss_finish=None, zero_ws=True):
    """One gnbv_clip_adam_step_ex on the Flat f.  sq = (lo, hi, partial fp64 tensor); skip = (lo, hi).  Returns (norm_out, ws)."""
    lib = _lib.load()
    a = _lib.GnbvAdamStep()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = (f[k].data_ptr() for k in STREAMS)
    a.n = f.n
    a.max_grad_norm, a.lr, a.beta1, a.beta2, a.eps = float(max_norm), LR, B1, B2, EPS
    a.step, a.stop_flag, a.grad_scale = f.step.data_ptr(), f.stop.data_ptr(), float(gs)
    a.kl_slot, a.target_kl = _lib.ptr(kl), float(target_kl)
    norm_out = _out(2)
    ws = torch.zeros(lib.gnbv_adam_workspace_bytes(), dtype=torch.uint8, device=DEV)
    if not zero_ws:
        ws.fill_(0xFF)
    a.norm_out, a.workspace, a.workspace_bytes = norm_out[0].data_ptr(), ws.data_ptr(), ws.numel()
    if sq is not None:
        a.sq_lo, a.sq_hi, a.sq_partial, a.sq_parts = sq[0], sq[1], sq[2].data_ptr(), sq[2].numel()
    if skip is not None:
        a.upd_skip_lo, a.upd_skip_hi = skip
    if loss_finish is not None:
        a.loss_finish = C.addressof(loss_finish)
    _lib.check(lib.gnbv_clip_adam_step_ex(C.byref(a), _stream()), "gnbv_clip_adam_step_ex")
    torch.cuda.synchronize()
    f.check_pads()
    assert bool((norm_out[1][2:] == SENTINEL).all())
    return norm_out[0], ws


def _adam_ref(s, t, max_norm, gs=1.0):
    """One fp64 step from the fp32 state s at step count t (already incremented), the kernel's fp32 hyperparameters."""
    lr, b1, b2, eps, tiny = _f32(LR), _f32(B1), _f32(B2), _f32(EPS), _f32(1e-6)
    g = s["g"].double()
    norm = math.sqrt(float((g * g).sum())) * gs
    coef = (min(1.0, _f32(max_norm) / (norm + tiny)) if max_norm > 0 else 1.0) * gs
    gi = g * coef
    m, v, p = s["m"].double(), s["v"].double(), s["p"].double()
    m1 = m + (gi - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * gi * gi
    ss, b2s = lr / (1 - math.pow(b1, t)), math.sqrt(1 - math.pow(b2, t))
    denom = v1.sqrt() / b2s + eps
    p1 = p - ss * (m1 / denom)
    mag = (1 - b1) * (gi.abs() + m.abs())
    return dict(norm=norm, coef=coef, p=p1, m=m1, v=v1,
                bp=2 * torch.maximum(_ulp(p), _ulp(p1)) + SAFETY * 16 * U * ss * (m1.abs() + mag) / denom,
                bm=8 * U * (m1.abs() + mag), bv=16 * U * v1 + TINY)


def _check_adam(what, f, s, t, norm_out, max_norm, gs=1.0, where=None):
    """The kernel's step (f after, s = the state before it) against _adam_ref; `where`: the elements the step updated."""
    r = _adam_ref(s, t, max_norm, gs)
    ratios = {"norm": abs(float(norm_out[0]) - r["norm"]) / float(_ulp(torch.tensor(r["norm"], dtype=F64))),
              "coef": abs(float(norm_out[1]) - r["coef"]) / (3 * float(_ulp(torch.tensor(r["coef"], dtype=F64))))}
    sl = slice(None) if where is None else where
    for k, b in (("p", "bp"), ("m", "bm"), ("v", "bv")):
        ratios[k] = _ratio(f[k][sl], r[k][sl], r[b][sl] if k == "p" else SAFETY * r[b][sl])
    return _report(what, ratios)


ADAM_SIZES = [1, 3, 4, 5, 255, 4097, 2097152, 2097153, 8388613, "G20", "G64"]
LAYOUTS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1)]


@pytest.mark.parametrize("n", ADAM_SIZES, ids=[str(s) for s in ADAM_SIZES])
def test_clip_adam_step_vs_fp64(n):
    """One clipped step (the clip binds) per layout -- every stream aligned, then each stream in turn 1-3 floats off -- against fp64;
    then the same inputs with max_grad_norm = -1 (coef exact): every layout gives the aligned run's bits."""
    n = _policy_n(int(n[1:])) if isinstance(n, str) else n
    d = _adam_data(n, seed=n % 100003)
    gnorm = float(d["g"].double().norm())
    bits = None
    for offs in LAYOUTS:
        f = Flat(d, offs)
        s = f.state()
        norm_out, _ = _adam_step(f, max_norm=0.5 * gnorm)
        assert int(f.step) == 1 and int(f.stop) == 0
        _check_adam(f"adam n={n} offs={offs} clipped", f, s, 1, norm_out, 0.5 * gnorm)
        f = Flat(d, offs)
        norm_out, _ = _adam_step(f, max_norm=-1.0)
        got = tuple(f[k].clone() for k in ("p", "m", "v"))
        if bits is None:
            bits = got
            _check_adam(f"adam n={n} unclipped", f, s, 1, norm_out, -1.0)
        else:
            for k, x, y in zip("pmv", got, bits):
                assert torch.equal(x, y), f"offs={offs}: {k} differs from the aligned run"


@pytest.mark.parametrize("n", [4097, 2097153])
@pytest.mark.parametrize("gs", [0.5, 0.125])
def test_clip_adam_grad_scale(n, gs):
    """grad_scale = 1/world: norm and factor of the scaled (mean) gradient, clipped and not."""
    d = _adam_data(n, seed=n + 17)
    gnorm = float(d["g"].double().norm()) * gs
    for max_norm in (0.25 * gnorm, 4 * gnorm):
        f = Flat(d)
        s = f.state()
        norm_out, _ = _adam_step(f, max_norm=max_norm, gs=gs)
        _check_adam(f"adam n={n} grad_scale={gs} max_norm={max_norm:.3g}", f, s, 1, norm_out, max_norm, gs)


@pytest.mark.parametrize("preset", [0, 1, 9999, 999999])
def test_clip_adam_step_counts(preset):
    """The step counter preset to t - 1: the bias corrections at t = 1, 2, 1e4, 1e6 match fp64 pow; three consecutive steps, the
    reference restarting from the kernel's state each time."""
    d = _adam_data(4097, seed=preset + 3)
    f = Flat(d)
    f.step.fill_(preset)
    for k in range(3):
        d["g"] = _adam_data(4097, seed=preset + 100 + k)["g"]
        f["g"].copy_(d["g"])
        s = f.state()
        norm_out, _ = _adam_step(f, max_norm=1.0)
        assert int(f.step) == preset + k + 1
        _check_adam(f"adam t={preset + k + 1}", f, s, preset + k + 1, norm_out, 1.0)


def _sq_parts(g, lo, hi, parts, via_kernel):
    if via_kernel:
        lib = _lib.load()
        out = torch.full((int(lib.gnbv_sq_partials_count()),), -1.0, dtype=F64, device=DEV)
        _lib.check(lib.gnbv_sq_partials(g[lo:hi].data_ptr(), hi - lo, out.data_ptr(), _stream()), "gnbv_sq_partials")
        return out
    sq = g[lo:hi].double() ** 2
    return torch.stack([c.sum() for c in torch.tensor_split(sq, parts)]).contiguous()


SLICES = ["start", "start-unaligned", "middle", "middle-unaligned", "end", "end-unaligned", "all"]


def _slice(name, n):
    """[lo, hi) of the named slice of n: lo and hi multiples of 4, or not."""
    q = (n // 4) & ~3
    lo, hi = {"start": (0, q), "start-unaligned": (0, q + 1), "middle": (q, 2 * q), "middle-unaligned": (q + 1, 2 * q + 3),
              "end": (n - q, n), "end-unaligned": (n - q - 1, n), "all": (0, n)}[name]
    return lo, hi


@pytest.mark.parametrize("n", [4097, 2097153])
@pytest.mark.parametrize("parts", [1, 7, 844, "kernel"])
@pytest.mark.parametrize("sl", SLICES)
def test_clip_adam_sq_partial_slices(n, parts, sl):
    """sq_lo / sq_hi / sq_partial: the norm pass skips the slice and folds its producer's partial sums (fp64 torch sums in 1..844
    parts, or gnbv_sq_partials): the fp64 partials the launch leaves in the workspace add up to the unsliced sum of squares within
    fp64 round-off, and the step matches fp64."""
    lo, hi = _slice(sl, n)
    d = _adam_data(n, seed=n + lo + hi)
    f = Flat(d)
    s = f.state()
    part = _sq_parts(f["g"], lo, hi, 1 if parts == "kernel" else parts, parts == "kernel")
    gnorm = float(d["g"].double().norm())
    norm_out, ws = _adam_step(f, max_norm=0.5 * gnorm, sq=(lo, hi, part))
    total = float(ws[:1026 * 8].view(F64).sum())  # (the launch's partial sums; the workspace was zeroed)
    want = float((d["g"].double() ** 2).sum())
    assert abs(total - want) <= 1e-12 * want, (total, want)
    _check_adam(f"adam n={n} sq slice {sl} [{lo}, {hi}) parts={parts}", f, s, 1, norm_out, 0.5 * gnorm)


@pytest.mark.parametrize("n,lo,hi", [(4097, 1024, 3072), (4097, 1025, 3071), (2097153, 4, 1048580), (2097153, 3, 2097150)])
def test_upd_skip_then_shard_step_reproduces_the_unsharded_step(n, lo, hi):
    """upd_skip_lo / hi (with the slice's norm from sq_partial, as the sharded data-parallel step runs it): the slice is untouched bit
    for bit, the rest equals the unsharded step; gnbv_adam_shard_step on the slice with that launch's norm_out then reproduces the
    unsharded step there, bit for bit."""
    lib = _lib.load()
    d = _adam_data(n, seed=lo + hi)
    gnorm = float(d["g"].double().norm())
    fa = Flat(d)
    s = fa.state()
    part = _sq_parts(fa["g"], lo, hi, 844, False)
    norm_a, _ = _adam_step(fa, max_norm=0.5 * gnorm, sq=(lo, hi, part))
    _check_adam(f"adam n={n} unsharded", fa, s, 1, norm_a, 0.5 * gnorm)
    fb = Flat(d)
    norm_b, _ = _adam_step(fb, max_norm=0.5 * gnorm, sq=(lo, hi, part), skip=(lo, hi))
    assert torch.equal(norm_a, norm_b)
    for k in ("p", "m", "v"):
        assert torch.equal(fb[k][lo:hi], s[k][lo:hi]), f"{k}: the skipped slice was updated"
        assert torch.equal(fb[k][:lo], fa[k][:lo]) and torch.equal(fb[k][hi:], fa[k][hi:]), k
    _lib.check(lib.gnbv_adam_shard_step(*(fb[k][lo:].data_ptr() for k in STREAMS), hi - lo, norm_b.data_ptr(), LR, B1, B2, EPS,
                                        fb.step.data_ptr(), fb.stop.data_ptr(), _stream()), "gnbv_adam_shard_step")
    torch.cuda.synchronize()
    fb.check_pads()
    assert int(fb.step) == 1
    for k in ("p", "m", "v"):
        assert torch.equal(fb[k], fa[k]), f"{k}: shard step differs from the unsharded step"


@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_kl_slot_decision_is_strict(gs):
    """Data-parallel early stop: *stop_flag = 1 iff kl_slot * grad_scale > 1.5 target_kl (fp32).  Equality and just below update
    and count the step; just above stops: params, exp_avg, exp_avg_sq bit-identical and the step not counted."""
    target = 0.02
    thr = torch.tensor(1.5, dtype=torch.float32) * torch.tensor(target, dtype=torch.float32)
    at = thr / gs
    d = _adam_data(4097, seed=99)
    for kl, stops in ((at, False), (torch.nextafter(at, torch.tensor(0.0)), False), (torch.nextafter(at, torch.tensor(1.0)), True)):
        f = Flat(d)
        s = f.state()
        kl_dev = torch.tensor([float(kl)], dtype=torch.float32, device=DEV)
        norm_out, _ = _adam_step(f, max_norm=1.0, gs=gs, kl=kl_dev, target_kl=target)
        assert int(f.stop) == int(stops), (float(kl), gs)
        if stops:
            assert int(f.step) == 0
            for k in STREAMS:
                assert torch.equal(f[k], s[k]), k
        else:
            assert int(f.step) == 1
            _check_adam(f"adam kl_slot={float(kl):.9g} gs={gs}", f, s, 1, norm_out, 1.0, gs)


@pytest.mark.parametrize("trip", [False, True])
def test_loss_finish_inside_the_norm_launch(trip, monkeypatch):
    """GnbvAdamStep.loss_finish: the norm launch's extra workgroup writes the statistics row gnbv_ppo_loss writes with defer_stats = 0,
    bit for bit; a tripped KL masks the same launch's update and does not count the step, an untripped one counts it once."""
    B = 128
    cfg = Cfg(target_kl=1e-9 if trip else 10.0)
    x = _loss_inputs(SIX, B, cfg, seed=21)
    a0, o0 = _loss_struct(SIX, B, cfg, x)
    _run_loss(a0, monkeypatch)
    d = _adam_data(4097, seed=5)
    f = Flat(d)
    s = f.state()
    a1, o1 = _loss_struct(SIX, B, cfg, x, defer=1, stop=f.stop)
    _run_loss(a1, monkeypatch)
    norm_out, _ = _adam_step(f, max_norm=1.0, loss_finish=a1)
    assert torch.equal(o1["stats"][0][0], o0["stats"][0][0])
    assert float(o1["stats"][0][0, 6]) == 1.0 and int(o1["stats_row"]) == 1
    assert int(f.stop) == int(trip) == int(o0["stop_flag"])
    if trip:
        assert int(f.step) == 0
        for k in STREAMS:
            assert torch.equal(f[k], s[k]), k
    else:
        assert int(f.step) == 1
        _check_adam("adam loss_finish", f, s, 1, norm_out, 1.0)


def test_flat_step_matches_torch_adam_and_clip_grad_norm():
    """Ties the fp64 oracle to the reference optimizer: a few steps against torch.optim.Adam (fp32, foreach=False) after
    clip_grad_norm_, relative 1e-6 of the parameters' update scale."""
    d = _adam_data(4097, seed=1)
    d["m"].zero_()
    d["v"].zero_()
    f = Flat(d)
    p = torch.nn.Parameter(d["p"].clone())
    opt = torch.optim.Adam([p], lr=_f32(LR), betas=(_f32(B1), _f32(B2)), eps=_f32(EPS), foreach=False)
    for k in range(4):
        g = _adam_data(4097, seed=10 + k)["g"]
        f["g"].copy_(g)
        p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p], 0.5, foreach=False)
        opt.step()
        _adam_step(f, max_norm=0.5)
    err = (f["p"].double() - p.detach().double()).abs()
    scale = (p.detach().double() - d["p"].double()).abs().max()
    r = float(err.max() / (1e-6 * scale + 2 * _ulp(p.detach()).max()))
    _report("adam vs torch.optim.Adam", {"p": r})


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the rollout sampler
# ---------------------------------------------------------------------------------------------------------------------------------
U_MAX = 1.0 - 2.0 ** -24  # the largest float32 torch.rand returns


def _sample(logits, dims, uniforms, deterministic=False):
    lib = _lib.load()
    B = logits.shape[0]
    acts, abuf = _out(B, len(dims), dtype=torch.int64, fill=-7)
    lp, lbuf = _out(B)
    hd = (C.c_int * len(dims))(*dims)
    _lib.check(lib.gnbv_multicategorical_sample(logits.data_ptr(), B, sum(dims), len(dims), hd, _lib.ptr(uniforms), int(deterministic),
                                                acts.data_ptr(), lp.data_ptr(), _stream()), "gnbv_multicategorical_sample")
    torch.cuda.synchronize()
    _check_written("log_prob", lp, lbuf)
    assert bool((abuf[acts.numel():] == int(SENTINEL)).all()) and int(acts.min()) >= 0
    return acts, lp


def _check_sample(what, logits, dims, u, acts, lp):
    """Every action is the fp64 inverse CDF at u (either neighbour where u is within the rounding margin of a CDF step) and has
    non-zero mass; log_prob matches fp64 within the error model."""
    hs = _heads(logits, dims)
    want_lp = torch.zeros(logits.shape[0], dtype=F64, device=DEV)
    blp = torch.zeros_like(want_lp)
    abs_lp = torch.zeros_like(want_lp)
    for i, h in enumerate(hs):
        a = acts[:, i]
        assert int(a.min()) >= 0 and int(a.max()) < h["n"], f"head {i}: action out of range"
        p = h["p"]
        pa = p.gather(1, a[:, None]).squeeze(1)
        zero = pa == 0
        assert not bool(zero.any()), (f"{what} head {i}: {int(zero.sum())} of {a.numel()} rows sampled a zero-mass category "
                                      f"(e.g. row {int(zero.nonzero()[0])}: action {int(a[zero][0])} of {h['n']})")
        cdf = torch.cumsum(p, 1) / p.sum(1, keepdim=True)
        hi_ = cdf.gather(1, a[:, None]).squeeze(1)
        lo_ = torch.where(a > 0, cdf.gather(1, (a - 1).clamp_min(0)[:, None]).squeeze(1), torch.zeros_like(hi_))
        tol = SAFETY * U * (2 * math.ceil(h["n"] / 64) + 16)
        ui = u[:, i].double()
        ok = (ui >= lo_ - tol) & (ui < hi_ + tol)
        assert bool(ok.all()), (f"{what} head {i}: {int((~ok).sum())} rows off the inverse CDF, e.g. row {int((~ok).nonzero()[0])}")
        lpa = h["lp"].gather(1, a[:, None]).squeeze(1)
        want_lp += lpa
        blp += h["d_lse"] + U * lpa.abs()
        abs_lp += lpa.abs()
    blp += len(dims) * U * abs_lp
    return _ratio(lp, want_lp, SAFETY * blp)


SAMPLE_DIMS = [[1], [13], [64], [65], [81], [129], [200], SIX, [200, 1, 65], [13, 129, 64, 65, 1, 81, 7, 200]]


@pytest.mark.parametrize("dims", SAMPLE_DIMS, ids=["-".join(map(str, d)) for d in SAMPLE_DIMS])
def test_sample_is_the_fp64_inverse_cdf(dims):
    """Explicit uniforms (random, 0, 1 - 2^-24), logits with leading and trailing zero-mass categories (logit -1e4) in a third of
    the rows: the fp64 inverse CDF, never a zero-mass category, log_prob within the error model."""
    gen = torch.Generator(device=DEV).manual_seed(sum(dims) + len(dims))
    B, nh = 3072, len(dims)
    logits = torch.randn(B, sum(dims), generator=gen, device=DEV) * 2
    off = 0
    for d in dims:
        if d >= 3:  # rows 0 mod 3: zero mass at both ends of every head
            k = max(1, d // 5)
            logits[0::3, off:off + k] = -1e4
            logits[0::3, off + d - k:off + d] = -1e4
        off += d
    u = torch.rand(B, nh, generator=gen, device=DEV)
    u[1::6] = 0.0
    u[2::6] = U_MAX
    u[3::6] = U_MAX
    acts, lp = _sample(logits, dims, u.contiguous())
    _report(f"sample {dims}", {"log_prob": _check_sample(f"sample {dims}", logits, dims, u, acts, lp)})


@pytest.mark.parametrize("d", [13, 51, 81])
def test_sample_at_the_top_uniform_skips_trailing_zero_mass(d):
    """u = 1 - 2^-24 with trailing zero-mass categories: the scan that walks the CDF adds exp(x - mx) in another order than the total
    u * sum was taken from, so no lane may exceed the target; the answer must still be the last category with mass, not one
    of probability 0 (whose log-prob of about -1e4 makes a later PPO ratio overflow)."""
    gen = torch.Generator(device=DEV).manual_seed(d)
    B = 4096
    logits = torch.randn(B, d, generator=gen, device=DEV) * 2
    logits[:, d - d // 3:] = -1e4
    u = torch.full((B, 1), U_MAX, device=DEV)
    acts, lp = _sample(logits, [d], u)
    _report(f"sample top-u d={d}", {"log_prob": _check_sample(f"sample top-u d={d}", logits, [d], u, acts, lp)})


@pytest.mark.parametrize("dims", [[13], [81], [200, 1, 65], SIX])
def test_sample_deterministic_is_the_first_argmax(dims):
    """deterministic = 1 with tied maxima (integer logits): the first arg-max of every head, log_prob within the error model."""
    gen = torch.Generator(device=DEV).manual_seed(len(dims) * 1000 + sum(dims))
    B = 1024
    logits = torch.randint(-3, 3, (B, sum(dims)), generator=gen, device=DEV).float()
    acts, lp = _sample(logits, dims, None, deterministic=True)
    off = 0
    for i, d in enumerate(dims):
        xs = logits[:, off:off + d]
        idx = torch.arange(d, device=DEV).expand_as(xs)
        first = torch.where(xs == xs.amax(1, keepdim=True), idx, d).amin(1)
        assert int((xs == xs.amax(1, keepdim=True)).sum(1).max()) > 1 or d == 1
        assert torch.equal(acts[:, i], first), f"head {i}"
        off += d
    hs = _heads(logits, dims)
    lps = [h["lp"].gather(1, acts[:, i:i + 1]).squeeze(1) for i, h in enumerate(hs)]
    bound = sum(h["d_lse"] + U * v.abs() for h, v in zip(hs, lps)) + len(dims) * U * sum(v.abs() for v in lps)
    _report(f"sample deterministic {dims}", {"log_prob": _ratio(lp, sum(lps), SAFETY * bound)})
