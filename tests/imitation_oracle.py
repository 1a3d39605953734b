"""fp64 torch oracle of the soft-target imitation loss (include/gennbv_hip.h: GnbvImitationLoss) and its error model.

`reference` writes the loss with torch expressions in fp64 and takes its gradient by autograd; `bounds` carries the rounding of the
fp32 kernel elementwise from the reference's own magnitudes (u = 2^-24), extending the model of tests/test_ppo_kernels_gpu.py
(d_lse, d_lp, d_p, d_H per head) by
* the candidates' weights: Q is a k-term sum (lane-serial, then a 6-stage butterfly) and q_j / Q one division, so a normalised
  weight is off by r_q = (ceil(k/64) + 8) u of itself; the marginal adds up to k of them serially and is smoothed with three more
  roundings: d_m = (1 - eps)(r_q + k u) m_raw + 3u m;
* ce = -sum m lp: d_ce = sum_h [sum_c (d_m |lp| + m d_lp) + (ceil(n/64) + 8) u sum m |lp|] + n_heads u sum_h |ce_h|;
* W, a B-term sum in the fixed order of the last workgroup (256 strided partial sums, a 6-stage wave reduction, four partials), and
  its reciprocal: r_W = (ceil(B/256) + 10) u;
* a gradient element (w_b / W)(t1 + t2), t1 = p - m, t2 = c_e p (lp + H): (w_b / W)(d_p + d_m + c_e (d_p |lp + H| + p (d_lp + d_H)))
  + (r_W + 6u)(w_b / W)(|t1| + |t2|);
* a weighted mean statistic: the weighted mean of the per-sample bounds + (2 r_W + 4u) of the weighted mean |term|.
"""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
F64 = torch.float64


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def liveness(dims, cand, cand_w, sample_w):
    """(live [B] bool, flags int, q [B,k] fp64 candidate weights, w [B] fp64) by the rules of the header."""
    B, k, nh = cand.shape
    dev = cand.device
    q = cand_w.double() if cand_w is not None else torch.cat([torch.ones(B, 1, dtype=F64, device=dev), torch.zeros(B, k - 1, dtype=F64, device=dev)], 1)
    w = sample_w.double() if sample_w is not None else torch.ones(B, dtype=F64, device=dev)
    bad_w = ~(torch.isfinite(w) & (w >= 0)) | (~(torch.isfinite(q) & (q >= 0))).any(1)
    hd = torch.tensor(dims, dtype=torch.int64, device=dev)
    oob = ((cand < 0) | (cand >= hd)).any(2) & (q != 0)
    weighs = ~bad_w & (w != 0) & (torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0).sum(1) != 0)
    bad_i = weighs & oob.any(1)
    live = weighs & ~bad_i
    flags = (1 if bool(bad_i.any()) else 0) | (2 if bool(bad_w.any()) else 0)
    return live, flags, q, w


def head_stats(x, dims):
    """fp64 statistics of every head (the error model of tests/test_ppo_kernels_gpu.py::_heads)."""
    out, off = [], 0
    for n in dims:
        xs = x[:, off:off + n].double()
        mx = xs.amax(1)
        lse = torch.logsumexp(xs, 1)
        lp = xs - lse[:, None]
        p = lp.exp()
        H = -(p * lp).sum(1)
        kk = math.ceil(n / 64)
        d_lse = U * (lse.abs() + mx.abs() + 2 * (p * (xs - mx[:, None]).abs()).sum(1) + kk + 12)
        d_lp = d_lse[:, None] + U * lp.abs()
        d_p = p * (d_lp + 2 * U) + TINY
        d_H = (d_p * lp.abs() + p * d_lp).sum(1) + (kk + 8) * U * (p * lp.abs()).sum(1)
        out.append(dict(off=off, n=n, mx=mx, lse=lse, lp=lp, p=p, H=H, d_lse=d_lse, d_lp=d_lp, d_p=d_p, d_H=d_H))
        off += n
    return out


def marginals(dims, cand, qn, eps):
    """[B, n] fp64 target of every head: (1 - eps) sum_j qn_j [cand_j == c] + eps / n; indices out of range match nothing."""
    out = []
    for h, n in enumerate(dims):
        idx = cand[:, :, h]
        ok = (idx >= 0) & (idx < n)
        m = torch.zeros(cand.shape[0], n, dtype=F64, device=cand.device)
        m.scatter_add_(1, idx.clamp(0, n - 1), torch.where(ok, qn, torch.zeros_like(qn)))
        out.append((1.0 - eps) * m + eps / n)
    return out


def torch_loss(dims, x, v, cand, cand_w, sample_w, returns, eps, ec, vf):
    """The loss written with torch on logits x [B, n_logits] and values v [B] or None (any float dtype, differentiable), the labels
    as given: dict(loss, and detached ce, ent, err, nll, agree, live, flags, wl, W, qn, ms, jstar), or loss None without a live sample."""
    B = cand.shape[0]
    dt, dev = x.dtype, x.device
    live, flags, q, w = liveness(dims, cand, cand_w, sample_w)
    out = dict(live=live, flags=flags, loss=None)
    if int(live.sum()) == 0:
        return out
    q, w = q.to(dt), w.to(dt)
    wl = torch.where(live, w, torch.zeros_like(w))
    qs = torch.where(live[:, None], q, torch.zeros_like(q))
    Q = qs.sum(1)
    qn = qs / torch.where(live, Q, torch.ones_like(Q))[:, None]
    W = wl.sum()
    ms = [m.to(dt) for m in marginals(dims, cand, qn.double(), eps)]
    ce = torch.zeros(B, dtype=dt, device=dev)
    ent, nll = torch.zeros_like(ce), torch.zeros_like(ce)
    agree = torch.ones(B, dtype=torch.bool, device=dev)
    jstar = qs.argmax(1)  # the first of the largest
    off = 0
    for h, n in enumerate(dims):
        lp = torch.log_softmax(x[:, off:off + n], 1)
        ce = ce - (ms[h] * lp).sum(1)
        ent = ent - (lp.exp() * lp).sum(1)
        cs = cand[torch.arange(B, device=dev), jstar, h].clamp(0, n - 1)
        nll = nll - lp.detach().gather(1, cs[:, None]).squeeze(1)
        if n > 1:
            agree = agree & (x.detach()[:, off:off + n].argmax(1) == cs)
        off += n
    err = (v - returns.to(dt)) if (v is not None and returns is not None) else torch.zeros_like(ce)
    per = ce - ec * ent + vf * err * err
    out.update(loss=(wl * per).sum() / W, ce=ce.detach(), ent=ent.detach(), err=err.detach(), nll=nll, agree=agree, wl=wl, W=W, qn=qn, ms=ms,
               jstar=jstar)
    return out


def stats_row(t):
    """The kernel's statistics row [8] from torch_loss's dict."""
    wl, W, lf = t["wl"], t["W"], t["live"].to(t["wl"].dtype)
    n_live = lf.sum()
    return torch.stack([(wl * t["ce"]).sum() / W, (wl * t["err"] * t["err"]).sum() / W, (wl * t["ent"]).sum() / W,
                        (lf * t["agree"].to(lf.dtype)).sum() / n_live, (lf * t["nll"]).sum() / n_live, t["loss"].detach(), n_live,
                        torch.zeros((), dtype=lf.dtype, device=lf.device)])


def reference(dims, logits, values, cand, cand_w, sample_w, returns, label_smoothing=0.0, ent_coef=0.0, vf_coef=0.0):
    """dict(d_logits, d_values, stats [8], live, flags, ...) in fp64; the hyperparameters enter with their fp32 values."""
    eps, ec, vf = f32(label_smoothing), f32(ent_coef), f32(vf_coef)
    B = cand.shape[0]
    x = logits.double().clone().requires_grad_()
    v = values.double().clone().requires_grad_() if values is not None else None
    out = torch_loss(dims, x, v, cand, cand_w, sample_w, returns, eps, ec, vf)
    live = out["live"]
    if out["loss"] is None:
        out.update(d_logits=torch.zeros_like(x), d_values=torch.zeros(B, dtype=F64, device=x.device), stats=torch.zeros(8, dtype=F64, device=x.device))
        return out
    out["loss"].backward()
    out["d_logits"] = torch.where(live[:, None], x.grad, torch.zeros_like(x.grad))
    out["d_values"] = (torch.where(live, v.grad, torch.zeros_like(v.grad)) if (v is not None and v.grad is not None)
                       else torch.zeros(B, dtype=F64, device=x.device))
    out["stats"] = stats_row(out)
    return out


def bounds(dims, logits, cand, ref, label_smoothing=0.0, ent_coef=0.0, vf_coef=0.0):
    """dict(d_logits [B,n_logits], d_values [B], stats [8]) of the error model above (not yet doubled); `ref` from reference()
    with at least one live sample."""
    eps, ec, vf = f32(label_smoothing), f32(ent_coef), f32(vf_coef)
    B, k, nh = cand.shape
    live, wl, W = ref["live"], ref["wl"], ref["W"]
    hs = head_stats(logits, dims)
    r_q = (math.ceil(k / 64) + 8) * U
    r_W = (math.ceil(B / 256) + 10) * U
    sw = (wl / W)[:, None]
    bl = []
    d_ce = torch.zeros(B, dtype=F64, device=logits.device)
    ce_abs = torch.zeros_like(d_ce)
    d_nll = torch.zeros_like(d_ce)
    nll_abs = torch.zeros_like(d_ce)
    for h, (st, m) in enumerate(zip(hs, ref["ms"])):
        n = st["n"]
        if n == 1:
            bl.append(torch.zeros(B, 1, dtype=F64, device=logits.device))
            continue
        m_raw = (m - eps / n) / (1.0 - eps)
        d_m = (1.0 - eps) * (r_q + k * U) * m_raw.abs() + 3 * U * m
        lpH = st["lp"] + st["H"][:, None]
        t1, t2 = st["p"] - m, ec * st["p"] * lpH
        bl.append(sw * (st["d_p"] + d_m + ec * (st["d_p"] * lpH.abs() + st["p"] * (st["d_lp"] + st["d_H"][:, None])))
                  + (r_W + 6 * U) * sw * (t1.abs() + t2.abs()))
        mlp = (m * st["lp"].abs()).sum(1)
        d_ce = d_ce + (d_m * st["lp"].abs() + m * st["d_lp"]).sum(1) + (math.ceil(n / 64) + 8) * U * mlp
        ce_abs = ce_abs + mlp
        cs = cand[torch.arange(B, device=logits.device), ref["jstar"], h].clamp(0, n - 1)
        lpa = st["lp"].gather(1, cs[:, None]).squeeze(1).abs()
        d_nll = d_nll + st["d_lse"] + U * lpa
        nll_abs = nll_abs + lpa
    d_ce = d_ce + nh * U * ce_abs
    d_nll = d_nll + nh * U * nll_abs
    d_ent = sum(st["d_H"] for st in hs if st["n"] > 1) + nh * U * sum(st["H"].abs() for st in hs)
    err = ref["err"]
    d_err = U * err.abs()
    out = dict(d_logits=torch.where(live[:, None], torch.cat(bl, 1), torch.zeros(B, sum(dims), dtype=F64, device=logits.device)))
    out["d_values"] = (wl / W) * 2 * vf * (d_err + (r_W + 6 * U) * err.abs())
    wm = lambda t: (wl * t).sum() / W  # noqa: E731
    lf = live.double()
    lm = lambda t: (lf * t).sum() / lf.sum()  # noqa: E731
    rs = 2 * r_W + 4 * U
    sb = [wm(d_ce) + rs * wm(ce_abs), wm(2 * err.abs() * d_err + U * err * err) + rs * wm(err * err), wm(d_ent) + rs * wm(ref["ent"].abs()),
          2 * U * ref["stats"][3], lm(d_nll) + rs * lm(nll_abs)]
    st = ref["stats"]
    sb.append(sb[0] + ec * sb[2] + vf * sb[1] + 3 * U * (st[0].abs() + (ec * st[2]).abs() + (vf * st[1]).abs()))
    sb += [torch.zeros((), dtype=F64, device=logits.device)] * 2
    out["stats"] = torch.stack([torch.as_tensor(s, dtype=F64, device=logits.device) for s in sb])
    return out
