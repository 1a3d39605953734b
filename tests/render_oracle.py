"""fp64 brute-force ray / triangle oracle of the closed-loop renderer (csrc/render.hip), plain torch.

The rays are rebuilt bit for bit as the kernel builds them (fp32, same operation order: cam = Kinv (u, v, 1), d = R cam),
then every ray is intersected with every triangle of its env in fp64 (Moller-Trumbore, edges inclusive) and with the
ground plane z = 0.  Only the intersection arithmetic differs from the kernel's, which is what the tests measure.
"""
from __future__ import annotations

import torch

T_MIN = 1e-3


def rays(c2w: torch.Tensor, kinv: torch.Tensor, h: int, w: int):
    """fp32 origins [N,3] and directions [N,H,W,3] exactly as k_render_depth computes them."""
    dev = c2w.device
    k = kinv.to(dev, torch.float32)
    u = torch.arange(w, device=dev, dtype=torch.float32)[None, :].expand(h, w)
    v = torch.arange(h, device=dev, dtype=torch.float32)[:, None].expand(h, w)
    cam = [k[i, 0] * u + k[i, 1] * v + k[i, 2] for i in range(3)]  # each op rounded to fp32 like the kernel (no FMA)
    m = c2w.to(torch.float32)
    d = [m[:, i, 0, None, None] * cam[0] + m[:, i, 1, None, None] * cam[1] + m[:, i, 2, None, None] * cam[2] for i in range(3)]
    return m[:, :3, 3].clone(), torch.stack(d, -1)


def render(tris_per_env, ids_per_env, c2w: torch.Tensor, kinv: torch.Tensor, h: int, w: int, chunk: int = 2048):
    """-> t [N,H,W] f64 (inf: miss), obj [N,H,W] int64 (0: ground / miss)."""
    o32, d32 = rays(c2w, kinv, h, w)
    n = c2w.shape[0]
    dev = c2w.device
    t_out = torch.full((n, h * w), float("inf"), dtype=torch.float64, device=dev)
    obj_out = torch.zeros(n, h * w, dtype=torch.int64, device=dev)
    for e in range(n):
        o = o32[e].double()
        d = d32[e].reshape(-1, 3).double()
        dz32 = d32[e].reshape(-1, 3)[:, 2]
        tg = -o[2] / d[:, 2]
        tg = torch.where((dz32 < -1e-6) & (tg > T_MIN), tg, torch.full_like(tg, float("inf")))
        best, obj = tg.clone(), torch.zeros(h * w, dtype=torch.int64, device=dev)
        tri = tris_per_env[e].to(dev, torch.float64)
        ids = ids_per_env[e].to(dev, torch.int64)
        if tri.shape[0]:
            v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]  # [T,3]
            s = o[None] - v0  # [T,3]
            for a in range(0, h * w, chunk):
                dd = d[a:a + chunk]  # [R,3]
                p = torch.cross(dd[:, None, :].expand(-1, tri.shape[0], -1), e2[None].expand(dd.shape[0], -1, -1), dim=-1)
                det = (e1[None] * p).sum(-1)  # [R,T]
                inv = 1.0 / det
                bu = (s[None] * p).sum(-1) * inv
                q = torch.cross(s, e1, dim=-1)  # [T,3]
                bv = (dd @ q.T) * inv
                t = (e2 * q).sum(-1)[None] * inv
                ok = (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > T_MIN)
                t = torch.where(ok, t, torch.full_like(t, float("inf")))
                tmin, arg = t.min(-1)
                closer = tmin < best[a:a + chunk]
                best[a:a + chunk] = torch.where(closer, tmin, best[a:a + chunk])
                obj[a:a + chunk] = torch.where(closer, ids[arg], obj[a:a + chunk])
        t_out[e], obj_out[e] = best, obj
    return t_out.view(n, h, w), obj_out.view(n, h, w)


def silhouette(obj: torch.Tensor) -> torch.Tensor:
    """Pixels [N,H,W] whose 3x3 neighbourhood holds more than one object id (0 = ground / sky counts as one)."""
    x = obj.double()[:, None]
    mx = torch.nn.functional.max_pool2d(x, 3, 1, 1)
    mn = -torch.nn.functional.max_pool2d(-x, 3, 1, 1)
    return (mx != mn)[:, 0]


def shade(obj: torch.Tensor) -> torch.Tensor:
    """synthetic.render_depth's RGBA for object ids obj [...] (0: ground / sky)."""
    s = (obj * 29 % 200 + 40).to(torch.uint8)
    is_obj = obj > 0
    out = torch.empty(*obj.shape, 4, dtype=torch.uint8, device=obj.device)
    out[..., 0] = torch.where(is_obj, s, torch.full_like(s, 90))
    out[..., 1] = torch.where(is_obj, 255 - s, torch.full_like(s, 120))
    out[..., 2] = torch.where(is_obj, s // 2 + 60, torch.full_like(s, 70))
    out[..., 3] = 255
    return out
