"""mesh_io: read a Wavefront OBJ scene into MeshScene.from_triangles' per-env input.

    tris, ids = load_obj("house.obj")               # [T,3,3] f32, [T] i32
    mesh = MeshScene.from_triangles([tris], [ids], device="cuda:0")
    gt = mesh.ground_truth(cfg.grid_size)           # grid_gt from the same triangles

Only geometry is read: `v` positions and `f` faces (`i`, `i/t`, `i//n`, `i/t/n` references, negative = relative to
the last vertex so far); polygons are fan-triangulated.  Object ids number the `o` / `g` names in order of first
appearance from 1; faces before any name get id 1.  Every other record (vt, vn, usemtl, s, l, ...) is ignored.
"""
from __future__ import annotations

from typing import Tuple

import torch


def _ref(tok: str, nverts: int, where: str) -> int:
    head = tok.split("/", 1)[0]
    try:
        i = int(head)
    except ValueError:
        raise ValueError(f"{where}: bad vertex reference {tok!r}") from None
    k = i - 1 if i > 0 else nverts + i
    if i == 0 or not 0 <= k < nverts:
        raise ValueError(f"{where}: vertex reference {i} out of range ({nverts} vertices so far)")
    return k


def load_obj(path: str, up: str = "z", recenter: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(triangles [T,3,3] f32, object ids [T] i32) of an OBJ file.

    up="y" rotates a Y-up file to Z-up ((x, y, z) -> (x, -z, y)).  recenter moves the centre of the triangles' xy
    bounding box to 0 and their lowest z to 0: the reference's scene frame, which MeshScene.grid_spec's default range
    assumes.  Malformed input raises ValueError naming the line."""
    if up not in ("z", "y"):
        raise ValueError(f"up must be 'z' or 'y', got {up!r}")
    verts, faces, fids = [], [], []
    names = {}
    cur = 1
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            tok = line.split()
            where = f"{path}:{ln}"
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{where}: a vertex needs x y z")
                try:
                    verts.append([float(t) for t in tok[1:4]])
                except ValueError:
                    raise ValueError(f"{where}: bad vertex {line!r}") from None
            elif tok[0] == "f":
                if len(tok) < 4:
                    raise ValueError(f"{where}: a face needs at least 3 vertices")
                idx = [_ref(t, len(verts), where) for t in tok[1:]]
                for j in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[j], idx[j + 1]))
                    fids.append(cur)
            elif tok[0] in ("o", "g"):
                name = " ".join(tok[1:])
                cur = names.setdefault(name, len(names) + 1)
    v = torch.tensor(verts, dtype=torch.float64).reshape(-1, 3)
    if not torch.isfinite(v).all():
        raise ValueError(f"{path}: vertex coordinates must be finite")
    if up == "y":
        v = torch.stack([v[:, 0], -v[:, 2], v[:, 1]], -1)
    tris = v[torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)]  # [T,3,3]
    if recenter and tris.shape[0]:
        p = tris.reshape(-1, 3)
        lo, hi = p.amin(0), p.amax(0)
        shift = torch.stack([0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), lo[2]])
        tris = tris - shift
    return tris.to(torch.float32).contiguous(), torch.tensor(fids, dtype=torch.int32)
