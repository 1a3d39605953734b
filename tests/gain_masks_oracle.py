"""CPU oracle of the view-gain masks (include/gennbv_hip.h gnbv_view_gain_masks), composed from tests/view_gain_oracle.py.

TEST INFRASTRUCTURE.  Per env and candidate the rays' voxels come from `view_gain_oracle.ray_voxels`, the stop rule is
`view_gain_env`'s (in front of the first occupied voxel), and the two sets are written as bit masks: bit lin & 31 of word lin >> 5.
The camera matrices are an INPUT, as there.
"""
from __future__ import annotations

import numpy as np

from tests import view_gain_oracle as VO


def min_words(g: int) -> int:
    """The smallest legal row length: ceil(g^3 / 32) rounded up to a multiple of 4."""
    return ((g ** 3 + 31) // 32 + 3) // 4 * 4


def bits_of(lins, words: int) -> np.ndarray:
    """Distinct linear voxel indices -> uint32 [words] with bit lin & 31 of word lin >> 5 set."""
    out = np.zeros(words, np.uint32)
    lins = np.unique(np.asarray(lins, np.int64))
    np.bitwise_or.at(out, lins >> 5, (np.uint32(1) << (lins & 31).astype(np.uint32)))
    return out


def masks_env(tri, c2w, range_gt, voxel_size, inv_intri, h, w, stride, range_m, words):
    """One env: tri [g,g,g], c2w [K,4,4] -> (unknown_bits, hit_bits) uint32 [K, words]."""
    tri = np.asarray(tri)
    g = tri.shape[0]
    cls = np.sign(tri.reshape(-1).astype(np.int64))
    c2w = np.asarray(c2w, np.float32).reshape(-1, 4, 4)
    ub = np.zeros((c2w.shape[0], words), np.uint32)
    hb = np.zeros((c2w.shape[0], words), np.uint32)
    if VO.lattice_count(h, w, stride) == 0:
        return ub, hb
    steps = np.arange(3 * g)[None, :]
    for j in range(c2w.shape[0]):
        lin, valid = VO.ray_voxels(c2w[j], range_gt, voxel_size, inv_intri, h, w, stride, range_m, g)
        c = cls[lin]
        occ = (c == 1) & valid
        blocked = occ.any(1)
        stop = np.where(blocked, occ.argmax(1), 3 * g)  # the first occupied voxel: not counted
        unk = valid & (steps < stop[:, None]) & (c == 0)
        ub[j] = bits_of(lin[unk], words)
        hb[j] = bits_of(lin[unk & blocked[:, None]], words)
    return ub, hb


def masks(tri, c2w, range_gt, voxel_size, inv_intri, h, w, stride, range_m, words=None):
    """tri [N,g,g,g] or [N,g^3], c2w [N,K,4,4] -> (unknown_bits, hit_bits) uint32 [N, K, words] (words None: min_words(g))."""
    tri = np.asarray(tri)
    n = tri.shape[0]
    g = round(tri[0].size ** (1.0 / 3.0))
    assert g ** 3 == tri[0].size
    words = min_words(g) if words is None else int(words)
    c2w = np.asarray(c2w, np.float32).reshape(n, -1, 4, 4)
    out = [masks_env(tri[e].reshape(g, g, g), c2w[e], np.asarray(range_gt)[e], np.asarray(voxel_size)[e], inv_intri, h, w, stride,
                     range_m, words) for e in range(n)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def random_tri(n: int, g: int, occ, seed: int):
    """int8 torch [n, g^3]: occupied with density `occ`, 40 % of the rest free, the rest unknown (test_view_gain_gpu._random_tri's
    recipe); occ None: all unknown."""
    import torch
    if occ is None:
        return torch.zeros(n, g ** 3, dtype=torch.int8)
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(n, g ** 3, generator=gen)
    return torch.where(r < occ, 1, torch.where(r < occ + 0.4 * (1 - occ), -1, 0)).to(torch.int8)


def unpack(bits) -> np.ndarray:
    """uint32 [..., words] -> bool [..., words * 32], element lin = bit lin & 31 of word lin >> 5."""
    b = np.ascontiguousarray(np.asarray(bits).astype(np.uint32))
    return np.unpackbits(b.view(np.uint8).reshape(b.shape[:-1] + (-1,)), axis=-1, bitorder="little").astype(bool)
