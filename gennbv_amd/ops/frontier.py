"""Frontier: the boundary between what the scanned map knows to be free and what it does not know (csrc/frontier.hip).

    fr = Frontier(num_envs, grid_size, block=4, device="cuda:0")
    blocks = fr(tri)                       # one launch: int32 [N, nb^3, 4] = {count, sum x, sum y, sum z} per block of block^3 voxels
    fr.count()                             # int64 [N]: frontier voxels per env
    idx, cnt = fr.top(8)                   # the 8 blocks holding the most frontier voxels, ties to the lowest block index
    c = fr.centroids(idx, range_gt, voxel_size)   # fp64 [N,8,3] world xyz of their frontier centroids (NaN where a block is empty)

A voxel is a frontier voxel iff it is unknown and one of its six face neighbours inside the grid is free (include/gennbv_hip.h:
gnbv_frontier_tri).  `tri` is the tri-class grid in either form BeliefFlightField.refresh takes: int8 [N, >= G^3] or the fp32 grid
slice of an observation, obs[:, state_dim:state_dim + grid_dim], any row stride.  With `keep_bits` the kernel also writes one bit
per voxel into `bits` [N, ceil(G^3 / 32)].  GPU only; `top` and `centroids` are torch on whatever device the records live on.
"""
from __future__ import annotations

from typing import Tuple

import torch

from .. import _lib


def block_grid(grid_size: int, block: int) -> int:
    """nb = ceil(G / block): blocks per axis."""
    return (int(grid_size) + int(block) - 1) // int(block)


def top_blocks(blocks: torch.Tensor, m: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(block_index int64 [N,m], count int64 [N,m]) of blocks [N, nb^3, 4]: the m records of the largest count; the key
    count * nb^3 + (nb^3 - 1 - b) is distinct per block, so torch.topk has a single answer on every device: ties go to the lowest
    block index."""
    count = blocks[..., 0].to(torch.int64)
    nblk = count.shape[1]
    if not 1 <= int(m) <= nblk:
        raise ValueError(f"top: m must be in 1..{nblk}, got {m}")
    key = count * nblk + (nblk - 1 - torch.arange(nblk, device=count.device))
    idx = torch.topk(key, int(m), dim=1).indices
    return idx, count.gather(1, idx)


def block_centroids(blocks: torch.Tensor, index: torch.Tensor, range_gt: torch.Tensor, voxel_size: torch.Tensor) -> torch.Tensor:
    """fp64 [N,m,3]: c_a = o_a + (sum_a / count + 0.5) v_a of the records blocks[e, index[e, j]], in the voxel frame of
    gnbv_flight_blocked_tri: v_a = (double)voxel_size[a], o_a = (double)fp32(range_gt[2a+1] - fp32(0.5f * voxel_size[a])).  NaN where
    the block is empty."""
    dev = blocks.device
    vs = voxel_size.to(dev, torch.float32)
    o = (range_gt.to(dev, torch.float32)[:, 1::2] - 0.5 * vs).double()  # the subtraction in fp32, then widened
    rec = blocks.gather(1, index[..., None].expand(-1, -1, 4)).double()
    return o[:, None] + (rec[..., 1:] / rec[..., :1] + 0.5) * vs.double()[:, None]


class Frontier:
    def __init__(self, num_envs: int, grid_size: int, block: int = 4, device="cuda:0", keep_bits: bool = False, slab: int = 0):
        n, g, b = int(num_envs), int(grid_size), int(block)
        if n < 1 or not 1 <= g <= 128 or not 1 <= b <= 16 or int(slab) < 0:
            raise ValueError(f"Frontier: num_envs >= 1, grid_size in 1..128, block in 1..16, slab >= 0; got {num_envs}, {grid_size}, "
                             f"{block}, {slab}")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.GennbvHipError("Frontier runs on the GPU only (no CPU fallback)")
        self.lib = _lib.load()
        self.num_envs, self.grid_size, self.block, self.slab, self.device = n, g, b, int(slab), device
        self.nb = block_grid(g, b)
        self.blocks = torch.zeros(n, self.nb ** 3, 4, dtype=torch.int32, device=device)
        self.bits = torch.zeros(n, (g ** 3 + 31) // 32, dtype=torch.int32, device=device) if keep_bits else None  # u32 bits
        self.launches = 0

    def __call__(self, tri: torch.Tensor) -> torch.Tensor:
        """One gnbv_frontier_tri launch on the current stream into `blocks` (and `bits`); returns `blocks`."""
        n, g3 = self.num_envs, self.grid_size ** 3
        _lib.check(self.lib.gnbv_frontier_tri(*_lib.tri_args(tri, n, g3, "Frontier"), self.grid_size, n, self.block, _lib.ptr(self.bits),
                                              self.blocks.data_ptr(), self.slab, _lib.stream_ptr(self.device)), "gnbv_frontier_tri")
        self.launches += 1
        return self.blocks

    def count(self) -> torch.Tensor:
        """int64 [N]: the frontier voxels of each env at the last call."""
        return self.blocks[..., 0].sum(dim=1)

    def top(self, m: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return top_blocks(self.blocks, m)

    def centroids(self, index: torch.Tensor, range_gt: torch.Tensor, voxel_size: torch.Tensor) -> torch.Tensor:
        return block_centroids(self.blocks, index, range_gt, voxel_size)
