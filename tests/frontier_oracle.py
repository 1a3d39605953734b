"""The frontier of gnbv_frontier_tri (csrc/frontier.hip) restated in plain numpy: integers only, so the comparison with the kernel is
exact on every u32 of the bits and every int32 of the block records.  A voxel is a frontier voxel iff it is unknown (== 0) and one
of its six face neighbours inside the grid is free (< 0)."""
import numpy as np


def frontier_bool(tri):
    """bool [N,G,G,G] from tri [N,G,G,G] (any signed dtype: < 0 free, 0 unknown, > 0 occupied).  The class array is padded with
    "occupied" on every side, so a neighbour outside the grid is no neighbour."""
    tri = np.asarray(tri)
    cls = np.sign(tri.astype(np.int64)).astype(np.int8)
    pad = np.pad(cls, ((0, 0), (1, 1), (1, 1), (1, 1)), constant_values=1)
    free = pad < 0
    near = np.zeros(cls.shape, bool)
    for ax in (1, 2, 3):
        for d in (0, 2):
            sl = [slice(None), slice(1, -1), slice(1, -1), slice(1, -1)]
            sl[ax] = slice(d, d + cls.shape[ax])
            near |= free[tuple(sl)]
    return near & (cls == 0)


def pack_words(front):
    """bool [N,G,G,G] (or [N,M]) -> uint32 [N, ceil(M / 32)], bit vox & 31 of word vox >> 5, padding bits clear."""
    flat = front.reshape(front.shape[0], -1)
    n, m = flat.shape
    words = (m + 31) // 32
    full = np.zeros((n, words * 32), bool)
    full[:, :m] = flat
    return (full.reshape(n, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def block_records(front, block):
    """int32 [N, nb^3, 4], nb = ceil(G / block): {count, sum x, sum y, sum z} of the frontier voxels of block (bx nb + by) nb + bz."""
    n, g = front.shape[0], front.shape[1]
    b = int(block)
    nb = (g + b - 1) // b
    out = np.zeros((n, nb ** 3, 4), np.int64)
    e, x, y, z = np.nonzero(front)
    rec = ((x // b) * nb + (y // b)) * nb + (z // b)
    for col, val in enumerate((np.ones_like(x), x, y, z)):
        np.add.at(out[:, :, col], (e, rec), val)
    return out.astype(np.int32)


def frontier(tri, block):
    """(words uint32 [N, ceil(G^3 / 32)], records int32 [N, nb^3, 4]) of tri [N,G,G,G]."""
    f = frontier_bool(tri)
    return pack_words(f), block_records(f, block)


def top_blocks(records, m):
    """Frontier.top restated: (index int64 [N,m], count int64 [N,m]), the m blocks of the largest count, ties to the lowest block
    index."""
    count = records[..., 0].astype(np.int64)
    nblk = count.shape[1]
    key = count * nblk + (nblk - 1 - np.arange(nblk))
    idx = np.argsort(-key, axis=1, kind="stable")[:, :m]
    return idx, np.take_along_axis(count, idx, 1)


def centroids(records, index, range_gt, voxel_size):
    """Frontier.centroids restated, fp64 [N,m,3]: c_a = o_a + (sum_a / count + 0.5) v_a with the voxel frame of gnbv_flight_blocked_tri
    (o_a = (double)fp32(range_gt[2a+1] - fp32(0.5f * v_a))); NaN where the block is empty."""
    f32, f64 = np.float32, np.float64
    r, vs = np.asarray(range_gt, f32), np.asarray(voxel_size, f32)
    o = (r[:, 1::2] - f32(0.5) * vs).astype(f32).astype(f64)
    rec = np.take_along_axis(records.astype(f64), index[..., None], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = rec[..., 1:] / rec[..., :1]
    return o[:, None] + (mean + 0.5) * vs.astype(f64)[:, None]
