"""The depth sensor model restated in numpy from include/gennbv_hip.h (gnbv_depth_sensor): Philox4x32-10 in uint64, every other
operation in np.float32 (numpy rounds each fp32 operation once and fuses nothing, so the bits are the header's)."""
import numpy as np

NO_RETURN = np.float32(-2.0 ** -100)
MASK = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint64 arrays holding the 32-bit outputs."""
    c = [np.asarray(x).astype(np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def gauss_table():
    from statistics import NormalDist
    nd = NormalDist()
    return np.array([nd.inv_cdf((i + 0.5) / 4096) for i in range(4096)], np.float64)


def classify(depth, min_range, max_range):
    """-> (t, ret, miss, far, void) of f32 depth."""
    t = -depth
    fin = np.isfinite(t)
    ret = fin & (t >= np.float32(min_range)) & (t <= np.float32(max_range))
    miss = depth == -np.inf
    far = fin & (t > np.float32(max_range))
    return t, ret, miss, far, ~(ret | miss | far)


def drops(threshold, word):
    threshold = int(threshold)
    if threshold == 0xFFFFFFFF:
        return np.ones(word.shape, bool)
    return (word < np.uint64(threshold)) if threshold != 0 else np.zeros(word.shape, bool)


def edge_pixels(t, ret, radius, edge_abs, edge_rel):
    """[n,h,w] bool: step 2's verdict (meaningful on RET pixels)."""
    n, h, w = t.shape
    edge = np.zeros(t.shape, bool)
    if radius == 0:
        return edge
    thr = np.float32(edge_abs) + np.float32(edge_rel) * t
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if (dy == 0 and dx == 0) or abs(dy) >= h or abs(dx) >= w:
                continue
            py, px = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
            qy, qx = slice(max(0, dy), h + min(0, dy)), slice(max(0, dx), w + min(0, dx))
            tq, rq = t[:, qy, qx], ret[:, qy, qx]
            step = np.abs(tq - t[:, py, px]) > thr[:, py, px]
            edge[:, py, px] |= ~rq | (rq & step)
    return edge


def sensor(depth, seg, frame, P, lut=None, env0=0):
    """depth, seg f32 [n,h,w]; frame int32 [n]; P: dict of the struct's parameters (seed, min_range, max_range, edge_radius, edge_abs,
    edge_rel, edge_drop, drop, sigma0..2, quant).  env0: the env number of depth[0] (a slice of a batch).
    -> depth_out, seg_out, info (the masks the non-degeneracy checks read)."""
    depth, seg = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(seg, np.float32)
    n, h, w = depth.shape
    f32 = np.float32
    with np.errstate(all="ignore"):
        t, ret, miss, far, void = classify(depth, P["min_range"], P["max_range"])
        pix = (np.arange(h, dtype=np.uint64)[:, None] * np.uint64(w) + np.arange(w, dtype=np.uint64)[None, :])[None]
        env = (np.arange(n, dtype=np.uint64) + np.uint64(env0))[:, None, None]
        fr = (np.asarray(frame).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)[:, None, None]
        seed = int(P["seed"])
        w0, w1, w2, _ = philox4x32_10((pix, env, fr, np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))
        edge = edge_pixels(t, ret, P["edge_radius"], P["edge_abs"], P["edge_rel"]) & ret
        edge_dropped = edge & drops(P["edge_drop"], w0)
        rand_dropped = ret & drops(P["drop"], w1)
        dropped = edge_dropped | rand_dropped
        if lut is None:
            z = np.zeros(depth.shape, f32)
        else:
            z = np.asarray(lut, f32)[(w2 >> np.uint64(20)).astype(np.int64)]
        sigma = (f32(P["sigma0"]) + f32(P["sigma1"]) * t) + f32(P["sigma2"]) * (t * t)
        t1 = t + sigma * z
        q = f32(P["quant"])
        t2 = q / np.rint(q / t1) if q > 0 else t1
        t2 = t2.astype(f32)
        below = ret & ~dropped & ~(t2 >= f32(P["min_range"]))
        beyond = ret & ~dropped & ~below & (t2 > f32(P["max_range"]))
        kept = ret & ~dropped & ~below & ~beyond
        d_out = np.full(depth.shape, NO_RETURN, f32)
        d_out[miss | far | beyond] = -np.inf
        d_out[kept] = -t2[kept]
        s_out = np.zeros(depth.shape, f32)
        s_out.view(np.uint32)[kept] = seg.view(np.uint32)[kept]
    info = dict(ret=ret, miss=miss, far=far, void=void, edge=edge, edge_dropped=edge_dropped, rand_dropped=rand_dropped, below=below,
                beyond=beyond, kept=kept, t=t, t1=t1, t2=t2, z=z, w1=w1)
    return d_out, s_out, info
