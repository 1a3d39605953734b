"""Numpy reference of gnbv_cover_greedy (include/gennbv_hip.h): greedy set cover over per-candidate bit masks, in its
exhaustive form (the definition) and in the lazy form (upper bounds, refreshed in descending (bound, -j) order, `waves` per
pass, until the largest key belongs to a candidate refreshed this round).  All integers."""
import numpy as np

UNKNOWN = 2 ** 31 - 1


_BITS16 = np.unpackbits(np.arange(1 << 16, dtype=">u2").view(np.uint8).reshape(-1, 2), axis=1).sum(1).astype(np.int64)


def popcount(a):
    """uint32 [..., W] -> int64 [...]: set bits per row"""
    a = np.asarray(a, dtype=np.uint32)
    return (_BITS16[a & 0xFFFF] + _BITS16[a >> 16]).sum(-1)


def keys(score, k):
    """One key per candidate, strictly larger for the lower index at equal score (eval.baselines.choose)."""
    return score.astype(np.int64) * k + (k - 1 - np.arange(k))


def exhaustive(masks, covered, contact, rounds):
    """masks uint32 [K, W], covered uint32 [W], contact [K] -> (choice [T], gain [T], covered [W], gains0 [K])"""
    k = masks.shape[0]
    cov = covered.copy()
    choice, gain, gains0 = [], [], None
    for _ in range(rounds):
        g = popcount(masks & ~cov)
        if gains0 is None:
            gains0 = g.copy()
        b = int(keys(np.where(contact != 0, -1, g), k).argmax())
        choice.append(b)
        gain.append(int(g[b]))
        cov |= masks[b]
    return np.array(choice), np.array(gain), cov, gains0


def lazy(masks, covered, contact, rounds, ub=None, waves=4):
    """The same results from upper bounds -> (choice, gain, covered, ub at exit, evaluations made)"""
    k = masks.shape[0]
    cov = covered.copy()
    ub = np.full(k, UNKNOWN, np.int64) if ub is None else ub.astype(np.int64).copy()
    choice, gain, evals = [], [], 0
    for _ in range(rounds):
        fresh = np.zeros(k, bool)
        while True:
            key = keys(np.where(contact != 0, -1, ub), k)
            b = int(key.argmax())
            if fresh[b]:
                break
            todo = [j for j in np.argsort(-key, kind="stable") if not fresh[j]][:waves]
            for j in todo:
                ub[j] = popcount(masks[j] & ~cov)
                fresh[j] = True
                evals += 1
        choice.append(b)
        gain.append(int(ub[b]))
        cov |= masks[b]
    return np.array(choice), np.array(gain), cov, ub, evals


def random_masks(rng, k, words, density, valid_bits=None):
    """uint32 [k, words] with each bit set with probability `density`; bits from valid_bits on are zero"""
    m = np.packbits(rng.random((k, words, 32)) < density, axis=-1, bitorder="little").view(np.uint32).reshape(k, words)
    if valid_bits is not None:
        keep = np.packbits(np.arange(words * 32) < valid_bits, bitorder="little").view(np.uint32)
        m &= keep
    return m


def batch_exhaustive(masks, covered, contact, rounds):
    """masks [N, K, W], covered [N, W], contact [N, K] -> choice [N,T], gain [N,T], covered [N,W], gains0 [N,K]"""
    out = [exhaustive(masks[e], covered[e], contact[e], rounds) for e in range(masks.shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))
