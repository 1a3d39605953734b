"""Numpy reference of gnbv_cover_greedy_w (include/gennbv_hip.h): greedy set cover over P planes of per-candidate bit masks
under the score s_j = sum_p weight_p popcount(mask_p[j] & ~covered_p), in its exhaustive form (the definition) and in the lazy
form (upper bounds of the score, refreshed in descending (bound, -j) order, `waves` per pass, until the largest key belongs to
a candidate refreshed this round).  Built on cover_greedy_oracle's popcount and keys.  All integers."""
import numpy as np

from tests.cover_greedy_oracle import UNKNOWN, keys, popcount


def plane_gains(masks, cov):
    """masks: P arrays uint32 [K, W]; cov: P arrays uint32 [W] -> int64 [P, K]"""
    return np.stack([popcount(m & ~c) for m, c in zip(masks, cov)])


def scores(masks, cov, weights):
    """-> int64 [K]: sum_p weight_p g_pj"""
    return (np.asarray(weights, np.int64)[:, None] * plane_gains(masks, cov)).sum(0)


def exhaustive(masks, covered, weights, contact, rounds):
    """masks: P x uint32 [K, W]; covered: P x uint32 [W]; weights: P ints; contact [K]
    -> (choice [T], gain [T], plane_gain [T, P], covered P x [W], gains0 [K])"""
    k = masks[0].shape[0]
    cov = [c.copy() for c in covered]
    choice, gain, pgain, gains0 = [], [], [], None
    for _ in range(rounds):
        g = plane_gains(masks, cov)
        s = (np.asarray(weights, np.int64)[:, None] * g).sum(0)
        if gains0 is None:
            gains0 = s.copy()
        b = int(keys(np.where(contact != 0, -1, s), k).argmax())
        choice.append(b)
        gain.append(int(s[b]))
        pgain.append(g[:, b].copy())
        for p, m in enumerate(masks):
            cov[p] |= m[b]
    return np.array(choice), np.array(gain), np.array(pgain).reshape(rounds, len(masks)), cov, gains0


def lazy(masks, covered, weights, contact, rounds, ub=None, waves=4):
    """The same results from upper bounds of the score -> (choice, gain, plane_gain, covered, ub at exit, evaluations made)"""
    k = masks[0].shape[0]
    cov = [c.copy() for c in covered]
    w = np.asarray(weights, np.int64)
    ub = np.full(k, UNKNOWN, np.int64) if ub is None else ub.astype(np.int64).copy()
    choice, gain, pgain, evals = [], [], [], 0
    for _ in range(rounds):
        fresh = np.zeros(k, bool)
        while True:
            key = keys(np.where(contact != 0, -1, ub), k)
            b = int(key.argmax())
            if fresh[b]:
                break
            todo = [j for j in np.argsort(-key, kind="stable") if not fresh[j]][:waves]
            for j in todo:
                ub[j] = int(sum(int(w[p]) * int(popcount(m[j] & ~cov[p])) for p, m in enumerate(masks)))
                fresh[j] = True
                evals += 1
        choice.append(b)
        gain.append(int(ub[b]))
        pgain.append([int(popcount(m[b] & ~cov[p])) for p, m in enumerate(masks)])  # (the OR pass: before the OR)
        for p, m in enumerate(masks):
            cov[p] |= m[b]
    return np.array(choice), np.array(gain), np.array(pgain).reshape(rounds, len(masks)), cov, ub, evals


def batch_exhaustive(masks, covered, weights, contact, rounds):
    """masks: P x [N, K, W]; covered: P x [N, W]; contact [N, K]
    -> choice [N,T], gain [N,T], plane_gain [N,T,P], covered [P,N,W], gains0 [N,K]"""
    n = masks[0].shape[0]
    out = [exhaustive([m[e] for m in masks], [c[e] for c in covered], weights, contact[e], rounds) for e in range(n)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.stack([np.stack([o[3][p] for o in out]) for p in range(len(masks))]), np.stack([o[4] for o in out]))
