"""numpy / plain-Python restatement of the summaries of a closure study (gpbayestools_hic_amd/closure.py: ClosureResult), written
element by element from their definitions:
    rank[k, j]       the number of stored samples of set k strictly below truths[k, j]
    coverage(level)  per parameter the share of sets with |rank / n - 1/2| <= level / 2: the truth inside the central interval
    histogram(bins)  per parameter the sets counted by min(rank * bins // n, bins - 1)
"""
import numpy as np


def rank(chain, truths):
    """chain [K, nwalkers, nstored, ndim], truths [K, ndim] -> [K, ndim] int64"""
    K, _, _, d = chain.shape
    out = np.zeros((K, d), dtype=np.int64)
    for k in range(K):
        for j in range(d):
            out[k, j] = int((chain[k, :, :, j] < truths[k, j]).sum())
    return out


def coverage(rk, n, level):
    K, d = rk.shape
    out = np.zeros(d)
    for j in range(d):
        hits = 0
        for k in range(K):
            if abs(int(rk[k, j]) / n - 0.5) <= level / 2:
                hits += 1
        out[j] = hits / K
    return out


def histogram(rk, n, bins):
    K, d = rk.shape
    out = np.zeros((d, bins), dtype=np.int64)
    for j in range(d):
        for k in range(K):
            out[j, min(int(rk[k, j]) * bins // n, bins - 1)] += 1
    return out
