"""Plain NumPy, float64 restatement of the conditional posteriors, the four cost scalars and the sufficient statistics
(include/phmrf.h, b3) that stays finite at the log-likelihoods a fit produces -- the yardstick of posterior_kernel.

oracle.ref_numpy.compute_posteriors_graph restates the reference's formula as written, exp(logprob - pp) without a
shift: with |logprob| in the thousands every exp underflows and the row is 0 / 0.  Both soft-maxes are invariant under
a per-row constant, so here the row maximum is subtracted before the exp; wherever the un-shifted formula is finite
the two agree to rounding (tests/test_posterior_reference.py).

  pp[i,k]  = sum_{e in inc(i)} V[l_other(e), k] * w'_e,   V = beta * (1 - delta),  w'_e = w_e if estimate_type == 3 else 1
             isolated node: pp[i,:] = V[l_i,:]
  post     = softmax_k(logprob - pp)            ppn = softmax_k(-pp)
  costs    = un-normalised sums over the nodes (include/phmrf.h):
             [0] sum_i sum_{e in inc(i)} V[l_other, l_i] * w'_e      [1] sum_i -log(ppn[i,l_i] + 1e-16)
             [2] sum_i -logprob[i,l_i]                                [3] [1] + [2]
  stats    = post | obs | obs*obs.T  (oracle.ref_numpy.sufficient_statistics)
"""
import numpy as np

from oracle import ref_numpy as R


def softmax_rows(a):
    """softmax over the last axis with the row maximum subtracted before the exp"""
    a = np.asarray(a, dtype=np.float64)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def posteriors_costs_stats(labels, logprob, X, edge_ids, w, beta, estimate_type):
    """-> (post[n,K], costs[4] un-normalised, stats dict with the keys post, obs, obs*obs.T)"""
    labels = np.asarray(labels).astype(np.int64)
    logprob = np.asarray(logprob, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    edge_ids = np.asarray(edge_ids, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64)
    n, K = logprob.shape
    V = R.potts_matrix(K, beta)
    pp = R.pairwise_compare(labels, edge_ids, w, V, estimate_type)
    post = softmax_rows(logprob - pp)
    ppn = softmax_rows(-pp)
    idx = np.arange(n)
    a, b = edge_ids[:, 0], edge_ids[:, 1]
    ww = w if estimate_type == 3 else np.ones_like(w)
    costs = np.empty(4)
    costs[0] = np.sum(V[labels[b], labels[a]] * ww) + np.sum(V[labels[a], labels[b]] * ww)
    costs[1] = -np.sum(np.log(ppn[idx, labels] + R.SMALL_EPS))
    costs[2] = -np.sum(logprob[idx, labels])
    costs[3] = costs[1] + costs[2]
    return post, costs, R.sufficient_statistics(post, X)
