"""Plain NumPy, float64 restatement of phmrf_ancestral (include/phmrf.h): the posterior-weighted and the called-state affine
maps of the observations, from the posteriors `post` [n, K], the labels [n], the observations X [n, S] and the tables
affine [K, A, S+1] (c, then the row of G) and cond_var [K, A] -- the yardstick of ancestral_kernel, with the per-element
error bounds of its float32 arithmetic, and the simulation of the tree recursion the tables are checked against.

    mu[i, k, a] = c[k, a] + sum_s G[k, a, s] X[i, s]
    posterior:  mean[a, i] = sum_k post[i, k] mu[i, k, a]
                var[a, i]  = sum_k post[i, k] (v[k, a] + (mu[i, k, a] - mean[a, i])^2)
    called:     mean[a, i] = mu[i, l_i, a],   var[a, i] = v[l_i, a]
"""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of float32
POST_TOL = 2e-5                 # the pinned bound of the device's posteriors, per entry (tests/posterior_cases.py)


def state_maps(X, affine):
    """-> mu [n, K, A]"""
    X = np.asarray(X, dtype=np.float64)
    affine = np.asarray(affine, dtype=np.float64)
    return affine[None, :, :, 0] + np.einsum("kas,ns->nka", affine[:, :, 1:], X)


def reconstruct(post, labels, X, affine, cond_var, weighting):
    """-> (mean [A, n], var [A, n]) in float64"""
    mu = state_maps(X, affine)
    v = np.asarray(cond_var, dtype=np.float64)
    if weighting == "called":
        lab = np.asarray(labels).astype(np.int64)
        return mu[np.arange(len(lab)), lab].T.copy(), v[lab].T.copy()
    assert weighting == "posterior", weighting
    p = np.asarray(post, dtype=np.float64)
    mean = np.einsum("nk,nka->na", p, mu)
    var = np.einsum("nk,nka->na", p, v[None] + (mu - mean[:, None, :]) ** 2)
    return mean.T.copy(), var.T.copy()


def bounds(post, labels, X, affine, cond_var, weighting):
    """-> (mean_bound [A, n], var_bound [A, n]): per element, what float32 arithmetic in the kernel's order may differ from
    reconstruct() by, with u = 2^-24 and the device's posteriors within POST_TOL of `post` per entry.

    One map mu_ka(x) is c and S fused multiply-adds: S roundings, each relative to a partial sum of at most
    M_ka = |c| + sum_s |G_s x_s|, so (S + 2) 2u M_ka with two roundings to spare                           ... eps_mu
    called mean:     that map of the called state.
    called variance: sd = sqrtf(v) within one ulp (2u relative), squared by the test: 5u v.
    posterior mean:  sum_k dp_k mu_k = sum_k dp_k (mu_k - ref) + ref sum_k dp_k: the first term is at most
                     POST_TOL sum_k |mu_k - ref|; the device's p sums to 1 within its own roundings, which with the K
                     accumulating fmaf (each relative to a partial sum of at most max_k |mu_k| <= max_k M_k) and the maps'
                     own error is (K + S + 2) 2u max_k M_k                                                  ... E_m
    variance (sd^2): with t_k = v_k + (mu_k - m)^2: the posteriors POST_TOL sum_k t_k; the error of the device's
                     d_k = mu_k - mean, at most eps_mu,k + E_m, enters t_k as 2 |mu_k - m| (eps_mu,k + E_m); the
                     subtraction, the two fmaf of t_k and of the sum, the K accumulations (all terms >= 0), sqrtf and the
                     test's squaring: (K + 4) 2u sum_k p_k t_k."""
    X = np.asarray(X, dtype=np.float64)
    affine = np.asarray(affine, dtype=np.float64)
    v = np.asarray(cond_var, dtype=np.float64)
    K, A, S1 = affine.shape
    S = S1 - 1
    M = np.abs(affine[None, :, :, 0]) + np.einsum("kas,ns->nka", np.abs(affine[:, :, 1:]), np.abs(X))      # [n, K, A]
    eps_mu = (S + 2) * 2 * U * M
    if weighting == "called":
        lab = np.asarray(labels).astype(np.int64)
        return eps_mu[np.arange(len(lab)), lab].T.copy(), 5 * U * v[lab].T
    assert weighting == "posterior", weighting
    p = np.asarray(post, dtype=np.float64)
    mu = state_maps(X, affine)
    mean = np.einsum("nk,nka->na", p, mu)
    dev = np.abs(mu - mean[:, None, :])
    E_m = POST_TOL * dev.sum(axis=1) + (K + S + 2) * 2 * U * M.max(axis=1)                                 # [n, A]
    t = v[None] + dev ** 2
    E_v = (POST_TOL * t.sum(axis=1) + np.einsum("nk,nka->na", p, 2 * dev * (eps_mu + E_m[:, None, :]))
           + (K + 4) * 2 * U * np.einsum("nk,nka->na", p, t))
    return E_m.T.copy(), E_v.T.copy()


def simulate(tree, params, n, rng):
    """n draws of ALL tree nodes of ONE state by node_moments' recursion: X_root ~ N(theta_root, v0),
    X_i = e_i X_parent + (1 - e_i) theta_i + eps_i, Var eps_i = ratio_i (1 - e_i^2)  -> Z [n, N]"""
    v0, beta, lam, theta = tree.split(np.asarray(params, dtype=np.float64))
    _, _, e, ratio = tree.node_moments(params)
    Z = np.zeros((n, tree.node_num))
    for r in np.flatnonzero(tree.parent < 0):
        Z[:, r] = theta[r] + np.sqrt(v0) * rng.standard_normal(n)
    for i in tree.order:
        sd = np.sqrt(ratio[i] * (1.0 - e[i] ** 2))
        Z[:, i] = e[i] * Z[:, tree.parent[i]] + (1.0 - e[i]) * theta[i] + sd * rng.standard_normal(n)
    return Z
