"""The contract of include/tsf.h "tree reconciliation" restated in numpy, for tests/test_tree_ref.py (CPU) and
tests/test_gpu_tree.py.  Every function performs the header's operations in the header's order on float64 arrays
(numpy's elementwise +, -, *, / are the IEEE operations; nothing here fuses), so a comparison with the library is bit
for bit.  A tree is (group [N], n_nodes [L], parent: L - 1 arrays), levels 1 .. L; per-level quantities are lists of L
arrays.  `dense` is the projection the recursion stands for, solved as a dense weighted least squares problem in
np.longdouble; solve_errors is the running error analysis the tests' bounds come from."""
import numpy as np

U = 2.0 ** -53      # the unit roundoff of float64

# The tree of the tests: 9 members in 5 groups (group 3 empty; groups 1 and 3 without a total), 3 parents (parent 2 has a
# single child, parent 0 no total), one root
GROUP = np.array([0, 1, 1, 2, 2, 2, 2, 4, 4], dtype=np.int64)
N_NODES = [5, 3, 1]
PARENT = [np.array([0, 0, 1, 1, 2], dtype=np.int64), np.array([0, 0, 0], dtype=np.int64)]
V = [np.array([1.3, np.nan, 2.0, np.nan, 0.7]), np.array([np.nan, 1.1, 0.9]), np.array([2.5])]


def shares(group, w, n_nodes, parent, v):
    """tsf_reconcile_tree_shares: w [N] or None (all 1.0); v: per level [n] (NaN: no total) ->
    (share [N], mu, e, kappa per level)"""
    group = np.asarray(group, dtype=np.int64)
    N, L = len(group), len(n_nodes)
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    E = np.zeros(n_nodes[0])
    for n in range(N):
        E[group[n]] = E[group[n]] + w[n]
    share = np.zeros(N)
    for n in range(N):
        share[n] = w[n] / E[group[n]]
    mu, e, kappa = [], [], []
    for k in range(L):
        vk = np.asarray(v[k], dtype=np.float64)
        m, ee = np.zeros(n_nodes[k]), np.zeros(n_nodes[k])
        for i in range(n_nodes[k]):
            if not np.isnan(vk[i]) and E[i] > 0.0:
                m[i] = E[i] / (vk[i] + E[i])
                ee[i] = (E[i] * vk[i]) / (vk[i] + E[i])
            else:
                ee[i] = E[i]
        mu.append(m)
        e.append(ee)
        ka = np.zeros(n_nodes[k])
        if k + 1 < L:
            Ep = np.zeros(n_nodes[k + 1])
            for c in range(n_nodes[k]):
                Ep[parent[k][c]] = Ep[parent[k][c]] + ee[c]
            for c in range(n_nodes[k]):
                if Ep[parent[k][c]] != 0.0:
                    ka[c] = ee[c] / Ep[parent[k][c]]
            E = Ep
        kappa.append(ka)
    return share, mu, e, kappa


def gather(m, parent, n):
    """A_p = the sum of the children's m from +0.0 in ascending child index; m [n_children][...] -> [n][...]"""
    A = np.zeros((n,) + m.shape[1:])
    for c in range(len(m)):
        A[parent[c]] = A[parent[c]] + m[c]
    return A


def solve(acc, tot, has, n_nodes, parent, mu, kappa):
    """tsf_rollup_solve_tree on cells of any trailing shape: acc [G][...]; tot, has per level ([n][...] or None, [n] of
    0 / 1 or None: no total at that level) -> (delta [G][...] = c_1 - acc, c per level, A per level); c[0] is the
    level-1 c itself (what the library does not keep: tsf_rollup_tree_totals reads acc + delta there)"""
    L = len(n_nodes)
    A, m = [acc], []
    for k in range(L):
        if k:
            A.append(gather(m[k - 1], parent[k - 1], n_nodes[k]))
        mk = A[k].copy()
        for i in range(n_nodes[k]):
            if has[k] is not None and has[k][i]:
                mk[i] = A[k][i] + mu[k][i] * (tot[k][i] - A[k][i])
        m.append(mk)
    c = [None] * L
    c[L - 1] = m[L - 1]
    for k in range(L - 2, -1, -1):
        ck = np.empty_like(m[k])
        for i in range(n_nodes[k]):
            p = parent[k][i]
            ck[i] = m[k][i] + kappa[k][i] * (c[k + 1][p] - A[k + 1][p])
        c[k] = ck
    return c[0] - acc, c, A


def members(x, group, share, delta):
    """x [N][...] -> x + share[n] * delta[group[n]]"""
    out = np.empty_like(x)
    for n in range(len(x)):
        out[n] = x[n] + share[n] * delta[group[n]]
    return out


def group_totals(acc, delta):
    """tsf_rollup_tree_totals at level 1: acc + delta"""
    return acc + delta


def dense(x, w, group, n_nodes, parent, tot, v):
    """The weighted least squares projection, dense, in np.longdouble: minimise sum_i (x_i - b_i)^2 / w_i +
    sum_n (t_n - c_n)^2 / v_n over the members b, c_n the sum of the b_i below node n; nodes whose v is NaN or which
    have no member carry no total.  x [N][S], tot per level [n][S] -> (b [N][S] (longdouble), its own error [S]), by
    Gaussian elimination with partial pivoting on the normal equations (numpy's solvers do not take longdouble).  The
    error allowed for the reference itself: forming the equations and solving them loses at most about
    4 N cond(M) 2^-64 relative to the largest |b_i| of the cell (2^-64: longdouble's unit roundoff; M is symmetric
    positive definite, so elimination has no growth)."""
    ld = np.longdouble
    N = len(group)
    Sm = np.zeros((n_nodes[0], N), dtype=ld)
    Sm[np.asarray(group), np.arange(N)] = 1
    rows, var, yh = [np.eye(N, dtype=ld)], [np.asarray(w, dtype=ld)], [np.asarray(x, dtype=ld)]
    for k in range(len(n_nodes)):
        if k:
            up = np.zeros((n_nodes[k], n_nodes[k - 1]), dtype=ld)
            up[np.asarray(parent[k - 1]), np.arange(n_nodes[k - 1])] = 1
            Sm = up @ Sm
        vk = np.asarray(v[k], dtype=np.float64)
        keep = ~np.isnan(vk) & (Sm.sum(axis=1) > 0)
        if keep.any():
            rows.append(Sm[keep])
            var.append(vk[keep].astype(ld))
            yh.append(np.asarray(tot[k], dtype=ld)[keep])
    Sa, Wi, ya = np.vstack(rows), 1 / np.concatenate(var), np.vstack(yh)
    M = Sa.T @ (Wi[:, None] * Sa)
    b = Sa.T @ (Wi[:, None] * ya)
    cond = float(np.linalg.cond(M.astype(np.float64)))
    for i in range(N):
        j = i + int(np.argmax(np.abs(M[i:, i])))
        M[[i, j]], b[[i, j]] = M[[j, i]], b[[j, i]]
        for r in range(i + 1, N):
            f = M[r, i] / M[i, i]
            M[r] = M[r] - f * M[i]
            b[r] = b[r] - f * b[i]
    out = np.zeros_like(b)
    for i in range(N - 1, -1, -1):
        out[i] = (b[i] - M[i, i + 1:] @ out[i + 1:]) / M[i, i]
    return out, 4 * N * cond * 2.0 ** -64 * np.abs(out).max(axis=0).astype(np.float64)


def scalar_roundings(group, n_nodes, parent, v):
    """How many relative roundings u the computed share, mu and kappa carry at most, first order, from the operations of
    tsf_reconcile_tree_shares (all of them on positive numbers: no cancellation, so relative errors add):
      W_g, a sum of n_g weights: n_g - 1;  share = w / W: n_g
      mu = E / (v + E): r_E for E, r_E + 1 for the add, 1 for the divide: 2 r_E + 2
      e = (E v) / (v + E): (r_E + 1) + (r_E + 1) + 1 = 2 r_E + 3;  e = E without a total: r_E
      E_p, a sum of n_c values e_c: max r_e + n_c - 1;  kappa = e / E_p: r_e + r_Ep + 1
    -> (r_share [N], r_mu, r_kappa per level)"""
    group = np.asarray(group, dtype=np.int64)
    n_g = np.bincount(group, minlength=n_nodes[0])
    r_E = np.maximum(n_g - 1, 0).astype(np.float64)
    r_share = n_g[group].astype(np.float64)
    r_mu, r_kappa = [], []
    for k in range(len(n_nodes)):
        has = ~np.isnan(np.asarray(v[k], dtype=np.float64))
        r_mu.append(2 * r_E + 2)
        r_e = np.where(has, 2 * r_E + 3, r_E)
        if k + 1 < len(n_nodes):
            n_c = np.bincount(parent[k], minlength=n_nodes[k + 1])
            r_Ep = np.zeros(n_nodes[k + 1])
            np.maximum.at(r_Ep, parent[k], r_e)
            r_Ep = r_Ep + np.maximum(n_c - 1, 0)
            r_kappa.append(r_e + r_Ep[parent[k]] + 1)
            r_E = r_Ep
        else:
            r_kappa.append(np.zeros(n_nodes[k]))
    return r_share, r_mu, r_kappa


def _sum_err(err, mag, index, n):
    """the error of a sum from +0.0 of the values with errors err and magnitudes mag, gathered by index into n cells:
    the summands' errors plus (count - 1) u sum |summand|"""
    cnt = np.bincount(index, minlength=n)
    extra = np.maximum(cnt - 1, 0).reshape((n,) + (1,) * (mag.ndim - 1))
    return gather(err, index, n) + extra * U * gather(mag, index, n)


def _scaled_err(s, r_s, d, e_d):
    """the error of fl(s * d), s a computed scalar in [0, 1] with r_s relative roundings, d computed with error e_d:
    s e_d + r_s u s |d| + u |s d|"""
    s, r_s = (np.reshape(a, (-1,) + (1,) * (d.ndim - 1)) for a in (s, r_s))
    return s * e_d + (r_s + 1) * U * s * np.abs(d)


def solve_errors(x, group, share, tot, has, n_nodes, parent, mu, kappa, v):
    """A running first-order error analysis of the recursion: a bound on |computed - exact| for the members' result, the
    group totals acc + delta and every upper level's c, `exact` being the recursion in exact arithmetic on the same
    inputs x and t with exact scalars (which is the weighted least squares projection).  Every operation of solve and
    members is followed with the two rules  |fl(a op b) - (a op b)| <= u |fl(a op b)|  and
    err(a +- b) <= err(a) + err(b),  err(s d) <= s err(d) + r_s u s |d|  for a scalar s in [0, 1] with r_s relative
    roundings (scalar_roundings); magnitudes are taken from the computed values.  Terms of second order in u are below
    2^-40 of the first-order ones (a few hundred operations at most): the result is multiplied by 1 + 2^-30.
    -> (e_members [N][...], e_level per level: [n][...])"""
    r_share, r_mu, r_kappa = scalar_roundings(group, n_nodes, parent, v)
    L = len(n_nodes)
    acc = gather(x, group, n_nodes[0])
    e_acc = _sum_err(np.zeros_like(x), np.abs(x), group, n_nodes[0])
    A, eA, m, em = [acc], [e_acc], [], []
    for k in range(L):
        if k:
            A.append(gather(m[k - 1], parent[k - 1], n_nodes[k]))
            eA.append(_sum_err(em[k - 1], np.abs(m[k - 1]), parent[k - 1], n_nodes[k]))
        mk, ek = A[k].copy(), eA[k].copy()
        for i in range(n_nodes[k]):
            if has[k] is not None and has[k][i]:
                d = tot[k][i] - A[k][i]
                e_d = eA[k][i] + U * np.abs(d)
                mk[i] = A[k][i] + mu[k][i] * d
                ek[i] = eA[k][i] + _scaled_err(mu[k][i], r_mu[k][i], d[None], e_d[None])[0] + U * np.abs(mk[i])
        m.append(mk)
        em.append(ek)
    c, ec = [None] * L, [None] * L
    c[L - 1], ec[L - 1] = m[L - 1], em[L - 1]
    for k in range(L - 2, -1, -1):
        p = parent[k]
        d = c[k + 1][p] - A[k + 1][p]
        e_d = ec[k + 1][p] + eA[k + 1][p] + U * np.abs(d)
        kap = np.reshape(kappa[k], (-1,) + (1,) * (d.ndim - 1))
        c[k] = m[k] + kap * d
        ec[k] = em[k] + _scaled_err(kappa[k], r_kappa[k], d, e_d) + U * np.abs(c[k])
    delta = c[0] - acc
    e_delta = ec[0] + e_acc + U * np.abs(delta)
    dm = delta[group]
    sh = np.reshape(share, (-1,) + (1,) * (x.ndim - 1))
    b = x + sh * dm
    e_b = _scaled_err(share, r_share, dm, e_delta[group]) + U * np.abs(b)
    e_c1 = e_acc + e_delta + U * np.abs(acc + delta)
    f = 1 + 2.0 ** -30
    return e_b * f, [e_c1 * f] + [e * f for e in ec[1:]]


def two_level_error(x, group, lam, top, has_top):
    """The same analysis of the two-level contract (tests/reconcile_ref.py: x + lam (top - acc), lam = w / (v + W), which
    carries n_g + 1 relative roundings: the sum, the add, the divide) -> e [N][...]"""
    G = len(top)
    acc = gather(x, group, G)
    e_acc = _sum_err(np.zeros_like(x), np.abs(x), group, G)
    n_g = np.bincount(group, minlength=G)
    out = np.zeros_like(x)
    for n in range(len(x)):
        g = group[n]
        if has_top[g]:
            d = top[g] - acc[g]
            out[n] = (_scaled_err(lam[n:n + 1], n_g[g:g + 1] + 1.0, d[None], (e_acc[g] + U * np.abs(d))[None])[0]
                      + U * np.abs(x[n] + lam[n] * d))
    return out * (1 + 2.0 ** -30)


def two_level_total_error(x, group, mu, top, has_top):
    """... and of its total acc + mu (top - acc), mu = W / (v + W) with n_g + 1 relative roundings -> e [G][...]"""
    G = len(top)
    acc = gather(x, group, G)
    e_acc = _sum_err(np.zeros_like(x), np.abs(x), group, G)
    n_g = np.bincount(group, minlength=G)
    d = np.where(np.reshape(has_top, (-1,) + (1,) * (acc.ndim - 1)) != 0, top - acc, 0.0)
    mu_ = np.reshape(mu, (-1,) + (1,) * (acc.ndim - 1))
    e = e_acc + _scaled_err(mu, n_g + 1.0, d, e_acc + U * np.abs(d)) + U * np.abs(acc + mu_ * d)
    return e * (1 + 2.0 ** -30)


def sum_bound(n_children, abs_children_sum):
    """the error of a test's own sum of n_children values from +0.0: (n_children - 1) u sum |child|"""
    return max(n_children - 1, 0) * U * abs_children_sum
