"""The long double reference of the Q2 operator (q2_reference.py) against an independently assembled matrix, and the bound
(K + K_REF) u mag against planted errors: it catches what a 1e-12 max-norm check lets through."""
import numpy as np

import q2_reference as R

LD = R.LD
N_CELLS = (2, 3, 2)
H = (0.5, 1.0 / 3.0, 0.5)


def _lagrange(nodes, x):
    """values and derivatives of the Lagrange polynomials on `nodes` at x, by the product formula"""
    p = len(nodes)
    v, d = [], []
    for i in range(p):
        vi = LD(1)
        for j in range(p):
            if j != i:
                vi *= (x - nodes[j]) / (nodes[i] - nodes[j])
        di = LD(0)
        for j in range(p):
            if j == i:
                continue
            t = 1 / (nodes[i] - nodes[j])
            for k in range(p):
                if k != i and k != j:
                    t *= (x - nodes[k]) / (nodes[i] - nodes[k])
            di += t
        v.append(vi)
        d.append(di)
    return v, d


def _assembled(n, h, coef, con):
    """dense Q2 matrix from explicit 27 x 27 element matrices: per quadrature point the three gradient rows g and
    A_e += c JxW g^T g; identity rows and columns on the constrained entries"""
    # QGauss(3) on [0, 1] from its closed form (numpy's leggauss is double)
    r = np.sqrt(LD(3) / LD(5)) / 2
    pts = [LD(0.5) - r, LD(0.5), LD(0.5) + r]
    w = [LD(5) / 18, LD(8) / 18, LD(5) / 18]
    nodes = [LD(0), LD(0.5), LD(1)]
    VD = [_lagrange(nodes, p) for p in pts]
    hh = [LD(v) for v in h]
    N = [2 * v + 1 for v in n]
    nd = N[0] * N[1] * N[2]
    A = np.zeros((nd, nd), dtype=LD)
    cell = 0
    for k in range(n[2]):
        for j in range(n[1]):
            for i in range(n[0]):
                ids = [(2 * i + a) + N[0] * ((2 * j + b) + N[1] * (2 * k + c)) for c in range(3) for b in range(3) for a in range(3)]
                Ae = np.zeros((27, 27), dtype=LD)
                for qc in range(3):
                    for qb in range(3):
                        for qa in range(3):
                            cw = LD(coef[cell, qa + 3 * qb + 9 * qc]) * w[qa] * w[qb] * w[qc] * hh[0] * hh[1] * hh[2]
                            g = np.zeros((3, 27), dtype=LD)
                            m = 0
                            for c in range(3):
                                for b in range(3):
                                    for a in range(3):
                                        g[0, m] = VD[qa][1][a] * VD[qb][0][b] * VD[qc][0][c] / hh[0]
                                        g[1, m] = VD[qa][0][a] * VD[qb][1][b] * VD[qc][0][c] / hh[1]
                                        g[2, m] = VD[qa][0][a] * VD[qb][0][b] * VD[qc][1][c] / hh[2]
                                        m += 1
                            Ae += cw * (g.T @ g)
                A[np.ix_(ids, ids)] += Ae
                cell += 1
    A[con, :] = 0
    A[:, con] = 0
    A[con, con] = 1
    return A


def _setup(seed=0):
    rng = np.random.default_rng(seed)
    cells = int(np.prod(N_CELLS))
    coef = 10.0 ** rng.uniform(-1, 1, (cells, 27))
    N = [2 * v + 1 for v in N_CELLS]
    con = np.zeros(N[::-1], dtype=bool)
    for ax in range(3):
        sl = [slice(None)] * 3
        sl[ax] = 0
        con[tuple(sl)] = True
        sl[ax] = -1
        con[tuple(sl)] = True
    con = con.reshape(-1)
    x = R.six_decades(rng, con.size)
    return coef, con, x


def test_reference_equals_the_assembled_matrix():
    coef, con, x = _setup()
    ref = R.Q2Reference(N_CELLS, H, coef, con)
    y, mag = ref.apply(x)
    A = _assembled(N_CELLS, H, coef, con)
    ya = A @ x.astype(LD)
    assert np.all(np.abs(y - ya) <= 1e-15 * mag)
    assert np.abs(y - ya).max() <= 1e-15 * np.abs(ya).max()
    d, _ = ref.diagonal()
    assert np.all(np.abs(d - np.diag(A)) <= 1e-15 * np.abs(d))
    # the scipy form of the reference is the same matrix
    assert np.abs(ref.assemble().toarray() - A.astype(np.float64)).max() <= 1e-14 * np.abs(A).max()


def _judge(got, ref, mag):
    ok, worst = R.within_bound(got.astype(np.float64), ref, mag, R.K_APPLY)
    loose = np.abs(got.astype(np.float64).astype(LD) - ref).max() <= 1e-12 * np.abs(ref).max()
    return ok, loose, worst


def test_bound_accepts_the_rounded_reference():
    coef, con, x = _setup()
    y, mag = R.Q2Reference(N_CELLS, H, coef, con).apply(x)
    ok, loose, worst = _judge(y, y, mag)
    assert ok and loose and worst < 1.0


def test_planted_errors_are_caught():
    coef, con, x = _setup()
    y, mag = R.Q2Reference(N_CELLS, H, coef, con).apply(x)
    passed_loose = []
    # one table entry off by 1e-13 relative
    V, D, _ = R.tables()
    V = V.copy()
    V[0, 1] *= 1 + LD(1e-13)
    got, _ = R.Q2Reference(N_CELLS, H, coef, con, V=V).apply(x)
    ok, loose, worst = _judge(got, y, mag)
    assert not ok, worst
    passed_loose.append(loose)
    # one cell's coefficient index shifted by one point
    shifted = coef.copy()
    shifted[5] = np.roll(coef[5], 1)
    got, _ = R.Q2Reference(N_CELLS, H, shifted, con).apply(x)
    ok, loose, worst = _judge(got, y, mag)
    assert not ok, worst
    passed_loose.append(loose)
    # a constrained column not masked
    got, _ = R.Q2Reference(N_CELLS, H, coef, con, mask_columns=False).apply(x)
    ok, loose, worst = _judge(got, y, mag)
    assert not ok, worst
    passed_loose.append(loose)
    # what a 1e-12 max-norm check would have let through
    assert passed_loose[0], "the table error of 1e-13 is invisible to a 1e-12 max-norm check"
    assert any(passed_loose)
