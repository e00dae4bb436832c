"""A numpy model of the Karatsuba split of fold_coeff.hip's Toeplitz products (d = 1024), and
rho built to sit at the edges of each level's i8 range. Shared by tests/
test_fold_karatsuba_model.py (CPU) and tests/test_gpu_fold_karatsuba.py.

A generator G of an n x n Toeplitz matrix T[c][j] = G[c - j] is stored with delta = c - j at
index delta + n - 1 (length 2 n - 1). Every function is linear in the generator along axis 0,
so it also runs on the integer matrix that maps rho's coefficients to a table's entries:
that is how the tests compute the places of the coefficients that make an entry +128."""
import numpy as np

D = 1024
I8 = (-128, 127)


def generator(rho):
    """g[delta] = rho[delta] (delta >= 0), -rho[delta + d] (delta < 0): R[c][j] = g[c - j]"""
    return np.concatenate([-rho[1:], rho])


def toeplitz(G):
    n = (len(G) + 1) // 2
    c, j = np.mgrid[0:n, 0:n]
    return G[c - j + n - 1]


def blocks(G):
    """the generators of A, B, C of a Toeplitz [A B; C A]: A[delta] = G[delta],
    B[delta] = G[delta - n / 2], C[delta] = G[delta + n / 2], |delta| < n / 2"""
    n = (len(G) + 1) // 2
    h = n // 2
    return G[h:h + n - 1], G[0:n - 1], G[n:2 * n - 1]


def split_general(G):
    """[A B; C A] [U0; U1]: S_a = A (U0 + U1), S_b = (C - A) U0, S_c = (B - A) U1"""
    A, B, C = blocks(G)
    return A, C - A, B - A


def split_top(g):
    """level 1 on the negacyclic R (B = -T2): T1, T2 - T1, T1 + T2"""
    T1, _, T2 = blocks(g)
    return T1, T2 - T1, T1 + T2


def tables(g, level):
    """the generators whose products level `level` multiplies: 1, 3 or 9 of them"""
    out = [g]
    for l in range(level):
        out = [t for G in out for t in (split_top(G) if l == 0 else split_general(G))]
    return out


def mul_general(G, U, level):
    if level == 0:
        return toeplitz(G) @ U
    h = len(U) // 2
    Ga, Gb, Gc = split_general(G)
    Sa = mul_general(Ga, U[:h] + U[h:], level - 1)
    Sb = mul_general(Gb, U[:h], level - 1)
    Sc = mul_general(Gc, U[h:], level - 1)
    return np.concatenate([Sa + Sc, Sa + Sb])


def mul(rho, V, level):
    """R V for the negacyclic Toeplitz R of rho, V [d][E], through `level` levels of the split"""
    g = generator(rho)
    if level == 0:
        return toeplitz(g) @ V
    h = len(V) // 2
    Ga, Gb, Gc = split_top(g)
    Pa = mul_general(Ga, V[:h] + V[h:], level - 1)
    Pb = mul_general(Gb, V[:h], level - 1)
    Pc = mul_general(Gc, V[h:], level - 1)
    return np.concatenate([Pa - Pc, Pa + Pb])


def fold(rc, Dp, level):
    """f0_coeff [N][d] = sum_i R_i D_i: rc [2K][d] signed, Dp [2][K][N][d] digit planes"""
    K = Dp.shape[1]
    tot = 0
    for i in range(2 * K):
        tot = tot + mul(rc[i], Dp[i // K, i % K].T.astype(np.int64), level)
    return tot.T


def fits(rc, level):
    """whether every entry of every level-`level` table of every rho_i lies in i8"""
    return all(I8[0] <= int(t.min()) and int(t.max()) <= I8[1] for r in rc for t in tables(generator(r), level))


def best_level(rc, built):
    """the level the device picks: the highest built one whose tables fit (0: the dense product)"""
    for level in range(built, 0, -1):
        if fits(rc, level):
            return level
    return 0


def entry_maps(level):
    """per level-`level` table, the integer matrix [entries][d] with entry = row . rho"""
    return tables(generator(np.eye(D, dtype=np.int64)), level)


def widest_entry(level):
    """the first table entry of `level` that combines the most coefficients of rho (two at level
    1, four at level 2) with the most of them negated: (table, entry, places, signs)"""
    best = None
    for t, M in enumerate(entry_maps(level)):
        n, neg = (M != 0).sum(1), (M < 0).sum(1)
        row = int(np.lexsort((-neg, -n))[0])
        if best is None or (n[row], neg[row]) > best[0]:
            best = (n[row], neg[row]), (t, row, np.flatnonzero(M[row]), M[row][M[row] != 0])
    return best[1]


def short_rho(nw, seed, lo=-32, hi=31):
    """[nw][d] coefficients over short_challenge's range, both ends in every rho_i"""
    rng = np.random.default_rng(seed)
    rc = rng.integers(lo, hi + 1, size=(nw, D), dtype=np.int64)
    for i in range(nw):
        a, b = rng.choice(D, 2, replace=False)
        rc[i, a], rc[i, b] = lo, hi
    return rc


def level2_entry_at(nw, seed, plus, i=7):
    """short rho whose rho_i has the four coefficients of widest_entry(2) at -32 where the entry
    negates them and at `plus` where it does not. No level-2 entry takes four coefficients with
    one sign (three and one, or two and two), so over short_challenge's [-32, 31] the entry is at
    most 3 * 32 + 31 = 127; plus = 32 makes it +128: level 2 is out, level 1 (|entry| <= 64) is in"""
    rc = short_rho(nw, seed)
    _, _, places, signs = widest_entry(2)
    rc[i, places] = np.where(signs < 0, -32, plus)
    return rc


def level1_entry_128(nw, seed, i=22):
    """short rho but for two coefficients of rho_i at +-64 that a level-1 entry combines to +128.
    Every coefficient is still inside [-127, 127], so the coefficient-form fold runs, at level 0"""
    rc = short_rho(nw, seed)
    _, _, places, signs = widest_entry(1)
    rc[i, places] = 64 * signs
    return rc
