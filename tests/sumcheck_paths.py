"""The sumcheck launch paths and the cases that reach them.

Every round launcher of csrc/sumcheck.hip takes its grid and its kernel from one plan
(lfk::round_plan; lfk::dot_plan for the MLE dot products), which lf_sumcheck_round_plan and
lf_sumcheck_dot_plan return as the launchers use it. This module holds the table of cases
that tests/test_gpu_sumcheck_paths.py runs against the oracle and, for a case, the plan of
each of its rounds: round i of an nv-variable prove sums over half = 2^(nv-1-i) points, so
one prove walks down a ladder of plans. census() names the cells (kernel, slot width, path)
the table reaches; tests/test_sumcheck_paths.py asserts on the CPU that none of REQUIRED is
empty, so a change of FILL_THREADS, PT_THREADS, the grid.x cap or the block size cannot move
the cases off a path unnoticed.

A case is a dict. Its inputs are built from the oracle's fill_uniform and numpy generators
seeded by the case, so the census (which needs the sparse point lists but no MLE data) and
the GPU test see the same lists."""
import numpy as np

import latticeum_amd as LA
import oracle as O

P = LA.P
FOLD, LIN, LIN_EQ = LA.PLAN_FOLDING, LA.PLAN_LIN, LA.PLAN_LIN_EQ
KIND_NAME = {FOLD: "fold", LIN: "lin", LIN_EQ: "lin_eq"}


def tb_of(d):
    return 3 if d == 24 else 1


def rand(n, seed):
    return O.fill_uniform(n, seed)


# ------------------------------------------------------------------ the case table
def sweep_sizes(D):
    """multisets of a degree-D linearization polynomial: the largest legal one, and 2, 1, 0 factors"""
    return [D - 1, min(2, D - 1), min(1, D - 1), 0]


SMALL = {5: [2, 1, 1, 2, 0], 3: [2, 1, 1], 2: [2, 1], 1: [2]}  # small multisets by q (degree 3)
ZERO_C = {5: 3, 3: 2}                                          # the c_i that is zero in every slot


def lin_case(d, nv, sizes, degree, zero_c=None, dead=False, rounds=None, weak=False):
    """a linearization case: multiset sizes, c_0 zero in the first half of the words, c_[zero_c]
    zero everywhere; dead: the sparse lists hold no point at all; rounds: None = a whole prove,
    1 = the single round 0; weak: the directed values of WEAK_CASES"""
    return dict(d=d, nv=nv, sizes=list(sizes), degree=degree, zero_c=zero_c, dead=dead, rounds=rounds, weak=weak,
                seed=4000 + 131 * d + 17 * nv + 7 * degree + len(sizes),
                id=f"d{d}-nv{nv}-D{degree}-q{len(sizes)}" + ("-dead" if dead else "") + ("-weak" if weak else ""))


def small_lin(d, nv, q, **kw):
    return lin_case(d, nv, SMALL[q], 3, zero_c=ZERO_C.get(q), **kw)


# A. the split-eq provers (lf_sumcheck_prove_lin and, over MLEs with zeroed lines, _lin_sparse)
LIN_EQ_SWEEP = [lin_case(d, nv, sweep_sizes(D), D) for d, nv in ((1024, 6), (64, 10), (24, 13)) for D in range(1, 10)]
LIN_EQ_LADDERS = [small_lin(1024, 9, 5), small_lin(24, 16, 3)]          # nchunk 1, 2, 4, 5 and 1, 2, 3
LIN_EQ_CAPPED = [small_lin(16, 16, 2), small_lin(512, 12, 2), small_lin(24, 17, 2)]
LIN_EQ_ONE = [small_lin(24, 12, 1), small_lin(64, 9, 1)]                # one multiset: nothing to chunk
# The weakly reduced product chain of k_round_lin_eq (multisets of three or more factors end in
# s_mul_w, whose result may be any u64 congruent to the product, and are canonicalised before
# they are summed). A weak value v + p with v < 2^32 - 1 turns up once in 2^32 uniform products,
# and gl::add is still right with one such operand, so only directed values can tell whether the
# canonicalisation is there: in one slot of one point, at e = 0, multiset 0 (no factor) adds
# p - 1 and multisets 1 and 2 each add the product (2^32 - 1)(2^32 + 1) = 2^64 - 1 = (2^32 - 2) + p
# out of s_mul_w; uncanonicalised, the second of them wraps 2^64 twice in gl::add. All three must
# fall into one chunk of the templated kernel (24 multisets over 8 chunks at 2^15 threads).
WEAK_POINT = 5
WEAK_SLOT = {24: 5, 64: 40}
LIN_EQ_WEAK = [lin_case(d, nv, [0, 3, 3] + [1] * 21, 4, weak=True) for d, nv in ((24, 13), (64, 10))]
LIN_EQ_CASES = LIN_EQ_SWEEP + LIN_EQ_LADDERS + LIN_EQ_CAPPED + LIN_EQ_ONE + LIN_EQ_WEAK
SPARSE_DEAD = [small_lin(24, 4, 3, dead=True), small_lin(64, 4, 3, dead=True)]  # sparse only: no active point
SPARSE_CASES = LIN_EQ_CASES + SPARSE_DEAD

# B. the unsplit linearization: single rounds (lf_dev_sumcheck_round) and proves (lf_sumcheck_prove, _ptrs)
LIN_ROUNDS = ([lin_case(d, nv, sweep_sizes(D), D, rounds=1) for d, nv in ((24, 5), (64, 4)) for D in range(1, 10)] +
              [small_lin(24, 5, 1, rounds=1), small_lin(64, 4, 1, rounds=1), small_lin(24, 17, 2, rounds=1)])
LIN_PROVES = [small_lin(1024, 9, 5), small_lin(16, 16, 2), small_lin(24, 16, 3)]


# C. the folding polynomial
def fold_case(d, nv, nk, tau, bs, rounds=None):
    return dict(d=d, nv=nv, nk=nk, tau=tau, bs=bs, rounds=rounds, seed=5000 + 131 * d + 17 * nv + 7 * bs + nk,
                id=f"d{d}-nv{nv}-nk{nk}-tau{tau}-BS{bs}")


FOLD_ROUNDS = ([fold_case(d, nv, nk, tau, bs, rounds=1) for d, nv, nk, tau in ((24, 6, 4, 3), (16, 5, 4, 1), (1024, 2, 3, 1))
                for bs in (1, 2, 3, 4)] + [fold_case(24, 17, 1, 3, 2, rounds=1)])
FOLD_PROVES = [fold_case(1024, 9, 5, 1, 2), fold_case(1024, 9, 5, 1, 3), fold_case(24, 16, 1, 3, 2),
               fold_case(16, 16, 2, 1, 2), fold_case(16, 3, 1, 1, 2), fold_case(24, 3, 1, 1, 2)]


# D. the digit round 0 (lf_sumcheck_prove_fold_digits): rows of digits in {-1, 0, 1}
def digit_case(d, nv, K, N, rows="uniform", mu="uniform", gap=0):
    return dict(d=d, nv=nv, K=K, N=N, rows=rows, mu=mu, gap=gap, seed=6000 + 131 * d + 17 * nv + N,
                id=f"d{d}-nv{nv}-K{K}-N{N}-{rows}-mu_{mu}" + (f"-gap{gap}" if gap else ""))


DIGIT_ROWS = ("plus", "minus", "alt_mp", "alt_pm", "zero", "uniform")
DIGIT_MU = ("pm1", "zero", "one", "uniform")
DIGIT_CASES = (
    [digit_case(d, 5, 2, N, rows=r, mu=DIGIT_MU[i % 4]) for d, N in ((24, 31), (16, 29)) for i, r in enumerate(DIGIT_ROWS)] +
    [digit_case(d, 5, 2, N, mu=m) for d, N in ((24, 31), (16, 29)) for m in DIGIT_MU[:3]] +
    [digit_case(24, 4, 1, 1), digit_case(16, 4, 1, 1), digit_case(24, 4, 2, 16), digit_case(16, 5, 2, 32),
     digit_case(24, 5, 2, 16), digit_case(16, 5, 2, 13), digit_case(24, 5, 2, 31, gap=24 * 3 + 5),
     digit_case(16, 5, 2, 29, gap=7), digit_case(1024, 8, 3, 255), digit_case(1024, 9, 3, 512)])

# E. evaluation and combination entries: (d, nv) for the three nsplit cells of each slot width
DOT_SHAPES = [(24, 3), (24, 8), (24, 12), (64, 1), (64, 6), (64, 9), (1024, 1), (1024, 4), (1024, 7)]


# ------------------------------------------------------------------ plans
def nf_of(case):
    return case["nk"] * case["tau"] if "nk" in case else len(case["sizes"])


def plans(case, kind):
    """the plan of every round the case runs, round 0 first"""
    nv, n = case["nv"], case["rounds"] or case["nv"]
    out = []
    for i in range(n):
        pl = LA.sumcheck_round_plan(case["d"], 1 << (nv - 1 - i), nf_of(case), kind)
        pl.update(round=i, half=1 << (nv - 1 - i), nf=nf_of(case), kind=KIND_NAME[kind])
        out.append(pl)
    return out


def digit_plans(case):
    nv, nf = case["nv"], 2 * case["K"] * tb_of(case["d"])
    out = []
    for i in range(nv):
        pl = LA.sumcheck_round_plan(case["d"], 1 << (nv - 1 - i), nf, FOLD)
        pl.update(round=i, half=1 << (nv - 1 - i), nf=nf, kind="fold_digits" if i == 0 else "fold")
        out.append(pl)
    return out


# ------------------------------------------------------------------ inputs
def lin_structure(case):
    """(S, zero): the multisets' MLE indices and, per multiset, how its coefficient vanishes
    ('' not at all, 'slots' in some slots, 'all' everywhere)"""
    rng = np.random.default_rng(case["seed"])
    nmz = max(3, max(case["sizes"]))
    S = [[int(j) for j in rng.integers(0, nmz, k)] for k in case["sizes"]]
    if case["weak"]:
        S[1] = S[2] = [0, 1, 2]
    zero =["slots" if i == 0 else "all" if i == case["zero_c"] else "" for i in range(len(S))]
    return S, nmz, zero


def lin_inputs(case):
    """c, S, the Mz MLEs and beta (base-ring challenges broadcast into every slot)"""
    d, nv, seed = case["d"], case["nv"], case["seed"]
    S, nmz, zero = lin_structure(case)
    c = rand(len(S) * d, seed + 1)
    for i, z in enumerate(zero):
        if z == "slots":
            c[i * d:i * d + d // 2] = 0
        elif z == "all":
            c[i * d:(i + 1) * d] = 0
    mz = [rand((1 << nv) * d, seed + 2 + j) for j in range(nmz)]
    tb = tb_of(d)
    if case["weak"]:
        def put(arr, elem, v):  # the base-ring value v in the directed slot of element elem
            o = elem * d + WEAK_SLOT[d] * tb
            arr[o:o + tb] = 0
            arr[o] = v
        put(c, 0, P - 1)
        put(c, 1, 1)
        put(c, 2, 1)
        for m, v in zip(mz, (1, (1 << 32) - 1, (1 << 32) + 1)):
            put(m, 2 * WEAK_POINT, v)
    b = rand(nv * d, seed + 99)
    beta = np.concatenate([O.broadcast(b[i * d:i * d + tb], d) for i in range(nv)])
    return c, S, mz, beta


def sparse_lists(case, frac=0.3):
    """(live, act, off): per Mz MLE the lines (rows 2b, 2b + 1) that stay, the rest are zeroed
    (about frac of them; all of them in a dead case); each multiset's active points (every
    factor's line live; none where c_i is zero everywhere) and their offsets"""
    S, nmz, zero = lin_structure(case)
    half = 1 << (case["nv"] - 1)
    rng = np.random.default_rng(case["seed"] + 7)
    live = [np.zeros(half, bool) if case["dead"] else rng.random(half) >= frac for _ in range(nmz)]
    act, off = [], [0]
    for Si, z in zip(S, zero):
        on = np.ones(half, bool)
        for j in Si:
            on &= live[j]
        if z == "all":
            on[:] = False
        act.extend(np.nonzero(on)[0].tolist())
        off.append(len(act))
    return live, np.array(act or [0], np.int32), np.array(off, np.uint32)


def fold_inputs(case):
    """[eq(r0), g0, eq(r1), g1, eq(beta), f_hat (nk x tau)], mu, nm"""
    d, nv, nk, tau, seed = (case[k] for k in ("d", "nv", "nk", "tau", "seed"))
    n = 1 << nv
    r0, r1, beta = (rand(nv * d, seed + i) for i in range(3))
    mles = [O.eq_table(r0, nv, d), rand(n * d, seed + 3), O.eq_table(r1, nv, d), rand(n * d, seed + 4),
            O.eq_table(beta, nv, d)]
    mles += [rand(n * d, seed + 10 + i) for i in range(nk * tau)]
    return np.concatenate(mles), rand(nk * d, seed + 5), 5 + nk * tau


def to_field(x):
    x = np.asarray(x, np.int64)
    return np.where(x < 0, np.uint64(P - 1), x.astype(np.uint64))  # digits only: -1 -> p - 1


def digit_rows(case):
    """2K witnesses' digit rows [2K][N][d], canonical"""
    d, N, nw = case["d"], case["N"], 2 * case["K"]
    rng = np.random.default_rng(case["seed"])
    rows = case["rows"]
    if rows == "uniform":
        x = rng.integers(-1, 2, (nw, N, d))
    elif rows in ("plus", "minus", "zero"):
        x = np.full((nw, N, d), {"plus": 1, "minus": -1, "zero": 0}[rows])
    else:  # alternating along the points: every line's difference is +-2
        first = -1 if rows == "alt_mp" else 1
        x = np.broadcast_to((first * (-1) ** np.arange(N))[None, :, None], (nw, N, d))
    return to_field(x)


def digit_mu(case):
    d, nk = case["d"], 2 * case["K"]
    if case["mu"] == "uniform":
        return rand(nk * d, case["seed"] + 5)
    return np.full(nk * d, {"pm1": P - 1, "zero": 0, "one": 1}[case["mu"]], np.uint64)


def fhat_mles(fc, N, d, nv):
    """Witness::get_fhat of one witness's rows [N][d] as tau MLEs of 2^nv points, zero past N"""
    tau, n = tb_of(d), 1 << nv
    out = np.zeros((tau, n, d), np.uint64)
    rows = np.ascontiguousarray(fc).reshape(-1)
    if N:
        out[:, :N] = O.get_fhat_phi72(rows).reshape(tau, N, d) if d == 24 else rows.reshape(1, N, d)
    return out.reshape(tau, n * d)


# ------------------------------------------------------------------ census
def _round_cells(kind, tb, pl):
    k = f"{kind}/TB{tb}"
    cells = set()
    nf, nc = pl["nf"], pl["nchunk"]
    if nf == 1:
        cells.add(f"{k}/nf=1")
    elif nc == 1:
        cells.add(f"{k}/nchunk=1")
    elif nc == nf:
        cells.add(f"{k}/nchunk=nf")
    elif nf % nc:
        cells.add(f"{k}/nchunk uneven")
    if pl["capped"]:
        cells.add(f"{k}/capped")
    cells.add(f"{k}/ppb=1" if pl["ppb"] == 1 else f"{k}/ppb>1")
    if pl["gy"] > 1:
        cells.add(f"{k}/grid.y>1")
    if pl["gx"] * nc > 256:
        cells.add(f"{k}/partial blocks>256")
    return cells


def _size_cells(prefix, sizes, zero):
    cells = {f"{prefix}/multiset size {'>=3' if k >= 3 else k}" for k in sizes}
    cells |= {f"{prefix}/c zero in {z}" for z in zero if z}
    return cells


def census():
    """the cells the case table reaches"""
    cells = set()
    for case in FOLD_ROUNDS + FOLD_PROVES:
        tb = tb_of(case["d"])
        cells.add(f"fold/TB{tb}/BS={case['bs']}")
        for pl in plans(case, FOLD):
            cells |= _round_cells("fold", tb, pl)
    for case in LIN_ROUNDS + LIN_PROVES:
        tb = tb_of(case["d"])
        _, _, zero = lin_structure(case)
        cells.add(f"lin/TB{tb}/DEG={case['degree']}")
        cells |= _size_cells(f"lin/TB{tb}", case["sizes"], zero)
        for pl in plans(case, LIN):
            cells |= _round_cells("lin", tb, pl)
    for case in LIN_EQ_CASES:
        tb = tb_of(case["d"])
        _, _, zero = lin_structure(case)
        pls = plans(case, LIN_EQ)
        for name, on in (("lin_eq", any(not p["per_point"] for p in pls)), ("lin_eq_pt", any(p["per_point"] for p in pls))):
            if on:
                cells.add(f"{name}/TB{tb}/NQ={case['degree']}")
                cells |= _size_cells(f"{name}/TB{tb}", case["sizes"], zero)
        if case["weak"] and not pls[0]["per_point"] and len(case["sizes"]) // pls[0]["nchunk"] >= 3:
            cells.add(f"lin_eq/TB{tb}/weak chain summed in one chunk")  # chunk 0 holds multisets 0, 1 and 2
        if 0 < sum(p["per_point"] for p in pls) < len(pls):
            cells.add(f"lin_eq/TB{tb}/both sides of the per-point threshold")
        for pl in pls:
            if not pl["per_point"]:
                cells |= _round_cells("lin_eq", tb, pl)
    for case in SPARSE_CASES:
        tb = tb_of(case["d"])
        k = f"lin_eq_sparse/TB{tb}"
        _, _, zero = lin_structure(case)
        _, act, off = sparse_lists(case)
        pl = plans(case, LIN_EQ)[0]
        per, ppb = pl["sparse_block_points"], pl["ppb"]
        counts = np.diff(off.astype(np.int64))
        if not counts.any():
            cells.add(f"{k}/no active point at all")
            continue
        cells.add(f"{k}/NQ={case['degree']}")
        for i, (size, z) in enumerate(zip(case["sizes"], zero)):
            if counts[i]:  # only a multiset with a block reaches the kernel
                cells |= _size_cells(k, [size], [z])
        if (counts > per).any():
            cells.add(f"{k}/multiset over several blocks")
        if any((min(cnt - p, per)) % ppb for cnt in counts for p in range(0, int(cnt), per)):
            cells.add(f"{k}/block range not a multiple of ppb")
        if (counts == 0).any():
            cells.add(f"{k}/multiset with no active point")
    for d, nv in DOT_SHAPES:
        pl = LA.sumcheck_dot_plan(d, 1 << nv)
        k = f"dot/TB{tb_of(d)}"
        if (1 << nv) < pl["ppb"]:
            cells.add(f"{k}/n<ppb")
        if 1 < pl["nsplit"] < 64:
            cells.add(f"{k}/1<nsplit<64")
        if pl["nsplit"] == 64 and pl["passes"] > 1:
            cells.add(f"{k}/nsplit=64, several passes")
    for case in DIGIT_CASES:
        tb = tb_of(case["d"])
        pl = digit_plans(case)[0]
        cells.add(f"fold_digits/TB{tb}/nchunk={'1' if pl['nchunk'] == 1 else 'nf' if pl['nchunk'] == pl['nf'] else 'between'}")
        N, n = case["N"], 1 << case["nv"]
        cells.add(f"fold_digits/TB{tb}/N {'odd' if N % 2 else 'even'}")
        if N == n:
            cells.add(f"fold_digits/TB{tb}/N=2^nv")
        if N <= n // 2:
            cells.add(f"fold_digits/TB{tb}/upper half all padding")
    return cells


def required():
    """every cell the table must reach"""
    req = []
    for tb in (1, 3):
        for kind in ("fold", "lin", "lin_eq"):
            k = f"{kind}/TB{tb}"
            req += [f"{k}/nchunk=1", f"{k}/nchunk uneven", f"{k}/nchunk=nf", f"{k}/nf=1", f"{k}/capped", f"{k}/ppb>1",
                    f"{k}/partial blocks>256"]
            if tb == 1:  # a Phi_72 element has 8 slots: always 32 points per block and grid.y = 1
                req += [f"{k}/ppb=1", f"{k}/grid.y>1"]
        req += [f"lin_eq/TB{tb}/both sides of the per-point threshold", f"lin_eq/TB{tb}/weak chain summed in one chunk"]
        req += [f"{k}/TB{tb}/NQ={q}" for k in ("lin_eq", "lin_eq_pt", "lin_eq_sparse") for q in range(1, 10)]
        req += [f"lin/TB{tb}/DEG={q}" for q in range(1, 10)]
        req += [f"fold/TB{tb}/BS={b}" for b in (1, 2, 3, 4)]
        for k in ("lin", "lin_eq", "lin_eq_pt", "lin_eq_sparse"):
            req += [f"{k}/TB{tb}/multiset size {s}" for s in (0, 1, 2, ">=3")]
            req.append(f"{k}/TB{tb}/c zero in slots")
            if k != "lin_eq_sparse":  # a coefficient that is zero everywhere has no active point: no block runs it
                req.append(f"{k}/TB{tb}/c zero in all")
        k = f"lin_eq_sparse/TB{tb}"
        req += [f"{k}/multiset over several blocks", f"{k}/block range not a multiple of ppb",
                f"{k}/multiset with no active point", f"{k}/no active point at all"]
        req += [f"dot/TB{tb}/n<ppb", f"dot/TB{tb}/1<nsplit<64", f"dot/TB{tb}/nsplit=64, several passes"]
        req += [f"fold_digits/TB{tb}/N odd", f"fold_digits/TB{tb}/N=2^nv", f"fold_digits/TB{tb}/upper half all padding"]
    req += ["fold_digits/TB1/nchunk=1", "fold_digits/TB1/nchunk=between"]
    return req


# ------------------------------------------------------------------ comparison
def first_difference(got, want, pls, nev, d):
    """None if the proofs agree, else a message naming the first round whose message differs and its plan"""
    if np.array_equal(got, want):
        return None
    g, w = got.reshape(-1, nev * d), want.reshape(-1, nev * d)
    for i in range(len(w)):
        if not np.array_equal(g[i], w[i]):
            e = int(np.nonzero(g[i] != w[i])[0][0])
            return f"round {i}: message differs first at evaluation {e // d}, word {e % d}; plan {pls[i]}"
    return "proofs differ in length"
