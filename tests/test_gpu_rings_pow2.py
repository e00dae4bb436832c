"""GPU parity of the X^d + 1 rings whose degree is 2 4^k (d = 32, 128, 512, 2048:
ring::stockham4 runs one radix-2 pass in front of its radix-4 passes) against the
CPU oracle, bit for bit, through every layer that takes a ring degree: the
transforms, the ring product, the witness and decomposition kernels, both Ajtai
contractions, the commit+fold step (single, batched and column-sharded), the
folded-LCCCS helpers, the sumcheck and Mz kernels, and fold() end to end. The
oracle's convention at these degrees is pinned by tests/test_rings_pow2_oracle.py
and the LDS indexing by tests/test_stockham_model.py."""
import numpy as np
import pytest

import latticeum_amd as LA
import nifs as N
import oracle as O
from test_gpu_batch import make_step
from test_gpu_fold_prove import acc_dict, check_against_oracle, dev_wit, flat, proof_from_device, setup, witness, zeros
from test_gpu_mz import random_ccs
from test_gpu_parity import (assert_shards_match, check_ajtai, check_dev_fold_step, check_fold_outputs, dev, params,
                             rand, sharded_setup, valid_f_coeff)
from test_gpu_sumcheck import lin_case
from test_sumcheck_oracle import folding_case

pytestmark = pytest.mark.gpu
P = LA.P
NEW = [32, 128, 512, 2048]
LF_ERR_UNSUPPORTED_RING, LF_ERR_DECOMPOSITION_OVERFLOW = 2, 6  # lf.h


@pytest.fixture(scope="module")
def ctx():
    import torch
    c = LA.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def dev_transform(ctx, x, d, fwd):
    import torch
    t = dev(x)
    torch.cuda.synchronize()
    (ctx.dev_crt if fwd else ctx.dev_icrt)(t, d)
    ctx.sync()
    return host(t)


# ------------------------------------------------------------------ transforms
@pytest.mark.parametrize("d", NEW)
@pytest.mark.parametrize("n", [1, 3])
def test_dev_transforms_match_oracle(ctx, d, n):
    x = rand(n * d, 100 + d + n)
    F = dev_transform(ctx, x, d, True)
    assert np.array_equal(F, O.crt(x, d))
    assert np.array_equal(dev_transform(ctx, F, d, False), x)
    assert np.array_equal(dev_transform(ctx, x, d, False), O.icrt(x, d))


@pytest.mark.parametrize("d", NEW)
def test_dev_transforms_unit_vectors(ctx, d):
    """the d unit vectors X^j fix the slot order completely: crt(X^j)[k] = psi^((2k+1) j)"""
    x = np.eye(d, dtype=np.uint64).ravel()
    F = dev_transform(ctx, x, d, True)
    assert np.array_equal(F, O.crt(x, d))
    assert np.array_equal(dev_transform(ctx, F, d, False), x)
    assert np.array_equal(dev_transform(ctx, x, d, False), O.icrt(x, d))


@pytest.mark.parametrize("d", NEW)
def test_dev_transforms_all_p_minus_1(ctx, d):
    x = np.full(d, P - 1, np.uint64)
    assert np.array_equal(dev_transform(ctx, x, d, True), O.crt(x, d))
    assert np.array_equal(dev_transform(ctx, x, d, False), O.icrt(x, d))


@pytest.mark.parametrize("d", NEW)
def test_host_crt_montgomery_round_trip(ctx, d):
    x = rand(2 * d, 7 + d)
    xm = np.array([O.to_mont(int(v)) for v in x], np.uint64)
    ym = ctx.crt(xm, d, LA.REPR_MONTGOMERY)
    assert [O.from_mont(int(v)) for v in ym] == [int(v) for v in O.crt(x, d)]
    assert np.array_equal(ctx.icrt(ym, d, LA.REPR_MONTGOMERY), xm)


def test_dev_transform_block_loop_second_iteration(ctx):
    """n = 65537 elements of d = 32: one workgroup per element up to 65536 workgroups,
    so block 0 takes a second element"""
    d, n = 32, 65537
    x = rand(n * d, 131)
    F = dev_transform(ctx, x, d, True)
    assert np.array_equal(F, O.crt(x, d))
    assert np.array_equal(dev_transform(ctx, F, d, False), x)


# ------------------------------------------------------------------ ring product
@pytest.mark.parametrize("d", NEW)
def test_ring_mul(ctx, d):
    x1, xd = np.zeros(d, np.uint64), np.zeros(d, np.uint64)
    x1[1], xd[d - 1] = 1, 1
    minus_one = np.zeros(d, np.uint64)
    minus_one[0] = P - 1
    assert np.array_equal(ctx.icrt(ctx.ring_mul(ctx.crt(xd, d), ctx.crt(x1, d), d), d), minus_one)
    for i in range(3):
        a, b = rand(d, 200 + d + i), rand(d, 300 + d + i)
        assert np.array_equal(ctx.ring_mul(O.crt(a, d), O.crt(b, d), d), O.slot_mul(O.crt(a, d), O.crt(b, d), d))
        assert np.array_equal(ctx.icrt(ctx.ring_mul(ctx.crt(a, d), ctx.crt(b, d), d), d), O.poly_mul(a, b, d))


# ------------------------------------------------------------------ witness and decomposition
@pytest.mark.parametrize("d", NEW)
@pytest.mark.parametrize("W", [1, 3])
def test_witness_and_decomposition(ctx, d, W):
    pr = params(d)
    w = rand(W * d, 400 + d + W)
    fc, f = ctx.witness_from_w_ccs(w, pr)
    ofc, of = O.witness_from_w_ccs(w, d, pr.B, pr.L)
    assert np.array_equal(fc, ofc) and np.array_equal(f, of)
    f_in = rand(W * pr.L * d, 500 + d + W)
    fc2, w2 = ctx.witness_from_f(f_in, pr)
    ofc2, ow2 = O.witness_from_f(f_in, d, pr.B, pr.L)
    assert np.array_equal(fc2, ofc2) and np.array_equal(w2, ow2)
    got = ctx.decompose_witness(ofc, pr)
    want = O.decompose_witness(ofc, d, pr.B, pr.L, pr.b_small, pr.K)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)


@pytest.mark.parametrize("d", NEW)
def test_digit_boundaries(ctx, d):
    """coefficients on the base-B digit boundaries +-B/2, +-(B/2 - 1), p - 1 and 0 through
    from_w_ccs and on into decompose_witness; and |v| = 2^K - 1, the last value that K
    binary digits hold"""
    pr = params(d)
    h = pr.B // 2
    edge = np.array([h, P - h, h - 1, P - (h - 1), P - 1, 0], np.uint64)
    coeff = edge[np.arange(2 * d) % len(edge)]
    w = O.crt(coeff, d)
    fc, f = ctx.witness_from_w_ccs(w, pr)
    ofc, of = O.witness_from_w_ccs(w, d, pr.B, pr.L)
    assert np.array_equal(fc, ofc) and np.array_equal(f, of)
    got = ctx.decompose_witness(ofc, pr)
    for g, w_ in zip(got, O.decompose_witness(ofc, d, pr.B, pr.L, pr.b_small, pr.K)):
        assert np.array_equal(g, w_)
    top = (1 << pr.K) - 1
    fck = np.zeros(pr.L * d, np.uint64)
    fck[5], fck[d - 1], fck[pr.L * d - 1] = top, P - top, top
    got = ctx.decompose_witness(fck, pr)
    for g, w_ in zip(got, O.decompose_witness(fck, d, pr.B, pr.L, pr.b_small, pr.K)):
        assert np.array_equal(g, w_)


@pytest.mark.parametrize("d", NEW)
def test_decompose_overflow_is_an_error(ctx, d):
    pr = params(d)
    fc = np.zeros(pr.L * d, np.uint64)
    fc[3] = 1 << 20  # needs more than K=15 binary digits (reference panics)
    with pytest.raises(LA.LfError) as e:
        ctx.decompose_witness(fc, pr)
    assert e.value.code == LF_ERR_DECOMPOSITION_OVERFLOW
    ctx.decompose_witness(np.zeros(pr.L * d, np.uint64), pr)  # flag was cleared


# ------------------------------------------------------------------ commitments, both contractions
@pytest.mark.parametrize("d,kappa,ncols,nvec", [(32, 3, 40, 5), (128, 32, 70, 29), (512, 2, 9, 2), (2048, 2, 5, 1)])
def test_ajtai_mfma_shapes(ctx, d, kappa, ncols, nvec):
    check_ajtai(ctx, d, kappa, ncols, nvec, layout=1)


@pytest.mark.parametrize("d,kappa,ncols,nvec", [(32, 160, 40, 5), (512, 130, 9, 2)])
def test_ajtai_valu_wide_kappa(ctx, d, kappa, ncols, nvec):
    check_ajtai(ctx, d, kappa, ncols, nvec, layout=0)


@pytest.mark.parametrize("d,kappa,nvec", [(32, 32, 32), (128, 32, 32), (512, 8, 8), (2048, 3, 2)])
def test_ajtai_mfma_extreme_digits(ctx, d, kappa, nvec):
    """all-(p - 1) operands: every byte of both operand forms at the end of its range,
    over two 32-column chunks and a ragged third"""
    import torch
    ncols = 70
    A = np.full(kappa * ncols * d, P - 1, np.uint64).reshape(kappa, ncols, d)
    F = np.full(nvec * ncols * d, P - 1, np.uint64)
    sch = LA.AjtaiCommitmentScheme(ctx, A)
    assert sch.layout == 1
    Ft = torch.from_numpy(F.view(np.int64)).cuda()
    cm = torch.zeros(nvec * kappa * d, dtype=torch.int64, device="cuda")
    ctx.dev_ajtai_commit(sch, [Ft[v * ncols * d:(v + 1) * ncols * d] for v in range(nvec)], cm)
    ctx.sync()
    # (p-1)^2 = 1 per column, so every entry is ncols mod p
    assert set(host(cm).tolist()) == {ncols}


# ------------------------------------------------------------------ the commit+fold step
@pytest.mark.parametrize("d,W,kappa", [(32, 6, 3), (128, 3, 2), (512, 2, 2), (2048, 2, 2)])
def test_dev_fold_step_matches_oracle(ctx, d, W, kappa):
    check_dev_fold_step(ctx, d, W, kappa)


def test_fold_step_batch_equals_single_steps():
    import torch
    d, W, kappa, S = 128, 3, 2, 2
    pr = params(d)
    N_ = W * pr.L
    A = rand(kappa * N_ * d, 7000 + d)
    keys = ("f_coeff", "f", "cm", "f0", "f0_coeff", "w_ccs0", "cm0")
    lists = ("fk_coeff", "fk", "wk", "y")
    ctxs = [LA.Context(0) for _ in range(S)]
    try:
        At = torch.from_numpy(A.view(np.int64)).cuda()
        sch = LA.AjtaiCommitmentScheme(ctxs[0], device_tensor=At, kappa=kappa, ncols=N_, d=d)
        batch = [make_step(torch, A, kappa, d, W, 10 * i + 1, False) for i in range(S)]
        single = [make_step(torch, A, kappa, d, W, 10 * i + 1, False) for i in range(S)]
        torch.cuda.synchronize()
        ctxs[0].dev_fold_step_batch(ctxs[1:], sch, pr, W, [st["b"] for st in batch])
        for c in ctxs:
            c.sync()
        for st in single:
            ctxs[0].dev_fold_step(sch, pr, W, st["b"])
            ctxs[0].sync()
        for sb, ss in zip(batch, single):
            for k in keys:
                assert torch.equal(sb["keep"][k], ss["keep"][k]), k
            for k in lists:
                for s in range(2):
                    assert torch.equal(sb["keep"][k][s], ss["keep"][k][s]), k
            check_fold_outputs(host, sb["keep"], A, kappa, d, pr, W, sb["w_ccs"], sb["acc_cm"], sb["acc_fc"],
                               sb["rho"])
    finally:
        for c in ctxs:
            c.close()


def test_sharded_step_partial_finish(ctx):
    import torch
    d, W, kappa, world = 128, 20, 3, 2
    pr, keep, shards = sharded_setup(ctx, d, W, kappa, world, 1700 + d + W)
    n = ctx.fold_step_partial_len(shards[0]["sch"], pr)
    parts = []
    for sh in shards:
        p_ = dev(n=n)
        ctx.dev_fold_step_partial(sh["sch"], pr, sh["W"], sh["bufs"], p_)
        parts.append(p_)
    total = dev(n=n)
    ctx.dev_modp_sum(torch.cat(parts), world, n, total)
    for sh in shards:
        ctx.dev_fold_step_finish(sh["sch"], pr, sh["W"], sh["bufs"], total)
    ctx.sync()
    assert_shards_match(pr, d, W, kappa, keep, shards)


# ------------------------------------------------------------------ the rest of the folded LCCCS
@pytest.mark.parametrize("d", [32, 2048])
def test_fold_lcccs_and_compute_x_s(ctx, d):
    pr = params(d)
    nwit, t, l1, tau = 2 * pr.K, 7, 5, 1
    rng = np.random.default_rng(2200 + d)
    rc = [O.short_challenge(rng.integers(0, 256, 3 * d // 4, dtype=np.uint8).tobytes(), d) for _ in range(nwit - 1)]
    one = np.zeros(d, np.uint64)
    one[0] = 1
    rho_coeff = np.concatenate(rc + [one])
    rho = O.crt(rho_coeff, d)
    eta, xwh, theta = rand(nwit * t * d, 2201 + d), rand(nwit * l1 * d, 2202 + d), rand(nwit * tau * d, 2203 + d)
    got = ctx.fold_lcccs(d, rho, rho_coeff, eta, xwh, theta)
    assert np.array_equal(got["u0"], O.fold_cm0(rho, eta, nwit, t, d))
    assert np.array_equal(got["x0"], O.fold_cm0(rho, xwh, nwit, l1, d))
    assert np.array_equal(got["v0"], O.rot_lin_combination(rho_coeff, theta, d))
    x = rand(5 * d, 2300 + d)
    assert np.array_equal(ctx.compute_x_s(x, pr), O.compute_x_s(x, d, pr.B, pr.L, pr.b_small, pr.K))


# ------------------------------------------------------------------ sumcheck and Mz
@pytest.mark.parametrize("d,nv", [(32, 5), (512, 3)])
def test_sumcheck_kernels(ctx, d, nv):
    n = 1 << nv
    r = rand(nv * d, 10 + d)
    eq = dev(n=n * d)
    ctx.dev_eq_table(d, dev(r), nv, eq)
    ctx.sync()
    assert np.array_equal(host(eq), O.eq_table(r, nv, d))
    nm = 3
    mles = rand(nm * n * d, 11 + d)
    out = dev(n=nm * d)
    ctx.dev_mle_evaluate(d, dev(mles), nm, nv, dev(r), out)
    ctx.sync()
    want = np.concatenate([O.mle_evaluate(mles[m * n * d:(m + 1) * n * d], nv, d, r) for m in range(nm)])
    assert np.array_equal(host(out), want)
    # get_fhat: X^d + 1 takes the coefficients themselves, zero past N
    N_ = n - 3
    fc = rand(N_ * d, 40 + d)
    fh = dev(n=n * d)
    ctx.dev_fill_uniform(fh, 41 + d)
    ctx.dev_get_fhat(d, dev(fc), N_, nv, fh)
    ctx.sync()
    assert np.array_equal(host(fh)[:N_ * d], fc) and not host(fh)[N_ * d:].any()
    # one round of each combination kind
    nk, tau = 4, 1
    fm, mu, fnm = folding_case(d, nv, nk, tau, 500 + d + nv)
    ev = dev(n=5 * d)
    ctx.dev_sumcheck_round(LA.Comb.folding(dev(mu), nk, tau, 2), dev(fm), n * d, fnm, nv, d, 4, ev)
    ctx.sync()
    assert np.array_equal(host(ev), O.sumcheck_round(O.SumcheckComb.folding(mu, nk, tau, 2), fm, fnm, nv, d, 4))
    c, S, lm, lnm = lin_case(d, nv, 600 + d)
    ev = dev(n=5 * d)
    ctx.dev_sumcheck_round(LA.Comb.linearization(dev(c), S), dev(lm), n * d, lnm, nv, d, 4, ev)
    ctx.sync()
    assert np.array_equal(host(ev), O.sumcheck_round(O.SumcheckComb.linearization(c, S), lm, lnm, nv, d, 4))


@pytest.mark.parametrize("d", [32, 512])
def test_mz_products(ctx, d):
    t, m, n, nz, nv = 3, 27, 40, 3, 5
    mats = random_ccs(t, m, n, d, 40 + d)
    M = LA.CCSMatrices(ctx, d, m, n, mats)
    zs = [O.fill_uniform(n * d, 50 + d + i) for i in range(nz)]
    zd = dev(np.concatenate(zs))
    out = dev(n=nz * t * (1 << nv) * d)
    M.mz_mles(zd, nz, nv, out)
    ctx.sync()
    want = np.concatenate([O.mz_mles(mats, z, nv, d) for z in zs])
    assert np.array_equal(host(out), want)
    zeta = O.fill_uniform(nz * d, 60 + d)
    ch = dev(n=(1 << nv) * d)
    M.mz_challenged(zd, dev(zeta), nz, nv, ch)
    ctx.sync()
    assert np.array_equal(host(ch), O.mz_challenged(mats, zs, [zeta[i * d:(i + 1) * d] for i in range(nz)], nv, d))
    point = O.fill_uniform(nv * d, 70 + d)
    ev = dev(n=nz * t * d)
    M.mz_evaluate(zd, nz, nv, dev(point), ev)
    ctx.sync()
    w = want.reshape(nz * t, (1 << nv) * d)
    assert np.array_equal(host(ev), np.concatenate([O.mle_evaluate(w[k], nv, d, point) for k in range(nz * t)]))


# ------------------------------------------------------------------ fold() end to end
@pytest.mark.parametrize("d", [32, 128, 512])
def test_fold_prove_matches_oracle(d):
    """d = 2048 is left to the step-level tests above: the oracle's fold() alone takes
    about 12 s there"""
    W, l, t, deg, kappa = 5, 2, 4, 2, 2
    ctx = LA.Context(0)
    try:
        pr_o, ccs, A, prover = setup(ctx, d, W, l, t, deg, kappa, 7 + d + W)
        xa, Wa = witness(ccs, pr_o, 11)
        xi, Wi = witness(ccs, pr_o, 12)
        Nn = W * pr_o.L
        cma = O.ajtai_commit(A, kappa, Nn, d, Wa.f)
        cmi = O.ajtai_commit(A, kappa, Nn, d, Wi.f)
        acc = N.linearize_fresh(ccs, cma, xa, Wa, pr_o)
        o_out, o_w0, o_proof = N.fold_prove(ccs, A, kappa, acc, Wa, cmi, xi, Wi, pr_o)
        w_out = {"w_ccs": zeros(W * d), "f": zeros(Nn * d), "f_coeff": zeros(Nn * d)}
        out, pf = prover.fold_prove(acc_dict(acc), dev_wit(Wa), cmi, flat(xi), dev_wit(Wi), w_out)
        check_against_oracle(out, pf, w_out, o_out, o_w0, o_proof)
        # the restated verifier accepts the device's proof and re-derives its LCCCS
        v = N.fold_verify(ccs, acc, cmi, xi, proof_from_device(pf, d, pr_o.K, 1, ccs.t, l, kappa), pr_o)
        for k, want in acc_dict(v).items():
            assert np.array_equal(out[k], want), k
    finally:
        ctx.close()


# ------------------------------------------------------------------ still unsupported
@pytest.mark.parametrize("d", [8, 48, 8192])
def test_other_degrees_stay_unsupported(ctx, d):
    assert not LA.ring_supported(d)
    with pytest.raises(LA.LfError) as e:
        ctx.dev_crt(dev(n=d), d)
    assert e.value.code == LF_ERR_UNSUPPORTED_RING
    with pytest.raises(LA.LfError) as e:
        ctx.witness_from_w_ccs(np.zeros(d, np.uint64), LA.goldilocks_dp(d))
    assert e.value.code == LF_ERR_UNSUPPORTED_RING
