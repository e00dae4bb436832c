"""lf_fold_verify on proofs the device made, at the X^d + 1 rings: Prover.fold_prove on the GPU,
then the host verifier accepts the proof and returns exactly the prover's folded LCCCS -- the
end-to-end check of fold() at d = 2048 and 4096, where the Python oracle's prover is too slow
to stand in. The degrees are those at which the device prover takes another path:

  d = 16    the smallest ring, a block below one wave
  d = 32    a radix-2 pass in front of the radix-4 ones
  d = 1024  the register NTT, the fused decomposition, the coefficient-form fold
  d = 2048, 4096  the LDS transform with several butterflies per thread

Up to d = 1024 the oracle's restated verifier gives the same LCCCS; at 2048 and 4096 a bumped
y_s and a bumped theta_s are rejected at their checks instead. At d = 16 and 1024 a third
instance is folded onto the VERIFIER's LCCCS with the device's folded witness, and that proof
verifies too; at d = 1024 the proof also goes through its wire bytes."""
import functools

import numpy as np
import pytest

import latticeum_amd as LA
import nifs as N
import oracle as O
from latticeum_amd import wire
from test_gpu_fold_prove import acc_dict, dev_wit, flat, proof_from_device, setup, witness, zeros
from test_wire_proof import Shape, to_bytes

pytestmark = pytest.mark.gpu

CASES = {16: (7, 1, 5, 3, 3), 32: (5, 2, 4, 2, 3), 1024: (5, 2, 4, 2, 2), 2048: (5, 2, 4, 2, 2),
         4096: (5, 2, 4, 2, 2)}  # d: (W, l, t, deg, kappa)
CHAINED = (16, 1024)
VERIFY_DEC_Y, VERIFY_FOLD_CLAIM = 3, 8  # lf.h lf_verify_check


def verify(ccs, kappa, acc, cmi, xi, pf):
    return LA.fold_verify(LA.goldilocks_dp(ccs.d), ccs.t, ccs.m, ccs.l, ccs.degree, flat(ccs.c), ccs.S, kappa, acc,
                          cmi, flat(xi), pf)


def lcccs(a, d):
    return N.LCCCS(r=N.elems(a["r"], d), v=N.elems(a["v"], d), cm=a["cm"], u=N.elems(a["u"], d),
                   x_w=N.elems(a["x_w"], d), h=a["h"])


@functools.lru_cache(maxsize=None)
def folded(d):
    """one device fold per degree (and, where chained, a second one onto the verifier's LCCCS),
    shared read only by the tests below: everything as host arrays"""
    W, l, t, deg, kappa = CASES[d]
    ctx = LA.Context(0)
    try:
        pr_o, ccs, A, prover = setup(ctx, d, W, l, t, deg, kappa, 7 + d + W)
        (xa, Wa), (xi, Wi) = witness(ccs, pr_o, 11), witness(ccs, pr_o, 12)
        Nn = W * pr_o.L
        cma, cmi = O.ajtai_commit(A, kappa, Nn, d, Wa.f), O.ajtai_commit(A, kappa, Nn, d, Wi.f)
        acc, _ = prover.linearize(cma, flat(xa), dev_wit(Wa))  # initialize_accumulator's accumulator
        w_out = {"w_ccs": zeros(W * d), "f": zeros(Nn * d), "f_coeff": zeros(Nn * d)}
        out, pf = prover.fold_prove(acc, dev_wit(Wa), cmi, flat(xi), dev_wit(Wi), w_out)
        res = dict(pr=pr_o, ccs=ccs, kappa=kappa, acc=acc, cmi=cmi, xi=xi, out=out, pf=pf)
        if d in CHAINED:
            x3, W3 = witness(ccs, pr_o, 13)
            cm3 = O.ajtai_commit(A, kappa, Nn, d, W3.f)
            acc2 = verify(ccs, kappa, acc, cmi, xi, pf)  # the verifier's, not the prover's
            w_out2 = {"w_ccs": zeros(W * d), "f": zeros(Nn * d), "f_coeff": zeros(Nn * d)}
            out2, pf2 = prover.fold_prove(acc2, w_out, cm3, flat(x3), dev_wit(W3), w_out2)
            res.update(acc2=acc2, cm3=cm3, x3=x3, out2=out2, pf2=pf2)
        return res
    finally:
        ctx.close()


@pytest.mark.parametrize("d", sorted(CASES))
def test_verifier_accepts_the_device_proof(d):
    c = folded(d)
    got = verify(c["ccs"], c["kappa"], c["acc"], c["cmi"], c["xi"], c["pf"])
    assert sorted(got) == sorted(c["out"])
    for k, v in c["out"].items():
        assert np.array_equal(got[k], v), k
    if d <= 1024:  # and the restated verifier on the same proof
        ccs, l = c["ccs"], CASES[d][1]
        proof = proof_from_device(c["pf"], d, c["pr"].K, 1, ccs.t, l, c["kappa"])
        want = acc_dict(N.fold_verify(ccs, lcccs(c["acc"], d), c["cmi"], c["xi"], proof, c["pr"]))
        for k, v in want.items():
            assert np.array_equal(got[k], v), k


@pytest.mark.parametrize("d", [2048, 4096])
@pytest.mark.parametrize("field,elem,check", [("y_s", 3, VERIFY_DEC_Y), ("theta_s", 17, VERIFY_FOLD_CLAIM)])
def test_large_rings_reject_a_bumped_element(d, field, elem, check):
    c = folded(d)
    pf = dict(c["pf"])
    if field == "y_s":  # side 0
        side0 = pf["y_s"][0].copy()
        side0[elem * d:(elem + 1) * d] = N.add(side0[elem * d:(elem + 1) * d], N.one(d))
        pf["y_s"] = [side0, pf["y_s"][1]]
    else:
        th = pf["theta_s"].copy()
        th[elem * d:(elem + 1) * d] = N.add(th[elem * d:(elem + 1) * d], N.one(d))
        pf["theta_s"] = th
    with pytest.raises(LA.VerificationError) as e:
        verify(c["ccs"], c["kappa"], c["acc"], c["cmi"], c["xi"], pf)
    assert e.value.check == check


@pytest.mark.parametrize("d", CHAINED)
def test_chain_onto_the_verifiers_lcccs(d):
    c = folded(d)
    for k, v in c["out"].items():
        assert np.array_equal(c["acc2"][k], v), k
    got = verify(c["ccs"], c["kappa"], c["acc2"], c["cm3"], c["x3"], c["pf2"])
    for k, v in c["out2"].items():
        assert np.array_equal(got[k], v), k
    assert not np.array_equal(c["out2"]["r"], c["out"]["r"])


def test_wire_round_trip_of_the_device_proof():
    d = 1024
    c = folded(d)
    sh = Shape(c["ccs"], c["pr"], c["kappa"])
    data = to_bytes(c["pf"], sh)
    back = wire.deserialize_lfproof(data, *sh.args())
    assert to_bytes(back, sh) == data
    got = verify(c["ccs"], c["kappa"], c["acc"], c["cmi"], c["xi"], back)
    for k, v in c["out"].items():
        assert np.array_equal(got[k], v), k
