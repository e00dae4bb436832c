"""LF_ERR_NOT_SATISFIED (CSError::NotSatisfied) has a status string of its own. No GPU."""
import latticeum_amd as LA

LF_ERR_NOT_SATISFIED = 14  # lf.h


def test_not_satisfied_status_string():
    lib = LA.load()
    s = lib.lf_status_string(LF_ERR_NOT_SATISFIED)
    assert s and s != lib.lf_status_string(999)  # not the unknown-status string
    assert s not in [lib.lf_status_string(i) for i in range(LF_ERR_NOT_SATISFIED)]
    assert LA.ERR_NOT_SATISFIED == LF_ERR_NOT_SATISFIED
    # the Python errors of the relation checks
    e = LA.RelationError(LA.REL_CCS, 6)
    assert isinstance(e, LA.LfError) and (e.code, e.check, e.row) == (12, 7, 6)
    assert LA.RelationError(LA.REL_CM).row is None
