"""The premise of test_gpu_gm_advform_multidim.py, on the CPU: the oracle runs GM_AdvForm together
with the multi-dimensional schemes (oracle/thermo.c forms uRes, vRes, wRes and hands them to
gad_advection_dst3fl) on the two BASELINE experiments that carry GM/Redi, stays finite for 3
steps, has a bolus stream-function that is not zero, and tells the advective form from the
skew-flux form -- so a device that ignored the residual flow in its passes could not match it."""
import numpy as np
import pytest

GM_ADV = {"GM_AdvForm": 1, "GM_skewflx": 0.0}
GM_SKEW = {"GM_AdvForm": 0, "GM_skewflx": 1.0}


def adv(scheme, **over):
    return dict({"tempAdvScheme": scheme, "tempVertAdvScheme": scheme, "saltAdvScheme": scheme,
                 "saltVertAdvScheme": scheme, "multiDimAdvection": 1}, **over)


def _three_steps(factory, over):
    o, g = factory(params_over=over)
    for _ in range(3):
        o.forward_step()
    inner = (Ellipsis,) + g.sl(1, g.sNx, 1, g.sNy)
    fields = {n: np.array(o.arr(n)) for n in ("theta", "salt", "uVel", "vVel", "wVel", "etaN")}
    return fields, float(np.abs(np.array(o.arr("GM_PsiX"))).max()), float(fields["theta"][inner].sum())


@pytest.mark.parametrize("exp,scheme", [("ocean90", 30), ("ocean90", 33), ("cs32x15", 33), ("cs32x15", 30)])
def test_oracle_advform_multidim_finite_and_distinct_from_skew(exp, scheme):
    from oracle.harness import cs32x15_oracle, ocean90_oracle
    factory = ocean90_oracle if exp == "ocean90" else cs32x15_oracle
    fields, psi, total = _three_steps(factory, adv(scheme, **GM_ADV))
    for n, a in fields.items():
        assert np.isfinite(a).all(), n
    assert psi > 0.0
    _, psi_skew, total_skew = _three_steps(factory, adv(scheme, **GM_SKEW))
    assert psi_skew == 0.0
    print("%s scheme %d: max|GM_PsiX| = %.3f, sum(theta) = %.6f advective, %.6f skew" % (exp, scheme, psi, total, total_skew))
    assert total != total_skew
