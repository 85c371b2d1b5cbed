"""What makes tests/gad_reference.py a reference: checked on the CPU, before any GPU test leans on it.

1. The driver, against the oracle: with the module's own DST3FL (33) and DST3 (30), one
   pure-advection THERMODYNAMICS call (the tracer's diffusivities 0, implicitDiffusion = 0,
   ivdc_kappa = 0, no forcing, so the new tracer is T + dT * gAdv) equals the oracle bit for bit on
   the interior: advect_xy; the baroclinic gyre (4 tiles, spherical grid, land, 15 levels) from a
   state three steps old with the +12 K anomaly of test_gpu_3d.py; the same gyre with
   multiDimCompressible = 1.
2. Each new flux function against a closed form: upwind (1), DST2 (20), and OS7MP (7) on a linear
   profile, at zero transport and at a closed face.
3. Boundedness of scheme 1 over 80 steps of advect_xy(OL=4); the overshoot of scheme 7 in the same
   run is printed, not asserted (nobody has measured it).
"""
import numpy as np
import pytest

import gad_reference as gr


def _advect_xy(scheme, **kw):
    from mitgcm_amd import configs

    def cfg(**k2):
        g, p, s = configs.advect_xy(**dict(kw, **k2))
        p.update(saltAdvScheme=scheme, saltVertAdvScheme=scheme)
        return g, p, s
    return cfg


PURE = dict(diffKhT=0.0, diffKrT=0.0, implicitDiffusion=0, ivdc_kappa=0.0, tempForcing=0)


def _gyre(scheme, **over):
    from mitgcm_amd import configs

    def cfg(**kw):
        g, p, s = configs.baroclinic_gyre(tempAdvScheme=scheme, **kw)
        p.update(multiDimAdvection=1)
        p.update(over)
        return g, p, s
    return cfg


def _flow(o):
    return tuple(np.array(o.arr(n)) for n in ("uVel", "vVel", "wVel"))


# ---- 1. the driver, against the oracle -----------------------------------------------------

@pytest.mark.parametrize("scheme", [33, 30])
def test_driver_advect_xy_bitwise_vs_oracle(scheme):
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(_advect_xy(scheme))
    dT = o.get("deltaTtracer")
    inner = gr.interior(g)
    for n in range(18):
        if n in (0, 17):   # the disc at rest in the flow, and smeared over its neighbours
            S = np.array(o.arr("salt")).reshape(g.nTiles, 1, g.ny, g.nx)
            gAdv, _ = gr.gad_advection(g, S, *_flow(o), scheme, dT)
            want = (S + dT * gAdv)[inner]
            o.L.oracle_oceanic_phys(o.h)
            o.L.oracle_thermodynamics(o.h)
            got = np.array(o.arr("salt")).reshape(S.shape)[inner]
            assert np.array_equal(got, want), (n, np.abs(got - want).max())
            assert np.abs(got - S[inner]).max() > 1e-3   # (the call moved the disc)
            o.arr("salt").reshape(S.shape)[:] = S
        o.forward_step()


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("scheme", [33, 30])
def test_driver_gyre_bitwise_vs_oracle(scheme, comp):
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(_gyre(scheme, multiDimCompressible=comp, **PURE))
    for _ in range(3):
        o.forward_step()
    o.arr("theta")[:, 1, 10:16, 8:20] += 12.0
    dT = o.get("deltaTtracer")
    T = np.array(o.arr("theta"))
    u, v, w = _flow(o)
    assert np.abs(w).max() > 0.0 and (g.f["maskC"] == 0.0).any()
    gAdv, _ = gr.gad_advection(g, T, u, v, w, scheme, dT, comp=bool(comp))
    inner = gr.interior(g)
    want = (T + dT * gAdv)[inner]
    o.L.oracle_oceanic_phys(o.h)
    o.L.oracle_thermodynamics(o.h)
    got = np.array(o.arr("theta"))[inner]
    assert np.array_equal(got, want), np.abs(got - want).max()
    assert np.abs(got - T[inner]).max() > 1e-6


# ---- 2. the new flux functions, against closed forms ---------------------------------------

N, OL = 24, 4


def _line(rng, shape=(3, N + 2 * OL)):
    trans = rng.uniform(-5.0e3, 5.0e3, shape)
    cfl = rng.uniform(0.02, 0.98, shape)
    T = rng.uniform(-2.0, 30.0, shape)
    return trans, cfl, T


def _valid(scheme):
    lo, hi = gr._face_range(scheme, N, OL)
    return slice(lo + OL - 1, hi + OL)


def test_upwind_is_transport_times_upstream_cell():
    rng = np.random.default_rng(1)
    trans, cfl, T = _line(rng)
    af = gr.flux_h(1, trans, cfl, T, np.ones_like(T), N, OL)
    up = np.where(trans > 0.0, np.roll(T, 1, -1), T)
    sl = _valid(1)
    assert np.array_equal(af[..., sl], (trans * up)[..., sl])
    assert np.all(af[..., :sl.start] == 0.0)
    # vertical: rTrans > 0 is upward in the index (the cell below the face is upstream), maskC(k-1) outside
    L = rng.uniform(0.0, 30.0, (2, 9, 3, 4))
    rTr = rng.uniform(-1.0, 1.0, L.shape)
    mC = (rng.uniform(size=L.shape) > 0.2).astype(float)
    fv = gr.flux_r(1, rTr, np.full_like(L, 0.3), L, mC, -1.0)
    upv = np.where(rTr[:, 1:] > 0.0, L[:, 1:], L[:, :-1])   # rkSign = -1: wAbs = -|rTrans|
    assert np.array_equal(fv[:, 1:9], mC[:, :-1] * (rTr[:, 1:] * upv))
    assert np.all(fv[:, 0] == 0.0) and np.all(fv[:, 9] == 0.0)


def test_dst2_closed_form():
    """(uTrans+uAbs)/2 T(i-1) + (uTrans-uAbs)/2 T(i), uAbs = |uTrans| cfl.  The routine forms
    1 - xLimit (1 - cfl), which differs from cfl by at most 2^-53 absolute; with three roundings
    in each of the two evaluations the difference is below 6.5 * 2^-53 |uTrans| (|T(i-1)| + |T(i)|):
    bound 2^-50 of that scale."""
    rng = np.random.default_rng(2)
    trans, cfl, T = _line(rng)
    af = gr.flux_h(20, trans, cfl, T, np.ones_like(T), N, OL)
    tm1 = np.roll(T, 1, -1)
    uAbs = np.abs(trans) * cfl
    want = (trans + uAbs) / 2.0 * tm1 + (trans - uAbs) / 2.0 * T
    sl = _valid(20)
    tol = 2.0 ** -50 * np.abs(trans) * (np.abs(tm1) + np.abs(T))
    assert np.all(np.abs(af - want)[..., sl] <= tol[..., sl]), (np.abs(af - want) / tol)[..., sl].max()


@pytest.mark.parametrize("slope", [3.0, -7.0, 5.0])
def test_os7mp_linear_profile(slope):
    """Open masks, 0 < cfl < 1, an exactly representable linear profile: every correction past the
    first vanishes, the limiter leaves Phi = 1, the flux is uTrans (Qi + (1-cfl)/2 (Qip-Qi)) to
    4 ulp (Phi * recip_DelIp rounds once or twice)."""
    rng = np.random.default_rng(3)
    trans, cfl, _ = _line(rng)
    T = np.broadcast_to(11.0 + slope * np.arange(N + 2 * OL), trans.shape).copy()
    af = gr.flux_h(7, trans, cfl, T, np.ones_like(T), N, OL)
    tm1 = np.roll(T, 1, -1)
    Qi, Qip = np.where(trans > 0.0, tm1, T), np.where(trans > 0.0, T, tm1)
    want = trans * (Qi + (1.0 - cfl) / 2.0 * (Qip - Qi))
    sl = _valid(7)
    ulps = (np.abs(af - want) / np.spacing(np.abs(want)))[..., sl]
    print("OS7MP linear profile, slope %g: worst %.2f ulp" % (slope, ulps.max()))
    assert ulps.max() <= 4.0
    assert np.all(af[..., :sl.start] == 0.0) and np.all(af[..., sl.stop:] == 0.0)
    assert (trans[..., sl] > 0).any() and (trans[..., sl] < 0).any()


def test_os7mp_zero_transport_and_closed_face():
    rng = np.random.default_rng(4)
    trans, cfl, T = _line(rng)
    sl = _valid(7)
    trans[:, 10:14] = 0.0
    mask = np.ones_like(T)
    mask[:, 17] = 0.0
    mask[0, 20:22] = 0.0
    af = gr.flux_h(7, trans, cfl, T, mask, N, OL)
    assert np.all(af[:, 10:14] == 0.0)
    Qi = np.where(trans > 0.0, np.roll(T, 1, -1), T)
    closed = mask == 0.0
    closed[..., :sl.start] = False
    closed[..., sl.stop:] = False
    assert closed.sum() >= 5
    assert np.array_equal(af[closed], (trans * Qi)[closed])
    assert np.isfinite(af).all()


def test_os7mp_vertical_is_the_horizontal_stencil_turned():
    """Away from the clipped levels GAD_OS7MP_ADV_R is GAD_OS7MP_ADV_X along k with the transport's
    sign turned (rTrans > 0 has the cell below the face upstream): bitwise, with random masks."""
    rng = np.random.default_rng(5)
    Nr = 20
    L = rng.uniform(0.0, 30.0, (1, Nr, 2, 3))
    rTr = rng.uniform(-1.0, 1.0, L.shape)
    cfl = rng.uniform(0.05, 0.9, L.shape)
    mC = (rng.uniform(size=L.shape) > 0.15).astype(float)
    fv = gr.flux_r(7, rTr, cfl, L, mC, -1.0)
    mv = lambda a: np.moveaxis(a, 1, -1)
    fh = -gr.flux_h(7, mv(-rTr), mv(cfl), mv(L), mv(mC), Nr, 0)
    # faces k = 5 .. Nr-3 (array 4 .. Nr-4): no index clipped, and flux_h computed them at OL = 0
    assert np.array_equal(mv(fv[:, :Nr])[..., 4:Nr - 3], fh[..., 4:Nr - 3])
    assert np.all(fv[:, 0] == 0.0) and np.all(fv[:, Nr] == 0.0)
    # clipped differences are zeroed: with 5 levels nothing but levels 1..5 is ever read
    L5, r5, c5, m5 = L[:, :5], rTr[:, :5], cfl[:, :5], np.ones_like(L[:, :5])
    f5 = gr.flux_r(7, r5, c5, L5, m5, -1.0)
    assert np.isfinite(f5).all() and np.all(f5[:, 0] == 0.0) and np.all(f5[:, 5] == 0.0)


# ---- 3. boundedness ------------------------------------------------------------------------

def _run_advect_xy(scheme, nsteps=80):
    from mitgcm_amd import configs
    g, p, s = configs.advect_xy(OL=4)
    S, dT = s["salt"].copy(), p["deltaTtracer"]
    lo = hi = 0.0
    for _ in range(nsteps):
        gAdv, _ = gr.gad_advection(g, S, s["uVel"], s["vVel"], np.zeros_like(S), scheme, dT)
        S = g.exch(S + dT * gAdv)
        inner = S[gr.interior(g)]
        lo, hi = max(lo, 35.0 - inner.min()), max(hi, inner.max() - 36.0)
    return g, S, lo, hi


def test_upwind_bounded_on_advect_xy():
    """cfl = 0.25 in a uniform flow: every pass is a convex combination, so salt stays in [35, 36]."""
    g, S, lo, hi = _run_advect_xy(1)
    assert lo <= 1e-12 and hi <= 1e-12, (lo, hi)
    inner = S[gr.interior(g)]
    assert 35.0 < inner.mean() < 36.0 and inner.max() - inner.min() > 0.05   # (diffused, not gone)


def test_os7mp_overshoot_on_advect_xy_printed():
    g, S, lo, hi = _run_advect_xy(7)
    print("OS7MP on advect_xy(OL=4), 80 steps: undershoot %.3e below 35, overshoot %.3e above 36" % (lo, hi))
    assert np.isfinite(S).all()
