"""A numpy restatement of the reference's multi-dimensional tracer advection (GAD_ADVECTION with the
direct-space-time flux functions), for the tests only: the package never imports it.

Array code in the reference's operation order, so that a device result can be compared bit for
bit: numpy evaluates one IEEE double operation per ufunc call, with no fused multiply-add.

  flux functions (each over the faces its own loop computes; the others stay zero):
    GAD_DST3_ADV_X/Y/R       30   gad_dst3_adv_x.F:71-118, gad_dst3_adv_r.F:70-119
    GAD_DST3FL_ADV_X/Y/R     33   gad_dst3fl_adv_x.F:47-99, gad_dst3fl_adv_r.F:70-119
    GAD_DST2U1_ADV_X/Y/R   1, 20  gad_dst2u1_adv_x.F:57-81, gad_dst2u1_adv_r.F:57-90
    GAD_OS7MP_ADV_X/Y/R       7   gad_os7mp_adv_x.F:48-208, gad_os7mp_adv_r.F:46-204
  the lat-lon driver (gad_advection.F:292-1074, one pass with X then Y, then the k loop):
    gad_advection(..., comp=False)  the update with maskInC (:556-574, :779-797, :1061-1073)
    gad_advection(..., comp=True)   GAD_MULTIDIM_COMPRESSIBLE with the local volume
                                    (:302-310, :541-555, :764-778, :1034-1059)

Fields are tile arrays with their halos, (nTiles, Nr, ny, nx) and (nTiles, ny, nx), as Grid.f and
Model.get hold them; Fortran index i is array index i + OL - 1.  Only the interior of the result
is meaningful (what the device produces).  tests/test_gad_reference.py pins this module against
the oracle (schemes 30, 33) and against closed forms (1, 20, 7) on the CPU.
"""
import numpy as np

SCHEMES = (30, 33, 1, 20, 7)
_EPS = 1.0e-20


def _sh(a, o, axis=-1):
    """a shifted so that out[I] = a[I + o] along `axis` (wrapping; callers zero the faces whose
    stencil would wrap)."""
    return np.roll(a, -o, axis=axis)


def _face_range(scheme, n, OL):
    """First and last face (Fortran index) the scheme's routine computes along a direction of n
    points and overlap OL: gad_dst3fl_adv_x.F:66-72, gad_dst2u1_adv_x.F:60-64, gad_os7mp_adv_x.F:50-60."""
    if scheme in (1, 20):
        return 2 - OL, n + OL
    if scheme == 7:
        return 5 - OL, n + OL - 3
    return 3 - OL, n + OL - 1


def _dst3_limit(d0, d1, theta, cfl):
    psi = d0 + d1 * theta
    return np.maximum(0.0, np.minimum(np.minimum(1.0, psi), theta * (1.0 - cfl) / (cfl + 1.0e-20)))


def _dst3_theta(Rj, Ro):
    thetaMax = 1.0e+20
    big = np.abs(Rj) * thetaMax <= np.abs(Ro)
    with np.errstate(all="ignore"):
        return np.where(big, np.copysign(thetaMax, Ro * Rj), Ro / np.where(big, 1.0, Rj))


def os7mp_core(tr, cfl, Q, M):
    """The body of GAD_OS7MP_ADV_* past the stencil choice (gad_os7mp_adv_x.F:113-205).
    Q = (Qippp, Qipp, Qip, Qi, Qim, Qimm, Qimmm), M = (MskIpp, MskIp, MskI, MskIm, MskImm, MskImmm),
    upstream-ordered; tr == 0 gives 0 (:206-207)."""
    Qippp, Qipp, Qip, Qi, Qim, Qimm, Qimmm = Q
    MskIpp, MskIp, MskI, MskIm, MskImm, MskImmm = M
    with np.errstate(all="ignore"):
        Fac = 1.0
        DelP = (Qip - Qi) * MskI
        Phi = Fac * DelP
        Fac = Fac * (cfl + 1.0) / 3.0
        DelM = (Qi - Qim) * MskIm
        Del2 = DelP - DelM
        Phi = Phi - Fac * Del2
        Fac = Fac * (cfl - 2.0) / 4.0
        DelPP = (Qipp - Qip) * MskIp * MskI
        Del2P = DelPP - DelP
        Del3P = Del2P - Del2
        Phi = Phi + Fac * Del3P
        Fac = Fac * (cfl - 3.0) / 5.0
        DelMM = (Qim - Qimm) * MskImm * MskIm
        Del2M = DelM - DelMM
        Del3M = Del2 - Del2M
        Del4 = Del3P - Del3M
        Phi = Phi + Fac * Del4
        Fac = Fac * (cfl + 2.0) / 6.0
        # (:138-139: DelPPP is formed and not used, Del2PP = DelPP - DelP)
        Del2PP = DelPP - DelP
        Del3PP = Del2PP - Del2P
        Del4P = Del3PP - Del3P
        Del5P = Del4P - Del4
        Phi = Phi + Fac * Del5P
        Fac = Fac * (cfl + 2.0) / 7.0
        DelMMM = (Qimm - Qimmm) * MskImmm * MskImm * MskIm
        Del2MM = DelMM - DelMMM
        Del3MM = Del2M - Del2MM
        Del4M = Del3M - Del3MM
        Del5M = Del4 - Del4M
        Del6 = Del5P - Del5M
        Phi = Phi - Fac * Del6

        DelIp = (Qip - Qi) * MskI
        recip_DelIp = np.copysign(1.0, DelIp) / np.maximum(np.abs(DelIp), _EPS)
        Phi = Phi * recip_DelIp
        DelI = (Qi - Qim) * MskIm
        recip_DelI = np.copysign(1.0, DelI) / np.maximum(np.abs(DelI), _EPS)
        rp1h = DelI * recip_DelIp
        rp1h_cfl = rp1h / (cfl + _EPS)
        d2, d2p1, d2m1 = Del2, Del2P, Del2M
        A, B, C, D = 4.0 * d2 - d2p1, 4.0 * d2p1 - d2, d2, d2p1
        dp1h = (np.maximum(np.minimum(np.minimum(A, B), np.minimum(C, D)), 0.0) +
                np.minimum(np.maximum(np.maximum(A, B), np.maximum(C, D)), 0.0))
        A, B, C, D = 4.0 * d2m1 - d2, 4.0 * d2 - d2m1, d2m1, d2
        dm1h = (np.maximum(np.minimum(np.minimum(A, B), np.minimum(C, D)), 0.0) +
                np.minimum(np.maximum(np.maximum(A, B), np.maximum(C, D)), 0.0))
        PhiMD = 1.0 / (1.0 - cfl) * (DelIp - dp1h) * recip_DelIp
        PhiLC = rp1h_cfl * (1.0 + dm1h * recip_DelI)
        PhiMin = np.maximum(np.minimum(0.0, PhiMD), np.minimum(np.minimum(0.0, 2.0 * rp1h_cfl), PhiLC))
        PhiMax = np.minimum(np.maximum(2.0 / (1.0 - cfl), PhiMD), np.maximum(np.maximum(0.0, 2.0 * rp1h_cfl), PhiLC))
        Phi = np.maximum(PhiMin, np.minimum(Phi, PhiMax))
        Psi = Phi * 0.5 * (1.0 - cfl)
        out = tr * (Qi + Psi * DelIp)
    return np.where(tr != 0.0, out, 0.0)


def flux_h(scheme, trans, cfl, T, mask, n, OL):
    """The face flux along the LAST axis: face I lies between cells I - 1 and I.  trans, cfl, T and
    mask (maskLocW / maskLocS) are arrays of one shape; n, OL the tile's points and overlap along
    that axis.  Faces outside the routine's own loop are zero."""
    tm1, t0 = _sh(T, -1), T
    if scheme in (1, 20):
        xLimit = 1.0 if scheme == 20 else 0.0
        uAbs = np.abs(trans) * (1.0 - xLimit * (1.0 - cfl))
        af = (trans + uAbs) * 0.5 * tm1 + (trans - uAbs) * 0.5 * t0
    elif scheme in (30, 33):
        tm2, tp1 = _sh(T, -2), _sh(T, 1)
        oneSixth = 1.0 / 6.0
        Rjp = (tp1 - t0) * _sh(mask, 1)
        Rj = (t0 - tm1) * mask
        Rjm = (tm1 - tm2) * _sh(mask, -1)
        d0 = (2.0 - cfl) * (1.0 - cfl) * oneSixth
        d1 = (1.0 - cfl * cfl) * oneSixth
        if scheme == 30:
            af = (0.5 * (trans + np.abs(trans)) * (tm1 + (d0 * Rj + d1 * Rjm)) +
                  0.5 * (trans - np.abs(trans)) * (t0 - (d0 * Rj + d1 * Rjp)))
        else:
            psiP = _dst3_limit(d0, d1, _dst3_theta(Rj, Rjm), cfl)
            psiM = _dst3_limit(d0, d1, _dst3_theta(Rj, Rjp), cfl)
            af = 0.5 * (trans + np.abs(trans)) * (tm1 + psiP * Rj) + 0.5 * (trans - np.abs(trans)) * (t0 - psiM * Rj)
    elif scheme == 7:
        pos = trans > 0.0
        q = {o: _sh(T, o) for o in range(-4, 4)}
        m = {o: _sh(mask, o) for o in range(-3, 4)}
        Q = tuple(np.where(pos, q[a], q[b]) for a, b in ((2, -3), (1, -2), (0, -1), (-1, 0), (-2, 1), (-3, 2), (-4, 3)))
        M = tuple(np.where(pos, m[a], m[b]) for a, b in ((2, -2), (1, -1), (0, 0), (-1, 1), (-2, 2), (-3, 3)))
        af = os7mp_core(trans, cfl, Q, M)
    else:
        raise ValueError("scheme %r" % (scheme,))
    lo, hi = _face_range(scheme, n, OL)
    out = np.zeros_like(af)
    sl = slice(lo + OL - 1, hi + OL)
    out[..., sl] = af[..., sl]
    return out


def flux_r(scheme, rTrans, cfl, L, maskC, rkSign):
    """fVerT through the top of every level: (nTiles, Nr + 1, ny, nx), entry k - 1 for level k,
    zero at k = 1 and below Nr.  rTrans, cfl, L, maskC: (nTiles, Nr, ny, nx)."""
    Nr = L.shape[1]
    k = np.arange(1, Nr + 1)
    cl = lambda kk: np.clip(kk, 1, Nr)
    Q = lambda kk: L[:, kk - 1]
    MC = lambda kk: maskC[:, kk - 1]
    km1, km2, km3, km4, kp1, kp2, kp3 = cl(k - 1), cl(k - 2), cl(k - 3), cl(k - 4), cl(k + 1), cl(k + 2), cl(k + 3)
    if scheme in (1, 20):
        rLimit = 1.0 if scheme == 20 else 0.0
        wAbs = np.abs(rTrans) * rkSign * (1.0 - rLimit * (1.0 - cfl))
        fv = MC(km1) * ((rTrans + wAbs) * 0.5 * Q(km1) + (rTrans - wAbs) * 0.5 * Q(k))
    elif scheme in (30, 33):
        oneSixth = 1.0 / 6.0
        Rjp = (Q(k) - Q(kp1)) * MC(kp1)
        Rj = (Q(km1) - Q(k)) * MC(k) * MC(km1)
        Rjm = (Q(km2) - Q(km1)) * MC(km1)
        d0 = (2.0 - cfl) * (1.0 - cfl) * oneSixth
        d1 = (1.0 - cfl * cfl) * oneSixth
        if scheme == 30:
            fv = (0.5 * (rTrans + np.abs(rTrans)) * (Q(k) + (d0 * Rj + d1 * Rjp)) +
                  0.5 * (rTrans - np.abs(rTrans)) * (Q(km1) - (d0 * Rj + d1 * Rjm)))
        else:
            psiP = _dst3_limit(d0, d1, _dst3_theta(Rj, Rjm), cfl)
            psiM = _dst3_limit(d0, d1, _dst3_theta(Rj, Rjp), cfl)
            fv = (0.5 * (rTrans + np.abs(rTrans)) * (Q(k) + psiM * Rj) +
                  0.5 * (rTrans - np.abs(rTrans)) * (Q(km1) - psiP * Rj))
    elif scheme == 7:
        fl = lambda a, b: (a - b).astype(np.float64)[None, :, None, None]   # float(kp2-kp1): zero where clipped
        neg = rTrans < 0.0
        down = (Q(kp2), Q(kp1), Q(k), Q(km1), Q(km2), Q(km3), Q(km4))        # wTrans < 0 (:62-76)
        up = (Q(km3), Q(km2), Q(km1), Q(k), Q(kp1), Q(kp2), Q(kp3))          # wTrans > 0 (:77-91)
        mdown = (MC(kp2) * fl(kp2, kp1), MC(kp1) * fl(kp1, k), MC(k) * fl(k, km1), MC(km1) * fl(km1, km2),
                 MC(km2) * fl(km2, km3), MC(km3) * fl(km3, km4))
        mup = (MC(km2) * fl(km2, km3), MC(km1) * fl(km1, km2), MC(k) * fl(k, km1), MC(kp1) * fl(kp1, k),
               MC(kp2) * fl(kp2, kp1), MC(kp3) * fl(kp3, kp2))
        fv = os7mp_core(rTrans, cfl, tuple(np.where(neg, a, b) for a, b in zip(down, up)),
                        tuple(np.where(neg, a, b) for a, b in zip(mdown, mup)))
    else:
        raise ValueError("scheme %r" % (scheme,))
    out = np.zeros((L.shape[0], Nr + 1) + L.shape[2:])
    out[:, 1:Nr] = fv[:, 1:]
    return out


def _sw(a):
    return np.swapaxes(a, -1, -2)


def gad_advection(g, T, u, v, w, scheme, dT, comp=False, rkSign=-1.0, f=None):
    """gAdv of one tracer from GAD_ADVECTION's lat-lon form: the X pass, the Y pass on its result,
    the vertical pass and the tendency.  g: the Grid (sizes); f: the grid fields to use (default
    g.f; a model's own where r* has moved hFac); T, u, v, w: the tracer and the advecting flow
    (uVel, vVel, wVel, or GM_AdvForm's uRes, vRes, wRes), (nTiles, Nr, ny, nx).
    Returns (gAdv, loc): the tendency and the tracer after the three passes; interior only."""
    f = g.f if f is None else f
    OLx, OLy, sNx, sNy, Nr = g.OLx, g.OLy, g.sNx, g.sNy, g.Nr
    drF = np.asarray(f["drF"])[:Nr][None, :, None, None]
    rdrF = np.asarray(f["recip_drF"])[:Nr][None, :, None, None]
    rdrC = np.asarray(f["recip_drC"])[:Nr][None, :, None, None]
    b2 = lambda n: np.asarray(f[n])[:, None]
    rA, rrA, mIn = b2("rA"), b2("recip_rA"), b2("maskInC")
    hC, rhC, mC = f["hFacC"], f["recip_hFacC"], f["maskC"]
    shp = (g.nTiles, Nr, g.ny, g.nx)
    T, u, v, w = (np.asarray(x, dtype=np.float64).reshape(shp) for x in (T, u, v, w))

    uTr = u * (b2("dyG") * drF * f["hFacW"])
    vTr = v * (b2("dxG") * drF * f["hFacS"])
    cflU = np.abs(u * dT * b2("recip_dxC"))
    cflV = np.abs(v * dT * b2("recip_dyC"))
    loc = T.copy()
    if comp:
        vol = rA * drF * hC + (1.0 - mC)

    # X (gad_advection.F:386-574): every row, i = 2-OLx .. sNx+OLx-1
    af = flux_h(scheme, uTr, cflU, loc, f["maskW"], sNx, OLx)
    I = slice(1, g.nx - 1)
    dF = (_sh(af, 1) - af)[..., I]
    dU = (_sh(uTr, 1) - uTr)[..., I]
    if comp:
        tmpTrac = loc[..., I] * vol[..., I] - dT * dF * mIn[..., I]
        nv = vol[..., I] - dT * dU * mIn[..., I]
        vol[..., I] = nv
        loc[..., I] = tmpTrac / nv
    else:
        loc[..., I] = loc[..., I] - dT * rhC[..., I] * rdrF * rrA[..., I] * (dF - T[..., I] * dU) * mIn[..., I]

    # Y (:607-797) on the X pass's result: every column, j = 2-OLy .. sNy+OLy-1
    af = _sw(flux_h(scheme, _sw(vTr), _sw(cflV), _sw(loc), _sw(f["maskS"]), sNy, OLy))
    J = slice(1, g.ny - 1)
    dF = (_sh(af, 1, -2) - af)[..., J, :]
    dU = (_sh(vTr, 1, -2) - vTr)[..., J, :]
    if comp:
        tmpTrac = loc[..., J, :] * vol[..., J, :] - dT * dF * mIn[..., J, :]
        nv = vol[..., J, :] - dT * dU * mIn[..., J, :]
        vol[..., J, :] = nv
        loc[..., J, :] = tmpTrac / nv
    else:
        loc[..., J, :] = (loc[..., J, :] - dT * rhC[..., J, :] * rdrF * rrA[..., J, :] *
                          (dF - T[..., J, :] * dU) * mIn[..., J, :])

    # the k loop (:920-1074): rTrans = wFld rA maskC(k-1), 0 at the surface; kp1Msk = 0 at k = Nr
    rTr = np.zeros_like(T)
    rTr[:, 1:] = w[:, 1:] * rA * mC[:, :-1]
    cflW = np.abs(w * dT * rdrC)
    fv = flux_r(scheme, rTr, cflW, loc, mC, rkSign)
    kp1Msk = np.ones(Nr)
    kp1Msk[-1] = 0.0
    rTrKp = np.zeros_like(T)
    rTrKp[:, :-1] = rTr[:, 1:]
    rTrKp = kp1Msk[None, :, None, None] * rTrKp
    fUp, fDn = fv[:, :Nr], fv[:, 1:]
    if comp:
        tmpTrac = loc * vol - dT * (fDn - fUp) * rkSign * mIn
        lv = vol - dT * (rTrKp - rTr) * rkSign * mIn
        with np.errstate(all="ignore"):
            gAdv = (tmpTrac - T * lv) * rrA * rdrF * rhC / dT
            lt = tmpTrac / lv
    else:
        lt = loc - dT * rhC * rdrF * rrA * (fDn - fUp - T * (rTrKp - rTr)) * rkSign * mIn
        gAdv = (lt - T) / dT
    return gAdv, lt


def interior(g):
    """Index of the interior of a (nTiles, Nr, ny, nx) array."""
    return (slice(None), slice(None)) + g.sl(1, g.sNx, 1, g.sNy)
