"""Oracle restatements of the option variants the device path implements beyond the
BASELINE namelists (tests/test_gpu_options.py compares the device with them): implicit
vertical viscosity (MOM_U/V_IMPLICIT_R) and DST3 without limiter (scheme 30).  No
reference output exists for these variants in the tree (parity unpinned against the
reference); here: the options take effect, stay finite, and scheme 30 conserves the
tracer content of a closed basin as the flux form must.  An overlap smaller than GAD_CHECK
demands stops the oracle as it stops the reference and mgcm_init."""
import os
import subprocess
import sys

import numpy as np


def _gyre(scheme=2, **over):
    from mitgcm_amd import configs

    def cfg(**kw):
        g, params, state = configs.baroclinic_gyre(tempAdvScheme=scheme, **kw)
        params.update(over)
        return g, params, state
    return cfg


def _run(cfg, n):
    from oracle.harness import oracle_from_config
    o, g = oracle_from_config(cfg)
    for _ in range(n):
        o.forward_step()
    return o, g


def test_implicit_viscosity_changes_momentum_only_through_vertical_viscosity():
    o0, g = _run(_gyre(2), 3)
    o1, _ = _run(_gyre(2, implicitViscosity=1), 3)
    u0, u1 = np.array(o0.arr("uVel")), np.array(o1.arr("uVel"))
    assert np.isfinite(u1).all()
    d = np.abs(u1 - u0).max()
    # viscAr = 1e-2 over 3 steps of 1200 s: a small but non-zero change
    assert 0.0 < d < 1e-2 * np.abs(u0).max(), d


def test_dst3_scheme30_differs_from_33_and_stays_bounded():
    o30, g = _run(_gyre(30), 4)
    o33, _ = _run(_gyre(33), 4)
    t30, t33 = np.array(o30.arr("theta")), np.array(o33.arr("theta"))
    inner = (slice(None), slice(None)) + g.sl(1, g.sNx, 1, g.sNy)
    assert np.isfinite(t30).all()
    assert not np.array_equal(t30[inner], t33[inner])
    assert np.abs(t30[inner] - t33[inner]).max() < 1e-3



def test_oracle_aborts_on_an_overlap_gad_check_refuses():
    """GAD_CHECK (gad_check.F:115-130) stops the reference when OLx, OLy < minOlSize: 2 for the
    DST3 schemes (gad_init_fixed.F:50-51), doubled for multi-dimensional advection on the cube
    (:178-181).  The oracle's loops would run regardless and leave the outer halo fluxes at
    zero, so it aborts instead: DST3FL on a cube at OL = 3 (the device refuses the same case,
    test_gpu_options.py::test_unsupported_options_refused[dst3_cube_ol3]); at OL = 4 it steps.
    A child process: abort() ends the process it is called in."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = ("import resource, sys; sys.path.insert(0, %r)\n"
            "resource.setrlimit(resource.RLIMIT_CORE, (0, 0))\n"      # abort() leaves no core file behind
            "from mitgcm_amd import configs\n"
            "from oracle.harness import oracle_from_config\n"
            "over = dict(tempAdvScheme=33, tempVertAdvScheme=33, saltAdvScheme=33, saltVertAdvScheme=33)\n"
            "o, g = oracle_from_config(lambda: configs.cube_synthetic(9, 2, OL=int(sys.argv[1]), params_over=over))\n"
            "o.forward_step()\nprint('stepped')\n" % root)
    ok = subprocess.run([sys.executable, "-c", prog, "4"], capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0 and "stepped" in ok.stdout, ok.stderr
    bad = subprocess.run([sys.executable, "-c", prog, "3"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == -6 and "stepped" not in bad.stdout, (bad.returncode, bad.stdout)
    assert "Overlap Size OLx,OLy=3 3 too small" in bad.stderr, bad.stderr
