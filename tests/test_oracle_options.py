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


def test_oracle_aborts_on_u3_with_one_halo_row():
    """The same check for the U3 / C4 branches (GAD_OlMinSize 2, gad_init_fixed.F:44-49): their
    loops 1-OLx+2 .. sNx+OLx-1 would leave the tile-edge faces 1 and sNx+1 at zero flux with
    OL = 1.  The oracle is the reference of the passive tracers on schemes 3 and 4
    (test_gpu_ptracers_sweep.py), so it must refuse what mgcm_init refuses: the baroclinic gyre
    re-made with one halo row steps with scheme 2 and aborts with scheme 3; at OL = 2, the
    experiment's own, scheme 3 steps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = ("import resource, sys; sys.path.insert(0, %r)\n"
            "resource.setrlimit(resource.RLIMIT_CORE, (0, 0))\n"
            "import numpy as np\n"
            "from mitgcm_amd import configs\n"
            "from mitgcm_amd.grid import Grid\n"
            "from oracle.harness import oracle_from_config\n"
            "OL, scheme = int(sys.argv[1]), int(sys.argv[2])\n"
            "def cfg():\n"
            "    g, params, state = configs.baroclinic_gyre(nSx=1, nSy=1, tempAdvScheme=scheme)\n"
            "    if OL == g.OLx:\n"
            "        return g, params, state\n"
            "    h = Grid(g.sNx, g.sNy, OL, OL, g.Nr, 1, 1)\n"
            "    h.ini_vertical_grid(configs.BAROCLINIC_DELR)\n"
            "    h.ini_spherical_polar_grid(np.full(62, 1.0), np.full(62, 1.0), -1.0, 14.0)\n"
            "    h.ini_cori(selectCoriMap=2)\n"
            "    bathy = configs.read_bin(configs.os.path.join(configs.GOLDEN, 'tutorial_baroclinic_gyre', 'bathy.bin'), (62, 62))\n"
            "    h.ini_depths_masks(bathy, hFacMin=1.0, hFacMinDr=0.0, gBaro=9.81)\n"
            "    h.ini_cg2d(1200.0, 1200.0, 1e-7)\n"
            "    cut = lambda a: np.ascontiguousarray(a[..., g.OLy - OL:g.ny - g.OLy + OL, g.OLx - OL:g.nx - g.OLx + OL])\n"
            "    return h, params, {k: (cut(v) if np.ndim(v) >= 3 else v) for k, v in state.items()}\n"
            "o, g = oracle_from_config(cfg)\n"
            "assert (g.OLx, g.OLy) == (OL, OL)\n"
            "o.forward_step()\nprint('stepped')\n" % root)
    run = lambda OL, scheme: subprocess.run([sys.executable, "-c", prog, str(OL), str(scheme)], capture_output=True,
                                            text=True, timeout=120)
    for OL, scheme in ((2, 3), (1, 2)):
        ok = run(OL, scheme)
        assert ok.returncode == 0 and "stepped" in ok.stdout, (OL, scheme, ok.stderr)
    bad = run(1, 3)
    assert bad.returncode == -6 and "stepped" not in bad.stdout, (bad.returncode, bad.stdout)
    assert "Overlap Size OLx,OLy=1 1 too small: advection scheme 3 needs 2" in bad.stderr, bad.stderr
