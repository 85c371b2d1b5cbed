"""The fold's grids compiled for global_ocean.90x40x15's option set (MGCM_STEP_FUSE bit 65536,
common.h OptsGO90; kernels_step.hip k_dt_l2 / k_dt_l3 with their pinned instantiations).

Only which code is compiled changes, so everything is compared BITWISE:

  * config 2 re-tiled (5 x 5 tiles of 18 x 8 and 18 x 8 tiles of 5 x 5: ragged planes, blocks that
    cross tiles): 4 steps against the oracle with the default mask, 'specialised' on; the same
    model with the mask minus the bit, 'specialised' off; the two device runs against each other,
    every field of the state with its halos and the solve history, after one 6-step call (the
    pipelined head) and after 2 + 4 steps (a plain call, then a pipelined one);
  * three options moved off the pinned set, one at a time: 'specialised' is off and 4 steps are
    the oracle's;
  * a pinned option moved by mgcm_set_param after mgcm_init: after 4 specialised steps
    'specialised' flips off and the next 4 steps are the generic library's; moved before the first
    step, 4 steps are those of a model created with that value.
"""
import numpy as np
import pytest

import shapes
from test_gpu_refpin import STATE as OCEAN90_STATE
from test_gpu_step_pipeline import _differences

gpu = pytest.mark.gpu

SPEC_BIT = 65536
# MGCM_STEP_FUSE as common.h's default composes it (mg_fuse_mask)
FUSE_DEFAULT = 1 | 4 | 8 | 128 | 256 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768 | SPEC_BIT
TILINGS = [(5, 5), (18, 8)]


def _env(monkeypatch, on):
    monkeypatch.setenv("MGCM_OVERLAP", "1")   # (no timing-dependent choice of the layout)
    monkeypatch.setenv("MGCM_STEP_FUSE", str(FUSE_DEFAULT if on else FUSE_DEFAULT & ~SPEC_BIT))


def _ocean90(nSx=1, nSy=1, **over):
    from mitgcm_amd import configs
    return lambda: configs.global_ocean_90x40x15(nSx=nSx, nSy=nSy, params_over=over or None)


def _snapshot(m, nhist):
    out = {n: m.get(n) for n in OCEAN90_STATE}
    it, fr, lr = m.solve_history(nhist)
    out["cg2d_iters"], out["cg2d_init_res"], out["cg2d_last_res"] = it.astype(np.float64), fr, lr
    out["myIter"] = np.array([float(m.my_iter())])
    return out


def _run(cfg, calls, on, monkeypatch, before=None):
    """A model of cfg, before(m) on it, then forward_step(k) for k in calls.  Returns (snapshot
    after the last call with that call's solve history, step_layout())."""
    from mitgcm_amd import configs
    _env(monkeypatch, on)
    m = configs.make_model(cfg)
    try:
        if before is not None:
            before(m)
        for k in calls:
            m.forward_step(k)
        return _snapshot(m, calls[-1]), m.step_layout()
    finally:
        m.close()


# ---- config 2 re-tiled ----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("tiling", TILINGS, ids=["%dx%d" % t for t in TILINGS])
@pytest.mark.parametrize("on", [True, False], ids=["spec", "generic"])
def test_retiled_4_steps_vs_oracle(tiling, on, monkeypatch):
    """4 steps bit for bit against the oracle, default mask ('specialised') and mask minus the bit."""
    from oracle.harness import ocean90_oracle
    nSx, nSy = tiling
    _env(monkeypatch, on)
    _, _, layout = shapes.assert_bitexact_steps(_ocean90(nSx, nSy), 4, OCEAN90_STATE,
                                                oracle_factory=lambda cfg: ocean90_oracle(nSx=nSx, nSy=nSy))
    assert layout["dyn_thermo_fused"] and layout["specialised"] == on, layout


@gpu
@pytest.mark.parametrize("tiling", TILINGS, ids=["%dx%d" % t for t in TILINGS])
@pytest.mark.parametrize("calls", [(6,), (2, 4)], ids=["6", "2+4"])
def test_retiled_spec_against_generic(tiling, calls, monkeypatch):
    """The two device runs against each other: the state with its halos and the solve history."""
    cfg = _ocean90(*tiling)
    off, lay_off = _run(cfg, calls, False, monkeypatch)
    on, lay_on = _run(cfg, calls, True, monkeypatch)
    assert lay_on["specialised"] and lay_on["pipelined"] and lay_on["dyn_thermo_fused"], lay_on
    assert not lay_off["specialised"] and lay_off["pipelined"], lay_off
    assert np.isfinite(off["uVel"]).all() and np.abs(off["uVel"]).max() > 0.0
    bad = _differences(on, off)
    assert not bad, bad


def test_default_mask_has_the_bit(monkeypatch):
    """(host only) FUSE_DEFAULT above is the library's default mask with the new bit in it."""
    assert FUSE_DEFAULT & SPEC_BIT and FUSE_DEFAULT & ~SPEC_BIT == 1 | 4 | 8 | 128 | 256 | 1024 | 2048 | 4096 | 8192 | 16384 | 32768


# ---- options off the pinned set -------------------------------------------------------------
OFF_PIN = {"no_biharmonic": dict(viscA4D=0.0, viscA4Z=0.0), "free_slip_sides": dict(no_slip_sides=0),
           "no_nh_metric": dict(useNHMTerms=0)}


@gpu
@pytest.mark.parametrize("case", list(OFF_PIN))
def test_off_pin_generic_4_steps_vs_oracle(case, monkeypatch):
    """One option off the pinned set, default mask: the generic instantiation, the oracle's bits."""
    from oracle.harness import ocean90_oracle
    over = OFF_PIN[case]
    monkeypatch.setenv("MGCM_OVERLAP", "1")
    monkeypatch.delenv("MGCM_STEP_FUSE", raising=False)
    _, _, layout = shapes.assert_bitexact_steps(_ocean90(**over), 4, OCEAN90_STATE,
                                                oracle_factory=lambda cfg: ocean90_oracle(params_over=over))
    assert layout["dyn_thermo_fused"] and not layout["specialised"], layout


# ---- a pinned option moved after mgcm_init --------------------------------------------------
@gpu
def test_late_set_param_replans(monkeypatch):
    """4 specialised steps, then no_slip_sides = 0 through mgcm_set_param: the plan drops the pinned
    instantiation, and 4 more steps are those of a model that ran the same 8 steps and the same
    move with the generic kernels throughout."""
    from mitgcm_amd._lib import check, lib
    seen = {}

    def late(m):
        m.forward_step(4)
        seen["before"] = m.step_layout()["specialised"]
        check(lib().mgcm_set_param(m.h, b"no_slip_sides", 0.0), "mgcm_set_param")

    def early(m):
        # the same 4 steps by the generic kernels (bitwise the same state, the tests above), then the move
        m.forward_step(4)
        check(lib().mgcm_set_param(m.h, b"no_slip_sides", 0.0), "mgcm_set_param")

    cfg = _ocean90()
    a, lay_a = _run(cfg, (4,), True, monkeypatch, before=late)
    assert seen["before"] and not lay_a["specialised"], (seen, lay_a)
    b, lay_b = _run(cfg, (4,), False, monkeypatch, before=early)
    assert not lay_b["specialised"], lay_b
    bad = _differences(a, b)
    assert not bad, bad
    # and the moved option was seen: the state differs from 8 steps with no-slip sides
    c, lay_c = _run(cfg, (4, 4), True, monkeypatch)
    assert lay_c["specialised"] and c["uVel"].tobytes() != a["uVel"].tobytes()


@gpu
def test_set_param_after_init_equals_created_with(monkeypatch):
    """The option moved right after mgcm_init, before the first step: 4 steps are those of a model
    created with that value, and neither is specialised."""
    from mitgcm_amd._lib import check, lib

    def move(m):
        check(lib().mgcm_set_param(m.h, b"no_slip_sides", 0.0), "mgcm_set_param")

    a, lay_a = _run(_ocean90(), (4,), True, monkeypatch, before=move)
    b, lay_b = _run(_ocean90(no_slip_sides=0), (4,), True, monkeypatch)
    assert not lay_a["specialised"] and not lay_b["specialised"], (lay_a, lay_b)
    bad = _differences(a, b)
    assert not bad, bad
