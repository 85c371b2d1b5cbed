"""pkg/ptracers, host side (no GPU): the age tracer of tutorial_global_oce_latlon as a
parameter list, MONITOR's trcstat block of the cold start against the reference's step-0
monitor, the pickup_ptracers MDS round trip, the field names and the argument errors."""
import json
import os

import numpy as np
import pytest


def test_age_tracer_spec():
    """input/data.ptracers (advScheme 33, diffKh 0, diffKr 3e-5, no initial file) and the
    experiment's code/ptracers_forcing_surf.F (1/(10 days) relaxation to 0 at the surface) and
    code/ptracers_apply_forcing.F (+1 per second below it)."""
    from mitgcm_amd import configs
    specs = configs.global_oce_latlon_ptracers()
    assert len(specs) == 1
    sp = specs[0]
    assert sp["advScheme"] == 33 and sp["diffKh"] == 0.0 and sp["diffKr"] == 3e-5
    assert sp["surfRelaxTau"] == 10.0 * 86400.0 and sp["surfRelaxVal"] == 0.0 and sp["interiorSource"] == 1.0
    assert sp["init"] == 0.0 and "EvPrRn" not in sp and "useGMRedi" not in sp
    # the experiment itself keeps its 4-tuple
    assert len(configs.global_oce_latlon()) == 4


def test_trcstat_of_the_cold_start_is_the_references(golden_dir):
    from mitgcm_amd import configs
    from mitgcm_amd.model import trcstat_fields
    gold = json.load(open(os.path.join(golden_dir, "tutorial_global_oce_latlon", "monitor.json")))[0]
    g = configs.global_oce_latlon()[0]
    st = trcstat_fields(g, [np.zeros((g.nTiles, g.Nr, g.ny, g.nx))])
    keys = ["trcstat_ptracer01_%s" % s for s in ("max", "min", "mean", "sd", "del2")]
    assert sorted(st) == sorted(keys)
    for k in keys:
        assert st[k] == gold[k], (k, st[k], gold[k])
    # ... and the statistics are not blind: a uniform 2.5 has that mean, min and max, no spread
    st = trcstat_fields(g, [np.zeros((g.nTiles, g.Nr, g.ny, g.nx)), np.full((g.nTiles, g.Nr, g.ny, g.nx), 2.5)])
    assert st["trcstat_ptracer02_max"] == 2.5 and st["trcstat_ptracer02_min"] == 2.5
    # (the volume-weighted sums run over at most N = nTiles*Nr*sNy*sNx cells, each addition
    # rounding by at most 2^-53 relative: the mean is within 2.5 * N * 2^-52, and the standard
    # deviation of a uniform field is its distance from that mean)
    bound = 2.5 * g.nTiles * g.Nr * g.sNy * g.sNx * 2.0 ** -52
    assert abs(st["trcstat_ptracer02_mean"] - 2.5) <= bound and st["trcstat_ptracer02_sd"] <= bound
    assert st["trcstat_ptracer02_del2"] == 0.0


def test_pickup_ptracers_round_trip_on_2x2_tiles(tmp_path):
    from mitgcm_amd import configs, pickup
    g = configs.baroclinic_gyre(nSx=2, nSy=2)[0]
    rng = np.random.default_rng(5)
    shape = (g.nTiles, g.Nr, g.ny, g.nx)
    tr = [rng.standard_normal(shape) for _ in range(3)]
    gn = {1: rng.standard_normal(shape), 3: rng.standard_normal(shape)}   # tracers 1 and 3 are Adams-Bashforth ones
    base = pickup.write_pickup_ptracers_fields(g, tr, gn, str(tmp_path), 7, 7 * 1200.0, simulation="gyre")
    assert os.path.basename(base) == "pickup_ptracers.0000000007"
    Nx, Ny = g.sNx * g.nSx, g.sNy * g.nSy
    assert os.path.getsize(base + ".data") == 5 * g.Nr * Ny * Nx * 8
    meta = open(base + ".meta").read()
    assert "nDims = [   3 ]" in meta and "nrecords = [     5 ]" in meta and "'float64'" in meta
    assert "'pTr01   ' 'pTr02   ' 'pTr03   ' 'gPtr01m1' 'gPtr03m1'" in meta
    assert "timeStepNumber = [          7 ]" in meta
    # records: big-endian fp64, level by level, the global (Ny, Nx) array
    raw = np.fromfile(base + ".data", dtype=">f8").reshape(5, g.Nr, Ny, Nx)
    inner = g.sl(1, g.sNx, 1, g.sNy)
    assert raw[1, 4, g.sNy + 2, 3] == tr[1][2, 4][inner][2, 3]           # tile (bi 0, bj 1)
    assert raw[4, 0, 5, g.sNx + 6] == gn[3][1, 0][inner][5, 6]           # tile (bi 1, bj 0)
    tr2, gn2 = pickup.read_pickup_ptracers(g, base)
    assert len(tr2) == 3 and sorted(gn2) == [1, 3]
    sl = (Ellipsis,) + inner
    for a, b in zip(tr, tr2):
        assert np.array_equal(a[sl], b[sl])
        for k in range(g.Nr):   # the halos come back exchanged (PTRACERS_READ_PICKUP's EXCH)
            assert np.array_equal(b[:, k], g.exch(b[:, k].copy()))
    for no in gn:
        assert np.array_equal(gn[no][sl], gn2[no][sl])
    assert pickup.ptracer_is_ab(dict(advScheme=2)) and pickup.ptracer_is_ab(dict(advScheme=4))
    assert not pickup.ptracer_is_ab(dict(advScheme=33)) and pickup.ptracer_is_ab({})


def test_names_and_indices():
    from mitgcm_amd.model import ptracer_index, ptracer_name
    for i in (1, 9, 10, 42, 99):
        assert ptracer_index(ptracer_name(i)) == i
        assert ptracer_index("gpTrNm1_%02d" % i) == i
    assert ptracer_name(7) == "pTracer07"
    for bad in ("pTracer", "pTracer1", "pTracer001", "pTracer00", "pTracerAB", "gpTrNm1_7", "gpTrNm107", "theta", "salt"):
        assert ptracer_index(bad) is None, bad
    for bad in (0, 100, -1):
        with pytest.raises(ValueError):
            ptracer_name(bad)


def test_argument_errors():
    from mitgcm_amd.model import check_ptracer_specs
    with pytest.raises(ValueError, match="outside 1..99"):
        check_ptracer_specs([])
    with pytest.raises(ValueError, match="100 passive tracers outside 1..99"):
        check_ptracer_specs([{}] * 100)
    with pytest.raises(TypeError, match="passive tracer 2"):
        check_ptracer_specs([{}, 33])
    with pytest.raises(ValueError, match="passive tracer 1: unknown parameter.*diffKz"):
        check_ptracer_specs([dict(advScheme=2, diffKz=1.0)])
    assert len(check_ptracer_specs([dict(advScheme=33, diffKr=1e-5, init=0.0, name="x")] * 99)) == 99
