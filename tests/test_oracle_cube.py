"""Cubed-sphere path (pkg/exch2 + MOM_VECINV) pinned against the reference's committed
output of verification/solid-body.cs-32x32x1 (6 faces of 32x32, one tile each):
  - mitgcm_amd/exch2.py maps: every halo value comes from an interior point (so the
    device gather can run in place), all four exchange kinds; on tiles as wide as the halo
    the C-grid vector maps alone also copy halo points, never in a chain;
  - the host grid (INI_CURVILINEAR_GRID + EXCH2 Z/B/A/C-grid exchanges + CALC_GRID_ANGLES)
    against the grid statistics output.txt prints at start-up;
  - the oracle (MOM_VECINV, EXCH2 vector exchanges, CG2D on the cube, C2 salt advection)
    against the per-step %MON / cg2d lines."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import digits

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


# (n, sNx, sNy, OL); from (32, 16, 8, 4) on: faces divided in x as well (interior, one-edge
# and corner tiles, the tilings of test_gpu_shapes_cube.py), tiles as narrow as the halo
MAP_CASES = [(32, 32, 32, 2), (32, 32, 32, 4), (32, 32, 16, 4), (32, 16, 16, 3), (32, 16, 8, 4), (32, 8, 8, 4),
             (32, 8, 32, 4), (32, 4, 32, 4), (12, 4, 6, 4), (9, 3, 3, 3), (10, 5, 2, 2)]


@pytest.mark.parametrize("n,sN,sNy,OL", MAP_CASES,
                         ids=["%d-%d-%d" % c[1:] if c[0] == 32 else "n%d-%d-%d-%d" % c for c in MAP_CASES])
def test_exch2_maps_source_interior(n, sN, sNy, OL):
    from mitgcm_amd.exch2 import cube_topology
    T = cube_topology(n, sN, sNy, OL)
    N = T.nTiles * T.n2
    ar = np.arange(N)
    interior = np.array([T.is_interior(q) for q in range(N)])
    for name, ids, base in (("T", T.scalar_ids(), 0), ("Z", T.z_ids(), 0),
                            ("u", T.uv_ids(True)[0], 0), ("v", T.uv_ids(True)[2], N),
                            ("uA", T.agrid_ids(True)[0], 0), ("vB", T.bgrid_ids(False)[2], N)):
        changed = ids != ar + base
        assert not changed[interior].any(), name          # interiors are never written
        src = ids[changed] % N
        if name not in ("u", "v") or min(sN, sNy) > OL:
            assert interior[src].all(), name               # halos only copy interior points
    # The C-grid vector maps on tiles exactly as wide as the halo: the reference's second
    # EXCH2_RX2_CUBE pass copies, into a few corner-halo points, a halo value that only that
    # same pass fills -- its value from before the exchange.  Such a source is itself filled
    # from an interior point (no chains), so the device applies these entries in one launch
    # ahead of the others (csrc/model.hip uvPre) and the oracle gathers from a copy.
    u, _, v, _ = T.uv_ids(True)
    full = np.concatenate([u, v])
    written = full != np.arange(2 * N)
    early = written & written[full]
    assert early.any() == (min(sN, sNy) <= OL)
    assert not written[full[full[early]]].any()
    # every halo point of the scalar exchange is filled on a cube (corner halos included)
    assert (T.scalar_ids()[~interior] != ar[~interior]).all()


def test_exch2_vector_signs_are_rotations():
    """Across a rotated edge a C-grid u halo comes from +-v of the neighbour (and back)."""
    from mitgcm_amd.exch2 import cube_topology
    T = cube_topology(32, 32, 32, 2)
    N = T.nTiles * T.n2
    u, us, v, vs = T.uv_ids(True)
    cu, cv = T.uv_codes(True)
    from_v = (u >= N) & (u != np.arange(N))
    assert from_v.any() and (np.abs(cu[from_v]) - 1 >= N).all()
    assert set(np.unique(us)) <= {-1, 1} and (us == -1).any()


def test_solid_body_grid_matches_reference(golden_dir):
    from mitgcm_amd import configs
    from test_grid_sphere import mon_stats_rs
    g, params, state = configs.solid_body_cs32()
    gold = json.load(open(os.path.join(golden_dir, "solid-body.cs-32x32x1", "grid_monitor.json")))
    names = {"XC": "xC", "XG": "xG", "DXC": "dxC", "DXF": "dxF", "DXG": "dxG", "DXV": "dxV", "YC": "yC",
             "YG": "yG", "DYC": "dyC", "DYF": "dyF", "DYG": "dyG", "DYU": "dyU", "RA": "rA", "RAW": "rAw",
             "RAS": "rAs", "RAZ": "rAz", "AngleCS": "angleCosC", "AngleSN": "angleSinC", "fCori": "fCori",
             "fCoriG": "fCoriG", "fCoriCos": "fCoriCos"}
    worst = (99.0, None)
    for mon, f in names.items():
        st = mon_stats_rs(g, g.f[f])
        for k in ("max", "min", "mean", "sd"):
            d = digits(st[k], gold["%s_%s" % (mon, k)])
            if d < worst[0]:
                worst = (d, (mon, k))
    assert worst[0] >= 13.3, worst


def test_solid_body_oracle_matches_reference_output(golden_dir):
    from mitgcm_amd import configs
    from oracle.harness import oracle_from_config
    gold = json.load(open(os.path.join(golden_dir, "solid-body.cs-32x32x1", "monitor.json")))
    o, g = oracle_from_config(configs.solid_body_cs32)
    worst = (99.0, None)
    for n in range(1, 11):
        o.forward_step()
        r = o.dynstat()
        gs = gold[n]
        assert r["cg2d_iters"] == gs["cg2d_iters"], n
        for k, v in r.items():
            if k in gs and k != "cg2d_iters" and not k.startswith("dynstat_theta"):
                d = digits(v, gs[k])
                if d < worst[0]:
                    worst = (d, (n, k, v, gs[k]))
    # 14 printed digits; theta is the constant 300 K (its sd is round-off)
    assert worst[0] >= 13.0, worst
