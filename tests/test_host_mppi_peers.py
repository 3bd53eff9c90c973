"""MPPI with the peers' paths in the cost, the part that needs no GPU: the conditions the device cases have to meet, checked on the float64
yardstick alone (tests/helpers/mppi_peers_f64.py); the binding; the `SwarmMPPI` class's own refusals; and the host side of
`gpd_mppi_peers` against the launch stub under ASan + UBSan (tests/c/mppi_peers_host.c), which also evaluates csrc/mppi_peers_math.inc
at its corner values.  The sanitizers run in the stand-alone program only, never in this process."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_peers_f64 as yp  # noqa: E402

IDS = [c.name for c in yp.CASES]


# ---- the device cases on the yardstick --------------------------------------------------------------------------------------------------
def test_cases_cover_the_paths_of_the_kernel():
    """a lone wave with intruder rows, a full block and a block of one wave, three blocks; one sample per lane and the sample loop; one
    step and five; one sub-step and five; k = 1, 3, 32 with idx_ld = k + 2; one row set and a padded step stride; the three models; no
    list and a shared one; the three airframes; -1 in the middle of a row, a drone's own row, an entry beyond the table, a drone without
    peers, a NaN row that some drone's list names"""
    C = yp.CASES
    for field, values in (("N", {1, 5, 9}), ("M", {64, 128}), ("H", {1, 5}), ("S", {1, 5}), ("k", {1, 3, 32}), ("stride0", {False, True}),
                          ("act", {"rpm", "vel", "ctbr"}), ("obst", {"none", "shared"}), ("model", {"cf2x", "cf2p", "racer"})):
        assert {getattr(c, field) for c in C} == values, field
    assert len({c.name for c in C}) == len(C) and 8 <= len(C) <= 12
    assert all(c.extra == 3 for c in C if c.N == 1) and any(c.extra > 0 for c in C if c.N > 1)
    seen = features_of_the_lists()
    assert seen == {"minus-one-in-the-middle", "own-row", "beyond-the-table", "no-peers", "nan-row", "beyond-k-is-a-close-row"}, seen


def features_of_the_lists():
    seen = set()
    for c in yp.CASES:
        inp = yp.make_inputs(c)
        n_rows = inp.table.shape[1]
        assert inp.idx.shape == (c.N, c.k + 2) and inp.idx.dtype == np.int32 and inp.table.shape[0] == (1 if c.stride0 else c.H)
        for n in range(c.N):
            row = inp.idx[n, :c.k]
            live = np.flatnonzero(row >= 0)
            if len(live) and (row[:live[-1]] < 0).any():
                seen.add("minus-one-in-the-middle")
            if (row == n).any():
                seen.add("own-row")
            if (row >= n_rows).any():
                seen.add("beyond-the-table")
            if (row < 0).all():
                seen.add("no-peers")
            if any(np.isnan(inp.table[:, r]).all() for r in row if 0 <= r < n_rows):
                seen.add("nan-row")
            if c.k < n_rows - 1 and all(0 <= r < n_rows and r != n for r in inp.idx[n, c.k:]):
                seen.add("beyond-k-is-a-close-row")
    return seen


@functools.lru_cache(maxsize=None)
def planned(name):
    case = next(c for c in yp.CASES if c.name == name)
    inp = yp.make_inputs(case)
    return inp, yp.plan(case, inp)


@pytest.mark.parametrize("case", yp.CASES, ids=IDS)
def test_peer_term_acts_on_every_device_case(case):
    """A condition on the INPUTS, on the yardstick alone: in every case with a counted peer the peer term is > 0 for at least a quarter
    of the samples of at least one drone -- otherwise the device comparison could pass with the term never exercised.  Also: finite
    costs, every sample counted, an effective sample size above 1.5 for every drone (no plan hangs on one sample), and a drone
    without counted peers pays nothing and has no nearest peer"""
    inp, ref = planned(case.name)
    cnt = yp.counted(case, inp)
    assert any(cnt), "no counted peer at all"
    share = (ref["peer"] > 0.0).mean(axis=1)
    print(f"{case.name}: counted {[len(c) for c in cnt]} share of samples with a peer term {share.round(2)} largest {ref['peer'].max():.3g} "
          f"of costs {ref['costs'].min():.3g} .. {ref['costs'].max():.3g} ess {ref['stats'][:, 2].round(1)}")
    assert share.max() >= 0.25
    assert np.isfinite(ref["costs"]).all() and (ref["stats"][:, 3] == case.M).all() and (ref["stats"][:, 2] > 1.5).all()
    for n, c in enumerate(cnt):
        if not c:
            assert (ref["peer"][n] == 0.0).all() and np.isinf(ref["path"][:, n, 3]).all()
    assert np.isfinite(ref["path"][..., :3]).all()


def test_yardstick_without_peers_is_the_models_own_yardstick():
    """with the peer term off the restated rollout gives the costs of mppi_f64 / mppi_ctbr_f64 (the same oracle, the same order of
    operations: equal, not close), for one case of each model"""
    import mppi_ctbr_f64 as yc
    import mppi_f64 as y
    for case in (yp.CASES[0], yp.CASES[1], yp.CASES[5]):          # (RPM and VEL on cf2x, the airframe mppi_f64.plan flies; CTBR on cf2p)
        inp = yp.make_inputs(case)
        mine = yp.plan(case, inp, peers=False)
        b = yp.base_case(case)
        own = yc.plan(b, yc.make_inputs(b)) if case.act == "ctbr" else y.plan(b, y.make_inputs(b))
        np.testing.assert_allclose(mine["costs"], own["costs"], rtol=1e-13)
        np.testing.assert_allclose(mine["u_out"], own["u_out"], rtol=0, atol=1e-13)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_and_pins_nothing_else():
    from gym_pybullet_drones_amd import _native
    L = _native.lib()
    res, args = _native._SIGNATURES["gpd_mppi_peers"]
    assert "gpd_mppi_peers" in _native.exported_symbols() and L.gpd_mppi_peers.argtypes == args and len(args) == 17 and res is ctypes.c_int
    assert args[:6] == [ctypes.POINTER(t) for t in (_native.GpdParams, _native.GpdCtbr, _native.GpdState, _native.GpdStepCfg, _native.GpdMppi,
                                                    _native.GpdMppiPeers)]
    assert L.gpd_abi_version() == 9 and _native.ABI_VERSION == 9 and len(_native.UNITS) == 5
    assert ctypes.sizeof(_native.GpdMppi) == 104
    for name in ("mppi_peers_math.inc", "mppi_peers.inc"):
        assert name in _native.HEADERS and os.path.exists(os.path.join(_native.CSRC, name))
    abi = open(os.path.join(_native.CSRC, "abi.hip")).read()
    assert abi.index('#include "mppi_ctbr.inc"') < abi.index('#include "mppi_peers.inc"')
    hdr = open(os.path.join(_native.INCLUDE, "gpd.h")).read()
    assert "} GpdMppiPeers;" in hdr and re.search(r"^int gpd_mppi_peers\(const GpdParams\* params, const struct GpdCtbr\* ctbr", hdr, flags=re.M)


def test_python_class_rejects_what_the_entry_would_before_any_device_work():
    from gym_pybullet_drones_amd import mppi

    class Core:
        D, act_code, N, device = 2, 2, 4, "cpu"

    class Ctrl:
        n, device, thrust_max, rate_max = 4, "cpu", 40.9, 6.28
    with pytest.raises(ValueError, match="one drone"):
        mppi.SwarmMPPI(Core(), 5, 64, 1.0, 1.0)
    Core.D = 1
    for act in (1, 3, 4, 5, 6):
        Core.act_code = act
        with pytest.raises(ValueError, match="RPM or VEL"):
            mppi.SwarmMPPI(Core(), 5, 64, 1.0, 1.0)
    for act in (0, 1, 2, 3, 4):
        Core.act_code = act
        with pytest.raises(ValueError, match="RAW_RPM or DIRECT_RPM"):
            mppi.SwarmMPPI(Core(), 5, 64, 1.0, 1.0, ctrl=Ctrl())
    Core.act_code = 5
    for other in (type("Other", (Ctrl,), dict(n=3))(), object()):
        with pytest.raises(ValueError, match="VectorCTBR of 4 controllers"):
            mppi.SwarmMPPI(Core(), 5, 64, 1.0, 1.0, ctrl=other)
    assert issubclass(mppi.SwarmMPPI, mppi._Planner) and mppi.SwarmMPPI._ENTRY == "gpd_mppi_peers"
    assert mppi.SwarmMPPI.nominal is mppi.MPPI.nominal                  # shared, not copied
    from gym_pybullet_drones_amd.envs.VectorAviary import VectorAviary
    assert callable(VectorAviary.mppi_swarm)


# ---- the host side of the entry, and the arithmetic ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_run():
    import host_lib
    from gym_pybullet_drones_amd import _native
    return host_lib.run(host_lib.program("mppi_peers_host", include=(_native.CSRC,)))


def test_host_side_of_the_entry_under_asan_and_ubsan():
    """tests/c/mppi_peers_host.c linked to the host-only build of the units and the launch stub under -fsanitize=address,undefined: a good
    call launches the instantiation model x list that the arguments select, every refusal has its code, the entry's name and the reason,
    and launches nothing; sizeof(GpdMppiPeers) is the ctypes mirror's"""
    from gym_pybullet_drones_amd import _native
    run = host_run()
    print(run.stdout[-8000:])
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert run.returncode == 0 and "\n0 checks failed" in run.stdout, run.stdout[-3000:] + run.stderr[-2000:]
    assert run.stdout.count("\nok ") >= 100 and "FAIL" not in run.stdout
    for piece in ("<VEL, OBST>", "<VEL, no OBST>", "<RPM, OBST>", "<RPM, no OBST>", "<CTBR, OBST>", "<CTBR, no OBST>"):
        assert f"{piece}\n" in run.stdout, piece
    assert int(re.search(r"sizeof GpdMppiPeers (\d+)", run.stdout).group(1)) == ctypes.sizeof(_native.GpdMppiPeers) == 56


def test_peer_hinge_of_the_kernels_text_against_the_yardstick_at_its_corners():
    """csrc/mppi_peers_math.inc, compiled by the host program, against the yardstick's float64 hinge at d = 0, d = peer_dist and either
    side of it, NaN and infinite offsets, squares that overflow: within 1e-6 (fp32 rounding of a value of order one; exact where the
    yardstick gives 0 for a row that is not finite), d = 0 gives peer_dist^2, and the nearest distance never counts a NaN"""
    lines = re.findall(r"^pen (\S+) (\S+) (\S+) (\S+) -> (\S+) (\S+) (\S+)$", host_run().stdout, flags=re.M)
    assert len(lines) >= 14
    kinds = set()
    for line in lines:
        pd, dx, dy, dz, pen, d, near = (float.fromhex(v) if "0x" in v else float(v) for v in line)
        with np.errstate(invalid="ignore", over="ignore"):
            d64 = float(np.sqrt(np.float64(dx) ** 2 + np.float64(dy) ** 2 + np.float64(dz) ** 2))
        want = yp.hinge(pd, np.float64(d64))
        assert np.isfinite(pen) and abs(pen - want) <= 1e-6 * max(1.0, abs(want)), line
        if not np.isfinite(d64) or d64 > 1e19:          # (beyond 1e19 the fp32 squares overflow: the distance is +inf there)
            assert pen == 0.0 and near == 1.0 and not d < 1.0, line
            kinds.add("nan" if np.isnan(d64) else "inf")
            assert np.isnan(d) if np.isnan(d64) else d == np.inf, line
        else:
            assert abs(d - d64) <= 1e-6 * max(1.0, d64) and near == min(d, 1.0), line
            kinds.add("zero" if d64 == 0.0 else "edge" if abs(d64 - pd) < 1e-4 else "inside" if d64 < pd else "outside")
            if d64 == 0.0:
                assert pen == np.float32(pd) * np.float32(pd)
    assert kinds == {"nan", "inf", "zero", "edge", "inside", "outside"}, kinds
