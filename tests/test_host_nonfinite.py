"""Drones that are not finite, the part that needs no GPU: the scenes of tests/helpers/nonfinite.py examined on the float64 yardsticks
alone -- are they worth flying on the device (tests/test_gpu_nonfinite.py), and do the conditions hold that its comparisons rely on?
  1. the nine MPPI setups: finite, weights that matter, well conditioned; the poison sits where it is said to sit;
  2. the hard-wall plans: per drone at least a quarter of the samples on either side of FLT_MAX, at most a tenth within a relative
     1e-4 of it, an effective sample size strictly between 1 and the number of finite samples;
  3. the obstacle scenes: a floor in every list, the poison values, nothing else changed;
  4. the guard test's states."""
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))
import mppi_f64 as y  # noqa: E402
import mppi_peers_f64 as yp  # noqa: E402
import nonfinite as nf  # noqa: E402
import obst_task_f64 as yo  # noqa: E402


# ---- 1. the MPPI setups --------------------------------------------------------------------------------------------------------------------
def test_setups_cover_every_entry_and_action_type_at_the_shape_that_was_asked_for():
    seen = {(s.entry, getattr(s.case, "act", "ctbr")) for s in nf.SETUPS}
    assert seen == {("mppi", "rpm"), ("mppi", "vel"), ("ctbr", "ctbr"), ("peers", "rpm"), ("peers", "vel"), ("peers", "ctbr"),
                    ("plant", "rpm"), ("plant", "vel"), ("plant", "ctbr")}
    assert all((s.case.N, s.case.M, s.case.H) == (6, 192, 5) for s in nf.SETUPS)
    assert sorted(nf.POISONED + nf.CLEAN) == list(range(6)) and 3 in nf.POISONED and 4 in nf.POISONED       # 3: beside clean waves; 4: ragged block
    assert not any(getattr(s.case, "flags", 0) & 8 for s in nf.SETUPS) and all(n in nf.SETUP_IDS for n in nf.GROUNDED)
    names = {c.name for mod in nf.YARDSTICK.values() for c in mod.CASES}
    assert not names & set(nf.SETUP_IDS) and not names & set(nf.WALL_IDS), "the existing CASES are left alone"


@pytest.mark.parametrize("name", nf.SETUP_IDS)
def test_clean_launch_is_finite_has_weights_that_matter_and_is_well_conditioned(name):
    """as tests/test_host_mppi.py asks of its device cases: every cost finite, every drone's effective sample size above 1.5 and below
    0.95 M, and a relative error of 1e-6 in every cost moves u_out by less than 1e-5 -- a device result within 1e-4 is then a statement
    about the kernel"""
    setup, inp, ref = nf.clean_plan(name)
    M = setup.case.M
    S, ess = ref["costs"], ref["stats"][:, 2]
    lo, hi = inp.lo.astype(np.float64), inp.hi.astype(np.float64)
    assert np.isfinite(S).all() and (ref["stats"][:, 3] == M).all()
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(4):
        moved, _ = y.update(inp.u_in, ref["a"], S * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, size=S.shape)), inp.lam, lo, hi)
        worst = max(worst, float(y.rel_err(moved, ref["u_out"]).max()))
    print(f"{name}: lambda {inp.lam:.3g} costs {S.min():.3g} .. {S.max():.3g} ess {ess.round(1)} d u_out for 1e-6 of the costs {worst:.2e}")
    assert (ess > 1.5).all() and (ess < 0.95 * M).all(), ess
    assert worst < 1e-5


@pytest.mark.parametrize("name", nf.SETUP_IDS)
def test_poison_sits_in_three_start_states_and_nowhere_else(name):
    setup, inp, _ = nf.clean_plan(name)
    bad = nf.poisoned_inputs(setup, inp)
    assert np.isnan(bad.quat[1, 2]) and bad.vel[3, 0] == np.inf and bad.pos[4, 2] == -np.inf
    state = lambda i: np.concatenate([i.pos, i.quat, i.vel, i.rates], axis=1)       # noqa: E731
    gone = ~np.isfinite(state(bad))
    assert gone.sum() == 3 and sorted(np.flatnonzero(gone.any(axis=1))) == sorted(nf.POISONED) and np.isfinite(state(inp)).all()
    for f in inp._fields:
        if f not in ("pos", "quat", "vel", "table"):
            a, b = getattr(inp, f), getattr(bad, f)
            assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b)), f
    # the nominal of two poisoned drones has a row outside the bounds: clamp(u_in) is not u_in there
    out = ((inp.u_in < inp.lo) | (inp.u_in > inp.hi)).any(axis=-1)                  # [H, N]
    assert out[0, 0] and out[0, 1] and out[-1, 4] and out.sum() == 3
    if setup.entry == "peers":
        k = setup.case.k
        counted = yp.counted(setup.case, inp)
        for n in nf.CLEAN:
            assert not set(inp.idx[n, :].tolist()) & set(nf.POISONED) and len(counted[n]) >= 2, (n, inp.idx[n])
        assert inp.idx[2, 0] == 2 and np.array_equal(inp.idx, bad.idx) and inp.w_peer > 0
        rows = ~np.isfinite(bad.table[..., :3]).all(axis=(0, 2))
        assert set(np.flatnonzero(rows)) >= set(nf.POISONED) and np.array_equal(bad.table[:, list(nf.CLEAN)], inp.table[:, list(nf.CLEAN)], equal_nan=True)
        assert k == 3


# ---- 2. the hard wall ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.WALL_IDS)
def test_wall_splits_every_drones_samples_and_keeps_them_off_the_threshold(name):
    setup, inp, ref = nf.wall_plan(name)
    case = setup.case
    assert (case.N, case.M, case.H, case.S) == (3, 192, 1, 48)
    assert inp.obst.shape == (3, 1, 8) and (inp.obst[:, 0, 3] == yo.FLOOR).all()
    assert inp.weights.w_obs == float(np.float32(3e38)) and inp.weights.obst_margin == 2.0
    S = ref["costs"]
    over, band = nf.wall_classes(S)
    fin = ~over
    share, in_band = over.mean(axis=1), band.mean(axis=1)
    stats = ref["stats"]
    spread = np.array([S[n][fin[n]].max() - S[n][fin[n]].min() for n in range(case.N)])
    print(f"{name}: floors {inp.obst[:, 0, 2]}  overflow share {share.round(3)}  in the band {band.sum(axis=1)} of {case.M}  lambda {inp.lam:.3g}  "
          f"spread of the finite costs {spread}  ess {stats[:, 2].round(2)} of {stats[:, 3]}")
    assert (share >= nf.CLASS_SHARE).all() and (1.0 - share >= nf.CLASS_SHARE).all(), share
    assert (in_band <= nf.BAND_CAP).all(), in_band
    assert (S > 0).all() and np.isfinite(S).all()                    # (float64 holds them all)
    # lambda is of the order of the spread of the finite costs: the weights are neither all equal nor one sample's alone
    assert (0.01 * spread < inp.lam).all() and (inp.lam < spread).all()
    assert (stats[:, 3] == fin.sum(axis=1)).all()
    assert (stats[:, 2] > 1.0).all() and (stats[:, 2] < stats[:, 3]).all(), stats
    assert np.isfinite(stats).all() and np.isfinite(ref["u_out"]).all()
    # a sample that overflowed has no say: the update of the finite samples alone is the same
    for n in range(case.N):
        alone, st = y.update(inp.u_in[:, n:n + 1], ref["a"][n:n + 1, fin[n]], S[n:n + 1, fin[n]], inp.lam, inp.lo.astype(np.float64), inp.hi.astype(np.float64))
        np.testing.assert_allclose(alone[:, 0], ref["u_out"][:, n], atol=1e-13)
        np.testing.assert_allclose(st[0], stats[n], rtol=1e-12)


def test_mean_cost_of_a_wall_plan_needs_more_than_a_plain_float32_sum():
    """why the kernels scale the weighted cost sum: on these plans sum w S of the finite samples exceeds FLT_MAX although every S, and
    their weighted mean, are below it"""
    for name in nf.WALL_IDS:
        _, inp, ref = nf.wall_plan(name)
        S = ref["costs"]
        for n in range(len(S)):
            fin = S[n] <= nf.FLT_MAX
            w = np.exp(-(S[n][fin] - S[n][fin].min()) / inp.lam)
            assert (w * S[n][fin]).sum() > nf.FLT_MAX > ref["stats"][n, 1] > 0.0
            assert (w * S[n][fin]).sum() * 2.0 ** -11 < 0.5 * nf.FLT_MAX


# ---- 3. the obstacle scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nf.OBST_SCENES)
def test_obstacle_scene_has_a_floor_and_the_poison_that_was_asked_for(name):
    case, sc, poison = nf.obst_scene(name)
    _, plain, none = nf.obst_scene(name, poisoned=False)
    base = yo.scene(case)
    assert not none.start and not none.action
    assert np.array_equal(plain.kin, base.kin) and np.array_equal(plain.actions, base.actions) and np.isfinite(plain.kin).all()
    if base.n_obst == 1:
        assert plain.n_obst == 2 and np.array_equal(plain.table[0], base.table[0]) and plain.table[1, 3] == yo.FLOOR
    else:
        assert plain.n_obst == base.n_obst and np.array_equal(plain.table, base.table, equal_nan=True)
    N = case.N
    assert list(poison.start) == [3, 5, 64, N - 1]
    grounded = bool(case.flags & yo.GROUND)
    assert (np.isnan(sc.kin[9, 3]) and poison.start[3] == "vz") if grounded else (sc.kin[2, 3] == -np.inf and poison.start[3] == "pz")
    assert sc.kin[2, 5] == -np.inf and sc.kin[0, 64] == np.inf and np.isnan(sc.kin[4, N - 1])
    assert (~np.isfinite(sc.kin)).sum() == 4
    # z = -inf lies below the floor of its list: without the guard, a clearance of -inf and a contact
    assert len(poison.action) == (2 if case.act == "rpm" else 0)
    gone = ~np.isfinite(sc.actions)
    assert gone.sum() == len(poison.action) and (not poison.action or gone[1].sum() == 2)
    for n, v in poison.action.items():
        assert n not in poison.start and n < N and (np.isnan(sc.actions[1, n]).any() if np.isnan(v) else (sc.actions[1, n] == np.inf).any())
    assert np.array_equal(sc.table, plain.table, equal_nan=True)


def test_obstacle_scenes_are_the_three_that_were_asked_for():
    cases = [nf.obst_case(n) for n in nf.OBST_SCENES]
    assert [(c.N, c.rays, c.act, c.task, c.auto_reset) for c in cases] == [(257, 16, "rpm", "hover", 1), (70, 64, "vel", "none", 0), (257, 0, "rpm", "none", 0)]
    assert cases[1].obst[0] == "lists" and cases[0].obst == ("shared", 65)
    assert [bool(c.flags & yo.GROUND) for c in cases] == [True, True, False]         # z = -inf: caught by the plane / left where it is


# ---- 4. the guard byte's states ------------------------------------------------------------------------------------------------------------
def test_guard_states_poison_the_edges_of_waves_and_workgroups():
    kin, bad = nf.guard_kin()
    assert kin.shape == bad.shape == (13, 300) and kin.dtype == np.float32 and np.isfinite(kin).all()
    gone = ~np.isfinite(bad)
    assert sorted(np.flatnonzero(gone.any(axis=0))) == [0, 63, 64, 150, 255, 256, 299] and gone.sum() == 7
    assert np.array_equal(kin[~gone], bad[~gone])
    rows = {d: r for d, (r, _) in nf.GUARD_POISON.items()}
    groups = {"pos": range(0, 3), "quat": range(3, 7), "vel": range(7, 10), "rates": range(10, 13)}
    hit = {g for g, rr in groups.items() for r in rows.values() if r in rr}
    assert hit == set(groups)
    vals = [v for _, v in nf.GUARD_POISON.values()]
    assert any(np.isnan(v) for v in vals) and np.inf in vals and -np.inf in vals
    # unit quaternions, so that the clean flight is an ordinary one
    assert np.allclose(np.linalg.norm(kin[3:7], axis=0), 1.0, atol=1e-6)
