"""What the tests of the launch shapes share (tests/test_gpu_aviary_sizes.py, tests/test_gpu_parity.py, tests/test_gpu_rollout.py): the
tall-column scene of the large-aviary tests, the batch size that makes a size's packing ragged, and the comparison "one rollout of K
steps is K single steps, bit for bit".  Test infrastructure: nothing here touches a device by itself."""
import numpy as np
import torch

STATE = ("kin", "last_rpm", "pid", "step_counter", "obs12", "reward", "terminated", "truncated")


def tall_column(rng, E, D, z0=0.5):
    """(xyz, rpy) [E, D, 3]: a tall, slightly tilted column -- 0.3 m vertical spacing (away from the dz -> 0+ and dz = 0.6875 m
    singularities of the downwash model for the nearest neighbours), lateral jitter, small attitudes.  Its top: `column_top(D)`."""
    xyz = rng.uniform(-0.02, 0.02, size=(E, D, 3)) + np.arange(D)[None, :, None] * np.array([0.013, 0.007, 0.3]) + \
        np.array([0, 0, z0])
    rpy = rng.uniform(-0.05, 0.05, size=(E, D, 3))
    return xyz, rpy


def column_top(D, z0=0.5):
    """a height no drone of `tall_column` reaches within a few steps (a z_bound above the column)"""
    return z0 + 0.3 * D + 1.0


def ragged_envs(D):
    """The smallest number of aviaries of D drones that gives at least two workgroups and a ragged last one in both packings: a
    workgroup holds 256 // D aviaries in gpd_step_kernel and gpd_rollout_kernel, and 4 (64 // D) -- whole aviaries per wave -- in
    gpd_rollout1_kernel (D <= 64).  33 drones: 7 and 4 per workgroup, 9 aviaries; 64: 5; 86: 3."""
    per = [256 // D] + ([4 * (64 // D)] if D <= 64 else [])
    E = max(per) + 1
    while any(E % p == 0 for p in per):
        E += 1
    return E


def rollout_equals_steps(a, b, acts, keep_term):
    """`a` takes the K blocks of `acts` as K single steps, its twin `b` as one rollout: observation rows, reward and flags of every
    step, the state afterwards (`STATE`) and -- `keep_term` -- the terminal observations must have equal bits.  Returns the stacked
    (terminated, truncated) [K, E] of the single steps."""
    K, D = acts.shape[0], a.D
    obs_s, rew_s, te_s, tr_s, tobs_s = [], [], [], [], []
    for k in range(K):
        o, r, te, tr = a.step(acts[k])
        obs_s.append(o.clone()); rew_s.append(r.clone()); te_s.append(te.clone()); tr_s.append(tr.clone())
        if keep_term:
            tobs_s.append(a.term_obs12.clone())
    obs, rew, te, tr = b.rollout(acts)
    te_s, tr_s = torch.stack(te_s), torch.stack(tr_s)
    assert torch.equal(torch.stack(obs_s), obs)
    assert torch.equal(torch.stack(rew_s), rew)
    assert torch.equal(te_s, te) and torch.equal(tr_s, tr)
    for name in STATE:
        x, y = getattr(a, name), getattr(b, name)
        if x is not None:
            assert torch.equal(x, y), name
    if keep_term:
        # terminal observations: rollout row t holds the rows written at step t; the single-step buffer accumulates
        tob = b._rollout_buf[4]
        done = te_s | tr_s                                                                 # [K, E]
        for k in range(K):
            m = done[k].repeat_interleave(D)
            assert torch.equal(tob[k][m], tobs_s[k][m])
        # ... and the persistent term_obs12 afterwards is what the K single steps left (the plain rollout did not update it)
        if a.auto_reset:
            assert torch.equal(a.term_obs12, b.term_obs12)
    return te_s, tr_s
