#!/usr/bin/env python3
"""Generate tests/golden/adjacency_ctrl24.npz by running the REFERENCE'S OWN `_getAdjacencyMatrix`.

Run in the build container only (needs the reference, see make_golden.py):  python tests/golden/make_golden_adjacency.py

The reference's unmodified `CtrlAviary(num_drones=24, neighbourhood_radius=0.8, physics=DYN)` flies 60 control steps of
seeded random RPMs around hover from a seeded random cloud; at a handful of steps the positions (`env.pos`, float64) and
`env._getAdjacencyMatrix()` (`envs/BaseAviary.py:658-675`) are stored.  The cloud is chosen so that every stored matrix has
zeros as well as off-diagonal ones, and so that no pair is within 1e-4 m of the radius (a float32 restatement of the test then
decides every pair the same way); both are asserted here.
"""
import os

import numpy as np

from make_golden import HERE, _silence, load_reference

NUM_DRONES, RADIUS, STEPS, KEEP = 24, 0.8, 60, (0, 1, 15, 30, 45, 60)
SEED = 7


def main():
    _, ref = load_reference()
    E = ref["enums"]
    rng = np.random.default_rng(SEED)
    # a cloud a few radii wide: most drones see some of the others, none sees all
    init_xyzs = np.concatenate([rng.uniform(-1.2, 1.2, size=(NUM_DRONES, 2)), rng.uniform(0.6, 1.8, size=(NUM_DRONES, 1))], axis=1)
    with _silence():
        env = ref["CtrlAviary"](drone_model=E.DroneModel.CF2X, num_drones=NUM_DRONES, neighbourhood_radius=RADIUS,
                                initial_xyzs=init_xyzs, physics=E.Physics.DYN, pyb_freq=240, ctrl_freq=48)
        env.reset(seed=0)
    rpms = env.HOVER_RPM * (1.0 + 0.08 * rng.uniform(-1, 1, size=(STEPS, NUM_DRONES, 4)))
    pos, adj, steps = [], [], []

    def keep(step):
        p = np.array(env.pos, dtype=np.float64)
        a = np.array(env._getAdjacencyMatrix(), dtype=np.float64)
        d = np.linalg.norm(p[:, None, :] - p[None, :, :], axis=-1)
        off = ~np.eye(NUM_DRONES, dtype=bool)
        assert (a[off] == 0).any() and (a[off] == 1).any(), f"step {step}: the matrix is trivial"
        assert np.abs(d[off] - RADIUS).min() > 1e-4, f"step {step}: a pair within 1e-4 m of the radius"
        pos.append(p), adj.append(a), steps.append(step)

    if 0 in KEEP:
        keep(0)
    for s in range(1, STEPS + 1):
        env.step(rpms[s - 1])
        if s in KEEP:
            keep(s)
    out = os.path.join(HERE, "adjacency_ctrl24.npz")
    np.savez_compressed(out, pos=np.array(pos), adjacency=np.array(adj).astype(np.uint8), steps=np.array(steps, dtype=np.int64),
                        radius=np.float64(RADIUS), init_xyzs=init_xyzs, seed=np.int64(SEED))
    print(f"wrote {out}: {len(steps)} snapshots, {os.path.getsize(out)} bytes, "
          f"neighbours per drone {np.array(adj).sum(axis=2).mean() - 1:.2f}")


if __name__ == "__main__":
    main()
