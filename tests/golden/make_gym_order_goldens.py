#!/usr/bin/env python3
"""Flat vs nested observations of the REAL reference under a key-sorting gym Dict (run in the build container only: needs the
reference):
    python tests/golden/make_gym_order_goldens.py          -> tests/golden/gym_order.npz

The reference builds gym.spaces.Dict(obs_space) from a plain dict (envs/base/base.py:128-163) and flattens observations through it
(:211-223); gym <= 0.26 / gymnasium SORT the keys of such a Dict.  With a Dict that sorts as gym does, DiscreteMicrogridEnv.from_scenario(n)
for n = 0, 1, 2 is reset and stepped 5 times (action k % n_actions, np.random.seed(n)) twice: once with nested observations, once flat.
Stored per scenario n and step k: the flat observation (n{n}_k{k}_flat), each module's nested observation (n{n}_k{k}_<name>), and the
module names (load, pv, genset, battery, grid) the nested observation holds (n{n}_keys, JSON).  Everything stored is what the reference computed."""
import json
import os
import sys
import warnings
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refenv  # noqa: E402

warnings.simplefilter("ignore")
N_SCENARIOS, STEPS = 3, 5
MODULES = ("load", "pv", "genset", "battery", "grid")


class SortingDict(_refenv.Dict):                       # gym/spaces/dict.py: OrderedDict(sorted(spaces.items())) for a plain dict
    def __init__(self, spaces=None, seed=None, **kw):
        super().__init__(spaces, seed, **kw)
        self.spaces = OrderedDict(sorted(self.spaces.items()))


def main():
    _refenv.import_reference()
    import gym
    import pymgrid.envs.base.base as base_mod
    from pymgrid.envs import DiscreteMicrogridEnv
    out = {}
    gym.spaces.Dict = base_mod.Dict = SortingDict
    for n in range(N_SCENARIOS):
        nested_env = DiscreteMicrogridEnv.from_scenario(n)
        nested_env._flat_spaces = False
        flat_env = DiscreteMicrogridEnv.from_scenario(n)
        np.random.seed(n)
        o_n, o_f = nested_env.reset(), flat_env.reset()
        names = [name for name in MODULES if name in o_n]
        out[f"n{n}_keys"] = np.array(json.dumps(names))
        for k in range(STEPS):
            out[f"n{n}_k{k}_flat"] = np.asarray(o_f, dtype=np.float64)
            for name in names:
                out[f"n{n}_k{k}_{name}"] = np.asarray(o_n[name][0], dtype=np.float64)
            a = k % flat_env.action_space.n
            o_n, o_f = nested_env.step(a)[0], flat_env.step(a)[0]
    path = os.path.join(HERE, "gym_order.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays")


if __name__ == "__main__":
    main()
