"""Generate tests/golden/ref_adam.npz by EXECUTING the reference's position learning-rate schedule on the CPU:

  * utils/general_utils.py  get_expon_lr_func

with the reference's defaults (position_lr_init 0.00016, position_lr_final 0.0000016, position_lr_delay_mult 0.01,
position_lr_max_steps 30000, as scene/gaussian_model.py:175-178 passes them: no delay steps) at steps -1, 0, 1, 100, 15000,
30000, 40000; one delayed schedule (lr_delay_steps 1000, lr_delay_mult 0.01, max_steps 5000) at the same steps; and the
both-rates-zero case.  Recorded: the steps, the parameters and the float64 results.

Run where a checkout of the reference is at hand (it never travels with this repository):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_adam.py <reference checkout>

Data only: arrays of numbers produced by the reference's code.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = (-1, 0, 1, 100, 15000, 30000, 40000)
DEFAULT = dict(lr_init=0.00016, lr_final=0.0000016, lr_delay_mult=0.01, max_steps=30000)
DELAYED = dict(lr_init=0.01, lr_final=0.0001, lr_delay_steps=1000, lr_delay_mult=0.01, max_steps=5000)
ZERO = dict(lr_init=0.0, lr_final=0.0, max_steps=30000)


def _params(kw):
    return np.array([kw["lr_init"], kw["lr_final"], kw.get("lr_delay_steps", 0), kw.get("lr_delay_mult", 1.0), kw["max_steps"]], np.float64)


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, sys.argv[1])
    from utils.general_utils import get_expon_lr_func

    out = dict(steps=np.array(STEPS, np.int64))
    for name, kw in (("default", DEFAULT), ("delayed", DELAYED), ("zero", ZERO)):
        fn = get_expon_lr_func(**kw)
        out[name + "_params"] = _params(kw)          # lr_init, lr_final, delay_steps, delay_mult, max_steps
        out[name] = np.array([float(fn(s)) for s in STEPS], np.float64)
    path = os.path.join(HERE, "ref_adam.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
