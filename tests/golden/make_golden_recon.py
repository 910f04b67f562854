#!/usr/bin/env python3
"""Golden fixtures of the Stage-I / Dual steps at ``--recon_level`` 1 and 2, by RUNNING THE REAL REFERENCE.

    python tests/golden/make_golden_recon.py [--f64] [case ...]

Same procedure, same summary format as make_golden.py (whose helpers and step bodies this imports, unchanged): the
reference's ``VaeGan(device, z_size, recon_level=level)`` (models/vae_gan.py:240-247; the scripts pass the option at
train_vgan_stage1.py:62,237 and wae_vgan_stage1.py:71,199), the literal three ``backward()`` calls at the pre-update
weights, real ``torch.optim`` steps; logged losses, gate flags, ``tensor_summary`` rows of every gradient / forward
output / post-step state entry (``num_batches_tracked`` among them).  Needs the reference tree of make_golden.py.

Cases: stage1_rl1_b4, stage1_rl2_b4, stage1_rl2_betavae_b4, dual1_rl2_b4 (and, with --f64, their _f64 twins).
Fixtures are data only (numbers); no reference source is stored.
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as M  # noqa: E402
from make_golden import O  # noqa: E402


@contextlib.contextmanager
def reference_at_level(level: int):
    """Inside the block, the ``VaeGan`` of the module ``make_golden.load_reference`` returns is built with
    ``recon_level=level`` wherever the case bodies of make_golden.py construct one."""
    load = M.load_reference

    def load_leveled(cfg):
        vg = load(cfg)

        class VaeGanAtLevel(vg.VaeGan):
            def __init__(self, *args, **kw):
                kw.setdefault("recon_level", level)
                super().__init__(*args, **kw)

        # a view of the module with that one name replaced (the module's own code keeps seeing its own class)
        view = types.SimpleNamespace(**{k: v for k, v in vars(vg).items() if not k.startswith("__")})
        view.VaeGan = VaeGanAtLevel
        return view

    M.load_reference = load_leveled
    try:
        yield
    finally:
        M.load_reference = load


CASES = {
    "stage1_rl1_b4": lambda n: M.case_stage1(n, O.ArchCfg.px64(), B=4, seed=0, perturb=True),
    "stage1_rl2_b4": lambda n: M.case_stage1(n, O.ArchCfg.px64(), B=4, seed=0, perturb=True),
    "stage1_rl2_betavae_b4": lambda n: M.case_stage1(n, O.ArchCfg.px64(), B=4, seed=0, perturb=True, mode="beta-vae",
                                                     beta=4.0),
    "dual1_rl2_b4": lambda n: M.case_dual1(n, O.ArchCfg.px64(), B=4, seed=8, perturb=True),
}
LEVELS = {"stage1_rl1_b4": 1, "stage1_rl2_b4": 2, "stage1_rl2_betavae_b4": 2, "dual1_rl2_b4": 2}


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = [a for a in sys.argv[1:] if not a.startswith("--")] or list(CASES)
    if "--f64" in sys.argv[1:]:
        # as make_golden.py --f64: modules, recipe weights and inputs in double precision, written as <case>_f64.npz
        torch.set_default_dtype(torch.float64)
        _fill, _synth = O.fill_state, O.synth_batch
        dbl = lambda d: {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
        O.fill_state = lambda *a, **k: dbl(_fill(*a, **k))
        O.synth_batch = lambda *a, **k: dbl(_synth(*a, **k))
        _savez = np.savez_compressed

        def savez_f64(path, **out):
            assert path.endswith(".npz")
            return _savez(path[:-4] + "_f64.npz", **out)
        np.savez_compressed = savez_f64
    for name in which:
        with reference_at_level(LEVELS[name]):
            CASES[name](name)
        # the level is a property of the case: keep it next to the data
        suffix = "_f64.npz" if "--f64" in sys.argv[1:] else ".npz"
        path = os.path.join(HERE, name + suffix)
        with np.load(path, allow_pickle=False) as z:
            out = {k: z[k] for k in z.files}
        out["meta/recon_level"] = np.int64(LEVELS[name])
        (_savez if "--f64" in sys.argv[1:] else np.savez_compressed)(path, **out)
