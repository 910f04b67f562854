"""The CPU oracle's Stage-I / Dual steps at ``--recon_level`` 1, 2 or 3 (test side; oracle/ itself is not touched).

``O.stage1_step`` / ``O.dual_stage1_step`` call the module-level ``O.discriminator_fwd`` through ``O.vaegan_forward``, and
that function already takes ``recon_level`` (pinned to the reference by
tests/test_oracle_golden.py::test_discriminator_recon_levels_match_reference).  ``at_level`` swaps the module attribute for
a wrapper that passes the level and puts the original back on exit, whatever happens inside.
"""
import contextlib

from oracle import vaegan_oracle as O


@contextlib.contextmanager
def at_level(level: int):
    if level not in (1, 2, 3):
        raise ValueError(f"recon_level={level}: the reference Discriminator works for levels 1, 2, 3 only")
    orig = O.discriminator_fwd

    def discriminator_fwd(*args, **kw):
        kw.setdefault("recon_level", level)
        return orig(*args, **kw)

    O.discriminator_fwd = discriminator_fwd
    try:
        yield
    finally:
        O.discriminator_fwd = orig


def stage1_step_level(level: int, *args, **kw):
    """``O.stage1_step(*args, **kw)`` with the discriminator's feature tensor taken at block ``level``."""
    with at_level(level):
        return O.stage1_step(*args, **kw)


def dual_stage1_step_level(level: int, *args, **kw):
    """``O.dual_stage1_step(*args, **kw)`` with the discriminator's feature tensor taken at block ``level``."""
    with at_level(level):
        return O.dual_stage1_step(*args, **kw)
