"""The reference's epoch-end block written out in Python floats (train/train_vgan_stage1.py:447-458; torch's StepLR in
its chainable form for the learning rate) -- what the tests of the device-side EpochSchedule compare against.  Doubles
throughout; ``f32`` is the single rounding the engine applies when it hands a value to a kernel."""
import numpy as np


def epoch_end(v, new_epoch, lr_gamma=1.0, lr_step=1, decay_margin=1.0, decay_equilibrium=1.0, decay_mse=1.0):
    """One pass of the block on ``v`` = dict(lr=[...], margin, equilibrium, lambda_mse); ``new_epoch``: the index of the
    epoch that starts (``lr_scheduler.step()`` multiplies when it is a multiple of step_size)."""
    lr, margin, equilibrium, lambda_mse = list(v["lr"]), v["margin"], v["equilibrium"], v["lambda_mse"]
    if new_epoch % lr_step == 0:
        lr = [x * lr_gamma for x in lr]
    margin *= decay_margin
    equilibrium *= decay_equilibrium
    if margin > equilibrium:
        equilibrium = margin
    lambda_mse *= decay_mse
    if lambda_mse > 1:
        lambda_mse = 1
    return dict(lr=lr, margin=margin, equilibrium=equilibrium, lambda_mse=lambda_mse)


def at(base, epoch, **decays):
    """``epoch`` passes from the base values."""
    v = dict(base, lr=list(base["lr"]))
    for e in range(1, epoch + 1):
        v = epoch_end(v, e, **decays)
    return v


def f32(x):
    return np.float32(x)


GAN_BASE = dict(lr=[1e-4] * 3, margin=0.35, equilibrium=0.68, lambda_mse=1e-6)      # configs/gan_config.py:18-31
STAGE1_DECAYS = dict(lr_gamma=0.98, decay_margin=1.0, decay_equilibrium=1.0, decay_mse=1.0)
