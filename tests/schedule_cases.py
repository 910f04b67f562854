"""Fed steps with fixed seeds and weights for the GPU tests of the device-side schedule and training log
(tests/test_schedule_gpu.py, tests/test_trainlog_gpu.py).  A pool of 12 images in batches of 4 is three steps per epoch."""
import numpy as np
import torch

DEV = "cuda:0"
NPOOL, BATCH, RNG_SEED, FEED_SEED, V = 12, 4, 7, 11, 37
PER_EPOCH = NPOOL // BATCH
# strong enough that one missed or late epoch end changes every learning rate and the gate's three parameters
DECAYS = dict(lr_gamma=0.5, decay_margin=0.9, decay_equilibrium=0.8, decay_mse=2.0)


def _pool():
    return torch.from_numpy(np.random.RandomState(0).randint(0, 256, (NPOOL, 64, 64, 3), dtype=np.uint8)).to(DEV)


def _fmri():
    return torch.randn(NPOOL, V, generator=torch.Generator().manual_seed(3)).to(DEV)


def _fed(fmri=None):
    from fmri_hip.feed import DeviceDataset, DeviceFeed
    from fmri_hip.rng import DeviceRng
    g = DeviceRng(RNG_SEED, DEV)
    return g, DeviceFeed(DeviceDataset(_pool(), fmri), BATCH, FEED_SEED, rng=g, flip=True, max_shift=2)


def _finish():
    from fmri_hip import ops
    ops.join_side()
    torch.cuda.synchronize()


def _make(kind, schedule=None, **kw):
    """A fed step of ``kind`` with fixed seeds and weights."""
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import CognitiveStep, Stage1Step
    from fmri_hip.wae_steps import DualStage1Step, WaeStep
    cfg = ArchConfig.px64()
    g, feed = _fed(_fmri() if kind == "stage2" else None)
    if kind == "stage1":
        st = Stage1Step(cfg, DEV, rng=g, feed=feed, schedule=schedule, **kw)
        st.load_recipe(0, True)
    elif kind == "stage2":
        st = CognitiveStep(cfg, V, DEV, 2, rng=g, feed=feed, schedule=schedule, **kw)
        st.load_recipe(3, True)
    elif kind == "wae1":
        st = WaeStep(cfg, DEV, 1, rng=g, feed=feed, schedule=schedule, **kw)
        st.load_recipe(5, False)
    else:
        st = DualStage1Step(cfg, DEV, rng=g, feed=feed, schedule=schedule, **kw)
        st.load_recipe(8, True)
    return st


def _base(st, gan=True):
    hp = st.hp
    b = dict(lr=[o.lr for o in st.optims], margin=0.0, equilibrium=0.0, lambda_mse=0.0)
    if gan:
        b.update(margin=hp.margin, equilibrium=hp.equilibrium, lambda_mse=hp.lambda_mse)
    return b
