"""On-device validation pass of the fused steps (csrc/evalmetrics.hip; include/fmri_hip.h fmri_image_metrics).

The block of the scripts' epoch that a fused step could not run: the epoch-end metrics (train/train_vgan_stage1.py:487-520
and its copies) and ``evaluate()`` over a whole validation set (train/train_utils.py:678-749, without the Inception score
and the image dumps).  The eval-mode forward of the step's OWN networks -- BatchNorm from running statistics, applied in
the conv epilogues -- goes straight into one metrics kernel pair per batch, and a pass leaves one row in a device ring:

    ev = Evaluator(step, DeviceDataset(val_images_u8, val_fmri), batch=64, rng=DeviceRng(seed_eval, dev))
    for epoch in range(epochs):
        for _ in range(steps_per_epoch):
            replay()
        ev.train_batch()                # PCC / SSIM / MSE of the last training batch (train-mode x_tilde)
        ev.run()                        # the whole validation set in eval mode, one row
    h = ev.history()                    # ONE sync

The forward per step class follows models/vae_gan.py: ``Stage1Step`` / ``DualStage1Step`` decoder(mu + eps * exp(logvar / 2))
of encoder(x) (``VaeGan.forward`` reparameterises in eval mode too); ``CognitiveStep`` the same from
cognitive_encoder(fmri), against the dataset image; ``WaeStep`` decoder(encoder(x).mu) in Stage I and
decoder(cognitive_encoder(fmri).mu) in Stages II / III (no noise).

Columns of a row: ``epoch`` (of the step's training feed, read on the device; only with a feed), ``batches``,
``valid_PCC / valid_SSIM / valid_MSE`` (the LAST batch: what the scripts' epoch-end block leaves in
``result_metrics_valid``, overwritten per batch), ``mean_PCC / mean_SSIM / mean_MSE`` (the mean over the batches, every
batch weighted equally: what ``evaluate()`` returns) and ``train_PCC / train_SSIM / train_MSE`` (the last
``train_batch()`` since the previous row, NaN without one).

``identify=top`` adds n-way identification (the ``objective_assessment`` the scripts call beside ``evaluate()``,
train/train_utils.py:752-816; csrc/nway.hip, include/fmri_hip.h fmri_nway_scores): every batch's reconstructions against
the batch's ingested images -- always the normalised tensors, whatever ``denorm`` is -- with the ``top - 1`` distractors
of every image drawn on the device.  Columns ``nway_PCC / nway_SSIM`` (hits over images: ``tp / dataset_size``, weighted
by images, unlike ``mean_*``) and ``nway_exp_PCC / nway_exp_SSIM`` (the same score's expectation over the draws: no
sampling noise).  The draws are uniform over the batch's other images with replacement, as the reference's
``random.choice``, but not the host's draws.  They are made at the evaluator's generator offset on stream SID_DISTRACT
before the batch's advance, which stays ``blocks(b * latent_dim)`` where the forward samples -- ``eps``, and with it every
other column, has the same bits with and without ``identify`` -- and is ``blocks(b * (top - 1))`` where it does not and an
``rng`` was given.  Without an ``rng`` the two sampled columns are NaN.

``grids=`` / ``dump=`` / ``generate=`` add the pictures of the scripts' epoch (fmri_hip/egress.py, csrc/egress.hip): the
``make_grid`` of the training batch, its reconstruction, the validation output and ``model(None, g)`` into a device ring
whose slot follows this evaluator's pass counter, and ``evaluate(save=True)``'s per-image uint8 dumps.  The draw of
``generate`` is stream SID_GENERATE at the generator's offset at the end of the pass and moves nothing: every column
keeps its bits.

A pass leaves training where it was: ``bn.eval_mode`` is set for the pass and restored, no running statistic and no
``num_batches_tracked`` moves, nothing the step owns is written or re-bound (latent range scratch, noise, batch buffers and
the generator are the evaluator's own), and a step recorded with ``capture()`` before or after replays unchanged.  The pass
sees the weights and statistics of the last step, replayed ones included: the fp16 GEMM copies follow the groups' version
counters, and ``dec.fc_bn`` keeps its LIVE running statistics in engine order (ops.BatchNorm.enable_lazy_running), which is
what its eval-mode forward reads -- nothing has to be flushed.

Nothing here synchronises with the host except ``history()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import lib, ops
from .feed import DeviceDataset
from .ops import nhwc_to_images, pad8
from .rng import SID_DISTRACT, SID_EPS, SID_GENERATE, DeviceRng, blocks
from .schedule import TrainLog

_P = lib.ptr

METRICS = ("PCC", "SSIM", "MSE")
NWAY = ("nway_PCC", "nway_SSIM", "nway_exp_PCC", "nway_exp_SSIM")


def batch_ranges(n: int, batch: int) -> List[Tuple[int, int]]:
    """(first row, rows) of the batches of a pass over ``n`` dataset rows: in order, no drop-last -- the scripts'
    validation loaders have ``shuffle=False`` and the default ``drop_last``."""
    if n < 1 or batch < 1:
        raise ValueError("batch_ranges: n >= 1 and batch >= 1")
    return [(r, min(batch, n - r)) for r in range(0, n, batch)]


class Evaluator:
    """``step``: a Stage1Step / DualStage1Step / CognitiveStep / WaeStep.  ``dataset``: the validation set (with fMRI rows
    where the step takes fMRI).  ``rng``: the evaluator's OWN generator for ``eps`` (stream SID_EPS, advanced by the
    evaluator after every batch); needed only where the eval forward samples.  ``mean`` / ``std``: the ingest
    normalisation, as DeviceFeed.  ``denorm``: metrics on v * std + mean (``evaluate(norm=True)``, denormalize_image)
    instead of the normalised images.  ``capacity``: rows of the ring.  ``identify``: None, or the ``top`` of n-way
    identification (above); every batch of a pass, the last included, then needs at least two images.
    ``grids`` (egress.GridSink): the scripts' epoch-end image grids as uint8 pixels -- ``train_batch()`` writes the first
    ``count`` rows of the training truth and of the train-mode ``x_tilde``, ``run()`` those of the last batch's images and
    reconstructions and, with ``generate=g > 0`` (needs an ``rng``), of an eval-mode decoder forward of g rows of N(0, I)
    (``model(None, g)``).  ``dump`` (egress.ImageDump): ``run()`` also writes every reconstruction and every ingested
    image of the pass, normalised per image and resized, as ``evaluate(save=True)`` writes its files.  Without the three
    a pass enqueues exactly what it did before them.  ``weights``: ``"live"`` (default) the weights of the last step;
    ``"ema"`` the step's averaged ones (a step built with ``ema=WeightEma(...)``, fmri_hip/ema.py) -- ``run()`` only,
    ``train_batch()`` reads the training step's own tensors.  Two evaluators whose generators share a seed make a paired
    comparison.

    With ``distributed=True`` steps every rank evaluates the whole set by itself: there is no collective in a pass."""

    def __init__(self, step, dataset: DeviceDataset, batch: int, rng: Optional[DeviceRng] = None,
                 mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), denorm: bool = False, capacity: int = 1024,
                 identify: Optional[int] = None, grids=None, dump=None, generate: int = 0, weights: str = "live"):
        from .steps import CognitiveStep, Stage1Step
        from .wae_steps import WaeStep
        if weights not in ("live", "ema"):
            raise ValueError(f"Evaluator: weights must be 'live' or 'ema', got {weights!r}")
        if weights == "ema" and getattr(step, "ema", None) is None:
            raise ValueError("Evaluator: weights='ema' needs a step constructed with ema=WeightEma(...)")
        self.weights = weights
        if isinstance(step, WaeStep):
            self.enc, self.uses_fmri, self.samples = (step.img_enc if step.stage == 1 else step.cog), step.stage > 1, False
        elif isinstance(step, CognitiveStep):
            self.enc, self.uses_fmri, self.samples = step.cog, True, True
        elif isinstance(step, Stage1Step):
            self.enc, self.uses_fmri, self.samples = step.enc, False, True
        else:
            raise TypeError("Evaluator: step must be a Stage1Step, DualStage1Step, CognitiveStep or WaeStep")
        self.step, self.ds, self.dec = step, dataset, step.dec
        cfg = step.cfg
        N, H, W, _ = dataset.images.shape
        if (H, W) != (cfg.image_size, cfg.image_size):
            raise ValueError(f"Evaluator: validation images are {H} x {W}, the step's are {cfg.image_size} x "
                             f"{cfg.image_size}")
        if dataset.images.device != step.device:
            raise ValueError("Evaluator: the dataset lives on another device than the step")
        if self.uses_fmri and (dataset.fmri is None or dataset.fmri.shape[1] != step.n_voxels):
            raise ValueError("Evaluator: this step takes fMRI -- the dataset needs fp32 fMRI rows of n_voxels columns")
        if self.samples and rng is None:
            raise ValueError("Evaluator: the eval-mode forward of this step samples z = mu + eps * sigma -- pass "
                             "rng=DeviceRng(seed, device)")
        if rng is not None and rng.device != step.device:
            raise ValueError("Evaluator: rng lives on another device than the step")
        if int(batch) != batch or batch < 1:
            raise ValueError("Evaluator: batch must be an integer >= 1")
        self.rng = rng if self.samples else None
        self.B = B = min(int(batch), N)
        self.ranges = batch_ranges(N, B)
        if identify is not None:
            if int(identify) != identify or identify < 1:
                raise ValueError("Evaluator: identify must be an integer >= 1 (the `top` of objective_assessment)")
            if self.ranges[-1][1] < 2:
                raise ValueError(f"Evaluator: identify needs two images in every batch, the last batch of {N} images in "
                                 f"batches of {B} holds one (the reference's random.choice([]) raises there too)")
            if self.samples and identify - 1 > cfg.latent_dim:
                raise ValueError(f"Evaluator: identify - 1 = {identify - 1} distractors per image exceed latent_dim = "
                                 f"{cfg.latent_dim}, the generator's advance per image")
        self.identify = None if identify is None else int(identify)
        self._id_rng = rng if identify is not None else None
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if denorm:
            self._scale, self._shift = (C.c_float * 3)(*self.std), (C.c_float * 3)(*self.mean)
        else:
            self._scale = self._shift = None
        dev = step.device
        Z = cfg.latent_dim
        self.H, self.W, self.Z = H, W, Z
        # persistent buffers (a short last batch uses their first rows)
        self._idx = torch.arange(N, dtype=torch.int32, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._x16 = torch.empty(B, H, W, 8, dtype=torch.float16, device=dev)
        self._pred16 = torch.empty(B, H, W, 8, dtype=torch.float16, device=dev)
        self._fmri16 = (torch.empty(B, pad8(dataset.fmri.shape[1]), dtype=torch.float16, device=dev)
                        if self.uses_fmri else None)
        self._eps = torch.empty(B, Z, dtype=torch.float32, device=dev) if self.samples else None
        self._z16 = torch.empty(B, pad8(Z), dtype=torch.float16, device=dev)
        self._zst = torch.zeros(2, dtype=torch.float32, device=dev)          # [max |z|, range scale] of the batch
        self._last_rows = 0
        # metrics: one row [pcc, ssim, mse, running means, batches] per batch of the pass, written by the fold launch
        self._ws_bytes = lib.load().fmri_image_metrics_ws_bytes(B, H, W)
        self._ws = torch.empty(self._ws_bytes // 8, dtype=torch.float64, device=dev)
        self._acc = torch.zeros(4, dtype=torch.float64, device=dev)
        self._bm = torch.zeros(len(self.ranges), 7, dtype=torch.float32, device=dev)
        self._train = torch.full((7,), float("nan"), dtype=torch.float32, device=dev)
        last = (len(self.ranges) - 1) * 7
        flat = self._bm.view(-1)
        cols = [("epoch", step.feed._state, 1)] if step.feed is not None else []
        cols.append(("batches", flat, last + 6))
        cols += [(f"valid_{m}", flat, last + k) for k, m in enumerate(METRICS)]
        cols += [(f"mean_{m}", flat, last + 3 + k) for k, m in enumerate(METRICS)]
        cols += [(f"train_{m}", self._train, k) for k, m in enumerate(METRICS)]
        if self.identify is not None:
            # persistent, as the metrics buffers; one out8 row per batch, the running scores of the last row are the pass's
            self._id_bytes = lib.load().fmri_nway_ws_bytes(B, H, W)
            self._id_ws = torch.empty(self._id_bytes, dtype=torch.uint8, device=dev)
            self._id_sim = torch.zeros(2, B * B, dtype=torch.float32, device=dev)
            self._id_draws = (torch.zeros(B * (self.identify - 1), dtype=torch.int32, device=dev)
                              if self._id_rng is not None else None)
            self._id_acc = torch.zeros(6, dtype=torch.float64, device=dev)
            self._id_out = torch.zeros(len(self.ranges), 8, dtype=torch.float32, device=dev)
            cols += [(name, self._id_out.view(-1), (len(self.ranges) - 1) * 8 + 4 + k) for k, name in enumerate(NWAY)]
        self.log = TrainLog(capacity)
        self.log.attach(dev, cols, ())
        # the pictures (fmri_hip/egress.py): opt-in, without them a pass enqueues what it did before
        if int(generate) != generate or generate < 0:
            raise ValueError("Evaluator: generate must be an integer >= 0")
        self.grids, self.dump, self.generate = grids, dump, int(generate)
        if self.generate:
            if rng is None:
                raise ValueError("Evaluator: generate draws the decoder's input on the device -- pass "
                                 "rng=DeviceRng(seed, device)")
            if grids is None:
                raise ValueError("Evaluator: generate writes the `random` grid -- pass grids=GridSink(...)")
            self._gen_rng = rng
            self._gen_scale = 0.5 if isinstance(step, WaeStep) and step.stage == 1 else 1.0      # as SID_ZFAKE
            self._gen32 = torch.empty(self.generate, Z, dtype=torch.float32, device=dev)
            self._genz16 = torch.zeros(self.generate, pad8(Z), dtype=torch.float16, device=dev)
            self._gen16 = torch.empty(self.generate, H, W, 8, dtype=torch.float16, device=dev)
        if grids is not None:
            grids.attach(dev, H, W, self.log.counter)
        if dump is not None:
            dump.attach(dev, N, H, W, B)

    # ---- the metrics of one batch: two launches ----------------------------------------------------------------------
    def _metrics(self, pred16: torch.Tensor, truth16: torch.Tensor, out7: torch.Tensor, acc, acc_mode: int):
        n, H, W, cp = pred16.shape
        nbytes = lib.load().fmri_image_metrics_ws_bytes(n, H, W)
        if nbytes > self._ws_bytes:          # (a training batch larger than the validation batch)
            self._ws = torch.empty(nbytes // 8, dtype=torch.float64, device=pred16.device)
            self._ws_bytes = nbytes
        sc = None if self._scale is None else C.cast(self._scale, C.c_void_p)
        sf = None if self._shift is None else C.cast(self._shift, C.c_void_p)
        lib.call("fmri_image_metrics", _P(pred16), _P(truth16), n, H, W, 3, cp, sc, sf, _P(self._ws), self._ws_bytes,
                 _P(out7), _P(acc), acc_mode)

    # ---- n-way identification of one batch: five launches ----------------------------------------------------------------
    def _identify(self, pred16: torch.Tensor, truth16: torch.Tensor, k: int):
        """n-way identification of batch ``k`` of the pass: one fmri_nway_scores (five launches) into row k of the out8
        rows, on top of the accumulator from the second batch on."""
        b, H, W, cp = pred16.shape
        g = self._id_rng
        lib.call("fmri_nway_scores", _P(pred16), _P(truth16), b, H, W, 3, cp, self.identify,
                 None if g is None else _P(g._state), SID_DISTRACT, _P(self._id_ws), self._id_bytes, _P(self._id_sim[0]),
                 _P(self._id_sim[1]), _P(self._id_draws), _P(self._id_out[k]), _P(self._id_acc), 0 if k == 0 else 1)

    # ---- the eval-mode forward of one batch --------------------------------------------------------------------------
    def _forward(self, r0: int, b: int, advance: bool = True):
        ds, Z = self.ds, self.Z
        N, H, W, Cimg = ds.images.shape
        idx = self._idx[r0:r0 + b]
        x16, pred16, z16 = self._x16[:b], self._pred16[:b], self._z16[:b]
        m, s = self.mean, self.std
        lib.call("fmri_ingest_u8_gather", _P(ds.images), _P(idx), N, b, H, W, Cimg, None, None, m[0], m[1], m[2], s[0],
                 s[1], s[2], _P(x16), None, _P(self._err))
        if self.uses_fmri:
            lib.call("fmri_gather_rows_f32", _P(ds.fmri), N, ds.fmri.shape[1], _P(idx), b, None, _P(self._fmri16[:b]),
                     _P(self._err))
            head32, _ = self.enc.forward(self._fmri16[:b])
        else:
            head32, _ = self.enc.forward(x16)
        if self.samples:
            eps = self._eps[:b]
            self.rng.normal(b, Z, SID_EPS, out=eps)
            if advance:
                self.rng.advance(blocks(b * Z))
            self._zst.zero_()
            ops.latent_ranged(head32, eps, b, Z, z16, self._zst[0:1], self._zst[1:2], sample=True)
            self.dec.forward(z16, 1, out=pred16, zscale=self._zst[1:2])
        else:
            lib.call("fmri_latent_fwd", _P(head32), None, b, Z, z16.shape[1], _P(z16), None, None, 0)      # z = mu
            self.dec.forward(z16, 1, out=pred16)
        self._last_rows = b
        return pred16, x16

    def _generate(self):
        """The `random` grid: an eval-mode decoder forward of ``generate`` rows of N(0, I) (Stage-I WAE: times 0.5), drawn
        on stream SID_GENERATE at the generator's offset at the end of the pass.  The offset is not advanced: ``eps``, the
        distractor draws and with them every column have the bits of a pass without ``generate``."""
        g, Z = self.generate, self.Z
        self._gen_rng.normal(g, Z, SID_GENERATE, scale=self._gen_scale, out=self._gen32)
        lib.call("fmri_rows_f32_to_f16", _P(self._gen32), _P(self._genz16), g, Z, self._genz16.shape[1], 1.0)
        self.dec.forward(self._genz16, 1, out=self._gen16)
        self.grids.write("random", self._gen16)

    def run(self):
        """One pass over the validation set in eval mode and one row in the ring; enqueues only.  ``weights="ema"``: the
        whole pass runs inside ``step.ema.swapped()`` -- the same columns, grids and dumps from the averaged weights."""
        if self.weights == "ema":
            with self.step.ema.swapped():
                self._run()
        else:
            self._run()

    def _run(self):
        ops.require_gpu(self.ds.images)
        bns = [bn for net in (self.enc, self.dec) for bn in net.all_bns()]
        was = [bn.eval_mode for bn in bns]
        for bn in bns:
            bn.eval_mode = True
        try:
            for k, (r0, b) in enumerate(self.ranges):
                # with identify, the batch's advance waits for the distractor draws made at the same offset
                pred16, x16 = self._forward(r0, b, advance=self.identify is None)
                self._metrics(pred16, x16, self._bm[k], self._acc, 0 if k == 0 else 1)
                if self.identify is not None:
                    self._identify(pred16, x16, k)
                    if self._id_rng is not None:
                        self._id_rng.advance(blocks(b * (self.Z if self.samples else self.identify - 1)))
                if self.dump is not None:
                    self.dump.write(0, r0, pred16)
                    self.dump.write(1, r0, x16)
                if self.grids is not None and k == len(self.ranges) - 1:
                    self.grids.write("valid_truth", x16)
                    self.grids.write("valid_output", pred16)
            if self.generate:
                self._generate()
        finally:
            for bn, w in zip(bns, was):
                bn.eval_mode = w
        self.log.append()
        self._train.fill_(float("nan"))          # a train_batch() counts for the next row only

    def train_batch(self):
        """PCC / SSIM / MSE of the step's last TRAINING batch -- its train-mode ``x_tilde`` against the block the script
        compares it with (``x`` in Stage I, the ``x_gt`` the model returned in Stages II / III) -- into the ``train_*``
        columns of the next row; enqueues only."""
        from .wae_steps import WaeStep
        fw = self.step.fw
        if not fw:
            raise RuntimeError("Evaluator.train_batch(): the step has not run yet")
        if isinstance(self.step, WaeStep):
            pred16, truth16 = fw["y"], fw["x16"]
        else:
            B, d = fw["B"], fw["disc_in"]
            pred16, truth16 = d[B:2 * B], d[:B]
        self._metrics(pred16, truth16, self._train, None, 0)
        if self.grids is not None:
            self.grids.write("train_truth", truth16)
            self.grids.write("train_output", pred16)

    # ---- reading back ---------------------------------------------------------------------------------------------------
    def history(self) -> Dict[str, np.ndarray]:
        """ONE sync: column name -> numpy array over the last min(passes, capacity) passes, oldest first, and ``"pass"``,
        their absolute numbers."""
        h = self.log.history()
        h["pass"] = h.pop("step")
        h["batches"] = np.rint(h["batches"]).astype(np.int64)
        return h

    def batch_metrics(self) -> torch.Tensor:
        """Device fp32 [n_batches, 3]: PCC, SSIM, MSE of every batch of the last pass (a view: the next pass rewrites it)."""
        return self._bm[:, :3]

    def _identifying(self, what: str):
        if self.identify is None:
            raise RuntimeError(f"Evaluator.{what}(): built without identify")

    def identification(self) -> torch.Tensor:
        """Device float64 [6] of the last pass: hits (PCC, SSIM), expected hits (PCC, SSIM), images, batches (a view)."""
        self._identifying("identification")
        return self._id_acc

    def batch_identification(self) -> torch.Tensor:
        """Device fp32 [n_batches, 8] of the last pass: per batch hits / n and expectation / n (PCC, SSIM each), then the
        same four over the images up to and including that batch (a view)."""
        self._identifying("batch_identification")
        return self._id_out

    def last_similarity(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(S_pcc, S_ssim), fp32 [rows, rows] views: reconstruction i against image j of the last batch of the last pass."""
        self._identifying("last_similarity")
        b = self._last_rows
        return self._id_sim[0, :b * b].view(b, b), self._id_sim[1, :b * b].view(b, b)

    def last_distractors(self) -> Optional[torch.Tensor]:
        """int32 [rows, identify - 1] view of the last batch's draws; None without an rng."""
        self._identifying("last_distractors")
        if self._id_draws is None:
            return None
        k = self.identify - 1
        return self._id_draws[:self._last_rows * k].view(self._last_rows, k)

    def last_output(self) -> torch.Tensor:
        """fp32 NCHW reconstructions of the last batch of the last pass."""
        return nhwc_to_images(self._pred16[:self._last_rows], 3)

    def last_truth(self) -> torch.Tensor:
        """fp32 NCHW ingested (normalised) images of the last batch of the last pass."""
        return nhwc_to_images(self._x16[:self._last_rows], 3)

    def last_noise(self) -> Optional[torch.Tensor]:
        """fp32 [rows, latent_dim] ``eps`` of the last batch of the last pass (a copy); None where nothing is sampled."""
        return self._eps[:self._last_rows].clone() if self.samples else None
