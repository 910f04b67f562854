"""Gradient parity helpers for the fused-step tests (GPU engine vs the CPU oracle).

Two references per tensor:
  * the oracle run under its 16-bit storage model (``oracle.vaegan_oracle.STORAGE16``): same fp32 arithmetic, but every
    tensor the engine stores in fp16 is rounded where the engine rounds it, so the ReLU masks agree with the engine's
    and the gradients can be compared tightly (relative L2 error per tensor);
  * the plain fp32 oracle (what the golden vectors pin): fp16 activations flip the ReLU mask of the ~1e-3 of elements
    whose pre-activation lies within rounding of zero, which adds unbiased noise to back-propagated gradients -- there the
    engine's gradient must keep the direction (cosine) and the length along the reference (projection).

The first reference is tight only with the ENGINE's ReLU masks pinned in the oracle (``pinned``).  ``Recorder`` collects
them from a step's networks while the step runs; one ordering function per step kind (``stage1_masks``,
``cognitive_masks``, ``wae_masks``, ``dual_masks``, ``literal_masks``) puts them into the oracle's call order -- the
order tests/test_relu_masks_host.py documents and counts.  Measured figures: profiles/step_grad_parity.md.
"""
import contextlib
import os

import torch

TOL16 = 1e-2        # relative L2 error against the 16-bit-storage oracle, per tensor
COS32 = 0.95        # cosine against the fp32 oracle
PROJ32 = 0.08       # |<g, r> / <r, r> - 1| against the fp32 oracle (B = 4: mask flips move small tensors by 3-7 %: the 64-element
                    # decoder.conv.2.bn gradients of the 100-px config read 0.952 / 0.933 with igemm_tc5 / igemm_tc5w at err16 2e-3)


LOOSE16 = 0.15      # what the 16-bit bound was while a step's masks were not pinned (``tol16=None``): no test uses it as
                    # its bound any more; tests/test_relu_masks_host.py keeps it to show what a pinned run sees and it did not


@contextlib.contextmanager
def storage16(O):
    O.STORAGE16 = True
    try:
        yield
    finally:
        O.STORAGE16 = False


@contextlib.contextmanager
def pinned(O, masks):
    """An oracle run under the 16-bit storage model with its ReLU masks pinned to ``masks`` (one entry per ReLU call of
    the run, in call order; ``None`` = that call keeps its own mask).  Both switches are restored whatever happens; a
    body that ends without an exception must have consumed every entry (one mask too few is the IndexError of the
    oracle's ``pop``)."""
    was16, was_masks = O.STORAGE16, O.RELU_MASKS
    O.STORAGE16, O.RELU_MASKS = True, list(masks)
    try:
        yield
        left = len(O.RELU_MASKS)
    finally:
        O.STORAGE16, O.RELU_MASKS = was16, was_masks
    assert left == 0, f"{left} of {len(masks)} pinned ReLU masks were not consumed"


@contextlib.contextmanager
def recording(O, out):
    """An oracle run that appends the (x > 0) mask of every ReLU call to the list ``out`` (``oracle.RELU_RECORD``)."""
    was = O.RELU_RECORD
    O.RELU_RECORD = out
    try:
        yield out
    finally:
        O.RELU_RECORD = was


# ----------------------------------------------------------------------------------------------------------------------
# the engine's ReLU masks, in the oracle's call order
# ----------------------------------------------------------------------------------------------------------------------
_SAVED = ("acts", "hfc", "h", "hs")      # what a forward context keeps of its ReLU outputs (fmri_hip/nets.py)


def _snapshot(ctx):
    """(stored activation > 0) of every saved ReLU output of a forward context, taken when the forward returns: on the
    device, behind the forward's launches on the current stream, so nothing a later pass does to the context matters."""
    out = {}
    for k in _SAVED:
        v = ctx.get(k)
        if v is not None:
            out[k] = [t > 0 for t in v] if isinstance(v, (list, tuple)) else v > 0
    return out


class Recorder:
    """Keeps, in call order, the ReLU masks of every forward pass a step's networks make.  Test side: ``forward`` (and
    the discriminator's ``forward_head``) are wrapped as instance attributes, the library is not touched.  Two steps do
    not keep the contexts themselves: CognitiveStep.forward drops the teacher encoder's, WaeStep.step holds all of its
    in locals -- and the latent discriminator's two passes (D phase, penalty on the updated weights) are told apart by
    their order only: ``rec["wd"][0]`` and ``rec["wd"][1]``.
    ``Recorder(None, enc=net, dec=net, ...)``: networks that belong to no step (the engine networks behind the drop-in
    modules of models/vae_gan.py), under the same names."""
    NETS = ("img_enc", "cog", "teacher_enc", "enc", "dec", "dis", "wd")

    def __init__(self, st=None, **nets):
        self.calls = []                              # (attribute name of the network, snapshot of its context)
        seen = set()
        assert set(nets) <= set(self.NETS), nets.keys()
        for name in self.NETS:
            net = nets.get(name, getattr(st, name, None))
            if net is None or id(net) in seen:       # (WaeStep.enc is img_enc or cog: recorded under that name)
                continue
            seen.add(id(net))
            self._wrap(net, name, "forward", lambda r: r[-1])
            if name == "dis":
                self._wrap(net, "dis.head", "forward_head", None)

    def _wrap(self, net, name, method, ctx_of):
        inner = getattr(net, method)

        def wrapped(*a, **k):
            r = inner(*a, **k)
            # forward_head completes the context it is handed in place (first argument)
            ctx = ctx_of(r) if ctx_of is not None else (a[0] if a else k["ctx"])
            self.calls.append((name, _snapshot(ctx)))
            return r
        setattr(net, method, wrapped)

    def clear(self):
        del self.calls[:]

    def __getitem__(self, name):
        return [c for n, c in self.calls if n == name]

    def one(self, name):
        got = self[name]
        assert len(got) == 1, (name, len(got), [n for n, _ in self.calls])
        return got[0]


def _nchw(t):
    return (t.float() > 0).permute(0, 3, 1, 2).float().cpu()


def _rows(t):
    return (t.float() > 0).float().cpu()


def _enc(ctx):
    """Encoder: 3 conv blocks, fc."""
    return [_nchw(ctx["acts"][i]) for i in (1, 2, 3)] + [_rows(ctx["hfc"])]


def _cog(ctx):
    return [_rows(ctx["h"])]


def _dec(ctx, B, g):
    """Call group ``g`` (rows [g B, (g + 1) B) of the stacked batch) of a decoder pass: fc, 3 deconv blocks."""
    sl = slice(g * B, (g + 1) * B)
    a = ctx["acts"]
    assert a[0].shape[0] % B == 0 and a[0].shape[0] >= (g + 1) * B, (tuple(a[0].shape), B, g)
    # fc: (H,W,C) engine order -> the reference's (C,H,W)
    return [_nchw(a[0][sl]).reshape(B, -1)] + [_nchw(a[i][sl]) for i in (1, 2, 3)]


def _dis(ctx, level=3):
    """The image discriminator's one pass standing for the oracle's 'REC' call -- conv0 and the blocks below block
    ``level``, whose raw output it returns -- and its 'GAN' call (conv0, blocks 1-3, fc)."""
    a = ctx["acts"]
    return [_nchw(a[i]) for i in range(level)] + [_nchw(a[i]) for i in range(4)] + [_rows(ctx["hfc"])]


def _wd(ctx, rows=None):
    """Latent discriminator: 4 hidden layers (``hs[0]`` is its input), of the rows ``rows`` of a stacked pass."""
    hs = ctx["hs"]
    assert len(hs) == 5, len(hs)
    return [_rows(h if rows is None else h[rows]) for h in hs[1:]]


def stage1_masks(e, d, c, B, level=3):
    """vaegan_forward: encoder, decoder(z), decoder(z_p), discriminator 'REC' and 'GAN' -- 17 + level ReLU calls."""
    return _enc(e) + _dec(d, B, 0) + _dec(d, B, 1) + _dis(c, level)


def _engine_relu_masks(st):
    """The ReLU masks of a Stage-I step's last forward (``st.fw``) in the call order of the oracle's ReLUs."""
    fw = st.fw
    return stage1_masks(fw["ectx"], fw["dctx"], fw["sctx"], fw["B"], st.dis.level)


def stage1_masks_of(rec, B, level=3):
    return stage1_masks(rec.one("enc"), rec.one("dec"), rec.one("dis"), B, level)


def cognitive_masks(rec, B, teacher):
    """cognitive_forward (Stage II / III).  With the teacher (Stage II, 'vae-gan') the engine stacks the decoder's batch
    as (teacher, x_tilde, x_p) while the oracle calls decoder(z), the teacher encoder, decoder(z_teacher), decoder(z_p):
    25 calls; without it (x_tilde, x_p) on both sides: 17."""
    d = rec.one("dec")
    if teacher:
        m = _cog(rec.one("cog")) + _dec(d, B, 1) + _enc(rec.one("teacher_enc")) + _dec(d, B, 0) + _dec(d, B, 2)
    else:
        assert not rec["teacher_enc"]
        m = _cog(rec.one("cog")) + _dec(d, B, 0) + _dec(d, B, 1)
    return m + _dis(rec.one("dis"), 3)


def _latent_d_phase(rec, B):
    """_wae_dis_phase: d_real then d_fake, two oracle calls for the engine's one pass over [real ; fake]."""
    wd = rec["wd"]
    assert len(wd) == 2, len(wd)             # the D phase, then the penalty pass on the updated weights
    assert wd[0]["hs"][1].shape[0] == 2 * B and wd[1]["hs"][1].shape[0] == B
    return _wd(wd[0], slice(0, B)) + _wd(wd[0], slice(B, 2 * B))


def wae_masks(rec, B, stage, penalty="gan"):
    """wae_stage{1,2,3}_step (24 / 30 / 22 calls) and, ``penalty='mmd'``, tests/mmd_oracle.py's wae_mmd_step, which makes
    the same calls without the latent discriminator's (12 / 18 / 10).  The engine runs every generator-side network
    once where the scripts repeat a pass on the same weights: those masks repeat."""
    gan = penalty == "gan"
    dphase = _latent_d_phase(rec, B) if gan else []
    pen = _wd(rec["wd"][1]) if gan else []
    if not gan:
        assert not rec["wd"]
    d = rec.one("dec")
    if stage == 1:
        e = _enc(rec.one("img_enc"))
        return e + dphase + e + _dec(d, B, 0) + pen
    t, c = _enc(rec.one("img_enc")), _cog(rec.one("cog"))
    if stage == 2:
        # the decoder's batch is (z_teacher, z): x_gt = decoder(z_teacher) comes first and feeds no gradient
        return t + _dec(d, B, 0) + c + t + dphase + c + _dec(d, B, 1) + pen
    return c + t + dphase + c + pen + _dec(d, B, 0)


def dual_masks(rec, B, level=3):
    """dual_stage1_step: the Stage-I forward, the encoder again (no_grad), the latent D phase, the encoder a third time,
    decoder(z_real2) -- no gradient flows through it and the oracle keeps its own masks (None) --, the penalty pass:
    41 + level calls."""
    e = _enc(rec.one("enc"))
    return (stage1_masks_of(rec, B, level) + e + _latent_d_phase(rec, B) + e + [None] * 4 + _wd(rec["wd"][1]))


def report(got, ref32, ref16, skip=()):
    rows = []
    for k, r16 in ref16.items():
        if r16 is None or k in skip:
            continue
        g = got[k].detach().double().cpu().reshape(-1)
        a = r16.detach().double().reshape(-1)
        b = ref32[k].detach().double().reshape(-1)
        e16 = ((g - a).norm() / (a.norm() + 1e-30)).item()
        cos = (g @ b / (g.norm() * b.norm() + 1e-30)).item()
        proj = (g @ b / (b @ b + 1e-30)).item()
        rows.append((k, e16, cos, proj, g.numel()))
    return rows


def check(got, ref32, ref16, what="", skip=(), tol16=TOL16, cos32=COS32, proj32=PROJ32, small=64, loose16=LOOSE16):
    """Assert the criteria for every tensor.  ``ref16`` comes from an oracle run with the engine's ReLU masks pinned
    (``pinned``, with the masks one of the ordering functions above gives for the step) -> bound ``tol16``.  Every fused
    step is held to that; a 16-bit-storage run WITHOUT pinned masks (``tol16=None``) only has masks as far from the
    engine's as the fp32 run's and could be held to ``loose16`` only, which lets a 3 % misweighting of one loss term
    through (tests/test_relu_masks_host.py).  Tensors with fewer than ``small``
    elements (the 3-element bias of the decoder's last convolution, scalar biases: sums that cancel over the batch) are
    held to 5x the 16-bit bound only."""
    if tol16 is None:
        tol16 = loose16
    rows = report(got, ref32, ref16, skip)
    rows.sort(key=lambda r: -r[1])
    log = os.environ.get("FMRI_GRADLOG")
    if log:
        with open(log, "a") as f:
            f.write(f"# {what}: worst err16 {max(r[1] for r in rows):.3e}, min cos32 "
                    f"{min(r[2] for r in rows if r[4] >= small):.4f}, max |proj32-1| "
                    f"{max(abs(r[3] - 1) for r in rows if r[4] >= small):.4f} (bounds {tol16} / {cos32} / {proj32})\n")
            for k, e16, cos, proj, n in rows[:5]:
                f.write(f"{what} {k} err16 {e16:.3e} cos32 {cos:.4f} proj32 {proj:.4f} n {n}\n")
    for k, e16, cos, proj, n in rows[:8]:
        print(f"{what} grad {k}: err16 {e16:.2e} cos32 {cos:.4f} proj32 {proj:.4f} n {n}")
    print(f"{what} worst err16 {max(r[1] for r in rows):.2e}  min cos32 {min(r[2] for r in rows if r[4] >= small):.4f}")
    bad = []
    for k, e16, cos, proj, n in rows:
        if n < small:
            if e16 > 5 * tol16:
                bad.append((k, e16, cos, proj, n))
            continue
        if e16 > tol16 or cos < cos32 or abs(proj - 1.0) > proj32:
            bad.append((k, e16, cos, proj, n))
    assert not bad, (what, bad[:6])
    return rows


def literal_masks(rec, B, level=3):
    """A loop body written out call by call on the drop-in modules (models/vae_gan.py) makes the oracle's calls in the
    oracle's order, one engine pass each: the recorded calls one after the other.  The discriminator: a 'REC' call runs
    the conv stack only (no fc activation in its context) and stands for conv0 and the blocks below ``level``; a 'GAN'
    call is its fc head -- on the conv activations of the 'REC' call before it where the module re-uses them, inside a
    whole pass of its own otherwise."""
    m = []
    for name, c in rec.calls:
        if name == "dis.head":
            m += [_nchw(c["acts"][i]) for i in range(4)] + [_rows(c["hfc"])]
        elif name == "dis":
            if "hfc" not in c:
                m += [_nchw(c["acts"][i]) for i in range(level)]
        elif name == "dec":
            assert c["acts"][0].shape[0] == B
            m += _dec(c, B, 0)
        elif name == "cog":
            m += _cog(c)
        elif name == "wd":
            m += _wd(c)
        else:
            m += _enc(c)
    return m
