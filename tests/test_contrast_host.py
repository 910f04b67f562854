"""Host-side checks of the contrastive latent alignment (no GPU): the float64 oracle of tests/contrast_oracle.py (autograd
against the closed form the kernel implements, a naive double loop, the zero-row convention, top-1 and margins), the data
recipe of the kernel test, the composed oracle step, the C ABI declaration and argument checks of fmri_latent_nce, and the
Python surface (LatentContrast, GPU tensors only, contrast=)."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import contrast_oracle as CO

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def _pair(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, d, generator=g, dtype=torch.float64) * 0.6 + 0.1
    q = t + torch.randn(n, d, generator=g, dtype=torch.float64) * 0.8
    return q, t


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n,d,tau", [(2, 3, 0.07), (3, 8, 1.0), (7, 5, 0.01), (12, 16, 0.07), (40, 64, 0.03)])
def test_closed_form_equals_autograd(n, d, tau, symmetric):
    q, t = _pair(n, d, 100 * n + d)
    r = CO.nce64(q, t, tau, symmetric)
    assert abs(float(r["loss"] - r["loss_cf"])) < 1e-12
    assert (r["grad"] - r["grad_cf"]).abs().max().item() < 1e-12, (n, d, tau)
    assert r["grad"].abs().max().item() > 0


def test_loss_equals_the_double_loop():
    n, d, tau = 6, 5, 0.2
    q, t = _pair(n, d, 3)
    a = [[v / math.sqrt(sum(x * x for x in row)) for v in row] for row in q.tolist()]
    b = [[v / math.sqrt(sum(x * x for x in row)) for v in row] for row in t.tolist()]
    s = [[math.fsum(x * y for x, y in zip(a[i], b[j])) / tau for j in range(n)] for i in range(n)]
    l_row = math.fsum(math.log(math.fsum(math.exp(s[i][j]) for j in range(n))) - s[i][i] for i in range(n)) / n
    l_col = math.fsum(math.log(math.fsum(math.exp(s[i][j]) for i in range(n))) - s[j][j] for j in range(n)) / n
    assert abs(CO.nce_loss(q, t, tau, True).item() - 0.5 * (l_row + l_col)) < 1e-12
    assert abs(CO.nce_loss(q, t, tau, False).item() - l_row) < 1e-12


def test_loss_passes_gradcheck():
    q, t = _pair(5, 4, 9)
    q.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: CO.nce_loss(x, t, 0.3), (q,), eps=1e-6, atol=1e-8)


def test_top1_margins_and_perfect_alignment():
    q, t = _pair(9, 16, 4)
    r = CO.nce64(t * 3.0, t, 0.07)                 # q parallel to t: every row retrieves itself
    assert bool(r["hit"].all()) and bool((r["margin"] > 0).all())
    perm = torch.roll(torch.arange(9), 1)
    r = CO.nce64(t[perm], t, 0.07)                 # every row paired with another row's image
    assert not bool(r["hit"].any()) and bool((r["margin"] < 0).all())
    r = CO.nce64(q, t, 0.07)
    s = r["s"]
    for i in range(9):
        others = [s[i, j].item() for j in range(9) if j != i]
        assert abs(r["margin"][i].item() - (s[i, i].item() - max(others))) < 1e-15
        assert bool(r["hit"][i]) == (s[i, i].item() >= max(others))
    hits, near = CO.top1_count(r, 1e-9)
    assert hits == int(r["hit"].sum()) and not bool(near.any())
    _, near = CO.top1_count(r, 1e9)
    assert bool(near.all())


def test_zero_row_convention():
    n, d, tau = 7, 8, 0.07
    q, t = _pair(n, d, 11)
    q[3] = 0.0
    t[5] = 0.0
    r = CO.nce64(q, t, tau)
    assert torch.isfinite(r["loss"]) and bool(torch.isfinite(r["grad"]).all())
    assert bool((r["s"][3] == 0).all()) and bool((r["s"][:, 5] == 0).all())
    assert bool((r["grad"][3] == 0).all()) and bool((r["grad_cf"][3] == 0).all())
    assert (r["grad"] - r["grad_cf"]).abs().max().item() < 1e-12


def test_recipe_is_not_the_trivial_all_hits_case():
    qw, tw = CO.recipe(256, 128, pad_q=4, pad_t=12)
    assert qw.shape == (256, 132) and tw.shape == (256, 140)
    r = CO.nce64(qw[:, :128], tw[:, :128], 0.07)
    hits = int(r["hit"].sum())
    assert 100 < hits < 250, hits
    assert 0.05 < float(r["loss"]) < 6.0
    b = CO.bounds(r, 128, 0.07)
    assert abs(b["eps_s"] - 136 * 2.0 ** -24 / 0.07) < 1e-18 and b["loss"] > 2 * b["eps_s"]
    assert bool((b["grad"] > 0).all())
    with pytest.raises(ValueError):
        CO.bounds(CO.nce64(qw[:, :64], tw[:, :64], 1.0), 64, 1.0)     # outside the condition of the derivation


@pytest.mark.parametrize("penalty", ["gan", "mmd"])
@pytest.mark.parametrize("stage", [2, 3])
def test_composed_step_adds_the_term_to_the_encoder_loss(stage, penalty):
    """weight = 0 reproduces the plain oracle step; weight > 0 moves the Stage-II encoder and leaves Stage III's frozen
    encoder alone."""
    import mmd_oracle as MO
    from oracle import vaegan_oracle as O
    cfg, V, B = O.ArchCfg.px64(), 64, 4
    data = O.synth_batch(B, cfg, n_voxels=V, seed=3, steps=1)

    def state():
        teacher = O.fill_state(O.encoder_spec(cfg) + O.decoder_spec(cfg) + O.wae_discriminator_spec(cfg), 5, True)
        P = dict(O.fill_state(O.cognitive_encoder_spec(cfg, V), 105, True))
        P.update({k: v for k, v in teacher.items() if k.startswith("decoder.")})
        P.update(O.fill_state(O.wae_discriminator_spec(cfg), 205, True))
        P.update({"teacher_net." + k: v for k, v in teacher.items() if k.startswith("encoder.")})
        return P

    def opts():
        return {k: O.OptState(kind="adam", lr=1e-3) for k in ("encoder", "decoder", "discriminator")}
    P0, P1, P2 = state(), state(), state()
    r0 = CO.wae_nce_step(P0, opts(), stage, cfg, data["x"], data["fmri"], V, penalty, weight=0.0)
    if penalty == "gan":
        fn = O.wae_stage2_step if stage == 2 else O.wae_stage3_step
        plain = fn(P1, opts(), data["fmri"], data["x"], cfg, V)
    else:
        plain = MO.wae_mmd_step(P1, opts(), stage, cfg, data["x"], None, data["fmri"], V)
    for k, v in plain["logs"].items():
        assert r0["logs"][k] == v, k
    assert r0["logs"]["loss_contrast"] == 0.0
    for k in P1:
        assert torch.equal(P0[k], P1[k]), k
    r2 = CO.wae_nce_step(P2, opts(), stage, cfg, data["x"], data["fmri"], V, penalty, weight=1.0, keep_grads=True)
    want = CO.nce_loss(r2["fw"]["z_real"], r2["fw"]["z_teacher"], 0.07).item()
    assert abs(r2["logs"]["loss_contrast"] - want) < 1e-6 * max(1.0, want) and want > 0
    moved = [k for k in P1 if k.startswith("encoder.") and "running" not in k and "num_batches" not in k
             and not torch.equal(P1[k], P2[k])]
    assert bool(moved) == (stage == 2)


def test_fmri_latent_nce_is_declared_and_exported(lib):
    from fmri_hip import lib as L
    # declared in the header fmri_hip.h includes for them; lib.py derives their prototypes from it
    main = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    assert re.search(r'^#include "fmri_hip_contrast\.h"', main, re.M)
    hdr = open(os.path.join(ROOT, "include", "fmri_hip_contrast.h")).read()
    assert re.search(r"\bint fmri_latent_nce\s*\(", hdr)
    assert re.search(r"\bint64_t fmri_latent_nce_ws_bytes\s*\(", hdr)
    assert L.EXT_EXPORTS == {"fmri_latent_nce": "fmri_hip_contrast.h", "fmri_latent_nce_ws_bytes": "fmri_hip_contrast.h"}
    assert not set(L.EXT_EXPORTS) & set(L.EXPORTS)
    assert L.prototype("fmri_latent_nce")[1] is ctypes.c_int and L.prototype("fmri_mmd_imq")[0] == L._SIGS["fmri_mmd_imq"]
    # what tests/test_abi.py holds every entry point of fmri_hip.h to, for these two: the symbol is exported, one derived
    # type per declared parameter, a launch ends in the stream and returns int
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S)
    assert set(re.findall(r"\b(fmri_[a-z0-9_]+)\s*\(", code)) == set(L.EXT_EXPORTS)
    for name in L.EXT_EXPORTS:
        assert hasattr(lib, name), f"{name} declared in include/fmri_hip_contrast.h but not exported"
        m = re.search(r"([\w*]+)\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        params = " ".join(m.group(2).split())
        args, ret = L.prototype(name)
        assert len(args) == params.count(",") + 1, name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ret
        if params.endswith("void* stream"):
            assert m.group(1) == "int" and args[-1] is ctypes.c_void_p and ret is ctypes.c_int, name
    i, l, f, p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert L.prototype("fmri_latent_nce") == ([p, i, p, i, i, i, f, i, f, p, p, p, i, f, p, l, p], i)
    assert L.prototype("fmri_latent_nce_ws_bytes") == ([i, i], l)
    assert lib.fmri_latent_nce_ws_bytes.restype is ctypes.c_int64
    assert len(lib.fmri_latent_nce.argtypes) == 17
    assert lib.fmri_latent_nce.argtypes[6] is ctypes.c_float and lib.fmri_latent_nce.argtypes[7] is ctypes.c_int


def test_fmri_latent_nce_argument_checks_without_gpu(lib):
    """Rejected on the host before anything is enqueued: n outside [2, 4096], unsupported d, tau outside [0.01, 1], short
    leading dimensions, misaligned rows, a workspace below fmri_latent_nce_ws_bytes."""
    for n, d in ((1, 128), (4097, 128), (64, 96), (64, 2048), (64, 0)):
        assert lib.fmri_latent_nce_ws_bytes(n, d) < 0, (n, d)
    for n, d in ((2, 128), (17, 512), (1000, 1024), (64, 64), (4096, 1024)):
        assert lib.fmri_latent_nce_ws_bytes(n, d) > 0
    # the n x n logits and the per-split slabs fit the stated budget
    assert lib.fmri_latent_nce_ws_bytes(4096, 1024) < (64 << 20) + (32 << 20) + (16 << 20)
    z = ctypes.c_void_p(256)
    big = 1 << 40

    def call(q=z, ldq=128, t=z, ldt=128, n=8, d=128, tau=0.07, dq=z, ldd=128, ws=z, nb=big):
        return lib.fmri_latent_nce(q, ldq, t, ldt, n, d, tau, 1, 1.0, None, None, dq, ldd, 1.0, ws, nb, None)
    assert call(n=1) == -1
    assert call(n=4097) == -2
    assert call(ldq=64) == -1 and call(ldt=100) == -1 and call(ldd=64) == -1
    assert call(tau=0.005) == -1 and call(tau=1.5) == -1 and call(tau=float("nan")) == -1
    assert call(q=None) == -1 and call(t=None) == -1 and call(ws=None) == -1
    assert call(q=ctypes.c_void_p(260)) == -1
    assert call(ldq=130) == -1
    assert call(d=96, ldq=128, ldt=128, ldd=128) == -2
    assert call(d=2048, ldq=2048, ldt=2048, ldd=2048) == -2
    assert call(nb=16) == -4


def test_latent_contrast_validates_its_ranges():
    from fmri_hip.contrast import LatentContrast
    c = LatentContrast()
    assert (c.weight, c.temperature, c.symmetric) == (1.0, 0.07, True)
    assert LatentContrast(0.0, 0.01, False).temperature == 0.01 and LatentContrast(2.0, 1.0).temperature == 1.0
    for bad in (0.005, 1.5, 0.0, -0.07, float("nan")):
        with pytest.raises(ValueError):
            LatentContrast(temperature=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            LatentContrast(weight=bad)


def test_info_nce_has_no_cpu_fallback():
    from fmri_hip.contrast import info_nce, latent_nce
    q, t = _pair(4, 64, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        info_nce(q.float(), t.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        latent_nce(q.float(), t.float(), 0.07)


def test_wae_step_surface():
    from fmri_hip.contrast import LatentContrast
    from fmri_hip.params import ArchConfig
    from fmri_hip.wae_steps import W_CON, W_TOP1, WaeStep
    sig = inspect.signature(WaeStep.__init__)
    assert sig.parameters["contrast"].default is None
    assert 26 <= W_CON < W_TOP1 < 32
    with pytest.raises(ValueError, match="stage 2 or 3"):
        WaeStep(ArchConfig.px64(), "cpu", 1, contrast=LatentContrast())
    with pytest.raises(ValueError):
        WaeStep(ArchConfig.px64(), "cpu", 2, 512, contrast=0.07)
    # the kernel's geometry is checked when the step is built, not inside its first step
    import dataclasses
    for z in (100, 32, 2048):
        with pytest.raises(ValueError, match="multiple of 64"):
            WaeStep(dataclasses.replace(ArchConfig.px64(), latent_dim=z), "cpu", 2, 512, contrast=LatentContrast())
