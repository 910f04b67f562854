"""Host side of on-device n-way identification (include/fmri_hip.h fmri_nway_scores; csrc/nway.hip): the argument checks
that come back before anything is launched, the workspace size, and the distractor mapping restated in numpy on the Philox
oracle.  No GPU."""
import ctypes

import numpy as np
import pytest

import rng_oracle as RO

E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from fmri_hip import build, lib as L
    build.build(verbose=False)
    return L.load()


def distractors(seed, offset, n, top, sid):
    """d[i][k] of fmri_nway_scores: element i (top - 1) + k of the stream mapped to [0, n - 2], then past i."""
    k = top - 1
    u = RO.integers(seed, offset, n * k, 0, n - 2, sid).reshape(n, k)
    return u + (u >= np.arange(n)[:, None])


def test_argument_errors_before_any_launch(lib):
    P = ctypes.c_void_p
    a = dict(pred=P(0x1000), truth=P(0x2000), n=4, H=16, W=16, C=3, Cp=8, top=5, rng=P(0x3000), sid=10, ws=P(0x4000),
             nb=1 << 40, sp=P(0x5000), ss=P(0x6000), d=P(0x7000), out=P(0x8000), acc=P(0x9000), mode=0)

    def call(**kw):
        v = dict(a, **kw)
        return lib.fmri_nway_scores(v["pred"], v["truth"], v["n"], v["H"], v["W"], v["C"], v["Cp"], v["top"], v["rng"],
                                    v["sid"], v["ws"], v["nb"], v["sp"], v["ss"], v["d"], v["out"], v["acc"], v["mode"],
                                    None)
    assert call(n=1) == E_BADARG and call(n=0) == E_BADARG
    assert call(top=0) == E_BADARG
    for name in ("pred", "truth", "ws", "sp", "ss", "out", "acc"):
        assert call(**{name: None}) == E_BADARG, name
    assert call(pred=P(0x1008)) == E_BADARG                  # 16-byte alignment of the image layout
    assert call(mode=2) == E_BADARG
    assert call(H=10) == E_UNSUPPORTED and call(W=10) == E_UNSUPPORTED
    assert call(Cp=4) == E_UNSUPPORTED and call(Cp=16) == E_UNSUPPORTED
    assert call(C=5) == E_UNSUPPORTED                        # the workspace is sized for at most 4 real channels
    need = lib.fmri_nway_ws_bytes(4, 16, 16)
    assert call(nb=need - 1) == E_WORKSPACE and call(nb=0) == E_WORKSPACE
    # bad arguments win over an unsupported geometry and a short workspace
    assert call(n=1, H=10, nb=0) == E_BADARG and call(H=10, nb=0) == E_UNSUPPORTED


def test_workspace_size(lib):
    sizes = [lib.fmri_nway_ws_bytes(n, 64, 64) for n in (1, 2, 3, 4, 16, 17, 64, 256)]
    assert all(s > 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.fmri_nway_ws_bytes(0, 64, 64) < 0 and lib.fmri_nway_ws_bytes(-3, 64, 64) < 0
    assert lib.fmri_nway_ws_bytes(4, 0, 64) < 0
    assert lib.fmri_nway_ws_bytes(4, 24, 20) < lib.fmri_nway_ws_bytes(4, 64, 64)


@pytest.mark.parametrize("n", [2, 3, 19])
def test_distractor_mapping_never_draws_the_image_itself_and_covers_the_rest(n):
    from fmri_hip.rng import SID_DISTRACT
    assert SID_DISTRACT == 10
    top = 41
    d = distractors(0x1234567, 77, n, top, SID_DISTRACT)
    assert d.shape == (n, top - 1) and d.min() >= 0 and d.max() <= n - 1
    seen = set()
    for off in range(8):
        d = distractors(0x1234567, 77 + 1000 * off, n, top, SID_DISTRACT)
        for i in range(n):
            assert i not in d[i]
            seen |= {(i, int(v)) for v in d[i]}
    assert seen == {(i, j) for i in range(n) for j in range(n) if j != i}
    # another stream id gives other draws; the same arguments the same
    a = distractors(5, 0, 19, 5, SID_DISTRACT)
    assert np.array_equal(a, distractors(5, 0, 19, 5, SID_DISTRACT))
    assert not np.array_equal(a, distractors(5, 0, 19, 5, 9))
