"""Host checks of the float64 restatement of the differentiable augmentation (tests/diffaug_oracle.py): the stated
adjoint really is the adjoint of T's linear part, the torch version the step tests differentiate equals the numpy one,
the neutral row is the identity, and the rows decoded from Philox words stay inside their ranges."""
import numpy as np
import pytest
import torch

import diffaug_oracle as A
import rng_oracle

SIZES = (16, 25)


def _hand_rows(H):
    sh, cut = A.sizes(H)
    odd = cut % 2
    rows = [A.NEUTRAL.copy()]
    for ty in (-sh, sh):
        for tx in (-sh, sh):
            rows.append(np.array([0.3, 0.4, 1.4, ty, tx, H // 2, H // 3, cut], np.float64))
    for cy, cx in ((0, 0), (H - odd, H - odd), (0, H - odd), (H - odd, 0)):
        rows.append(np.array([-0.2, 1.7, 0.6, 1, -1, cy, cx, cut], np.float64))
    rows.append(np.array([0.1, 0.9, 1.1, 0, 0, H // 2, H // 2, H], np.float64))          # everything cut
    rows.append(np.array([0.25, 1, 1, 0, 0, 0, 0, 0], np.float64))                        # one stage at a time
    rows.append(np.array([0, 0.0, 1, 0, 0, 0, 0, 0], np.float64))
    rows.append(np.array([0, 1, 0.5, 0, 0, 0, 0, 0], np.float64))
    rows.append(np.array([0, 1, 1, -sh, 1, 0, 0, 0], np.float64))
    rows.append(np.array([0, 1, 1, 0, 0, 3, H - 2, cut], np.float64))
    return rows


def _rows(H):
    sh, cut = A.sizes(H)
    drawn = A.table_rows(5, 17, 6, 2, A.SID_DAUG, H, sh, cut)
    return _hand_rows(H) + list(drawn)


@pytest.mark.parametrize("H", SIZES)
def test_adjoint_identity_in_float64(H):
    """<T(x) - T(x'), g> = <x - x', L^T g> to 1e-9 over hand-built and drawn rows."""
    rs = np.random.RandomState(H)
    for p in _rows(H):
        x, x2, g = rs.uniform(-1, 1, (H, H, 3)), rs.uniform(-1, 1, (H, H, 3)), rs.standard_normal((H, H, 3))
        lhs = np.sum((A.transform(x, p) - A.transform(x2, p)) * g)
        rhs = np.sum((x - x2) * A.adjoint(g, p))
        assert abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs)), (p, lhs, rhs)


@pytest.mark.parametrize("H", SIZES)
def test_torch_transform_equals_numpy_and_its_gradient_is_the_adjoint(H):
    rs = np.random.RandomState(100 + H)
    rows = _rows(H)
    n = len(rows)
    x = rs.uniform(-1, 1, (n, H, H, 3))
    g = rs.standard_normal((n, H, H, 3))
    xt = torch.tensor(x.transpose(0, 3, 1, 2), dtype=torch.float64, requires_grad=True)
    yt = A.torch_transform(xt, np.stack(rows))
    (yt * torch.tensor(g.transpose(0, 3, 1, 2))).sum().backward()
    for i, p in enumerate(rows):
        np.testing.assert_allclose(yt[i].detach().numpy().transpose(1, 2, 0), A.transform(x[i], p), rtol=0, atol=1e-12)
        np.testing.assert_allclose(xt.grad[i].numpy().transpose(1, 2, 0), A.adjoint(g[i], p), rtol=0, atol=1e-12)


@pytest.mark.parametrize("H", SIZES)
def test_neutral_row_is_the_identity(H):
    rs = np.random.RandomState(7)
    x16 = np.zeros((3, H, H, 8), np.float16)
    x16[..., :3] = rs.uniform(-1, 1, (3, H, H, 3)).astype(np.float16)
    x16[0, 0, 0, 0] = np.float16(6e-8)                   # a subnormal and a signed zero survive too
    x16[0, 0, 1, 1] = np.float16(-0.0)
    table = np.tile(A.NEUTRAL, (2, 1))
    assert A.forward16(x16, table, 1).tobytes() == x16.tobytes()
    assert A.adjoint16(x16[1:], table, 1, 1).tobytes() == x16[1:].tobytes()
    t = A.torch_transform(torch.tensor(x16[..., :3].astype(np.float32)).permute(0, 3, 1, 2), table[[0, 0, 1]])
    assert torch.equal(t.permute(0, 2, 3, 1), torch.tensor(x16[..., :3].astype(np.float32)))


@pytest.mark.parametrize("H", (16, 25, 64, 100, 128))
def test_decoded_rows_respect_every_range(H):
    sh, cut = A.sizes(H)
    assert (sh, cut) == {16: (2, 8), 25: (3, 13), 64: (8, 32), 100: (13, 50), 128: (16, 64)}[H]
    p = A.table_rows(3, 1 << 33, 4096, 5, A.SID_DAUG_P, H, sh, cut)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)              # fp32 values
    assert p[:, 0].min() >= -0.5 and p[:, 0].max() < 0.5
    assert p[:, 1].min() >= 0.0 and p[:, 1].max() < 2.0
    assert p[:, 2].min() >= 0.5 and p[:, 2].max() <= 1.5           # (u + 0.5 is rounded to fp32 from 1 on: 1.5 at the top)
    for col in (3, 4):
        assert set(np.unique(p[:, col])) == set(range(-sh, sh + 1))
    for col in (5, 6):
        assert set(np.unique(p[:, col])) == set(range(0, H - cut % 2 + 1))
    assert np.all(p[:, 7] == cut)
    # the extreme words, column by column
    lo = A.decode(np.zeros((1, 8), np.uint64), H, sh, cut)[0]
    hi = A.decode(np.full((1, 8), 0xFFFFFFFF, np.uint64), H, sh, cut)[0]
    assert list(lo) == [-0.5, 0.0, 0.5, -sh, -sh, 0, 0, cut]
    top = 1.0 - 2.0 ** -24
    assert list(hi) == [top - 0.5, 2 * top, 1.5, sh, sh, H - cut % 2, H - cut % 2, cut]
    # a policy that is off leaves the neutral values of its columns
    w = np.full((1, 8), 0x89ABCDEF, np.uint64)
    assert list(A.decode(w, H, sh, cut, policy=A.TRANSLATION)[0][[0, 1, 2, 5, 6, 7]]) == [0, 1, 1, 0, 0, 0]
    assert list(A.decode(w, H, sh, cut, policy=A.COLOR)[0][3:]) == [0, 0, 0, 0, 0]
    assert list(A.decode(w, H, sh, cut, policy=A.CUTOUT)[0][:5]) == [0, 1, 1, 0, 0]


def test_rows_are_slices_of_the_stream():
    """Row r of a draw at row0 is row row0 + r of the draw from 0: a rank's slice of the global batch."""
    H, (sh, cut) = 64, A.sizes(64)
    full = A.table_rows(11, 40, 12, 0, A.SID_DAUG, H, sh, cut)
    assert np.array_equal(A.table_rows(11, 40, 4, 8, A.SID_DAUG, H, sh, cut), full[8:])
    w = rng_oracle.raw_words(11, 40, 96, A.SID_DAUG).reshape(12, 8)
    assert np.array_equal(A.decode(w, H, sh, cut), full)
    st = A.step_table(11, 40, 4, H, row0=4)
    assert np.array_equal(st[:4], full[4:8])
    assert not np.array_equal(st[4:], st[:4])                                     # the sampled rows: another stream
