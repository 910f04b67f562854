"""n-way identification kernels (csrc/ident.hip through fmri_hip.ident) against the float64 restatement
(ident_oracle.pcc_matrix64 / ssim_matrix64) at the shapes where tile, chunk and mask errors live: several 16 x 16 Gram
tiles in both directions and partial last tiles, a partial 16-wide K step and a last K chunk of one element, SSIM
windows that span a whole image and images one pixel past an SSIM tile, ssim_matrix in more than one row block, the
grid-stride path of the PCC epilogue.  Also: bitwise position independence across tiles, chunks and row blocks,
degenerate images (constant, NaN), the padded ``ldS`` of the C ABI and empty batches.

The images lie in [-1, 1] with a clearly nonzero mean per image, and every fourth image of a batch is tanh-saturated
or has flat regions at exactly +1 or -1 (white and black backgrounds after the loader's Normalize(0.5, 0.5)).  The bar
is 2e-6 absolute against float64 for every PCC and every SSIM value.  The kernels keep the Gram in fp64 across 16-wide
K steps and every SSIM statistic in fp64, so both sit far below it (about 1e-7).  fp32 arithmetic of the formulas
would not: the reference's own fp32 SSIM is 2.4e-5 from float64 on a saturated reconstruction against a flat target,
where E[x^2] - mu^2 cancels against C2 = 9e-4, and a single fp32 chain over a 1024-element K chunk was 5e-6 off."""
import pytest
import torch

import ident_oracle as IO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-6


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    """The float64 oracle on at most 16 CPU threads, for this module only."""
    was = torch.get_num_threads()
    torch.set_num_threads(min(16, was))
    yield
    torch.set_num_threads(was)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(what, got, want, fp32=None):
    """max |got - want| <= BAR over every entry (no NaN on either side); prints the maximum.  ``fp32``: a callable
    giving the fp32 oracle's values, evaluated only on failure, to tell a kernel defect from fp32 rounding of the
    formula."""
    got = got.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(want).any() and not torch.isnan(got).any(), what
    err = (got - want).abs().max().item()
    print(f"{what}: max |err| vs fp64 = {err:.3g}")
    if err > BAR:
        e32 = (fp32().double() - want).abs().max().item() if fp32 else float("nan")
        pytest.fail(f"{what}: max |err| vs fp64 {err:.3g} > {BAR} (fp32 oracle on the same inputs: {e32:.3g})")
    return err


@pytest.fixture(scope="module")
def px100():
    """The reference's inference batch: 64 x 3 x 100 x 100 (D = 30000), with the fp64 matrices."""
    pred, truth = IO.edge_batch(64, 64, 3, 100, 100, 2024)
    return pred, truth, IO.pcc_matrix64(pred, truth), IO.ssim_matrix64(pred, truth)


def test_inference_batch_and_remainders_against_fp64(px100):
    """64 x 64 (4 x 4 tiles, D = 30000 = 29 chunks + 304 = 19 sixteen-steps), and the remainder batches 49 x 64 and
    64 x 49 (a partial last tile in each direction): every PCC and SSIM entry."""
    from fmri_hip import ident
    pred, truth, P64, S64 = px100
    pd, td = pred.to(DEV), truth.to(DEV)
    for (n, m) in ((64, 64), (49, 64), (64, 49)):
        a, b = pd[:n], td[:m]
        _check(f"pcc {n}x{m} 3x100x100", ident.pcc_matrix(a, b), P64[:n, :m],
               lambda: IO.pcc_matrix(pred[:n], truth[:m]))
        _check(f"ssim {n}x{m} 3x100x100", ident.ssim_matrix(a, b), S64[:n, :m],
               lambda: IO.ssim_matrix(pred[:n], truth[:m]))


@pytest.mark.parametrize("n,m,c,h,w", [
    (17, 33, 3, 64, 64),      # one row / column past a tile
    (20, 20, 1, 25, 41),      # D = 1025: a last chunk of one element
    (16, 16, 1, 11, 13),      # D = 143: a partial 16-step in a single chunk; the window spans the whole height
    (16, 16, 1, 32, 32),      # D = 1024: exactly one chunk
    (16, 16, 3, 11, 11),      # the smallest SSIM geometry
    (16, 16, 3, 17, 16),      # one pixel past an SSIM tile, non-square
    (16, 16, 3, 16, 17),
])
def test_geometry_edges_against_fp64(n, m, c, h, w):
    from fmri_hip import ident
    pred, truth = IO.edge_batch(n, m, c, h, w, 100 + h * w + c)
    pd, td = pred.to(DEV), truth.to(DEV)
    tag = f"{n}x{m} {c}x{h}x{w}"
    _check(f"pcc {tag}", ident.pcc_matrix(pd, td), IO.pcc_matrix64(pred, truth), lambda: IO.pcc_matrix(pred, truth))
    _check(f"ssim {tag}", ident.ssim_matrix(pd, td), IO.ssim_matrix64(pred, truth),
           lambda: IO.ssim_matrix(pred, truth))


@pytest.fixture(scope="module")
def small300():
    """300 x 300 images of 1 x 11 x 11: ssim_matrix issues rows 0..217 and 218..299 as two blocks (65 536 // 300 = 218
    rows).  pred 218 is a copy of pred 217 and truth 218 a copy of truth 10: duplicates across the block boundary."""
    pred, truth = IO.edge_batch(300, 300, 1, 11, 11, 300)
    pred[218], truth[218] = pred[217], truth[10]
    return pred, truth


def test_ssim_matrix_in_two_row_blocks_against_fp64(small300):
    from fmri_hip import ident
    pred, truth = small300
    pd, td = pred.to(DEV), truth.to(DEV)
    _check("pcc 300x300 1x11x11", ident.pcc_matrix(pd, td), IO.pcc_matrix64(pred, truth))
    S = ident.ssim_matrix(pd, td)
    _check("ssim 300x300 1x11x11", S, IO.ssim_matrix64(pred, truth), lambda: IO.ssim_matrix(pred, truth))
    # the duplicates: a row of each block, and a column, bitwise
    Sb = _bits(S)
    assert torch.equal(Sb[217], Sb[218]) and torch.equal(Sb[:, 10], Sb[:, 218])
    assert torch.equal(Sb[217, 10], Sb[218, 218])


def test_ssim_pairs_across_pair_chunks_equals_the_matrix(small300):
    """70 000 random pairs: two fmri_ssim_pairs launches of ssim_pairs (_PAIR_CHUNK = 65 536), bitwise equal to the
    matching entries of ssim_matrix."""
    from fmri_hip import ident
    pred, truth = small300
    pd, td = pred.to(DEV), truth.to(DEV)
    g = torch.Generator().manual_seed(70000)
    pairs = torch.stack([torch.randint(0, 300, (70000,), generator=g), torch.randint(0, 300, (70000,), generator=g)], 1)
    v = ident.ssim_pairs(pd, td, pairs)
    S = ident.ssim_matrix(pd, td)
    assert torch.equal(_bits(v), _bits(S)[pairs[:, 0], pairs[:, 1]])


def test_pcc_epilogue_grid_stride_against_fp64():
    """1100 x 1100 pairs (1.21 M > 4096 blocks x 256 threads): ident_pcc_final_kernel takes its grid-stride loop."""
    from fmri_hip import ident
    pred, truth = IO.edge_batch(1100, 1100, 1, 11, 11, 1100)
    _check("pcc 1100x1100 1x11x11", ident.pcc_matrix(pred.to(DEV), truth.to(DEV)), IO.pcc_matrix64(pred, truth))


def _near_rows(S, margin):
    """Rows with a comparison |S[i, i] - S[i, j]| (j != i) below ``margin``."""
    d = (S.diagonal()[:, None] - S).abs()
    d.fill_diagonal_(float("inf"))
    return (d < margin).any(1)


def _slack(P64, S64):
    """Per metric, the number of rows whose count may differ from the fp64 count: margin below 4e-6 (2 x the bar)."""
    return torch.tensor([float(_near_rows(P64, 4e-6).sum()), float(_near_rows(S64, 4e-6).sum())], dtype=torch.float64)


def test_n_way_expected_counts_against_fp64(px100):
    """n_way_expected at 64 x 64 against the counting of the fp64 matrices: one row's count may differ only where that
    row has a comparison margin below 4e-6 (2 x the bar), and changes the mean by at most 1 / N."""
    from fmri_hip import ident
    pred, truth, P64, S64 = px100
    slack = _slack(P64, S64)
    print(f"n_way_expected 64x64: rows with a margin < 4e-6 (pcc, ssim) = {slack.tolist()}")
    for top in (2, 5, 10):
        got = ident.n_way_expected(pred.to(DEV), truth.to(DEV), top).cpu()
        want = IO.n_way_expected_from(P64, S64, top)
        assert ((got - want).abs() * 64 <= slack + 1e-9).all(), (top, got, want, slack)


def _cover(n, m):
    """(i, j) pairs that put every row and every column in every lane position 0..15 of every 16-tile."""
    out = []
    for t in range(4):
        for lane in range(16):
            i, j = 16 * t + lane, 16 * ((t + lane) % 4) + 15 - lane
            out += [(i, j), (j, i)]
    return [(i, j) for i, j in out if i < n and j < m]


def test_pair_values_are_position_independent_across_tiles(px100):
    """A pair's PCC and SSIM are bitwise those of the pair alone (N = M = 1 or a one-pair list), wherever it sits in a
    64 x 64 or 49 x 64 batch."""
    from fmri_hip import ident
    pred, truth = px100[:2]
    pd, td = pred.to(DEV), truth.to(DEV)
    for n, m in ((64, 64), (49, 64)):
        P, S = _bits(ident.pcc_matrix(pd[:n], td[:m])), _bits(ident.ssim_matrix(pd[:n], td[:m]))
        pairs = _cover(n, m)
        assert {i % 16 for i, _ in pairs} == set(range(16)) and {j // 16 for _, j in pairs} == {0, 1, 2, 3}
        for i, j in pairs:
            a, b = pd[i:i + 1], td[j:j + 1]
            assert torch.equal(_bits(ident.pcc_matrix(a, b))[0, 0], P[i, j]), (n, m, i, j)
            assert torch.equal(_bits(ident.ssim_pairs(a, b, [[0, 0]]))[0], S[i, j]), (n, m, i, j)
        v = _bits(ident.ssim_pairs(pd[:n], td[:m], torch.tensor(pairs)))
        assert torch.equal(v, S[[i for i, _ in pairs], [j for _, j in pairs]])


def test_duplicates_in_other_tiles_tie_bitwise(px100):
    """truth 3 = truth 40 and pred 5 = pred 50, each pair in different 16-tiles: the columns (rows) are bitwise equal, and
    the strict > of n_way counts the duplicate target as a miss, as the reference does on the host."""
    from fmri_hip import ident
    pred, truth = [t.clone() for t in px100[:2]]
    truth[3], pred[5] = truth[40], pred[50]
    pd, td = pred.to(DEV), truth.to(DEV)
    P, S = ident.pcc_matrix(pd, td), ident.ssim_matrix(pd, td)
    for M in (_bits(P), _bits(S)):
        assert torch.equal(M[:, 3], M[:, 40]) and torch.equal(M[5], M[50])
    d = torch.full((64, 1), 0, dtype=torch.int64)
    d[0, 0], d[3, 0], d[40, 0] = 1, 40, 3
    hit = ident.n_way(pd, td, d).cpu()
    assert not hit[3].any() and not hit[40].any()
    assert torch.equal(hit, IO.n_way_from(P.cpu(), S.cpu(), d))


def test_degenerate_images():
    """Constant and NaN images in a 16 x 16 batch of 3 x 64 x 64 (the rest: edge_batch data).
    pred 0 = 0.5, pred 1 = -1.0, truth 4 = 0.5, truth 7 = -1.0 (exactly representable means): the reference's PCC is
    0 / 0 = NaN, and so is the engine's.  pred 2 = truth 5 = 0.1 (fp32 mean inexact): the reference's PCC is rounding
    noise of its fp32 mean; the engine's fp64 mean is exact, so its PCC is NaN (fmri_hip/ident.py).  pred 3 and truth 6
    are NaN images: PCC and SSIM are NaN in that row or column, as in the reference.  A NaN PCC or SSIM is never a hit.
    SSIM of the constant images is finite and checked against fp64; every finite PCC too."""
    from fmri_hip import ident
    pred, truth = IO.edge_batch(16, 16, 3, 64, 64, 77)
    pred[0], pred[1], pred[2], pred[3] = 0.5, -1.0, 0.1, float("nan")
    truth[4], truth[5], truth[6], truth[7] = 0.5, 0.1, float("nan"), -1.0
    pd, td = pred.to(DEV), truth.to(DEV)
    P, S = ident.pcc_matrix(pd, td).cpu(), ident.ssim_matrix(pd, td).cpu()
    P64, S64 = IO.pcc_matrix64(pred, truth), IO.ssim_matrix64(pred, truth)
    nan_p = torch.zeros(16, 16, dtype=torch.bool)
    nan_p[:4], nan_p[:, 4:8] = True, True
    nan_s = torch.zeros(16, 16, dtype=torch.bool)
    nan_s[3], nan_s[:, 6] = True, True
    assert torch.equal(torch.isnan(P), nan_p) and torch.equal(torch.isnan(P64), nan_p)
    assert torch.equal(torch.isnan(S), nan_s) and torch.equal(torch.isnan(S64), nan_s)
    _check("pcc degenerate (finite entries)", P[~nan_p], P64[~nan_p])
    _check("ssim degenerate (finite entries, constants included)", S[~nan_s], S64[~nan_s])
    # the reference's fp32 arithmetic: exact-mean constants are NaN too, the 0.1 constant is finite rounding noise
    ref = IO.pcc_matrix(pred[:3], truth[8:9])
    assert torch.isnan(ref[:2]).all() and torch.isfinite(ref[2]).all() and ref[2].abs().max() < 1e-6
    # never a hit: every row has a degenerate ground truth or reconstruction in PCC; rows 3 and 6 in SSIM too
    g = torch.Generator().manual_seed(16)
    for top in (2, 5):
        d = torch.stack([torch.randperm(15, generator=g)[:top - 1] for _ in range(16)])
        d = d + (d >= torch.arange(16)[:, None]).long()
        hit = ident.n_way(pd, td, d).cpu()
        assert not hit[:8, 0].any() and not hit[3].any() and not hit[6].any()
        far = ~(_near_rows(P64, 4e-6) | _near_rows(S64, 4e-6))
        assert torch.equal(hit[far], IO.n_way_from(P64, S64, d)[far]), (top, hit)
        slack = _slack(P64, S64)
        got, want = ident.n_way_expected(pd, td, top).cpu(), IO.n_way_expected_from(P64, S64, top)
        assert ((got - want).abs() * 16 <= slack + 1e-9).all(), (top, got, want)


def test_padded_ld_of_the_abi():
    """fmri_pcc_matrix with ldS = M + 8 into a NaN-filled [N, M + 8] buffer: the first M columns are bitwise
    pcc_matrix, the padding is untouched."""
    from fmri_hip import ident, lib
    pred, truth = IO.edge_batch(17, 33, 3, 64, 64, 8)
    pd, td = pred.to(DEV), truth.to(DEV)
    N, M, D = 17, 33, 3 * 64 * 64
    S = torch.full((N, M + 8), float("nan"), device=DEV)
    nb = lib.load().fmri_pcc_matrix_ws_bytes(N, M, D)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("fmri_pcc_matrix", pd.data_ptr(), td.data_ptr(), N, M, D, S.data_ptr(), M + 8, ws.data_ptr(), nb)
    S = S.cpu()
    assert torch.equal(_bits(S[:, :M]), _bits(ident.pcc_matrix(pd, td)))
    assert torch.isnan(S[:, M:]).all()


def test_empty_batches():
    """N = 0 or M = 0: empty results of the right shape, no launch."""
    from fmri_hip import ident
    pred, truth = [t.to(DEV) for t in IO.edge_batch(4, 4, 3, 12, 12, 5)]
    e = pred[:0]
    assert ident.pcc_matrix(torch.empty(0, 3, 8, 8, device=DEV), torch.rand(5, 3, 8, 8, device=DEV)).shape == (0, 5)
    for fn in (ident.pcc_matrix, ident.ssim_matrix):
        for a, b, shape in ((e, truth, (0, 4)), (pred, e, (4, 0)), (e, e, (0, 0))):
            out = fn(a, b)
            assert out.shape == shape and out.dtype == torch.float32 and out.is_cuda, (fn.__name__, shape)
    no_pairs = torch.zeros(0, 2, dtype=torch.int64)
    for a, b in ((e, truth), (pred, e), (e, e)):
        out = ident.ssim_pairs(a, b, no_pairs)
        assert out.shape == (0,) and out.dtype == torch.float32
    with pytest.raises(ValueError):
        ident.ssim_pairs(e, truth, torch.tensor([[0, 0]]))
    for k in (0, 1, 4):
        out = ident.n_way(e, e, torch.zeros(0, k, dtype=torch.int64))
        assert out.shape == (0, 2) and out.dtype == torch.bool and out.is_cuda, k
