"""The lambda pair-matrix and column-sum kernels at every slate tier, against the fp64 oracle.

Cases, inputs and the clamp-band precondition come from tests/lambda_tier_cases.py (checked on the CPU by test_lambda_tiers_cpu.py).
Per case: ltr_lambda_pairs_fwd through the C ABI with all three outputs, lambdaMask forward / backward, lambda_colsum forward /
backward, ltr_lambda_fwd_bwd, and the exact invariants between them; then ltr_lambda_colsum_sys_fwd/_bwd and the cached entry
ltr_lambda_risk_model_fwd.

Bar: max|delta| / max|ref| <= max(1e-5, 4 x the oracle's own fp32-vs-fp64 deviation on the same inputs); every
compared quantity goes to the parity ledger under `<entry>.<quantity> [S regime]`.  No pair is ever left out of a comparison.

Pairs with a padded document: the kernel evaluates the SAME expression as the oracle with the padded document's score -inf, gain 0
and clamped label 0 (d = clamp(s_i - s_j, +-1e8), NaN -> 0): log_b(eps) or w log_b(eps) when the first document is padded, 0 when
only the second is, w log_b(1/2) when both are.  The test pins that by comparing the whole matrix (`losses_all`), besides the
real-pair block and the kept pairs on their own scale.  `rank` holds, for a padded document, its rank among the padded ones by
index, after every real document.
"""
import pytest
import torch

import lambda_tier_cases as LT
import ltr_oracle as O
import ltr_risk_oracle as RO
from conftest import ledger_record, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()           # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def gate(quantity, S, got, ref, ref32, what):
    """Record and assert one quantity: err against the fp64 oracle, noise = the fp32 oracle against the fp64 oracle."""
    got, ref, ref32 = (t.detach().cpu().double().numpy() for t in (got, ref, ref32))
    assert got.shape == ref.shape, (quantity, got.shape, ref.shape)
    err, noise = relerr(got, ref), relerr(ref32, ref)
    bar = max(TOL, 4.0 * noise)
    ledger_record(f"{quantity} [S {LT.regime(S)}]", err, noise=noise, tol=TOL, note=what)
    print(f"{what} {quantity}: rel_err {err:.3e} oracle fp32 noise {noise:.3e} bar {bar:.3e}")
    assert err <= bar, (quantity, what, err, noise)


def largs_of(kw):
    from ltr_mi355x.functional import _lambda_args
    sid, kk, sigma, mu, eps, pad, lb = _lambda_args(LT.EPS, LT.PAD, kw["weighing_scheme"], kw["k"], kw["sigma"], kw["mu"],
                                                    kw["reduction_log"])
    assert kk >= 0
    return (sid, kk, sigma, mu, eps, pad, lb)


def mask_kw(kw):
    return dict(eps=LT.EPS, padded_value_indicator=LT.PAD, **kw)


@pytest.mark.parametrize("case", LT.tier_cases(), ids=LT.case_id)
def test_lambda_tier(case, dev):
    from losses.lambdaL import lambdaMask
    from ltr_mi355x._lib import check, lib
    from ltr_mi355x.functional import _ptr, _stream
    from ltr_mi355x.risk import lambda_colsum
    s, y, kw = LT.build(case)                       # asserts the clamp-band precondition before the GPU is touched
    B, S, what = case.B, case.S, LT.case_id(case)
    clamped = case.variant == "clamped"
    gen = torch.Generator().manual_seed(7000 + S)
    gup, gcol = torch.randn(B, S, S, generator=gen), torch.randn(B, S, generator=gen)
    o64 = LT.oracle_bundle(s, y, kw, gup, gcol, torch.float64)
    o32 = LT.oracle_bundle(s, y, kw, gup, gcol, torch.float32, grads=not clamped)
    keep_ref = o64["keep"]
    assert torch.equal(keep_ref, o32["keep"])
    real = LT.real_pairs(y)
    h, largs = lib(), largs_of(kw)
    sd, yd = s.to(dev), y.to(dev)

    # ---- a. ltr_lambda_pairs_fwd, all three outputs, into NaN / sentinel-filled buffers
    losses = torch.full((B, S, S), float("nan"), dtype=torch.float32, device=dev)
    keep = torch.full((B, S, S), 255, dtype=torch.uint8, device=dev)
    rank = torch.full((B, S), -7, dtype=torch.int32, device=dev)
    check(h.ltr_lambda_pairs_fwd(_ptr(sd), _ptr(yd), B, S, *largs, _ptr(losses), _ptr(keep), _ptr(rank), _stream()),
          "ltr_lambda_pairs_fwd")
    losses, keep, rank = losses.cpu(), keep.cpu(), rank.cpu()
    r_ref = O.rank_desc(torch.where(y == LT.PAD, torch.full_like(s, float("-inf")), s))
    assert torch.equal(rank.long(), r_ref), what
    assert torch.equal(keep, keep_ref.to(torch.uint8)), what
    assert not bool(torch.isnan(losses).any()), what
    gate("pairs_fwd.losses_real", S, losses[real], o64["losses"][real], o32["losses"][real], what)
    gate("pairs_fwd.losses_kept", S, losses[keep_ref], o64["losses"][keep_ref], o32["losses"][keep_ref], what)
    gate("pairs_fwd.losses_all", S, losses, o64["losses"], o32["losses"], what)

    # ---- b. lambdaMask: masked 1-D form, and the backward of the full matrix under a random upstream gradient
    masked = lambdaMask(sd, yd, **mask_kw(kw))
    assert masked.shape == o64["losses"][keep_ref].shape, what
    gate("lambdaMask.masked", S, masked, o64["losses"][keep_ref], o32["losses"][keep_ref], what)
    sr = sd.clone().requires_grad_(True)
    full = lambdaMask(sr, yd, return_losses=True, **mask_kw(kw))
    assert torch.equal(full.detach().cpu(), losses), what
    full.backward(gup.to(dev))
    assert bool(torch.isfinite(sr.grad).all()), what
    if not clamped:
        gate("pairs_bwd.dscores", S, sr.grad, o64["g_full"], o32["g_full"], what)

    # ---- c. column sums without the [B,S,S] tensor, forward and backward
    sc = sd.clone().requires_grad_(True)
    col = lambda_colsum(sc, yd, kw["weighing_scheme"], LT.EPS, LT.PAD, kw["k"], kw["sigma"], kw["mu"], kw["reduction_log"])
    gate("colsum_fwd.colsum", S, col, o64["col"], o32["col"], what)
    col.backward(gcol.to(dev))
    assert bool(torch.isfinite(sc.grad).all()), what
    if not clamped:
        gate("colsum_bwd.dscores", S, sc.grad, o64["g_col"], o32["g_col"], what)

    # ---- d'. ltr_lambda_fwd_bwd per slate (lambdaLoss itself: test_losses_gpu.py::test_lambda_oracle)
    slate = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    count = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    ds = torch.full((B, S), float("nan"), dtype=torch.float32, device=dev)
    check(h.ltr_lambda_fwd_bwd(_ptr(sd), _ptr(yd), B, S, *largs, 1.0, _ptr(slate), _ptr(count), _ptr(ds), _stream()),
          "ltr_lambda_fwd_bwd")
    slate, count, ds = slate.cpu(), count.cpu(), ds.cpu()
    assert bool(torch.isfinite(slate).all()) and bool(torch.isfinite(count).all()) and bool(torch.isfinite(ds).all()), what
    gate("fwd_bwd.slate_loss", S, slate, o64["slate"], o32["slate"], what)
    if not clamped:
        gate("fwd_bwd.dscores", S, ds, o64["g_sum"], o32["g_sum"], what)

    # ---- e. exact invariants between the entries, on the GPU results themselves
    n_kept = keep.long().sum(dim=(1, 2))
    assert torch.equal(n_kept, count.long()) and torch.equal(count, count.round()), (what, n_kept, count)
    for b in range(B):
        if int(n_kept[b]) == 0:
            assert float(slate[b]) == 0.0 and not bool(ds[b].any()), (what, b)
        if not bool((y[b] != LT.PAD).any()):                        # all padding: finite everywhere, zero loss / count / gradients
            assert int(n_kept[b]) == 0 and float(count[b]) == 0.0, (what, b)
            assert not bool(sr.grad[b].any()) and not bool(sc.grad[b].any()) and not bool(ds[b].any()), (what, b)
            assert bool(torch.isfinite(losses[b]).all()) and bool(torch.isfinite(col[b]).all()), (what, b)


SYS_OPTS = {0: (None, 1.0, "binary"), 2: (5, 2.0, "natural")}      # n_base -> (k, sigma, log): both option sets at no extra cost


@pytest.mark.parametrize("S", [17, 257, 1025, 2048])
@pytest.mark.parametrize("nb", [0, 2])
@pytest.mark.parametrize("scheme", list(O.SCHEMES))
def test_colsum_sys_and_cached_model(S, nb, scheme, dev):
    """ltr_lambda_colsum_sys_fwd (slate softmaxes inside the kernel): every system's column sums against RO._softmaxes +
    RO.pair_colsum in fp64, ltr_lambda_colsum_sys_bwd against fp64 autograd through the same; then ltr_lambda_risk_model_fwd
    (lt 1 / 2 / 3, n_cached 0 / 3, a cache_stride larger than n_cached + S) bit for bit against the chain
    ltr_lambda_colsum_sys_fwd + ltr_risk_matrix_fwd mode 1, as its header promises."""
    from ltr_mi355x import risk as R
    from ltr_mi355x._lib import check, lib
    from ltr_mi355x.functional import _ptr, _stream
    B = LT.batch_of(S)
    k, sigma, log = SYS_OPTS[nb]
    kw = dict(weighing_scheme=scheme, k=k, sigma=sigma, mu=LT.MU, reduction_log=log)
    what = f"sys-B{B}-S{S}-nb{nb}-{scheme}"
    gen = torch.Generator().manual_seed(9000 + S + nb)
    yp, yt = torch.randn(B, S, generator=gen), torch.randint(0, 5, (B, S), generator=gen).float()
    yb = torch.randn(B, S, nb, generator=gen) if nb else None
    gup = torch.randn(B, S, generator=gen)

    def oracle(dtype):
        x = yp.detach().clone().to(dtype).requires_grad_(True)
        pt, pp, pb = RO._softmaxes(x, yt.to(dtype), None if yb is None else yb.to(dtype))
        systems = [pp] + [pb[:, :, j] for j in range(nb)] + [pt]
        cols = [RO.pair_colsum(p, pt, scheme, k=k, sigma=sigma, pad=LT.PAD, reduction_log=log, mu=LT.MU) for p in systems]
        g, = torch.autograd.grad((cols[0] * gup.to(dtype)).sum(), x)
        return [p.detach() for p in systems], pt.detach(), torch.stack([c.detach() for c in cols]), g

    sys64, pt64, col64, g64 = oracle(torch.float64)
    for p in sys64:                                  # softmaxed score gaps are below 1: the same precondition, no ladder
        (band, _), = LT.band_counts(p, pt64, kw)
        assert band == 0, what
    _, _, col32, g32 = oracle(torch.float32)

    xd = yp.to(dev).requires_grad_(True)
    ytd = yt.to(dev)
    ybd = None if yb is None else yb.to(dev)
    out = R.lambda_colsum_systems(xd, ytd, ybd, scheme, LT.EPS, LT.PAD, k, sigma, LT.MU, log)
    assert tuple(out.shape) == (nb + 2, B, S)
    for j in range(nb + 2):
        gate(f"colsum_sys_fwd.colsum[{'model' if j == 0 else 'ideal' if j == nb + 1 else 'baseline'}]", S, out[j], col64[j],
             col32[j], what)
    (out[0] * gup.to(dev)).sum().backward()
    gate("colsum_sys_bwd.dy_pred", S, xd.grad, g64, g32, what)

    h, largs = lib(), largs_of(kw)
    cs = out.detach()
    for lt in (1, 2, 3):
        mat0 = torch.full((B, 1), float("nan"), dtype=torch.float32, device=dev)
        jac0 = torch.full((B, S), float("nan"), dtype=torch.float32, device=dev)
        check(h.ltr_risk_matrix_fwd(_ptr(cs[nb + 1]), _ptr(cs[0]), None, B, S, 0, 1, lt, 0, _ptr(mat0), _ptr(jac0), _stream()),
              "ltr_risk_matrix_fwd")
        for n_cached in (0, 3):
            stride = n_cached + S + 5
            cache = torch.randn(B, stride, generator=gen).to(dev)
            cache[:, n_cached:n_cached + S] = cs[nb + 1]
            mat = torch.full((B, 1 + n_cached), float("nan"), dtype=torch.float32, device=dev)
            jac = torch.full((B, S), float("nan"), dtype=torch.float32, device=dev)
            check(h.ltr_lambda_risk_model_fwd(_ptr(xd.detach()), _ptr(ytd), _ptr(cache), stride, n_cached, B, S, *largs, lt,
                                              _ptr(mat), _ptr(jac), _stream()), "ltr_lambda_risk_model_fwd")
            assert bool(torch.isfinite(mat0).all()) and bool(torch.isfinite(jac0).all()), (what, lt)
            assert torch.equal(mat[:, 0], mat0[:, 0]), (what, lt, n_cached)
            assert torch.equal(mat[:, 1:], cache[:, :n_cached]), (what, lt, n_cached)
            assert torch.equal(jac, jac0), (what, lt, n_cached)
