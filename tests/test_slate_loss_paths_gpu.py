"""approxNDCG and ListNet (csrc/ltr_slate_losses.h: approx_ndcg_slate, listnet_slate) on every code path at every slate tier, against
the fp64 oracle on the same fp32 inputs.

Cases, the declared path of every slate and the preconditions come from tests/slate_loss_cases.py (held on the CPU by
test_slate_loss_paths_cpu.py).  Entries: ltr_approxndcg_fwd_bwd / ltr_listnet_fwd_bwd through the C ABI (per-slate losses, gradient,
forward-only), the drop-in modules, the ragged twins through RaggedSlates (one query per tier length, regimes in rotation, and bit
equality with the rectangular entries on equal lengths).  The folded make_model ranker's one-launch step runs the same regimes in
tests/test_linear_fused_gpu.py.

Bar: max|delta| / max|ref| <= 1e-5 on the loss and on the gradient; the few cases named in slate_loss_cases.RELAXED take
max(1e-5, 4 x the oracle's own fp32-vs-fp64 deviation).  Every quantity goes to the parity ledger under
`<entry>.<quantity> [<path>, S <regime>]` with that deviation.  No pair is left out of a comparison."""
import numpy as np
import pytest
import torch

import ragged_cases as RC
import slate_loss_cases as SC
from conftest import ledger_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()           # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def gate(entry, quantity, c, path, got, ref, ref32, floor=0.0):
    """Record and assert one quantity: err against the fp64 oracle, noise = the fp32 oracle against the fp64 oracle."""
    got, ref, ref32 = (np.asarray(t.detach().cpu().double()) for t in (got, ref, ref32))
    assert got.shape == ref.shape, (entry, quantity, got.shape, ref.shape)
    assert np.isfinite(got).all(), (entry, quantity, SC.case_id(c))
    err, noise = SC.relerr(got, ref, floor), SC.relerr(ref32, ref, floor)
    bar = SC.bar_of(c, noise)
    ledger_record(f"{entry}.{quantity} [{path}, S {SC.regime_of(c.S)}]", err, noise=noise, tol=SC.TOL,
                  note=SC.case_id(c))
    print(f"{SC.case_id(c)} {entry}.{quantity} [{path}]: rel_err {err:.3e} oracle fp32 noise {noise:.3e} bar {bar:.3e}")
    assert err <= bar, (entry, quantity, SC.case_id(c), err, noise)


def path_label(paths):
    return "+".join(sorted(set(paths)))


def exact_zero_rows(got, ref, zero, what):
    """A slate whose gradient is identically zero BY STRUCTURE (fewer than two real documents, no document with a gain) comes back
    exactly zero.  (A saturated slate is not one of them: there the fp64 oracle's 1 - c rounds to 0 where the kernel's product of
    the two sigmoids keeps its 1e-20.)"""
    for b in range(ref.shape[0]):
        if zero[b]:
            assert not bool(ref[b].any()), (what, b)
            assert not bool(got[b].any()), (what, b, float(got[b].abs().max()))


def structurally_zero(y, pad):
    real = y != pad
    return [int(real[b].sum()) < 2 or not bool((y[b][real[b]] > 0).any()) for b in range(y.shape[0])]


def approx_abi(h, sd, yd, c, want_grad=True):
    from ltr_mi355x._lib import check
    from ltr_mi355x.functional import _ptr, _stream
    B, S = sd.shape
    slate = torch.full((B,), float("nan"), dtype=torch.float32, device=sd.device)
    ds = torch.full((B, S), float("nan"), dtype=torch.float32, device=sd.device) if want_grad else None
    check(h.ltr_approxndcg_fwd_bwd(_ptr(sd), _ptr(yd), B, S, c.alpha, c.eps, c.pad, 1.0, _ptr(slate), _ptr(ds) if want_grad else None,
                                   _stream()), "ltr_approxndcg_fwd_bwd")
    torch.cuda.synchronize()
    return slate.cpu(), (ds.cpu() if want_grad else None)


def listnet_abi(h, ytd, ypd, sig, want_grad=True):
    from ltr_mi355x._lib import check
    from ltr_mi355x.functional import _ptr, _stream
    B, S = ypd.shape
    slate = torch.full((B,), float("nan"), dtype=torch.float32, device=ypd.device)
    ds = torch.full((B, S), float("nan"), dtype=torch.float32, device=ypd.device) if want_grad else None
    check(h.ltr_listnet_fwd_bwd(_ptr(ytd), _ptr(ypd), B, S, int(sig), 1.0, _ptr(slate), _ptr(ds) if want_grad else None, _stream()),
          "ltr_listnet_fwd_bwd")
    torch.cuda.synchronize()
    return slate.cpu(), (ds.cpu() if want_grad else None)


# ---------------------------------------------------------------------------------------------------- dense, C ABI
@pytest.mark.parametrize("case", SC.approx_cases(), ids=SC.case_id)
def test_approxndcg_abi(case, dev):
    from ltr_mi355x._lib import lib
    c = case
    s, y, paths = SC.approx_inputs(c)
    ref = SC.reference(c)
    what, path = SC.case_id(c), path_label(paths)
    s0, y0 = s.clone(), y.clone()
    sd, yd = s.to(dev), y.to(dev)
    slate, ds = approx_abi(lib(), sd, yd, c)                      # dscores filled with NaN before the call
    assert bool(torch.isfinite(ds).all()), (what, "a gradient row was not written")
    assert not bool(ds[y == c.pad].any()), (what, "padded rows must be exactly 0")
    gate("approxndcg_fwd_bwd", "slate_loss", c, path, slate, ref.loss, ref.loss32)
    gate("approxndcg_fwd_bwd", "dscores", c, path, ds, ref.grad, ref.grad32, floor=SC.FLOOR if SC.uses_floor(c) else 0.0)
    exact_zero_rows(ds, ref.grad, structurally_zero(y, c.pad), what)
    fwd, _ = approx_abi(lib(), sd, yd, c, want_grad=False)        # dscores = NULL
    gate("approxndcg_fwd_bwd", "slate_loss(forward only)", c, path, fwd, ref.loss, ref.loss32)
    assert torch.equal(sd.cpu(), s0) and torch.equal(yd.cpu(), y0), what


@pytest.mark.parametrize("case", SC.list_cases(), ids=SC.case_id)
def test_listnet_abi(case, dev):
    from ltr_mi355x._lib import lib
    c = case
    yt, yp = SC.list_inputs(c)
    ref = SC.reference(c)
    what, path = SC.case_id(c), f"listnet {c.regime}" + (" sigmoid" if c.sigmoid else "")
    ytd, ypd = yt.to(dev), yp.to(dev)
    slate, ds = listnet_abi(lib(), ytd, ypd, c.sigmoid)
    assert bool(torch.isfinite(ds).all()), (what, "a gradient row was not written")
    gate("listnet_fwd_bwd", "slate_loss", c, path, slate, ref.loss, ref.loss32)
    gate("listnet_fwd_bwd", "dscores", c, path, ds, ref.grad, ref.grad32)
    exact_zero_rows(ds, ref.grad, [c.S == 1] * c.B, what)
    fwd, _ = listnet_abi(lib(), ytd, ypd, c.sigmoid, want_grad=False)
    gate("listnet_fwd_bwd", "slate_loss(forward only)", c, path, fwd, ref.loss, ref.loss32)
    assert torch.equal(ytd.cpu(), yt) and torch.equal(ypd.cpu(), yp), what


# ---------------------------------------------------------------------------------------------------- dense, drop-in modules
MODULE_APPROX = [c for c in SC.approx_cases() if c.S in SC.FULL_S and (c.regime in ("mixed", "offset") or c.variant in ("front", "front_inf"))]
MODULE_LIST = [c for c in SC.list_cases() if c.S in SC.FULL_S and c.regime.startswith("offset") and c.B <= 3]


@pytest.mark.parametrize("case", MODULE_APPROX, ids=SC.case_id)
def test_approxndcg_module(case, dev):
    from losses.approxNDCG import approxNDCGLoss
    c = case
    s, y, paths = SC.approx_inputs(c)
    ref = SC.reference(c)                                         # shared with test_approxndcg_abi: computed once
    sd, yd = s.to(dev).requires_grad_(True), y.to(dev)
    loss = approxNDCGLoss(sd, yd, eps=c.eps, padded_value_indicator=c.pad, alpha=c.alpha)
    loss.backward()
    path = path_label(paths)
    gate("approxNDCGLoss", "loss", c, path, loss.reshape(1), ref.loss.mean().reshape(1), ref.loss32.mean().reshape(1))
    gate("approxNDCGLoss", "dscores", c, path, sd.grad, ref.grad / c.B, ref.grad32 / c.B, floor=(SC.FLOOR if SC.uses_floor(c) else 0.0) / c.B)
    assert torch.equal(sd.detach().cpu(), s) and torch.equal(yd.cpu(), y), SC.case_id(c)       # inputs are not modified


@pytest.mark.parametrize("case", MODULE_LIST, ids=SC.case_id)
def test_listnet_module(case, dev):
    from losses.listnet import listnetLoss
    c = case
    yt, yp = SC.list_inputs(c)
    ref = SC.reference(c)
    ytd, ypd = yt.to(dev), yp.to(dev).requires_grad_(True)
    loss = listnetLoss(ytd, ypd, apply_sigmoid=c.sigmoid)
    loss.backward()
    path = f"listnet {c.regime}" + (" sigmoid" if c.sigmoid else "")
    gate("listnetLoss", "loss", c, path, loss.reshape(1), ref.loss.sum().reshape(1), ref.loss32.sum().reshape(1))
    gate("listnetLoss", "dscores", c, path, ypd.grad, ref.grad, ref.grad32)
    assert torch.equal(ypd.detach().cpu(), yp) and torch.equal(ytd.cpu(), yt), SC.case_id(c)


# ---------------------------------------------------------------------------------------------------- ragged
def _slates(lengths, dev):
    from ltr_mi355x.ragged import RaggedSlates
    return RaggedSlates(RC.bounds_of(lengths), device=dev)


def _ragged_launch(kind, sl, s, y, args, dev):
    from ltr_mi355x import lib, ragged
    from ltr_mi355x.functional import _ptr
    slate = torch.full((sl.n_queries,), float("nan"), dtype=torch.float32, device=dev)
    ds = torch.full((sl.n_docs,), float("nan"), dtype=torch.float32, device=dev)
    sd, yd = s.to(dev), y.to(dev)
    ragged.launch_loss(lib(), kind, sl, _ptr(sd), _ptr(yd), _ptr(slate), None, _ptr(ds), 1.0, args)      # one launch per tier
    torch.cuda.synchronize()
    return slate.cpu(), ds.cpu()


@pytest.mark.parametrize("shift", SC.RAGGED_SHIFTS)
def test_approxndcg_ragged_rotation(shift, dev):
    """One query per TIER_S length, regimes in rotation: a tier's launch mixes lengths and paths inside a workgroup."""
    lengths = RC.tier_lengths()
    assert sorted(lengths) == sorted(SC.TIER_S)
    s, y, info = SC.ragged_batch(lengths, shift=shift)
    assert {p for _, p in info} == {"noclamp", "fast", "perpair"}
    bounds, Q = RC.bounds_of(lengths), len(lengths)
    sl = _slates(lengths, dev)
    slate, ds = _ragged_launch(0, sl, s, y, (1.0, SC.EPS, SC.PAD), dev)
    ref = RC.oracle_ragged("approxNDCG", s, y, bounds)                                  # gradient of the MEAN over queries
    ref32 = RC.oracle_ragged("approxNDCG", s, y, bounds, dtype=torch.float32)
    assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(slate).all())
    for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        S, (regime, path) = int(b - a), info[q]
        c = SC.ragged_case(regime, S)
        gate("approxndcg_ragged_fwd_bwd", "slate_loss", c, path, slate[q:q + 1], ref["per_query"][q:q + 1], ref32["per_query"][q:q + 1].double())
        g64, g32 = ref["grad"][a:b] * Q, ref32["grad"][a:b].double() * Q
        gate("approxndcg_ragged_fwd_bwd", "dscores", c, path, ds[a:b], g64, g32, floor=SC.FLOOR if SC.uses_floor(c) else 0.0)
        if structurally_zero(y[a:b][None, :], SC.PAD)[0]:
            assert not bool(g64.any()) and not bool(ds[a:b].any()), (q, S, regime)


@pytest.mark.parametrize("sigmoid", [False, True])
def test_listnet_ragged_rotation(sigmoid, dev):
    lengths = RC.tier_lengths()
    yt, yp, cs = SC.list_ragged_batch(lengths, sigmoid)
    bounds = RC.bounds_of(lengths)
    sl = _slates(lengths, dev)
    slate, ds = _ragged_launch(1, sl, yp, yt, bool(sigmoid), dev)
    ref = RC.oracle_ragged("listnet", yp, yt, bounds, apply_sigmoid=sigmoid)
    ref32 = RC.oracle_ragged("listnet", yp, yt, bounds, dtype=torch.float32, apply_sigmoid=sigmoid)
    assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(slate).all())
    for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        c = cs[q]
        path = f"listnet {c.regime}" + (" sigmoid" if sigmoid else "")
        gate("listnet_ragged_fwd_bwd", "slate_loss", c, path, slate[q:q + 1], ref["per_query"][q:q + 1], ref32["per_query"][q:q + 1].double())
        gate("listnet_ragged_fwd_bwd", "dscores", c, path, ds[a:b], ref["grad"][a:b], ref32["grad"][a:b].double())
        if c.S == 1:
            assert not bool(ref["grad"][a:b].any()) and not bool(ds[a:b].any()), (q, c)


@pytest.mark.parametrize("S", [257, 1025])
@pytest.mark.parametrize("regime", ["noclamp", "perpair"])
def test_equal_lengths_are_the_rectangular_bits(regime, S, dev):
    """All lengths equal: the ragged launch is the rectangular launch's slate function, group size and reduction order."""
    from ltr_mi355x import lib
    A, alpha, eps, offset = SC.REGIMES[regime][0]
    c = SC.ApproxCase(regime, "tail", 2, S, alpha, eps, SC.PAD, A, offset)
    s, y, paths = SC.approx_inputs(c)
    assert set(paths) == {regime}
    sl = _slates([S] * c.B, dev)
    slate, ds = _ragged_launch(0, sl, s.reshape(-1), y.reshape(-1), (c.alpha, c.eps, c.pad), dev)
    r_slate, r_ds = approx_abi(lib(), s.to(dev), y.to(dev), c)
    assert torch.equal(slate, r_slate) and torch.equal(ds, r_ds.reshape(-1)), (regime, S)
    for sig in (False, True):
        lc = SC.ListCase("wide", sig, 2, S)
        yt, yp = SC.list_inputs(lc)
        slate, ds = _ragged_launch(1, sl, yp.reshape(-1), yt.reshape(-1), sig, dev)
        r_slate, r_ds = listnet_abi(lib(), yt.to(dev), yp.to(dev), sig)
        assert torch.equal(slate, r_slate) and torch.equal(ds, r_ds.reshape(-1)), ("listnet", sig, S)
