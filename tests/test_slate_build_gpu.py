"""GPU: fixed-length slates from a ragged collection and back (csrc/ltr_data.hip ltr_slates_*, ltr_mi355x/slates.py).

The kernels move and select, they compute nothing: every comparison is exact (torch.equal, floats as int32 bits) against the host
restatement of the selection (tests/slate_build_cases.py) and torch indexing on the CPU.  The two ranker tests compare a padded step
with the ragged step on the same batch at the bar tests/test_ragged_gpu.py uses for its padded-vs-ragged comparisons (TOL = 1e-5,
max-norm; parameter gradients through test_scorer_gpu.assert_grads at that bar)."""
import itertools

import numpy as np
import pytest
import torch

import ltr_metrics_oracle as MO
import slate_build_cases as SC
from conftest import relerr as _relerr
from test_scorer_gpu import _make, assert_grads

pytestmark = pytest.mark.gpu
TOL = 1e-5
CAN = -12345


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def select_batch(dev):
    """The slates of SC.SELECT_LENGTHS, shared by the select and the build tests."""
    from ltr_mi355x.ragged import RaggedSlates
    return RaggedSlates(SC.bounds_of(SC.SELECT_LENGTHS), device=dev)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _select_raw(dev, offsets, queries, n, S, mode, seed, out_rows, with_mask=True):
    """One raw ltr_slates_select launch into sentinel-filled buffers of out_rows rows."""
    from ltr_mi355x import lib
    rows = torch.full((out_rows, S), CAN, dtype=torch.int64, device=dev)
    mask = torch.full((out_rows, S), 77, dtype=torch.uint8, device=dev)
    rc = lib().ltr_slates_select(offsets.data_ptr(), None if queries is None else queries.data_ptr(), n, S, mode, seed, rows.data_ptr(),
                                 mask.data_ptr() if with_mask else None, _st())
    assert rc == 0
    torch.cuda.synchronize()
    return rows.cpu(), mask.cpu()


# ---------------------------------------------------------------------------------------------------- 6. select
def test_select_is_the_restatement(select_batch, dev):
    """Every slate length of SC.SELECT_S x both modes x both seeds, the lengths of SC.SELECT_LENGTHS in one batch."""
    sl = select_batch
    for S, mode, seed in itertools.product(SC.SELECT_S, ["first", "sample"], SC.SEEDS):
        case = (S, mode, seed)
        want_rows, want_mask = SC.select_host(sl.offsets_host, S, SC.MODES[mode], seed)
        rows, mask = _select_raw(dev, sl.offsets, None, sl.n_queries, S, SC.MODES[mode], seed, sl.n_queries)
        assert torch.equal(rows, torch.from_numpy(want_rows)), case
        assert torch.equal(mask, torch.from_numpy(want_mask)), case
        f = sl.fixed_length(S, mode=mode, seed=seed)                   # the host layer: the same launch
        assert torch.equal(f.rows.cpu(), rows) and torch.equal(f.mask.cpu(), mask), case
        assert f.kept.tolist() == [int(v) for v in (want_mask == 0).sum(axis=1)], case
        assert f.truncated == (max(SC.SELECT_LENGTHS) > S), case


def test_select_query_list_and_null_mask(select_batch, dev):
    sl = select_batch
    listed = [14, 3, 16, 0, 9, 11]                                     # a strict, unordered subset (1000, 5, 2048, 1, 100, 255 documents)
    q = torch.tensor(listed, dtype=torch.int32, device=dev)
    Q, S, seed = sl.n_queries, 32, 5
    for mode in ("first", "sample"):
        want_rows, want_mask = SC.select_host(sl.offsets_host, S, SC.MODES[mode], seed, listed)
        rows, mask = _select_raw(dev, sl.offsets, q, len(listed), S, SC.MODES[mode], seed, Q)
        assert torch.equal(rows[:len(listed)], torch.from_numpy(want_rows)), mode
        assert torch.equal(mask[:len(listed)], torch.from_numpy(want_mask)), mode
        assert bool((rows[len(listed):] == CAN).all()) and bool((mask[len(listed):] == 77).all()), mode     # nothing past the listed slots
        rows2, mask2 = _select_raw(dev, sl.offsets, q, len(listed), S, SC.MODES[mode], seed, Q, with_mask=False)
        assert torch.equal(rows2, rows) and bool((mask2 == 77).all()), mode


def test_select_pads_a_query_of_unsupported_length(dev):
    """Offsets are device data the launcher cannot check: a listed query of 0 or 2049 documents becomes S padding slots."""
    offsets = torch.tensor([0, 4, 4, 2053, 2060], dtype=torch.int64, device=dev)
    for mode in (SC.FIRST, SC.SAMPLE):
        rows, mask = _select_raw(dev, offsets, None, 4, 6, mode, 1, 4)
        want_rows, want_mask = SC.select_host(offsets.cpu().numpy(), 6, mode, 1)
        assert bool((torch.from_numpy(want_rows)[1:3] == -1).all())
        assert torch.equal(rows, torch.from_numpy(want_rows)) and torch.equal(mask, torch.from_numpy(want_mask))


# ---------------------------------------------------------------------------------------------------- 7. gather / scatter
# (row_floats, floats the bases are shifted by): 136 shifted by one float is 4-byte aligned only, so the 4-byte path runs on a row length
# the 16-byte path takes; 2048 and 4100 floats are the wide-row copy (one and two pieces per row) of the kernels shared with gather_rows.
ROW_CASES = [(1, 0), (3, 0), (4, 0), (136, 0), (138, 0), (136, 1), (2048, 0), (4100, 0)]


def _shifted(t, shift, dev):
    """t on the device at a base `shift` floats past an allocation's start."""
    buf = torch.empty(t.numel() + shift, dtype=torch.float32, device=dev)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * shift) % 16
    return v


def test_gather_vs_torch_indexing(dev):
    """Every case of ROW_CASES with fill 0, -1 and NaN."""
    for (row, shift), fill in itertools.product(ROW_CASES, [0.0, -1.0, float("nan")]):
        _gather_case(row, shift, fill, dev)


def _gather_case(row, shift, fill, dev):
    from ltr_mi355x import lib
    src_rows, n_slots = 37, 300 if row < 2048 else 21
    src = SC.special_payload(src_rows, row, 3 * row + shift)
    g = torch.Generator().manual_seed(row)
    rows = torch.randint(-1, src_rows + 1, (n_slots,), generator=g)                # -1 and src_rows are both out of range
    rows[:4] = torch.tensor([-1, src_rows, 0, src_rows - 1])
    want = src[rows.clamp(0, src_rows - 1)].clone()
    want[(rows < 0) | (rows >= src_rows)] = fill
    d_src = _shifted(src, shift, dev)
    out = _shifted(torch.full((n_slots, row), float(CAN)), shift, dev)
    rc = lib().ltr_slates_gather_f32(d_src.data_ptr(), src_rows, rows.to(dev).data_ptr(), n_slots, row, fill, out.data_ptr(), _st())
    assert rc == 0, (row, shift, fill)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want)), (row, shift, fill)


def test_scatter_vs_torch_indexing_and_round_trip(dev):
    for row, shift in ROW_CASES:
        _scatter_case(row, shift, dev)


def _scatter_case(row, shift, dev):
    from ltr_mi355x import lib
    dst_rows, n_slots = 50, 41
    src = SC.special_payload(n_slots, row, 5 * row + shift)
    g = torch.Generator().manual_seed(row + 1)
    rows = torch.randperm(dst_rows, generator=g)[:n_slots].clone()                 # no destination twice
    rows[[2, 11]] = -1
    rows[[5, 30]] = dst_rows
    named = (rows >= 0) & (rows < dst_rows)
    want = torch.full((dst_rows, row), float(CAN))
    want[rows[named]] = src[named]
    d_rows = rows.to(dev)
    out = _shifted(torch.full((dst_rows, row), float(CAN)), shift, dev)
    rc = lib().ltr_slates_scatter_f32(_shifted(src, shift, dev).data_ptr(), d_rows.data_ptr(), n_slots, row, dst_rows, out.data_ptr(), _st())
    assert rc == 0, (row, shift)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want)), (row, shift)                      # unnamed rows keep the sentinel
    # scatter(gather(t)) restores every named row of t
    t = SC.special_payload(dst_rows, row, 7 * row)
    mid = torch.empty((n_slots, row), dtype=torch.float32, device=dev)
    back = torch.full((dst_rows, row), float(CAN), device=dev)
    assert lib().ltr_slates_gather_f32(t.to(dev).data_ptr(), dst_rows, d_rows.data_ptr(), n_slots, row, 0.0, mid.data_ptr(), _st()) == 0
    assert lib().ltr_slates_scatter_f32(mid.data_ptr(), d_rows.data_ptr(), n_slots, row, dst_rows, back.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    want = torch.full((dst_rows, row), float(CAN))
    want[rows[named]] = t[rows[named]]
    assert torch.equal(_bits(back), _bits(want)), (row, shift)


def test_fixed_slates_gather_scatter_shapes(select_batch, dev):
    """The host layer over trailing shapes [n_docs], [n_docs, 3] and [n_docs, 2, 4]; scatter's zero fill and its out= form."""
    sl = select_batch
    f = sl.fixed_length(100, mode="sample", seed=9)
    rows = f.rows.cpu()
    for tail in ((), (3,), (2, 4)):
        t = torch.randn((sl.n_docs,) + tail, generator=torch.Generator().manual_seed(len(tail)))
        got = f.gather(t.to(dev), fill=-1.0)
        assert tuple(got.shape) == (sl.n_queries, 100) + tail
        assert torch.equal(got.cpu(), SC.pad_host(t, rows, -1.0))
        back = f.scatter(got)
        want = torch.zeros_like(t)
        want[rows[rows >= 0]] = t[rows[rows >= 0]]
        assert torch.equal(back.cpu(), want) and bool((want == 0).any())           # truncated queries: rows no slot names are 0
        out = torch.full_like(t, float(CAN)).to(dev)
        assert f.scatter(got, out=out) is out
        want[want == 0] = float(CAN)
        assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------- 8. build
def test_build_is_select_plus_two_gathers(select_batch, dev):
    """F in {136, 64, 10} x S in {5, 100} x both modes, pad -1, on the lengths of the select test."""
    from ltr_mi355x.slates import to_slates
    sl = select_batch
    for F in (136, 64, 10):
        X, y = SC.batch(SC.SELECT_LENGTHS, F, 1)
        Xd, yd = X.to(dev), y.to(dev)
        for S, mode in itertools.product((5, 100), ("first", "sample")):
            case = (F, S, mode)
            X3, y2, fixed = to_slates(Xd, yd, sl, S, mode=mode, seed=77, pad=-1.0)
            ref = sl.fixed_length(S, mode=mode, seed=77)                # ltr_slates_select, then ltr_slates_gather_f32 twice
            assert torch.equal(fixed.rows, ref.rows) and torch.equal(fixed.mask, ref.mask), case
            assert torch.equal(_bits(X3), _bits(ref.gather(Xd, fill=0.0))), case
            assert torch.equal(_bits(y2), _bits(ref.gather(yd, fill=-1.0))), case
            # and both are the restatement with torch indexing on the CPU
            rows, _ = SC.select_host(sl.offsets_host, S, SC.MODES[mode], 77)
            assert torch.equal(X3.cpu(), SC.pad_host(X, rows, 0.0)) and torch.equal(y2.cpu(), SC.pad_host(y, rows, -1.0)), case


def test_build_null_outputs_unaligned_base_and_baselines(select_batch, dev):
    from ltr_mi355x import lib
    from ltr_mi355x.slates import to_slates
    sl = select_batch
    S, F = 32, 136
    X, y = SC.batch(SC.SELECT_LENGTHS, F, 2)
    want, _, fixed, yb = to_slates(X.to(dev), y.to(dev), sl, S, mode="sample", seed=3, y_base=X[:, :3].contiguous().to(dev), base_fill=-2.0)
    assert torch.equal(yb.cpu(), SC.pad_host(X[:, :3], fixed.rows.cpu(), -2.0))
    # mask = rows = NULL, and X / X_out one float past a 16-byte boundary: the 4-byte copy on F % 4 == 0
    Xs = _shifted(X, 1, dev)
    X3 = _shifted(torch.full((sl.n_queries, S, F), float(CAN)), 1, dev)
    y2 = torch.empty((sl.n_queries, S), device=dev)
    rc = lib().ltr_slates_build(Xs.data_ptr(), y.to(dev).data_ptr(), sl.offsets.data_ptr(), None, sl.n_queries, S, F, 1, 3, -1.0,
                                X3.data_ptr(), y2.data_ptr(), None, None, _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(X3), _bits(want))


# ---------------------------------------------------------------------------------------------------- 9. autograd
def _small(dev, S=8, seed=4):
    from ltr_mi355x.ragged import RaggedSlates
    lengths = [3, 8, 20, 1, 9]
    sl = RaggedSlates(SC.bounds_of(lengths), device=dev)
    return lengths, sl, sl.fixed_length(S, mode="sample", seed=seed)


def test_gather_and_scatter_gradients_are_torch_indexing_gradients(dev):
    lengths, sl, f = _small(dev)
    rows = f.rows.cpu()
    real = rows >= 0
    g = torch.Generator().manual_seed(0)
    t, w = torch.randn(sl.n_docs, 3, generator=g), torch.randn(sl.n_queries, f.S, 3, generator=g)
    a = t.clone().requires_grad_(True)                                  # torch indexing on the CPU
    ref = torch.where(real[..., None], a[rows.clamp(min=0)], torch.full((), -1.0))
    (ref * w).sum().backward()
    b = t.to(dev).requires_grad_(True)
    got = f.gather(b, fill=-1.0)
    (got * w.to(dev)).sum().backward()
    assert torch.equal(got.detach().cpu(), ref.detach()) and torch.equal(b.grad.cpu(), a.grad)
    assert float(a.grad.abs().sum()) > 0 and bool((a.grad == 0).any())  # the sampled-out documents get exactly 0

    u, v = torch.randn(sl.n_queries, f.S, 3, generator=g), torch.randn(sl.n_docs, 3, generator=g)
    a = u.clone().requires_grad_(True)
    ref = torch.zeros(sl.n_docs, 3).index_put((rows[real],), a[real])
    (ref * v).sum().backward()
    b = u.to(dev).requires_grad_(True)
    got = f.scatter(b)
    (got * v.to(dev)).sum().backward()
    assert torch.equal(got.detach().cpu(), ref.detach()) and torch.equal(b.grad.cpu(), a.grad)
    assert bool((a.grad[~real] == 0).all())                             # padding slots


def test_backward_uses_forward_time_rows(dev):
    """The state test of the two lazily built nodes (ltr_mi355x.slates._row_map_functions): the backward runs on the rows of the
    forward, whatever happens to the FixedSlates' tensors in between."""
    lengths, sl, f = _small(dev)
    g = torch.Generator().manual_seed(1)
    t = torch.randn(sl.n_docs, generator=g).to(dev)
    u = torch.randn(sl.n_queries, f.S, generator=g).to(dev)
    w1, w2 = torch.randn(sl.n_queries, f.S, generator=g).to(dev), torch.randn(sl.n_docs, generator=g).to(dev)
    calls = {"gather": (lambda x, fx: fx.gather(x, fill=3.0), t, w1), "scatter": (lambda x, fx: fx.scatter(x), u, w2)}
    for name, (fn, x0, w) in calls.items():
        a = x0.clone().requires_grad_(True)
        (fn(a, sl.fixed_length(f.S, mode="sample", seed=4)) * w).sum().backward()
        want = a.grad.clone()
        fx = sl.fixed_length(f.S, mode="sample", seed=4)
        b = x0.clone().requires_grad_(True)
        out = fn(b, fx)
        assert out.grad_fn is not None and out.grad_fn.next_functions[0][0].variable is b, name        # one node
        with torch.no_grad():
            fx.rows.zero_()
            fx.mask.fill_(1)
        (out * w).sum().backward()
        assert torch.equal(b.grad, want) and float(want.abs().sum()) > 0, name


# ---------------------------------------------------------------------------------------------------- 10. FC rankers
STEP_LENGTHS = (3, 17, 32, 33, 50, 64)


@pytest.mark.parametrize("kind", ["double", "fc"])
def test_fc_ranker_on_padded_slates_is_the_ragged_step(kind, dev):
    """to_slates at S = the longest query keeps every document: the padded step (labels -1 in padding, which both losses mask) and
    step_ragged see the same queries.  Loss and every parameter gradient at test_ragged_gpu's padded-vs-ragged bar, for approxNDCG and
    lambdaLoss."""
    for loss in ("approxNDCG", "lambdaLoss"):
        _padded_vs_ragged_step(kind, loss, dev)


def _padded_vs_ragged_step(kind, loss, dev):
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.scorer import FusedRanker
    from ltr_mi355x.slates import to_slates
    if kind == "fc":
        from test_linear_fused_gpu import _model
        net = _model(dev)
    else:
        net, _ = _make("double", dev, 31)
    net.eval()                                                          # dropout off
    extra = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
    ranker = FusedRanker(net, loss=loss, **extra)
    X, y = SC.batch(STEP_LENGTHS, 136, 21)
    sl = RaggedSlates(SC.bounds_of(STEP_LENGTHS), device=dev)
    Xd, yd = X.to(dev), y.to(dev)
    want_loss = float(ranker.step_ragged(Xd, yd, sl))
    want = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    ranker.flat_ext.zero_()
    X3, y2, fixed = to_slates(Xd, yd, sl, sl.max_len, mode="first")
    assert not fixed.truncated and tuple(X3.shape) == (6, 64, 136)
    got_loss = float(ranker.step(X3, y2))
    got = {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}
    e = _relerr(got_loss, want_loss)
    print(f"{kind} {loss}: padded vs ragged loss rel err {e:.3e}")
    assert e < TOL
    assert max(float(np.abs(v).max()) for v in want.values()) > 0
    assert_grads(got, want, tol=TOL)


# ---------------------------------------------------------------------------------------------------- 11. transformer
def test_transformer_trains_on_ragged_collections_through_the_bridge(dev):
    from architeture.multiLayer import make_model
    from losses.listnet import listnetLoss
    from ltr_mi355x import ragged
    from ltr_mi355x.slates import from_slates, to_slates
    F, S = 16, 64
    torch.manual_seed(3)
    net = make_model(dict(sizes=[64], input_norm=False, activation=None, dropout=0.0),
                     dict(N=1, d_ff=128, h=2, dropout=0.0, positional_encoding=None), dict(d_output=1, output_activation=None), F).to(dev)
    net.train()
    bounds = SC.bounds_of(STEP_LENGTHS)
    sl = ragged.RaggedSlates(bounds, device=dev)
    X, y = SC.batch(STEP_LENGTHS, F, 22)
    Xd, yd = X.to(dev), y.to(dev)
    X3, y2, fixed = to_slates(Xd, yd, sl, S, mode="first")
    # the host-padded copy of the batch
    Xh, yh = torch.zeros(len(STEP_LENGTHS), S, F), torch.full((len(STEP_LENGTHS), S), -1.0)
    for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        Xh[q, :b - a], yh[q, :b - a] = X[a:b], y[a:b]
    mh = yh == -1.0
    assert torch.equal(X3.cpu(), Xh) and torch.equal(y2.cpu(), yh) and torch.equal(fixed.mask.cpu().bool(), mh)
    scores = net(X3, fixed.mask, None)
    host_scores = net(Xh.to(dev), mh.to(dev), None)
    assert tuple(scores.shape) == (len(STEP_LENGTHS), S) and torch.equal(scores, host_scores)
    # NDCG@10 after the scatter = per query from the host-padded scores
    flat = from_slates(scores, fixed)
    got = ragged.ndcg_at_k(yd, flat.detach(), sl, k=10)
    hs = host_scores.detach().cpu()
    unpadded = torch.cat([hs[q, :b - a] for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])
    assert torch.equal(flat.detach().cpu(), unpadded)
    assert torch.equal(got, ragged.ndcg_at_k(yd, unpadded.to(dev), sl, k=10))
    ref = np.array([MO.ndcg_per_query(y[a:b].numpy()[None], hs[q, :b - a].numpy()[None], k=10, no_relevant=True, gains="linear",
                                      stable=True)[0] for q, (a, b) in enumerate(zip(bounds[:-1], bounds[1:]))])
    assert float(np.abs(got.cpu().numpy() - ref).max()) < 1e-12
    # ListNet through the scatter trains every parameter ...
    loss = ragged.listnet(yd, flat, sl)
    loss.backward()
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    assert max(float(p.grad.abs().max()) for p in net.parameters()) > 0
    # ... and is not listnetLoss on the padded rectangle, which has no padding concept: that value is the wrong one
    padded = float(listnetLoss(y2, scores.detach()))
    bridged = float(loss.detach())
    print(f"ragged listnet through the bridge {bridged:.6f}, listnetLoss on the padded [B, S] tensors {padded:.6f}")
    assert abs(bridged - padded) > 1e-3 * abs(padded)
